"""RewardConfig — the reference's experience.RewardConfig (internal/experience/rewards.go:8-20) as the configurable reward of
the engine (VecEngine.experience_rewards(config=...)) and of the gym vector envs (reward_config=...).

The value is CalculateRewardWithConfig (rewards.go:45-85) in float32 and the reference's order of additions, computed by
one HIP launch from the snapshot taken before the step (gvec_experience_rewards_config, include/generals_vec.h):

    a finished game with a winner:  win_game for the winner, lose_game for everybody else        :49-56
    otherwise                       d_territory * territory_gained + d_army * army_gained        :59-68
                                    + cities gained * capture_city + cities lost * lose_city     :71-73
                                    + generals gained * capture_general + lost * lose_general    :76-78
                                    + army advantage in [-1, 1] * army_advantage                 :81-82
    clip                            NormalizeReward (:215-223): clamped to [-1, 1]
    an env re-dealt / not stepped   0
    invalid_action                  added last, where the env flagged the learner's action as refused

Two quirks of the reference are kept (parity wins):
  * TerritoryLost and ArmyLost are never read: a negative difference is multiplied by the *Gained* weight.  A config whose
    *_lost is not the negated *_gained would silently not mean what it says, so it is refused.
  * win_game / lose_game REPLACE the shaped terms on the last step of a game; they are not added to them.
"""
import dataclasses
import math

_WEIGHTS = ("win_game", "lose_game", "capture_city", "lose_city", "capture_general", "lose_general", "territory_gained",
            "territory_lost", "army_gained", "army_lost", "army_advantage", "invalid_action")

# names of the eight int32 of a `terms` row (gvec_experience_rewards_config); army_advantage_bits is a float32 bit pattern
REWARD_TERMS = ("d_territory", "d_army", "cities_gained", "cities_lost", "generals_gained", "generals_lost", "outcome",
                "army_advantage_bits")


@dataclasses.dataclass(frozen=True)
class RewardConfig:
    # DefaultRewardConfig (rewards.go:23-37)
    win_game: float = 1.0
    lose_game: float = -1.0
    capture_city: float = 0.1
    lose_city: float = -0.1
    capture_general: float = 0.5
    lose_general: float = -0.5
    territory_gained: float = 0.01
    territory_lost: float = -0.01
    army_gained: float = 0.001
    army_lost: float = -0.001
    army_advantage: float = 0.05
    # not in the reference: what a refused action costs (added after the clip), and NormalizeReward on / off
    invalid_action: float = 0.0
    clip: bool = False

    def __post_init__(self):
        for name in _WEIGHTS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"RewardConfig.{name} must be a finite number, not {v!r}")
        if not isinstance(self.clip, bool):
            raise ValueError(f"RewardConfig.clip must be a bool, not {self.clip!r}")
        for lost, gained in (("territory_lost", "territory_gained"), ("army_lost", "army_gained")):
            if getattr(self, lost) != -getattr(self, gained):
                raise ValueError(
                    f"RewardConfig.{lost} = {getattr(self, lost)} is not -{gained} = {-getattr(self, gained)}: the reference's "
                    f"CalculateRewardWithConfig never reads {lost} - it multiplies a negative difference by {gained} "
                    "(rewards.go:62, :68) - so a separate loss weight would be ignored; set it to the negated gain")

    @classmethod
    def go_default(cls):
        """DefaultRewardConfig() of the reference (rewards.go:23-37): what gvec_experience_rewards computes."""
        return cls()

    @classmethod
    def sparse(cls, invalid_action=0.0):
        """Outcome only: +1 for the winner and -1 for the losers on the last step of a game, 0 everywhere else."""
        return cls(win_game=1.0, lose_game=-1.0, capture_city=0.0, lose_city=0.0, capture_general=0.0, lose_general=0.0,
                   territory_gained=0.0, territory_lost=-0.0, army_gained=0.0, army_lost=-0.0, army_advantage=0.0,
                   invalid_action=invalid_action)

    @classmethod
    def clipped(cls, invalid_action=-0.1):
        """The reference's defaults through NormalizeReward, with the gym envs' -0.1 for a refused action: every step's
        reward lies in [-1.1, 1]."""
        return cls(invalid_action=invalid_action, clip=True)

    def scale(self):
        """A bound of |reward| on a terminal step: max(|win_game|, |lose_game|) (1 at most when clipped) + |invalid_action|.
        What a categorical value head's support is sized from."""
        top = max(abs(self.win_game), abs(self.lose_game))
        return (min(top, 1.0) if self.clip else top) + abs(self.invalid_action)

    def to_c(self):
        """The gvec_reward_config the kernels read."""
        from ._lib import REWARD_CLIP, RewardConfigC
        return RewardConfigC(win_game=self.win_game, lose_game=self.lose_game, capture_city=self.capture_city, lose_city=self.lose_city,
                             capture_general=self.capture_general, lose_general=self.lose_general, territory=self.territory_gained,
                             army=self.army_gained, army_advantage=self.army_advantage, invalid_action=self.invalid_action,
                             flags=REWARD_CLIP if self.clip else 0, reserved=0)
