"""generalsreinforcementlearning_amd — MI355X-native batched Generals.io turn engine.

Product code: hand-written HIP kernels for gfx950 (csrc/) behind the C ABI of
include/generals_vec.h, plus this thin host mirror of the reference's
``game.Engine`` method set.  There is no CPU fallback: importing works without a
GPU (the build check), but every compute call needs the HIP library and a device.
"""
from ._lib import GvecError, lib, lib_path, load  # noqa: F401
from .vec_engine import (ACTION_DTYPE, ACT_HALF, ACT_VALID, ERR_NAMES, TILE_CITY, TILE_GENERAL, TILE_MOUNTAIN,  # noqa: F401
                         TILE_NORMAL, VecEngine, make_actions, unpack_legal_bits)
from .env_state import VecEnvState  # noqa: F401
from .reward import REWARD_TERMS, RewardConfig  # noqa: F401
from .replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer  # noqa: F401
from .rollout import SelfPlayRolloutBuffer  # noqa: F401
from .policy_head import MaskedCategoricalHead, distill_loss  # noqa: F401
from .features import NUM_STRATEGIC_FEATURES, STRATEGIC_FEATURE_NAMES, strategic_features  # noqa: F401
from .memory import MEMORY_PLANE_NAMES, NUM_MEMORY_PLANES, ObservationMemory, remembered_observation  # noqa: F401
from .q_targets import categorical_target, double_q_target, valid_actions_mask_from_observation  # noqa: F401
from .symmetry import apply_symmetry, augment_transition, inverse_symmetry, num_symmetries, random_symmetries  # noqa: F401
from .arena import (Arena, ArenaResult, EpisodeTally, balanced_seating, expected_score, fit_elo, random_policy,  # noqa: F401
                    torch_policy)
from .search import HalvingSearch, PlayoutScore, PlayoutSearch, TreeSearch, halving_schedule, playout_policy  # noqa: F401

__all__ = ["VecEngine", "GvecError", "lib", "load", "lib_path", "ACTION_DTYPE", "make_actions", "unpack_legal_bits", "VecEnvState", "RewardConfig", "REWARD_TERMS",
           "DeviceReplayBuffer", "PrioritizedDeviceReplayBuffer", "SelfPlayRolloutBuffer", "MaskedCategoricalHead", "distill_loss", "strategic_features",
           "NUM_STRATEGIC_FEATURES", "STRATEGIC_FEATURE_NAMES", "ObservationMemory", "remembered_observation", "NUM_MEMORY_PLANES",
           "MEMORY_PLANE_NAMES", "valid_actions_mask_from_observation", "double_q_target", "categorical_target",
           "apply_symmetry", "augment_transition", "inverse_symmetry", "num_symmetries", "random_symmetries",
           "Arena", "ArenaResult", "EpisodeTally", "balanced_seating", "expected_score", "fit_elo", "random_policy", "torch_policy",
           "PlayoutScore", "PlayoutSearch", "playout_policy", "HalvingSearch", "halving_schedule", "TreeSearch"]
