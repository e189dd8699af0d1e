// gvec_api_gym.hip — the gym surface: observations, action decoding and the fused steps, for one learner or a set of them.
// Host only (gvec_handle.hpp); the kernels are in gvec_gym.hip.
#include "gvec_handle.hpp"

// the player stats the gym rewards are measured against, [B][3*MAXP]: allocated, zeroed, on first use (the handle's device is current)
int32_t ensure_gym_prev(gvec_handle* h) {
  if (!h->d_gym_prev) {
    const size_t bytes = (size_t)h->cfg.num_envs * 3 * h->var.maxp * 4;
    HIPCHK(hipMalloc(&h->d_gym_prev, bytes));
    HIPCHK(hipMemsetAsync(h->d_gym_prev, 0, bytes, h->stream));
  }
  return GVEC_OK;
}

// what every gym observation call takes from the handle (after ensure_gym_prev)
static GymArgs gym_args(gvec_handle* h, int32_t player, const int64_t* turn_count, int32_t max_turns, float* obs, uint8_t* mask, double* reward,
                        uint8_t* done, int8_t* winner) {
  GymArgs a = state_args<GymArgs>(h);
  a.turn_count = turn_count;
  a.obs = obs;
  a.mask = mask;
  a.reward = reward;
  a.done = done;
  a.winner = winner;
  a.prev_stats = h->d_gym_prev;
  a.num_envs = h->cfg.num_envs;
  a.fd = h->fd;
  a.row_dw = h->row_dw;
  a.stride = h->stride;
  a.player = player;
  a.max_turns = max_turns;
  return a;
}

// the fused steps end episodes by re-dealing, and their opponents are the on-device agent seeded per call
static int32_t gym_fused_step_args(gvec_handle* h, uint64_t agent_seed, const char* what, StepArgs* a) {
  if (!(h->cfg.auto_reset && h->pool_size > 0)) {
    set_err("%s needs auto_reset and a board pool (gvec_build_board_pool): episodes end by re-dealing", what);
    return GVEC_E_INVALID;
  }
  *a = base_args(h);
  set_agent_seed(a, agent_seed, 0);
  return GVEC_OK;
}

static int32_t gym_observe_impl(gvec_handle* h, int32_t player, const int64_t* turn_count, int32_t max_turns, float* obs, uint8_t* mask,
                                double* reward, uint8_t* done, int8_t* winner, const uint8_t* resetting, const uint8_t* played, int64_t* turn_io,
                                int64_t* turn_out, uint8_t* terminated, uint8_t* truncated, uint8_t* needs_reset) {
  if (!h || !turn_count || !obs || !mask || player < 0 || player >= h->maxp || max_turns < 1) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_gym_observe / gvec_gym_finish_step");
  HIPCHK(hipSetDevice(h->cfg.device));
  RET_IF(ensure_gym_prev(h));
  GymArgs a = gym_args(h, player, turn_count, max_turns, obs, mask, reward, done, winner);
  a.resetting = resetting;
  a.played = played;
  a.turn_io = turn_io;
  a.turn_out = turn_out;
  a.terminated = terminated;
  a.truncated = truncated;
  a.needs_reset = needs_reset;
  HIPCHK(launch_gym_observe(h->var, a, h->stream));
  return GVEC_OK;
}

// the checks both self-play calls share (each failure names itself in gvec_last_error); allocates the stored player stats
// on first use.  `ptrs_ok`: every required pointer is non-null
static int32_t gym_players_prepare(gvec_handle* h, uint32_t learners, bool ptrs_ok, int32_t max_turns, const char* what) {
  if (learners == 0u || (learners >> GVEC_MAX_PLAYERS) != 0u || (h && !h->sharded() && (learners >> h->maxp) != 0u)) {
    set_err("%s: learners must be a non-empty set of player ids below max_players", what);
    return GVEC_E_INVALID;
  }
  if (!h || !ptrs_ok || max_turns < 1) {
    set_err("%s: null handle, a required pointer is null, or max_turns < 1", what);
    return GVEC_E_INVALID;
  }
  if (h->sharded()) return sharded::unsupported(what);
  HIPCHK(hipSetDevice(h->cfg.device));
  RET_IF(ensure_gym_prev(h));
  return GVEC_OK;
}

extern "C" {

int32_t gvec_gym_observe(gvec_handle* h, int32_t player, const int64_t* turn_count, int32_t max_turns, float* obs, uint8_t* mask,
                         double* reward, uint8_t* done, int8_t* winner) {
  return gym_observe_impl(h, player, turn_count, max_turns, obs, mask, reward, done, winner, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr);
}

int32_t gvec_gym_finish_step(gvec_handle* h, int32_t player, int64_t* turn_count, int32_t max_turns, const uint8_t* resetting,
                             const uint8_t* played, float* obs, uint8_t* mask, double* reward, uint8_t* terminated, uint8_t* truncated,
                             int8_t* winner, uint8_t* needs_reset, int64_t* turn_out) {
  if (!resetting || !played) return GVEC_E_INVALID;
  return gym_observe_impl(h, player, turn_count, max_turns, obs, mask, reward, nullptr, winner, resetting, played, turn_count, turn_out, terminated,
                          truncated, needs_reset);
}

int32_t gvec_gym_actions(gvec_handle* h, int32_t player, const int64_t* gym_actions, const uint8_t* mask, const uint8_t* resetting,
                         gvec_action* actions, uint8_t* played, uint8_t* invalid, uint8_t* error) {
  if (!h || !gym_actions || !mask || !actions || player < 0 || player >= h->maxp) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_gym_actions");
  HIPCHK(hipSetDevice(h->cfg.device));
  GymActArgs a;
  memset(&a, 0, sizeof a);
  a.hdr = h->d_hdr;
  a.gym_actions = gym_actions;
  a.mask = mask;
  a.resetting = resetting;
  a.actions = actions;
  a.played = played;
  a.invalid = invalid;
  a.error = error;
  a.num_envs = h->cfg.num_envs;
  a.stride = h->stride;
  a.pstride = h->maxp;
  a.player = player;
  HIPCHK(launch_gym_actions(a, h->stream));
  return GVEC_OK;
}

int32_t gvec_gym_step(gvec_handle* h, int32_t player, uint64_t agent_seed, const int64_t* gym_actions, const uint8_t* resetting,
                      int64_t* turn_count, int32_t max_turns, float* obs, uint8_t* mask, double* reward, uint8_t* terminated,
                      uint8_t* truncated, int8_t* winner, uint8_t* needs_reset, int64_t* turn_out, uint8_t* played, uint8_t* invalid,
                      uint8_t* error) {
  if (!h || !gym_actions || !resetting || !turn_count || !obs || !mask || player < 0 || player >= h->maxp || max_turns < 1) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_gym_step");
  StepArgs a;
  RET_IF(gym_fused_step_args(h, agent_seed, "gvec_gym_step", &a));
  HIPCHK(hipSetDevice(h->cfg.device));
  RET_IF(ensure_gym_prev(h));
  GymStepArgs g;
  memset(&g, 0, sizeof g);
  g.gym_actions = gym_actions;
  g.resetting = resetting;
  g.turn_io = turn_count;
  g.turn_out = turn_out;
  g.obs = obs;
  g.mask = mask;
  g.reward = reward;
  g.terminated = terminated;
  g.truncated = truncated;
  g.winner = winner;
  g.needs_reset = needs_reset;
  g.played = played;
  g.invalid = invalid;
  g.error = error;
  g.prev_stats = h->d_gym_prev;
  g.stride = h->stride;
  g.player = player;
  g.max_turns = max_turns;
  HIPCHK(launch_gym_step(h->var, a, g, h->stream));
  h->legal_valid = false;  // the engine's own mask buffer was not refreshed
  return GVEC_OK;
}

int32_t gvec_gym_observe_players(gvec_handle* h, uint32_t learners, const int64_t* turn_count, int32_t max_turns, float* obs, uint8_t* mask,
                                 double* reward, uint8_t* done, int8_t* winner) {
  RET_IF(gym_players_prepare(h, learners, turn_count && obs && mask, max_turns, "gvec_gym_observe_players"));
  const GymArgs a = gym_args(h, -1, turn_count, max_turns, obs, mask, reward, done, winner);
  HIPCHK(launch_gym_observe_players(h->var, a, learners, h->stream));
  return GVEC_OK;
}

int32_t gvec_gym_step_players(gvec_handle* h, uint32_t learners, uint64_t agent_seed, const int64_t* gym_actions, const uint8_t* resetting,
                              int64_t* turn_count, int32_t max_turns, float* obs, uint8_t* mask, double* reward, uint8_t* terminated,
                              uint8_t* truncated, int8_t* winner, uint8_t* needs_reset, int64_t* turn_out, uint8_t* invalid, uint8_t* error,
                              uint8_t* alive) {
  RET_IF(gym_players_prepare(h, learners, gym_actions && resetting && turn_count && obs && mask, max_turns, "gvec_gym_step_players"));
  StepArgs a;
  RET_IF(gym_fused_step_args(h, agent_seed, "gvec_gym_step_players", &a));
  GymPlayersArgs g;
  memset(&g, 0, sizeof g);
  g.gym_actions = gym_actions;
  g.resetting = resetting;
  g.turn_io = turn_count;
  g.turn_out = turn_out;
  g.obs = obs;
  g.mask = mask;
  g.reward = reward;
  g.invalid = invalid;
  g.error = error;
  g.alive = alive;
  g.terminated = terminated;
  g.truncated = truncated;
  g.winner = winner;
  g.needs_reset = needs_reset;
  g.prev_stats = h->d_gym_prev;
  g.learners = learners;
  g.nl = __builtin_popcount(learners);
  g.stride = h->stride;
  g.max_turns = max_turns;
  HIPCHK(launch_gym_step_players(h->var, a, g, h->stream));
  h->legal_valid = false;  // the engine's own mask buffer was not refreshed
  return GVEC_OK;
}

}  // extern "C"
