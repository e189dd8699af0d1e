// gvec_gym.hip — python/generals_gym's GeneralsEnv on the device: observe and step, for one learner or a set of them.
#include "gvec_dispatch.hpp"
#include "gvec_gym_emit.hpp"
#include "gvec_turn.hpp"

namespace gvec {

// waves per SIMD asked of gym_step_players_kernel, per tile slot count, from a same-process A/B of 5 / 4 / 3 waves at 65,536
// envs: four up to 448 tiles (20x20 4P 0.86 ms against 0.93 with three, 1.17 with five), three above;
// -DGYM_PLAYERS_WAVES=n forces one value for A/B builds
#ifdef GYM_PLAYERS_WAVES
#define GYM_PLAYERS_WAVES_OF(NSLOT) GYM_PLAYERS_WAVES
#else
#define GYM_PLAYERS_WAVES_OF(NSLOT) ((NSLOT) <= 7 ? 4 : 3)
#endif

// setup_kernel belongs to the import (gvec_state.hip) and is compiled here for the step kernels' sake: the link-time optimiser
// propagates the arguments of PBoard::store_planes into it when every caller of a unit passes compile-time plane strides, as the
// two step kernels do, and 16 of their 72 instantiations then come out with other code than they had next to a caller with
// run-time strides (DESIGN.md "Translation units").  This is that caller.
// EngineInitializer.performInitialSetup (engine_initializer.go:218-225) for the envs an import marked
// (HF_SETUP): full stats pass, full fog pass, game-over check on the freshly imported board.
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void setup_kernel(ImportArgs A) {
  using B = Turn<MAXP, NSLOT>;
  const int i = wave_item();
  if (i >= A.n) return;
  const int env = A.env_ids ? uni(A.env_ids[i]) : A.dst_begin + i;
  if (env < 0 || env >= A.dst_envs) return;  // reported by the import kernel
  B b;
  b.larmy = nullptr;
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd, A.zeros);
  if (!(b.hflags & HF_SETUP)) return;  // this env's input was rejected: left as it was
  b.hflags &= ~HF_SETUP;
  b.initial_setup();
  settle_lists(b);
  b.store_hdr(A.hdr + (size_t)env * HDR_DW, 0u);
  b.store_planes(A.rows + (size_t)env * A.row_dw, A.fd, A.row_dw, false);
}

// =========================================================================================
// python/generals_gym/generals_env.py on the device: what GeneralsEnv builds from the GameState proto the
// server sends for its player token - observation (:291-342), valid-action mask (:344-387), reward
// (:499-561) - computed straight from the resident state with the proto's fog rules applied in the kernel
// (internal/grpc/gameserver/server.go:556-582: a tile that is neither visible nor "known in fog" shows type
// NORMAL / owner -1 / army 0; a fogged tile keeps its type, hides owner and army.  A hidden tile is a normal
// tile by definition (visibility_optimized.go:189-191), so the shown type is always the real one).
// =========================================================================================
// gym_emit, the stores of one env's observation and mask: gvec_gym_emit.hpp

// =========================================================================================
// The phases the four gym kernels below are put together from.  gym_observe_kernel and
// gym_observe_players_kernel read the plain Board layout, gym_step_kernel and gym_step_players_kernel play the turn on the
// packed Turn layout; every rule of the reference is cited once, on its phase.
// =========================================================================================
// GymView, the Turn layout's player_view / turn_view, gym_sources, gym_decode, turn_tile_counts, army_counts and gym_winner
// are gvec_turn.hpp's: the playout search (gvec_search.hip) reads a board the same way.
// Board layout: one register per player and plane kind.  pl is wave-uniform.
template <int MAXP, typename BT>
__device__ __forceinline__ GymView board_view(const BT& b, int pl) {
  uint32_t own_p = 0u, vis_p = 0u;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    own_p = (p == pl) ? b.own[p] : own_p;
    vis_p = (p == pl) ? b.vis[p] : vis_p;
  }
  return GymView{own_p, (b.hflags & HF_FOG) ? vis_p : b.valid};
}

// channel 7: min(turn_count / max_turns, 1.0) in float64, stored as float32 (:338-339)
__device__ __forceinline__ double gym_turn_channel(int64_t turns, int max_turns) {
  const double tcn = (double)turns / (double)max_turns;
  return tcn < 1.0 ? tcn : 1.0;
}

// _get_valid_actions_mask: from a source tile towards a neighbour on the board whose shown type is not MOUNTAIN; index
// tile*5 + {up, right, down, left}, +4 = half move ("valid iff a full move is")
struct GymMask {
  uint32_t m0, m1, m2, m3, many;
};
template <typename BT>
__device__ __forceinline__ GymMask gym_mask(const BT& b, const GymView& v) {
  const uint32_t src = gym_sources(b, v);
  const uint32_t m0 = src & b.ok[0], m1 = src & b.ok[1], m2 = src & b.ok[2], m3 = src & b.ok[3];
  return GymMask{m0, m1, m2, m3, m0 | m1 | m2 | m3};
}
// one player's observation and mask into slot `slot` of obs [.][9][stride] / mask [.][stride*5].  ms: see gym_emit
template <int NSLOT, typename BT>
__device__ __forceinline__ void gym_emit_player(const BT& b, const GymView& v, const GymMask& m, uint32_t own_any, double tcn, float* obs,
                                                uint8_t* mask, size_t slot, uint8_t* ms, int stride) {
  gym_emit<NSLOT>(b, v.seen, v.own, own_any, m.m0, m.m1, m.m2, m.m3, m.many, (float)tcn, obs + slot * 9 * (size_t)stride,
                  mask + slot * 5 * (size_t)stride, ms, stride);
}

// own_any: anybody's tiles, as a replicated flat plane; cnt[p]: PlayerState.tile_count = len(OwnedTiles) (server.go:536), a
// wave-wide reduction every lane takes part in
template <int MAXP, typename BT>
__device__ __forceinline__ void board_totals(const BT& b, uint32_t& own_any, uint32_t (&cnt)[MAXP]) {
  own_any = 0u;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    own_any |= b.own[p];
    cnt[p] = (uint32_t)b.count(b.lst[p]);
  }
}
// a[pl] (pl wave-uniform) / a[lane] without indexing registers
template <int MAXP>
__device__ __forceinline__ uint32_t pick(const uint32_t (&a)[MAXP], int pl) {
  uint32_t out = 0u;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) out = (p == pl) ? a[p] : out;
  return out;
}
template <typename B>
__device__ __forceinline__ uint32_t turn_own_any(const B& b) {
  uint32_t own_any = 0u;
#pragma unroll
  for (int k = 0; k < B::NR; ++k) own_any |= b.own[k];
  return B::or_rows(own_any);
}
// _calculate_reward (generals_env.py:499-561) for player `pl` against the stats the previous call stored.  cur_tc / cur_ac:
// the player's tile_count and ArmyCount now.  With several learners the caller stores the new stats (gym_store_stats) only
// after every learner's reward is computed.  Lane 0 calls it.
template <int MAXP>
__device__ __forceinline__ double gym_player_reward(int pl, int P, uint32_t alive, bool over, int winner, int32_t cur_tc, int32_t cur_ac,
                                                    const int32_t* prev) {
  double r = 0.0;
  r += (double)(cur_tc - prev[pl]) * 1.0;                                         // :540-542
  r += (double)(cur_ac - prev[MAXP + pl]) * 0.01;                                 // :544-546
  for (int q = 0; q < P; ++q)                                                     // :548-555
    if (q != pl && prev[2 * MAXP + q] != 0 && !((alive >> q) & 1u)) r += 50.0;
  if (over) r = (winner == pl) ? 100.0 : -100.0;                                  // :520-524
  return r;
}
// every player's stats for the next call's reward (tcl / acl: lane p < MAXP holds player p's); every lane calls it
template <int MAXP>
__device__ __forceinline__ void gym_store_stats(int32_t* prev, uint32_t tcl, uint32_t acl, uint32_t alive) {
  const int lane = lane_id();
  if (lane < MAXP) {
    prev[lane] = (int32_t)tcl;
    prev[MAXP + lane] = (int32_t)acl;
    prev[2 * MAXP + lane] = (int32_t)((alive >> lane) & 1u);
  }
}

struct GymFlowOut {
  double* reward;
  uint8_t* done;
  int8_t* winner;
  int64_t* turn_io;
  int64_t* turn_out;
  uint8_t* terminated;
  uint8_t* truncated;
  uint8_t* needs_reset;
};
// GeneralsEnv.step's episode flags (generals_env.py:243-259): terminated = game over, truncated = turn limit, neither for an
// env that sat the call out (!played) or was re-dealt (rs).  Lane 0 calls it.
__device__ __forceinline__ void gym_store_flags(int env, bool over, bool played, bool rs, int winner, int64_t turns, int max_turns,
                                                const GymFlowOut& O) {
  const bool term = over && played && !rs, trunc = turns >= (int64_t)max_turns && played && !rs;
  if (O.winner) O.winner[env] = (int8_t)(term ? winner : -1);
  O.turn_io[env] = turns;
  if (O.turn_out) O.turn_out[env] = turns;
  if (O.terminated) O.terminated[env] = (uint8_t)(term ? 1 : 0);
  if (O.truncated) O.truncated[env] = (uint8_t)(trunc ? 1 : 0);
  if (O.needs_reset) O.needs_reset[env] = (uint8_t)((term || trunc) ? 1 : 0);
}
// The single learner's reward, GeneralEnv.step's bookkeeping around it (:226-259) when `flow`, then the new stats.
// cur_tc / cur_ac: the learner's stats; tcl / acl: every player's.  Every lane calls it.
template <int MAXP>
__device__ __forceinline__ void gym_bookkeeping(int env, int pl, int P, uint32_t alive, bool over, int32_t cur_tc, int32_t cur_ac, uint32_t tcl,
                                                uint32_t acl, int32_t* prev, bool flow, bool rs, bool pl_ok, int64_t turns, int max_turns,
                                                const GymFlowOut& O) {
  const int winner = gym_winner(over, P, alive);
  if (lane_id() == 0) {
    const double r = gym_player_reward<MAXP>(pl, P, alive, over, winner, cur_tc, cur_ac, prev);
    if (flow) {
      if (O.reward) O.reward[env] = rs ? 0.0 : (pl_ok ? r : -0.1);   // :226-241 a refused action costs -0.1 and changes nothing
      gym_store_flags(env, over, pl_ok, rs, winner, turns, max_turns, O);
    } else {
      if (O.reward) O.reward[env] = r;
      if (O.winner) O.winner[env] = (int8_t)winner;
    }
    if (O.done) O.done[env] = (uint8_t)(over ? 1 : 0);
  }
  gym_store_stats<MAXP>(prev, tcl, acl, alive);
}

// The two step kernels' geometry K is a VariantGeom (ODD: see step_kernel).
// env's board into registers; stage / scratch: this wave's GYM_STAGE_DW and ACT_SCRATCH_DW dwords of LDS
template <typename K>
__device__ __forceinline__ ArmyRef gym_load_turn(Turn<K::MAXP, K::NSLOT>& b, const StepArgs& A, int env, int32_t* stage, uint32_t* scratch) {
  b.larmy = stage;
  b.lscr = scratch;
  const ArmyRef army_env = army_ref<K::NSLOT>(A.army16, A.army32, env);
  load_turn<true, lean_half_last(K::NSLOT, K::ODD)>(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * K::ROW_DW, army_env, K::FD, A.zeros);
  b.small = !(b.hflags & HF_WIDE) && !(A.flags & KF_BIGRATE);
  return army_env;
}
// The turn (step_kernel's body): an env that is over or `rs` is re-dealt; every other one plays the on-device agent's moves
// with the learners' lanes of the ActVec overwritten by learner_moves(av).  Then the state is stored.
template <typename K, typename F>
__device__ __forceinline__ void gym_play_turn(Turn<K::MAXP, K::NSLOT>& b, const StepArgs& A, int env, const ArmyRef& army_env, bool rs, F&& learner_moves) {
  constexpr int MAXP = K::MAXP, NSLOT = K::NSLOT, FD = K::FD, ROW_DW = K::ROW_DW;
  using B = Turn<MAXP, NSLOT>;
  uint32_t err = 0u;
  bool types_dirty = false;
  if ((b.hflags & HF_DONE) || rs) {
    redeal<MAXP, NSLOT>(b, A, env, FD, ROW_DW);
    types_dirty = true;
  } else {
    uint32_t m[B::NR][4];
    b.template legal_planes<false>(m);
    const uint32_t mine = agent_sample<MAXP, NSLOT>(b, m, env_key_of(A.seed_base, (uint32_t)env), A);
    typename B::ActVec av = agent_actvec<MAXP, NSLOT>(b, mine, A.invalid_permille > 0);
    learner_moves(av);
    bool aborted;
    err = b.turn_step(av, A, aborted);
    b.refresh_gt1();
    hdr_set(b, H_CNT_STEPS, hdr_get(b, H_CNT_STEPS) + 1u);
    if (aborted) hdr_set(b, H_CNT_ABORT, hdr_get(b, H_CNT_ABORT) + 1u);
    if (b.hflags & HF_DONE) hdr_set(b, H_CNT_DONE, hdr_get(b, H_CNT_DONE) + 1u);
  }
  store_army<true>(b, army_env);
  settle_lists(b);
  b.store_hdr(A.hdr + (size_t)env * HDR_DW, err);
  if (types_dirty) b.store_planes(A.rows + (size_t)env * ROW_DW, FD, ROW_DW, true);
  else b.store_planes_staged(A.rows + (size_t)env * ROW_DW, FD);
  if (A.err && lane_id() == 0) A.err[env] = (int32_t)err;
}

// gvec_gym_observe / gvec_gym_finish_step: A.player's observation, mask and reward of the state as it is, with
// GeneralsEnv.step's bookkeeping around them when asked for (A.played): a re-dealt env restarts its turn count, a refused
// action leaves it alone.
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gym_observe_kernel(GymArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  const GymView v = board_view<MAXP>(b, A.player);
  uint32_t own_any, cnt[MAXP];
  board_totals<MAXP>(b, own_any, cnt);
  const GymMask m = gym_mask(b, v);
  __shared__ uint32_t mask_stage[WAVES_PER_BLOCK][VariantGeom<MAXP, NSLOT, false>::GYM_STAGE_DW];
  const bool flow = A.played != nullptr;
  const bool rs = flow && A.resetting[env] != 0, pl_ok = !flow || A.played[env] != 0;
  const int64_t turns = flow ? (rs ? 0 : A.turn_count[env] + (pl_ok ? 1 : 0)) : A.turn_count[env];
  gym_emit_player<NSLOT>(b, v, m, own_any, gym_turn_channel(turns, A.max_turns), A.obs, A.mask, (size_t)env,
                         reinterpret_cast<uint8_t*>(mask_stage[block_wave()]), A.stride);
  const uint32_t tcl = pick<MAXP>(cnt, lane_id()), acl = army_counts<MAXP>(b);
  const GymFlowOut O{A.reward, A.done, A.winner, A.turn_io, A.turn_out, A.terminated, A.truncated, A.needs_reset};
  gym_bookkeeping<MAXP>(env, A.player, b.P, b.alive, (b.hflags & HF_DONE) != 0u, (int32_t)pick<MAXP>(cnt, A.player), (int32_t)rdlane(acl, A.player),
                        tcl, acl, A.prev_stats + (size_t)env * 3 * MAXP, flow, rs, pl_ok, turns, A.max_turns, O);
}

// GeneralsEnv.step for every env in ONE launch (gvec_gym_step) = gvec_agent_actions + gvec_gym_actions + gvec_step +
// gvec_gym_finish_step, which it equals bit for bit (tests/test_vector_env.py): the learner's action is decoded, the
// opponents' moves come from the on-device agent, the turn is played, and the observation / mask / reward / flags of the
// NEW state leave while the board is still in registers.  An env whose action was refused sits the call out.
// (Five waves per SIMD asked for by name: left alone the compiler takes 107-145 VGPRs - four waves, three for the largest
// boards; told to fit five it needs 81-96 and spills nothing except 24-28 bytes in <8,16>.  65,536 envs: 16x16 0.201 ->
// 0.184 ms, 20x20 4P 0.290 -> 0.260, 10x10 0.157 -> 0.140, 32x32 8P 0.586 -> 0.556, 15x15 and 25x25 unchanged; six waves
// (73-80 VGPRs) gain on boards of up to 256 tiles and lose 8-15 % on every larger one.)
template <int MAXP, int NSLOT, bool ODD>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5))) void gym_step_kernel(StepArgs A, GymStepArgs G) {
  using K = VariantGeom<MAXP, NSLOT, ODD>;
  using B = Turn<MAXP, NSLOT>;
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][K::GYM_STAGE_DW];
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  const ArmyRef army_env = gym_load_turn<K>(b, A, env, army_shadow[wave], act_scratch[wave]);
  const int pl = G.player;
  const long long a = (long long)uni64((uint64_t)G.gym_actions[env]);
  const bool rs = uni((int)G.resetting[env]) != 0;
  const GymMove mv = gym_decode(b, gym_sources(b, turn_view(b, pl)), a, G.stride);
  const bool played = mv.accepted || rs;
  if (lane == 0) {
    if (G.played) G.played[env] = (uint8_t)played;
    if (G.invalid) G.invalid[env] = (uint8_t)(!mv.valid && !rs);
    if (G.error) G.error[env] = (uint8_t)(mv.valid && !mv.accepted && !rs);
  }
  if (played) {
    gym_play_turn<K>(b, A, env, army_env, rs, [&](typename B::ActVec& av) {   // the learner's slot: the accepted move
      av.meta = (lane == pl) ? (16u | (mv.half ? 32u : 0u)) : av.meta;
      av.ft = (lane == pl) ? mv.from : av.ft;
      av.tt = (lane == pl) ? mv.tt : av.tt;
    });
  } else if (A.err && lane == 0) {
    A.err[env] = 0;
  }
  const GymView v = turn_view(b, pl);
  const uint32_t own_any = turn_own_any(b);
  const GymMask m = gym_mask(b, v);
  const int64_t turns = rs ? 0 : G.turn_io[env] + (played ? 1 : 0);
  const double tcn = gym_turn_channel(turns, G.max_turns);
  wave_lds_fence();  // the staged state stores above have read the stage
  gym_emit_player<NSLOT>(b, v, m, own_any, tcn, G.obs, G.mask, (size_t)env, reinterpret_cast<uint8_t*>(army_shadow[wave]), G.stride);
  const uint32_t tcl = turn_tile_counts(b), acl = army_counts<MAXP>(b);
  const GymFlowOut O{G.reward, nullptr, G.winner, G.turn_io, G.turn_out, G.terminated, G.truncated, G.needs_reset};
  gym_bookkeeping<MAXP>(env, pl, b.P, b.alive, (b.hflags & HF_DONE) != 0u, (int32_t)rdlane(tcl, pl), (int32_t)rdlane(acl, pl), tcl, acl,
                        G.prev_stats + (size_t)env * 3 * MAXP, true, rs, played, turns, G.max_turns, O);
}

// =========================================================================================
// self-play: every learner of a bit set in one launch (gvec_gym_observe_players / gvec_gym_step_players)
// =========================================================================================
// gvec_gym_observe_players: gym_observe_kernel's phases for every learner of the bit set `learners` (A.player unused):
// observation [B][L][9][stride], mask [B][L][stride*5], reward [B][L], done / winner [B], then every player's stats.
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void gym_observe_players_kernel(GymArgs A, uint32_t learners) {
  using B = Board<MAXP, NSLOT>;
  const int wave = block_wave(), lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  const int nl = __builtin_popcount(learners);
  uint32_t own_any, cnt[MAXP];
  board_totals<MAXP>(b, own_any, cnt);
  const uint32_t tcl = pick<MAXP>(cnt, lane), acl = army_counts<MAXP>(b);
  __shared__ uint32_t mask_stage[WAVES_PER_BLOCK][VariantGeom<MAXP, NSLOT, false>::GYM_STAGE_DW];
  const double tcn = gym_turn_channel(A.turn_count[env], A.max_turns);
  const bool over = (b.hflags & HF_DONE) != 0u;
  const int winner = gym_winner(over, b.P, b.alive);
  const int32_t* prev = A.prev_stats + (size_t)env * 3 * MAXP;
  int k = 0;
#pragma unroll 1
  for (int pl = 0; pl < MAXP; ++pl) {
    if (!((learners >> pl) & 1u)) continue;                  // wave-uniform
    const GymView v = board_view<MAXP>(b, pl);
    const GymMask m = gym_mask(b, v);
    const size_t slot = (size_t)env * nl + k;
    wave_lds_fence();  // the previous learner's mask copy has read the stage
    gym_emit_player<NSLOT>(b, v, m, own_any, tcn, A.obs, A.mask, slot, reinterpret_cast<uint8_t*>(mask_stage[wave]), A.stride);
    const int32_t cur_tc = (int32_t)rdlane(tcl, pl), cur_ac = (int32_t)rdlane(acl, pl);
    if (A.reward && lane == 0) A.reward[slot] = gym_player_reward<MAXP>(pl, b.P, b.alive, over, winner, cur_tc, cur_ac, prev);
    ++k;
  }
  if (lane == 0) {
    if (A.done) A.done[env] = (uint8_t)(over ? 1 : 0);
    if (A.winner) A.winner[env] = (int8_t)winner;
  }
  gym_store_stats<MAXP>(A.prev_stats + (size_t)env * 3 * MAXP, tcl, acl, b.alive);
}

// gvec_gym_step_players: gym_step_kernel's phases for every learner of a bit set at once.  Each learner's action is decoded
// against its own proto view; the players outside the set are the on-device agent.  A refused action puts NO move in the
// learner's lane and the env still plays its turn (with several learners one policy's mistake must not freeze the others):
// always a turn or a re-deal, never a skipped env.  The observation / mask / reward / alive of every learner leave while
// the board is in registers; every learner's reward is measured before the stats are rewritten (one gym_bookkeeping per
// learner would measure the second against the first's).
// With learners = 1 << p this equals gvec_agent_actions + gvec_gym_actions(p) + gvec_step + gvec_gym_finish_step(p) with
// the refusal rule above (tests/test_selfplay_env.py).
// (Waves per SIMD: see DESIGN.md §4.6, measured per register layout.)
template <int MAXP, int NSLOT, bool ODD>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) __attribute__((amdgpu_waves_per_eu(GYM_PLAYERS_WAVES_OF(NSLOT), GYM_PLAYERS_WAVES_OF(NSLOT))))
void gym_step_players_kernel(StepArgs A, GymPlayersArgs G) {
  using K = VariantGeom<MAXP, NSLOT, ODD>;
  using B = Turn<MAXP, NSLOT>;
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][K::GYM_STAGE_DW];
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  const ArmyRef army_env = gym_load_turn<K>(b, A, env, army_shadow[wave], act_scratch[wave]);
  const uint32_t learners = G.learners;
  const int nl = G.nl;
  const bool rs = uni((int)G.resetting[env]) != 0;
  const uint32_t alive0 = b.alive;
  const int P0 = b.P;
  // ---- every learner's action: lane pl ends up with learner pl's move; refused / invalid / error: bit pl, for learners
  // alive at the start of the step
  uint32_t l_meta = 0u;
  int l_ft = 0, l_tt = 0;
  uint32_t refused = 0u, invalid = 0u, error = 0u;
  {
    int k = 0;
#pragma unroll 1
    for (int pl = 0; pl < MAXP; ++pl) {
      if (!((learners >> pl) & 1u)) continue;                // wave-uniform
      const long long a = (long long)uni64((uint64_t)G.gym_actions[(size_t)env * nl + k]);
      ++k;
      const GymMove mv = gym_decode(b, gym_sources(b, turn_view(b, pl)), a, G.stride);
      l_meta = (lane == pl) ? (mv.accepted ? (16u | (mv.half ? 32u : 0u)) : 0u) : l_meta;
      l_ft = (lane == pl) ? mv.from : l_ft;
      l_tt = (lane == pl) ? mv.tt : l_tt;
      const bool counted = !rs && pl < P0 && ((alive0 >> pl) & 1u) != 0u;
      if (counted && !mv.accepted) refused |= 1u << pl;
      if (counted && !mv.valid) invalid |= 1u << pl;
      if (counted && mv.valid && !mv.accepted) error |= 1u << pl;
    }
  }
  gym_play_turn<K>(b, A, env, army_env, rs, [&](typename B::ActVec& av) {
    const bool is_learner = lane < MAXP && ((learners >> (lane & 31)) & 1u) != 0u;
    av.meta = is_learner ? l_meta : av.meta;
    av.ft = is_learner ? l_ft : av.ft;
    av.tt = is_learner ? l_tt : av.tt;
  });
  // ---- every learner's observation, mask, reward, alive; the env's flags
  const uint32_t own_any = turn_own_any(b);
  const uint32_t tcl = turn_tile_counts(b), acl = army_counts<MAXP>(b);
  const bool over = (b.hflags & HF_DONE) != 0u;
  const int winner = gym_winner(over, b.P, b.alive);
  const int64_t turns = rs ? 0 : G.turn_io[env] + 1;   // the turn counts as played whenever the env was not re-dealt
  const double tcn = gym_turn_channel(turns, G.max_turns);
  const int32_t* prev = G.prev_stats + (size_t)env * 3 * MAXP;
  {
    int k = 0;
#pragma unroll 1
    for (int pl = 0; pl < MAXP; ++pl) {
      if (!((learners >> pl) & 1u)) continue;                // wave-uniform
      const GymView v = turn_view(b, pl);
      const GymMask m = gym_mask(b, v);
      const size_t slot = (size_t)env * nl + k;
      wave_lds_fence();  // the staged state stores above / the previous learner's mask copy have read the stage
      gym_emit_player<NSLOT>(b, v, m, own_any, tcn, G.obs, G.mask, slot, reinterpret_cast<uint8_t*>(army_shadow[wave]), G.stride);
      const int32_t cur_tc = (int32_t)rdlane(tcl, pl), cur_ac = (int32_t)rdlane(acl, pl);
      if (lane == 0) {
        const bool ref = ((refused >> pl) & 1u) != 0u;
        if (G.reward) {
          const double r = gym_player_reward<MAXP>(pl, b.P, b.alive, over, winner, cur_tc, cur_ac, prev);
          G.reward[slot] = rs ? 0.0 : (ref ? r - 0.1 : r);    // a refused action costs -0.1 here too
        }
        if (G.invalid) G.invalid[slot] = (uint8_t)((invalid >> pl) & 1u);
        if (G.error) G.error[slot] = (uint8_t)((error >> pl) & 1u);
        if (G.alive) G.alive[slot] = (uint8_t)((b.alive >> pl) & 1u);
      }
      ++k;
    }
  }
  const GymFlowOut O{nullptr, nullptr, G.winner, G.turn_io, G.turn_out, G.terminated, G.truncated, G.needs_reset};
  if (lane == 0) gym_store_flags(env, over, true, rs, winner, turns, G.max_turns, O);
  gym_store_stats<MAXP>(G.prev_stats + (size_t)env * 3 * MAXP, tcl, acl, b.alive);
}

// GeneralsEnv.step's action handling for player `player` of every env (one thread per env):
// :226-241 an action the mask rejects is not submitted (the env sits the call out: GVEC_ACT_SKIP_ENV);
// _action_index_to_game_action :389-441 (a half move, index 4, takes the FIRST of up / right / down / left whose
// target is on the board - mountains are not checked there); the server then validates the move it received
// (action_validator.go:114-139): a half move whose first in-board direction is illegal is refused.
// `resetting` envs are re-dealt in this step (GVEC_ACT_RESET_ENV) whatever the action.
__global__ void gym_actions_kernel(GymActArgs A) {
  const int env = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (env >= A.num_envs) return;
  const uint32_t dims = A.hdr[(size_t)env * HDR_DW + H_DIMS];
  const int w = (int)(dims & 0xFFu), h = (int)((dims >> 8) & 0xFFu);  // unpack_dims' W and H, spelled out: through it this kernel is scheduled differently
  const long long a = A.gym_actions[env];
  const long long n5 = 5ll * A.stride;
  const uint8_t* mask = A.mask + (size_t)env * 5 * (size_t)A.stride;
  const bool in_range = a >= 0 && a < n5;
  const bool valid = in_range && mask[a] != 0;
  const int from = in_range ? (int)(a / 5) : 0, info = in_range ? (int)(a % 5) : 0;
  const int fx = from % w, fy = from / w;   // tile index with the env's own width (from < stride; a tile beyond the board has no mask bit)
  const bool half = info == 4;
  int d = half ? 3 : info;
  if (half) {
    if (fx - 1 >= 0) d = 3;
    if (fy + 1 < h) d = 2;
    if (fx + 1 < w) d = 1;
    if (fy - 1 >= 0) d = 0;
  }
  const bool accepted = valid && mask[(size_t)from * 5 + d] != 0;
  const bool resetting = A.resetting && A.resetting[env] != 0;
  const bool played = accepted || resetting;
  const int dx = (d == 1) - (d == 3), dy = (d == 2) - (d == 0);
  gvec_action* acts = A.actions + (size_t)env * A.pstride;
  gvec_action mine;
  mine.from_x = (int8_t)fx;
  mine.from_y = (int8_t)fy;
  mine.to_x = (int8_t)(fx + dx);
  mine.to_y = (int8_t)(fy + dy);
  mine.flags = (uint8_t)(played ? (GVEC_ACT_VALID | (half ? GVEC_ACT_HALF : 0u)) : 0u);
  mine.reserved[0] = mine.reserved[1] = mine.reserved[2] = 0;
  acts[A.player] = mine;
  uint8_t f0 = acts[0].flags & (uint8_t)~(GVEC_ACT_SKIP_ENV | GVEC_ACT_RESET_ENV);
  if (!played) f0 |= GVEC_ACT_SKIP_ENV;
  if (resetting) f0 |= GVEC_ACT_RESET_ENV;
  acts[0].flags = f0;
  if (A.played) A.played[env] = (uint8_t)played;
  if (A.invalid) A.invalid[env] = (uint8_t)(!valid && !resetting);
  if (A.error) A.error[env] = (uint8_t)(valid && !accepted && !resetting);
}

// =========================================================================================
// host-side launchers
// =========================================================================================
hipError_t launch_setup(const Variant& v, const ImportArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(setup_kernel<P, S>, a.n, s, a); });
}
hipError_t launch_gym_observe(const Variant& v, const GymArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(gym_observe_kernel<P, S>, a.num_envs, s, a); });
}
hipError_t launch_gym_observe_players(const Variant& v, const GymArgs& a, uint32_t learners, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(gym_observe_players_kernel<P, S>, a.num_envs, s, a, learners); });
}
hipError_t launch_gym_step(const Variant& v, const StepArgs& in, const GymStepArgs& g, hipStream_t s) {
  const StepArgs a = with_seed_bases(in);
  return dispatch(v, [&](auto P, auto S) {
    const int odd = plane_parity<P, S>(a);
    if (odd < 0) return hipErrorInvalidValue;
    if (odd) return launch_waves(gym_step_kernel<P, S, true>, a.num_envs, s, a, g);
    return launch_waves(gym_step_kernel<P, S, false>, a.num_envs, s, a, g);
  });
}
hipError_t launch_gym_step_players(const Variant& v, const StepArgs& in, const GymPlayersArgs& g, hipStream_t s) {
  const StepArgs a = with_seed_bases(in);
  return dispatch(v, [&](auto P, auto S) {
    const int odd = plane_parity<P, S>(a);
    if (odd < 0) return hipErrorInvalidValue;
    if (odd) return launch_waves(gym_step_players_kernel<P, S, true>, a.num_envs, s, a, g);
    return launch_waves(gym_step_players_kernel<P, S, false>, a.num_envs, s, a, g);
  });
}
hipError_t launch_gym_actions(const GymActArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gym_actions_kernel, dim3((unsigned)((a.num_envs + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace gvec
