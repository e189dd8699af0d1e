// gvec_kernels.hip — the engine's HIP kernels for gfx950 (MI355X): the turn (step, fused rollout), the queries of the resident
// state and the scripted opponent.  One wavefront per board; see gvec_device.hpp for the register layout
// and the reference citations.  The other subsystems are units of their own (DESIGN.md "Translation units").
#include "gvec_bot.hpp"
#include "gvec_dispatch.hpp"
#include "gvec_turn.hpp"

namespace gvec {

// ONE engine turn per launch, straight-line (gvec_step; per-turn rollouts).  AGENT: actions are
// sampled on device from the legal-move planes of the resident state.  (waves_for_regs: gvec_turn.hpp)
// Waves per SIMD asked of the register allocator: the board state a variant holds (planes, army
// slots, mask planes) plus ~32 working registers.  <4,7> fits 64 registers = 8 waves/SIMD without a
// spill, which is worth 7 % over 7 waves (one-process A/B): the turn is a long dependent chain of
// short cross-lane operations, and the VALU only stays fed with every wave slot occupied.
template <int MAXP, int NSLOT>
constexpr int step_waves() {
  const int state = Turn<MAXP, NSLOT>::STATE_REGS;
  return waves_for_regs(state + (state + 32 <= 62 ? 32 : 40));  // 8 waves only where they fit with room to spare
}

// The ORDINARY turn of the per-turn kernel (GVEC_ORDTURN, gvec_device.hpp), from the header's landing on: step_kernel found
// PBoard::ordinary_turn<ORD>() true and no forced re-deal.  The env is live and plays: no re-deal, no frozen env, no second
// fetch for lists or wide armies, the turn's guards on the loaded state folded (turn_step<ORD>), the mutable planes alone
// to store and the masks always stale.  What the turn itself brings about - an abort, an elimination, a finished game, an
// army beyond u16 - is tested here as in the general code below, whose statements these are.
template <int ORD, int MAXP, int NSLOT, bool AGENT, bool ODD>
__device__ __forceinline__ void step_ordinary(Turn<MAXP, NSLOT>& b, const StepArgs& A, int env, const uint32_t* rows_in, const ArmyRef& army_env) {
  constexpr int FD = VariantGeom<MAXP, NSLOT, ODD>::FD, ROW_DW = VariantGeom<MAXP, NSLOT, ODD>::ROW_DW;
  using B = Turn<MAXP, NSLOT>;
  const int lane = lane_id();
  load_turn_tail<ORD>(b, rows_in, army_env, FD);
  b.small = true;
  uint32_t m[B::NR][4];
  typename B::ActVec av;
  if constexpr (AGENT) {
    b.template legal_planes<false>(m);
    const uint32_t mine = agent_sample<MAXP, NSLOT>(b, m, env_key_of(A.seed_base, (uint32_t)env), A);
    av = agent_actvec<MAXP, NSLOT>(b, mine, A.invalid_permille > 0);
    if (A.actions_out) {
      uint32_t alo, ahi;
      agent_words<MAXP, NSLOT>(b, mine, alo, ahi);
      if (lane < A.pstride) reinterpret_cast<uint2*>(A.actions_out)[(size_t)env * A.pstride + lane] = make_uint2(alo, ahi);
    }
  } else {
    uint32_t alo = 0u, ahi = 0u;
    if (lane < A.pstride) {
      const uint2 w = reinterpret_cast<const uint2*>(A.actions)[(size_t)env * A.pstride + lane];
      alo = w.x;
      ahi = w.y;
    }
    av = b.prevalidate(alo, ahi);
  }
  bool aborted;
  const uint32_t err = b.template turn_step<ORD>(av, A, aborted);
  b.refresh_gt1();
  hdr_set(b, H_CNT_STEPS, hdr_get(b, H_CNT_STEPS) + 1u);
  if (aborted) hdr_set(b, H_CNT_ABORT, hdr_get(b, H_CNT_ABORT) + 1u);
  if (b.hflags & HF_DONE) hdr_set(b, H_CNT_DONE, hdr_get(b, H_CNT_DONE) + 1u);
  store_army<true>(b, army_env);
  settle_lists(b);
  b.store_hdr(A.hdr + (size_t)env * HDR_DW, err);
  b.template store_planes_staged<ORD>(A.rows + (size_t)env * ROW_DW, FD);
  if (A.err && lane == 0) A.err[env] = (int32_t)err;
  if (A.flags & KF_EMIT) {
    b.template legal_planes<false>(m);
    b.store_masks_staged(m, A.legal + (size_t)env * A.pstride * A.mask_dw, FD, A.pstride);
  }
}

// ODD: the planes are 2*NSLOT-1 dwords long (else 2*NSLOT): the plane stride is a compile-time
// constant here, so every plane access is one instruction with an immediate offset.
template <int MAXP, int NSLOT, bool AGENT, bool ODD>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, (step_waves<MAXP, NSLOT>())) void step_kernel(StepArgs A) {
  constexpr int FD = VariantGeom<MAXP, NSLOT, ODD>::FD, ROW_DW = VariantGeom<MAXP, NSLOT, ODD>::ROW_DW;
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][NSLOT * 64];  // per wave: the action phase's army copy
  using B = Turn<MAXP, NSLOT>;
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  bool force_redeal = false;
  if constexpr (!AGENT) {
    // GVEC_ACT_SKIP_ENV on player 0's action: this env sits the call out (nothing is read or
    // written; the host keeps the legal-mask buffer current for such calls)
    const uint32_t f0 = (uint32_t)uni((int)reinterpret_cast<const uint32_t*>(A.actions)[((size_t)env * A.pstride) * 2 + 1]);
    if (f0 & GVEC_ACT_SKIP_ENV) {
      if (A.err && lane == 0) A.err[env] = 0;
      return;
    }
    force_redeal = (f0 & GVEC_ACT_RESET_ENV) != 0u;  // the caller ends this episode (truncation): re-deal now
  }
  B b;
  b.larmy = army_shadow[wave];
  b.lscr = act_scratch[wave];
  const ArmyRef army_env = army_ref<NSLOT>(A.army16, A.army32, env);
  // GVEC_ORDTURN: ONE wave-uniform branch, taken as soon as the header words are there, sends the ordinary turn down its own
  // instantiation; everything below is the general code (profiling builds count phases of that code alone)
  // (GVEC_QUIET rides in ORD: the planes the ordinary turn's store leaves in memory because the turn did not change them)
  constexpr int ORD = (GVEC_PROFILE_SKIP | GVEC_PROFILE_DUP) != 0 ? 0 : (ordturn_bits(MAXP, NSLOT, AGENT, ODD) | quiet_bits(MAXP, NSLOT, AGENT, ODD));
  if constexpr (ORD != 0) {
    const uint32_t* rows_env = A.rows + (size_t)env * ROW_DW;
    load_turn_issue<lean_half_last(NSLOT, ODD)>(b, A.hdr + (size_t)env * HDR_DW, rows_env, army_env, FD, A.zeros);
    if (!force_redeal && b.template ordinary_turn<ORD>(A)) {
      step_ordinary<ORD, MAXP, NSLOT, AGENT, ODD>(b, A, env, rows_env, army_env);
      return;
    }
    load_turn_tail<0>(b, rows_env, army_env, FD);
  } else {
    load_turn<true, lean_half_last(NSLOT, ODD)>(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * ROW_DW, army_env, FD, A.zeros);
  }
  // one turn from armies <= 65535 at a rate below KF_BIGRATE's: every army of the turn stays below 2^24 (update_stats' mad24)
  b.small = !(b.hflags & HF_WIDE) && !(A.flags & KF_BIGRATE);
  const bool emit = (A.flags & KF_EMIT) != 0u;
  uint32_t m[B::NR][4];
  uint32_t err = 0u;
  bool types_dirty = false, changed = true;
  const bool can_redeal = (A.flags & KF_AUTORESET) && A.pool_size > 0;
  if (AGENT && A.actions_out && (b.hflags & HF_DONE)) {
    // a re-dealt or frozen env plays no move in this launch: its recorded actions are "none", not whatever an
    // earlier recorded step left in the buffer (gvec_experience_records builds acted bits from these words)
    if (lane < A.pstride) reinterpret_cast<uint2*>(A.actions_out)[(size_t)env * A.pstride + lane] = make_uint2(0u, 0u);
  }
  if (can_redeal && ((b.hflags & HF_DONE) || force_redeal)) {
    redeal<MAXP, NSLOT>(b, A, env, FD, ROW_DW);  // the pool board brings its own gt1 plane
    types_dirty = true;
  } else if (b.hflags & HF_DONE) {
    err = GVEC_ERR_GAME_OVER;  // turn_processor.go:95-113: the engine stays frozen
    changed = false;
  } else {
    typename B::ActVec av;
    if constexpr (AGENT) {
      // the agent's input: the legal-move planes of the resident state, rebuilt from the stored gt1 plane
      // (7 vector instructions; re-reading the 832-byte masks the previous launch wrote would cost more)
      b.template legal_planes<false>(m);
      uint32_t mine = (GVEC_PROFILE_SKIP & 1) ? 0u : agent_sample<MAXP, NSLOT>(b, m, env_key_of(A.seed_base, (uint32_t)env), A);
      if (GVEC_PROFILE_DUP & 64) { b.opaque(); b.template legal_planes<false>(m); }
      if (GVEC_PROFILE_DUP & 1) {
        b.opaque();
#pragma unroll
        for (int d = 0; d < 4; ++d) asm volatile("" : "+v"(m[0][d]));
        const uint32_t again = agent_sample<MAXP, NSLOT>(b, m, env_key_of(A.seed_base, (uint32_t)env), A);
        asm volatile("" : : "v"(again));
      }
      av = agent_actvec<MAXP, NSLOT>(b, mine, A.invalid_permille > 0);
      if (A.actions_out) {
        uint32_t alo, ahi;
        agent_words<MAXP, NSLOT>(b, mine, alo, ahi);
        if (lane < A.pstride) reinterpret_cast<uint2*>(A.actions_out)[(size_t)env * A.pstride + lane] = make_uint2(alo, ahi);
      }
    } else {
      uint32_t alo = 0u, ahi = 0u;
      if (lane < A.pstride) {
        const uint2 w = reinterpret_cast<const uint2*>(A.actions)[(size_t)env * A.pstride + lane];
        alo = w.x;
        ahi = w.y;
      }
      av = b.prevalidate(alo, ahi);
    }
    bool aborted;
    err = b.turn_step(av, A, aborted);
    if (!(GVEC_PROFILE_SKIP & 32)) b.refresh_gt1();
    if (GVEC_PROFILE_DUP & 32) { b.opaque_v(); b.refresh_gt1(); }
    hdr_set(b, H_CNT_STEPS, hdr_get(b, H_CNT_STEPS) + 1u);
    if (aborted) hdr_set(b, H_CNT_ABORT, hdr_get(b, H_CNT_ABORT) + 1u);
    if (b.hflags & HF_DONE) hdr_set(b, H_CNT_DONE, hdr_get(b, H_CNT_DONE) + 1u);
  }
  store_army<true>(b, army_env);  // picks the narrow / wide form: before the header, which records it
  settle_lists(b);                // ... and so is whether the list planes are stored
  b.store_hdr(A.hdr + (size_t)env * HDR_DW, err);
  if (types_dirty) b.store_planes(A.rows + (size_t)env * ROW_DW, FD, ROW_DW, true);
  else b.store_planes_staged(A.rows + (size_t)env * ROW_DW, FD);
  if (A.err && lane == 0) A.err[env] = (int32_t)err;
  if (!(GVEC_PROFILE_SKIP & 64) && emit && (changed || !(A.flags & KF_LMVALID))) {
    b.template legal_planes<false>(m);
    b.store_masks_staged(m, A.legal + (size_t)env * A.pstride * A.mask_dw, FD, A.pstride);
  }
}

// `turns` engine turns per launch with the board kept in registers / LDS (fused rollouts; always
// with the on-device agent)
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, (rollout_waves<MAXP, NSLOT>())) void rollout_kernel(StepArgs A) {
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][NSLOT * 64];
  using B = Turn<MAXP, NSLOT>;
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  b.larmy = army_shadow[wave];
  b.lscr = act_scratch[wave];
  const ArmyRef army_env = army_ref<NSLOT>(A.army16, A.army32, env);
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_env, A.fd, A.zeros);
  uint32_t m[B::NR][4];
  uint32_t err = 0u, n_steps = 0u, n_abort = 0u, n_done = 0u;
  const uint32_t ek = env_key_of(A.seed_base, (uint32_t)env);
  const bool can_redeal = (A.flags & KF_AUTORESET) && A.pool_size > 0;
  int k = 0;
  // The hot inner loop plays turns while the game is live; the rare events (game over: re-deal from
  // the pool, or freeze) sit in the outer loop so they do not shape the inner loop's registers.
  for (;;) {
    b.template legal_planes<false>(m);  // the planes of the CURRENT state: the agent's input, the output at the end
    while (k < A.turns && !(b.hflags & HF_DONE)) {
      const uint32_t mine = agent_sample<MAXP, NSLOT>(b, m, ek, A);
      bool aborted;
      err = b.turn_step(agent_actvec<MAXP, NSLOT>(b, mine, A.invalid_permille > 0), A, aborted);
      n_steps += 1u;
      n_abort += aborted ? 1u : 0u;
      n_done += (b.hflags & HF_DONE) ? 1u : 0u;
      ++k;
      b.refresh_gt1();
      b.template legal_planes<false>(m);
    }
    if (k >= A.turns) break;
    if (!can_redeal) {
      err = GVEC_ERR_GAME_OVER;  // frozen for the rest of the launch
      break;
    }
    redeal<MAXP, NSLOT>(b, A, env, A.fd, A.row_dw);  // this turn slot is spent re-dealing (vector-env auto-reset)
    err = 0u;
    ++k;
  }
  hdr_set(b, H_CNT_STEPS, hdr_get(b, H_CNT_STEPS) + n_steps);
  hdr_set(b, H_CNT_ABORT, hdr_get(b, H_CNT_ABORT) + n_abort);
  hdr_set(b, H_CNT_DONE, hdr_get(b, H_CNT_DONE) + n_done);
  store_army(b, army_env);
  settle_lists(b);
  b.store_hdr(A.hdr + (size_t)env * HDR_DW, err);
  b.store_planes(A.rows + (size_t)env * A.row_dw, A.fd, A.row_dw, true);
  if (A.err && lane == 0) A.err[env] = (int32_t)err;
  b.store_masks_staged(m, A.legal + (size_t)env * A.pstride * A.mask_dw, A.fd, A.pstride);
}

// legal masks / agent actions of the resident state (no turn is played)
// MODE 0: Engine.GetLegalActionMask   1: random-agent actions   2: Serializer.GenerateActionMask
template <int MAXP, int NSLOT, int MODE>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void query_kernel(StepArgs A) {
  using B = Turn<MAXP, NSLOT>;
  const int lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  b.larmy = nullptr;
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd, A.zeros);
  uint32_t m[B::NR][4];
  if constexpr (MODE == 2) b.template legal_planes<true>(m);
  else b.template legal_planes<false>(m);
  if constexpr (MODE == 1) {
    uint32_t alo = 0u, ahi = 0u;
    if (!(b.hflags & HF_DONE)) agent_words<MAXP, NSLOT>(b, agent_sample<MAXP, NSLOT>(b, m, env_key_of(A.seed_base, (uint32_t)env), A), alo, ahi);
    if (lane < A.pstride) reinterpret_cast<uint2*>(A.actions_out)[(size_t)env * A.pstride + lane] = make_uint2(alo, ahi);
  } else {
    b.store_masks(m, A.legal + (size_t)env * A.pstride * A.mask_dw, A.fd, A.pstride);
  }
}

// =========================================================================================
// scripted opponent (gvec_bot_actions; the rule itself: gvec_bot.hpp, DESIGN.md §6 "Scripted opponent")
// =========================================================================================
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void bot_kernel(StepArgs A, BotArgs G) {
  using B = Turn<MAXP, NSLOT>;
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][NSLOT * 64];
  const int wave = block_wave(), lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  b.larmy = &army_shadow[wave][0];
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd, A.zeros);
  uint32_t m[B::NR][4];
  b.template legal_planes<false>(m);
  const bool done = (b.hflags & HF_DONE) != 0u;
  const uint32_t ek = env_key_of(A.seed_base, (uint32_t)env);

  // slots that play the random agent's move instead (lane p = player p); the draw comes first: bot_sample overwrites m
  uint32_t agent_mine = 0u, rnd_bits = 0u;
  if (G.random_permille > 0) {
    agent_mine = agent_sample<MAXP, NSLOT>(b, m, ek, A);
    rnd_bits = bot_random_seats<MAXP>(ek, (uint32_t)b.turn, G.random_permille);
  }
  // the players the rule moves (alive implies player < P)
  const uint32_t movers = done ? 0u : (G.players & b.alive & ~rnd_bits);
  const uint32_t bot_mine = bot_sample<MAXP, NSLOT>(b, m, movers);
  const bool rnd = (rnd_bits >> lane) & 1u;
  uint32_t alo = 0u, ahi = 0u;
  if (!done) agent_words<MAXP, NSLOT>(b, rnd ? agent_mine : bot_mine, alo, ahi);
  if (lane < A.pstride && lane < MAXP && ((G.players >> lane) & 1u))
    reinterpret_cast<uint2*>(A.actions_out)[(size_t)env * A.pstride + lane] = make_uint2(alo, ahi);
}

// =========================================================================================
__global__ void counter_sum_kernel(const uint32_t* hdr, int32_t num_envs, unsigned long long* out) {
  unsigned long long s0 = 0, s1 = 0, s2 = 0;
  for (int e = (int)(blockIdx.x * blockDim.x + threadIdx.x); e < num_envs; e += (int)(gridDim.x * blockDim.x)) {
    const uint32_t* h = hdr + (size_t)e * HDR_DW;
    s0 += h[H_CNT_STEPS];
    s1 += h[H_CNT_ABORT];
    s2 += h[H_CNT_DONE];
  }
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_down(s0, off);
    s1 += __shfl_down(s1, off);
    s2 += __shfl_down(s2, off);
  }
  if ((threadIdx.x & 63u) == 0u) {
    atomicAdd(out + 0, s0);
    atomicAdd(out + 1, s1);
    atomicAdd(out + 2, s2);
  }
}

// device self-test of the wave primitives the engine relies on (run by tests / smoke)
__global__ void selftest_kernel(int32_t* out) {
  const int lane = lane_id();
  int fail = 0;
  const uint32_t v = (uint32_t)(lane * 3 + 1);
  if (from_prev(v) != (lane == 0 ? 0u : (uint32_t)((lane - 1) * 3 + 1))) fail = 1;
  if (from_next(v) != (lane == 63 ? 0u : (uint32_t)((lane + 1) * 3 + 1))) fail = fail ? fail : 2;
  uint32_t expect = 0u;
  for (int l = 0; l <= lane; ++l) expect += (uint32_t)(l * 3 + 1);
  if (wave_scan_add(v) != expect) fail = fail ? fail : 3;
  if (wave_sum(v) != (uint32_t)(63 * 64 / 2 * 3 + 64)) fail = fail ? fail : 4;
  if (bperm(4 * ((lane * 7) & 63), v) != (uint32_t)(((lane * 7) & 63) * 3 + 1)) fail = fail ? fail : 5;
  {  // per-lane k-th set bit: lane l asks for bit number l % popcount
    const uint32_t w = 0x80000105u ^ ((uint32_t)lane * 0x9E3779B1u);
    const uint32_t r = (uint32_t)lane % (uint32_t)__builtin_popcount(w);
    uint32_t want = 0u, seen = 0u;
    for (uint32_t i = 0; i < 32u; ++i)
      if ((w >> i) & 1u) {
        if (seen == r) want = i;
        ++seen;
      }
    if (kth_set_bit(w, r) != want) fail = fail ? fail : 7;
  }
  {  // row-wise scans and the row-last broadcast, 16- and 32-lane rows
    uint32_t e16 = 0u, e32 = 0u, o16 = 0u, o32 = 0u;
    for (int l = lane & ~15; l <= lane; ++l) e16 += (uint32_t)(l * 3 + 1), o16 |= 1u << (l & 31);
    for (int l = lane & ~31; l <= lane; ++l) e32 += (uint32_t)(l * 3 + 1), o32 |= 1u << (l & 31);
    if (row_scan_add<16>(v) != e16 || row_scan_add<32>(v) != e32) fail = fail ? fail : 8;
    if (row_scan_or<16>(1u << (lane & 31)) != o16 || row_scan_or<32>(1u << (lane & 31)) != o32) fail = fail ? fail : 9;
    if (row_last<16>(v) != (uint32_t)((lane | 15) * 3 + 1) || row_last<32>(v) != (uint32_t)((lane | 31) * 3 + 1)) fail = fail ? fail : 10;
  }
  {  // the packed layout's row idioms, 16- and 32-lane rows (6: the failure code nothing used)
    int32_t m16 = -1, m32 = -1;
    const int32_t x = (int32_t)((lane * 37) & 63) - 1;  // a permutation of -1 .. 62
    for (int l = lane & ~15; l <= lane; ++l) m16 = max(m16, (int32_t)((l * 37) & 63) - 1);
    for (int l = lane & ~31; l <= lane; ++l) m32 = max(m32, (int32_t)((l * 37) & 63) - 1);
    if (row_scan_max<16>(x) != m16 || row_scan_max<32>(x) != m32) fail = fail ? fail : 6;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(((lane * 5) & 7) < 3);  // lanes 0, 2, 5 of every 8
    if (row_slice<16>(bal, lane >> 4) != 0x2525u || row_slice<32>(bal, lane >> 5) != 0x25252525u) fail = fail ? fail : 13;
    // player p's row: row p % 4 of 16 lanes, p % 2 of 32
    if (player_lane<16>(lane, 3) != (lane & 3) * 16 + 3 || player_lane<32>(lane, 3) != (lane & 1) * 32 + 3 || player_row<16>(lane) != (lane & 3) * 16 ||
        player_row<32>(lane) != (lane & 1) * 32) fail = fail ? fail : 14;
    if (row_result<16>(v, lane & 3) != (uint32_t)(((lane & 3) * 16 + 15) * 3 + 1) ||
        row_result<32>(v, lane & 1) != (uint32_t)(((lane & 1) * 32 + 31) * 3 + 1)) fail = fail ? fail : 15;
  }
  if ((uint32_t)gvec_llvm_writelane(777, 5, (int)v) != (lane == 5 ? 777u : v)) fail = fail ? fail : 11;
  if (mad24(v, 3u, 5u) != v * 3u + 5u) fail = fail ? fail : 12;
  {  // the fixed-pattern moves between rows (GVEC_XLANE): the LDS and the vector-ALU spelling of each, both held to plain
     // arithmetic on data that differs in every lane (and so in every row).  Every cross-lane result lands in a local first:
     // the comparisons below diverge, the moves above them must not.
    auto val = [](int l) { return ((uint32_t)l * 0x9E3779B1u) ^ 0x80000105u; };
    const uint32_t w = val(lane);
    for (int r = 0; r < 4; ++r) {  // 16: row r of 16 lanes to every row
      const uint32_t a = row_to_all_lds<16>(w, r), c = row_to_all_valu<16>(w, r), e = val(16 * r + (lane & 15));
      if (a != e || c != e) fail = fail ? fail : 16;
    }
    for (int r = 0; r < 2; ++r) {  // 17: row r of 32 lanes to every row
      const uint32_t a = row_to_all_lds<32>(w, r), c = row_to_all_valu<32>(w, r), e = val(32 * r + (lane & 31));
      if (a != e || c != e) fail = fail ? fail : 17;
    }
    {  // 18, 19: the lane ^ 16 and lane ^ 32 partners under OR and under addition
      const LanePair a = with_partner_lds<16>(w), c = with_partner_valu<16>(w);
      const uint32_t o = val(lane ^ 16);
      if ((a.a | a.b) != (w | o) || (c.a | c.b) != (w | o) || a.a + a.b != w + o || c.a + c.b != w + o) fail = fail ? fail : 18;
      const LanePair a2 = with_partner_lds<32>(w), c2 = with_partner_valu<32>(w);
      const uint32_t o2 = val(lane ^ 32);
      if ((a2.a | a2.b) != (w | o2) || (c2.a | c2.b) != (w | o2) || a2.a + a2.b != w + o2 || c2.a + c2.b != w + o2) fail = fail ? fail : 19;
    }
    {  // 20: or_rows, four rows of 16 and two of 32
      const uint32_t a = PBoard<4, 7>::or_rows<false>(w), c = PBoard<4, 7>::or_rows<true>(w);
      const uint32_t a2 = PBoard<4, 16>::or_rows<false>(w), c2 = PBoard<4, 16>::or_rows<true>(w);
      const int c16 = lane & 15, c32 = lane & 31;
      const uint32_t e = val(c16) | val(c16 + 16) | val(c16 + 32) | val(c16 + 48), e2 = val(c32) | val(c32 + 32);
      if (a != e || c != e || a2 != e2 || c2 != e2) fail = fail ? fail : 20;
    }
    {  // 21: a row's last lane to the row
      const uint32_t a = row_last_lds<16>(w), c = row_last_valu<16>(w), a2 = row_last_lds<32>(w), c2 = row_last_valu<32>(w);
      if (a != val(lane | 15) || c != val(lane | 15) || a2 != val(lane | 31) || c2 != val(lane | 31)) fail = fail ? fail : 21;
    }
    // 22, 23: dwords 2s, 2s+1 of the row at row_base as the 64 tiles' lane mask (they differ: every lane's value does), for
    // every slot a row of 16 (7 slots) or 32 lanes (16 slots) can hold
    for (int rows = 4; rows >= 2; rows -= 2) {
      const int rowl = 64 / rows, slots = rows == 4 ? 7 : 16;
      for (int rb = 0; rb < 64; rb += rowl) {
        for (int s = 0; s < slots; ++s) {
          const uint32_t g0 = gather(w, s, rb), g1 = gather_valu(w, s, rb);
          const int32_t m0 = gather_mask(w, s, rb), m1 = gather_mask_valu(w, s, rb);
          const uint32_t e = (val(rb + 2 * s + (lane >> 5)) >> (lane & 31)) & 1u;
          if (g0 != e || g1 != e || m0 != -(int32_t)e || m1 != -(int32_t)e) fail = fail ? fail : (rows == 4 ? 22 : 23);
        }
      }
    }
  }
  // lane * 64 + code (callers only test for 0)
  const unsigned long long any = __builtin_amdgcn_ballot_w64(fail != 0);
  if (lane == 0) out[0] = any ? (int32_t)(__builtin_ctzll(any) * 64 + rdlane((uint32_t)fail, (int)__builtin_ctzll(any))) : 0;
}

// =========================================================================================
// host-side dispatch
// =========================================================================================
bool pick_variant(int max_players, int tile_stride, Variant* out) {
  static const int kP[] = {2, 4, 8};
  static const int kS[] = {1, 2, 4, 7, 10, 16};
  int need = (tile_stride + 63) / 64;
  out->maxp = 0;
  out->nslot = 0;
  for (int p : kP)
    if (max_players <= p) {
      out->maxp = p;
      break;
    }
  for (int s : kS)
    if (need <= s) {
      out->nslot = s;
      break;
    }
  return out->maxp && out->nslot;
}

hipError_t launch_step(const Variant& v, const StepArgs& in, hipStream_t s) {
  const StepArgs a = with_seed_bases(in);
  return dispatch(v, [&](auto P, auto S) {
    const int odd = plane_parity<P, S>(a);
    if (odd < 0) return hipErrorInvalidValue;
    const bool agent = (a.flags & KF_AGENT) != 0u;
    if (agent && odd) return launch_waves(step_kernel<P, S, true, true>, a.num_envs, s, a);
    if (agent) return launch_waves(step_kernel<P, S, true, false>, a.num_envs, s, a);
    if (odd) return launch_waves(step_kernel<P, S, false, true>, a.num_envs, s, a);
    return launch_waves(step_kernel<P, S, false, false>, a.num_envs, s, a);
  });
}
hipError_t launch_rollout(const Variant& v, const StepArgs& in, hipStream_t s) {
  const StepArgs a = with_seed_bases(in);
  return dispatch(v, [&](auto P, auto S) { return launch_waves(rollout_kernel<P, S>, a.num_envs, s, a); });
}
hipError_t launch_agent(const Variant& v, const StepArgs& in, hipStream_t s) {
  const StepArgs a = with_seed_bases(in);
  return dispatch(v, [&](auto P, auto S) { return launch_waves(query_kernel<P, S, 1>, a.num_envs, s, a); });
}
hipError_t launch_bot(const Variant& v, const StepArgs& in, const BotArgs& g, hipStream_t s) {
  const StepArgs a = with_seed_bases(in);
  return dispatch(v, [&](auto P, auto S) { return launch_waves(bot_kernel<P, S>, a.num_envs, s, a, g); });
}
hipError_t launch_legal(const Variant& v, const StepArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(query_kernel<P, S, 0>, a.num_envs, s, a); });
}
hipError_t launch_serializer_mask(const Variant& v, const StepArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(query_kernel<P, S, 2>, a.num_envs, s, a); });
}
hipError_t launch_counter_sum(const uint32_t* hdr, int32_t num_envs, unsigned long long* out, hipStream_t s) {
  int blocks = (num_envs + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(counter_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, s, hdr, num_envs, out);
  return hipGetLastError();
}
hipError_t launch_selftest(int32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(64), 0, s, out);
  return hipGetLastError();
}

}  // namespace gvec
