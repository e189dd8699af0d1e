// gvec_turn.hpp — device code every unit that plays or loads a turn shares: the random agent, the board loads and the
// auto-reset re-deal.  All of it is forced inline; the kernels are in gvec_kernels.hip, gvec_gym.hip and their siblings.
#pragma once
#include "gvec_launch.hpp"
#include "gvec_packed.hpp"

namespace gvec {

// All turn logic runs on PBoard (players packed into register rows, gvec_packed.hpp); Board is the plain
// layout of the conversion / experience kernels.
template <int MAXP, int NSLOT>
using Turn = PBoard<MAXP, NSLOT>;

// =========================================================================================
// random agent (DESIGN.md "Synthetic inputs"; mirrored by the oracle's agent_env)
// =========================================================================================
// Every alive player draws two hashes h1 = amix(key + turn*c1 + player*c2 + c3), h2 = amix(h1 ^ c4):
//   no action            if (h1 & 0xFFFF) < agent_noop
//   half move            if (h1 >> 16) < agent_half
//   unchecked move       if invalid_permille > 0 and ((h2 & 0xFFFF) * 1000 >> 16) < invalid_permille:
//                        tile ((h2 >> 16) * N) >> 16, direction (h1 >> 8) & 3  (H5 stress)
//   else the kk-th legal move, kk = ((h2 >> 16) * count) >> 16, of Engine.GetLegalActionMask(player) in the
//   order (t >> 5, d, t & 31): 32-tile blocks ascending, inside a block direction plane by direction plane
//   (up, right, down, left), inside a plane tiles ascending.  No legal move: no action.
// All players of a register are sampled at once: lane (row r, column c) counts the legal moves of player
// r in tile block c, one row-wise prefix scan finds each row's lane, that lane finds its bit.
// Returns, in lane p, player p's draw: t | d << 10 | act << 12 | half << 13.
template <int MAXP, int NSLOT>
__device__ __forceinline__ uint32_t agent_sample(const Turn<MAXP, NSLOT>& b, const uint32_t (&m)[Turn<MAXP, NSLOT>::NR][4], uint32_t ek,
                                                 const StepArgs& A) {
  using T = Turn<MAXP, NSLOT>;
  constexpr int NR = T::NR, PPR = T::PPR, ROWL = T::ROWL;
  const int lane = lane_id();
  const uint32_t sbase = ek + (uint32_t)b.turn * 0x9E3779B1u + 0x165667B1u;  // wave-uniform
  uint32_t mine = 0u;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const uint32_t player = (uint32_t)T::lane_player(k);
    const uint32_t h1 = amix(mad24(player, 0x4A7C15u, sbase));
    const uint32_t h2 = amix(h1 ^ 0x68E31DA4u);
    const uint32_t hi16 = h2 >> 16;
    const bool act = b.lane_flag(b.alive, k) && !((h1 & 0xFFFFu) < A.agent_noop);  // alive implies player < P
    const bool half = (h1 >> 16) < A.agent_half;
    const bool inv = A.invalid_permille > 0 && (__umul24(h2 & 0xFFFFu, 1000u) >> 16) < (uint32_t)A.invalid_permille;
    const uint32_t c0 = (uint32_t)__builtin_popcount(m[k][0]), c1 = c0 + (uint32_t)__builtin_popcount(m[k][1]);
    const uint32_t c2 = c1 + (uint32_t)__builtin_popcount(m[k][2]), cnt = c2 + (uint32_t)__builtin_popcount(m[k][3]);
    const uint32_t sc = row_scan_add<ROWL>(cnt);
    const uint32_t total = row_last<ROWL>(sc);     // this row's number of legal moves (< 4096)
    const uint32_t kk = __umul24(hi16, total) >> 16;
    const uint32_t below = sc - cnt;
    const bool sel = kk >= below && kk < sc;       // exactly one lane of a row with total > 0
    const uint32_t r = kk - below;
    const uint32_t d = (r >= c0 ? 1u : 0u) + (r >= c1 ? 1u : 0u) + (r >= c2 ? 1u : 0u);
    const uint32_t base = (d == 0u) ? 0u : (d == 1u) ? c0 : (d == 2u) ? c1 : c2;
    const uint32_t w = (d == 0u) ? m[k][0] : (d == 1u) ? m[k][1] : (d == 2u) ? m[k][2] : m[k][3];
    const uint32_t t_sel = 32u * (uint32_t)T::col() + kth_set_bit(w, r - base);
    const uint32_t pick = row_scan_or<ROWL>(sel ? (t_sel | (d << 10) | 0x8000u) : 0u);  // complete at the row's last lane
    const uint32_t unchecked = (__umul24(hi16, (uint32_t)b.N) >> 16) | (((h1 >> 8) & 3u) << 10) | 0x8000u;
    const uint32_t fin = inv ? unchecked : pick;
    const bool go = act && (fin & 0x8000u) != 0u;
    const uint32_t out = (fin & 0xFFFu) | (go ? 0x1000u : 0u) | (half ? 0x2000u : 0u);
    const uint32_t got = row_result<ROWL>(out, lane % PPR);  // lane p <- the last lane of row p % PPR of register p / PPR
    mine = (lane / PPR == k) ? got : mine;
  }
  return mine;
}

// the draw as gvec_action words (gvec_agent_actions, actions_out)
template <int MAXP, int NSLOT>
__device__ __forceinline__ void agent_words(const Turn<MAXP, NSLOT>& b, uint32_t mine, uint32_t& alo, uint32_t& ahi) {
  const bool act = lane_id() < MAXP && (mine & 0x1000u) != 0u;
  const int t = (int)(mine & 0x3FFu), d = (int)((mine >> 10) & 3u);
  const int y = (int)(__umul24((uint32_t)t, (uint32_t)b.recipW) >> 16), x = t - (int)__umul24((uint32_t)y, (uint32_t)b.W);  // t < 1024
  const int dx = (d == 1) - (d == 3), dy = (d == 2) - (d == 0);
  const uint32_t lo = ((uint32_t)x & 0xFFu) | (((uint32_t)y & 0xFFu) << 8) | (((uint32_t)(x + dx) & 0xFFu) << 16) |
                      (((uint32_t)(y + dy) & 0xFFu) << 24);
  alo = act ? lo : 0u;
  ahi = act ? (GVEC_ACT_VALID | ((mine & 0x2000u) ? GVEC_ACT_HALF : 0u)) : 0u;
}

// the draw as the turn's ActVec, skipping the coordinate round trip through gvec_action: what
// PBoard::prevalidate would derive from agent_words' output.  A legal move needs no static check (its
// target is on the board by construction of the mask); an unchecked one (invalid_permille) can only leave
// the board (core/action.go:58-64) - same tile and adjacency hold for every (tile, direction) pair.
template <int MAXP, int NSLOT>
__device__ __forceinline__ typename Turn<MAXP, NSLOT>::ActVec agent_actvec(const Turn<MAXP, NSLOT>& b, uint32_t mine, bool may_be_unchecked) {
  typename Turn<MAXP, NSLOT>::ActVec v;
  const bool act = lane_id() < MAXP && (mine & 0x1000u) != 0u;
  const int t = (int)(mine & 0x3FFu), d = (int)((mine >> 10) & 3u);
  uint32_t code = 0u;
  if (may_be_unchecked) {  // wave-uniform
    const int y = (int)(__umul24((uint32_t)t, (uint32_t)b.recipW) >> 16), x = t - (int)__umul24((uint32_t)y, (uint32_t)b.W);
    const bool off = (d == 0) ? (y == 0) : (d == 1) ? (x == b.W - 1) : (d == 2) ? (y == b.H - 1) : (x == 0);
    code = off ? GVEC_ERR_INVALID_COORDINATES : 0u;
  }
  v.meta = act ? (code | 16u | ((mine & 0x2000u) ? 32u : 0u)) : 0u;
  v.ft = t;
  v.tt = t + ((d == 0) ? -b.W : (d == 1) ? 1 : (d == 2) ? b.W : -1);
  return v;
}

// =========================================================================================
// step / rollout kernel: `turns` engine turns per launch for one board per wavefront
// =========================================================================================
template <typename BT>
__device__ __forceinline__ void load_board(BT& b, const uint32_t* hdr, const uint32_t* rows, const ArmyCRef& army, int fd) {
  b.load_hdr(hdr);
  load_army(b, army);
  b.load_planes(rows, fd);
}
// EARLY (the per-turn step kernel): every load of the board goes out before the header is decoded - one memory round
// trip per board instead of two, worth 10 % there (one-process A/B: 338.7 -> 305.6 us per 262,144 boards).  The fused
// rollout amortises its loads over many turns and runs 4 % faster with the plain order (fewer live registers).
// HALF_LAST (EARLY only): the board has at most 32*(2*NSLOT-1) tiles - see army_load_narrow.
template <bool EARLY = false, bool HALF_LAST = false, typename BT>
__device__ __forceinline__ void load_turn(BT& b, const uint32_t* hdr, const uint32_t* rows, const ArmyCRef& army, int fd, const uint32_t* zeros) {
  if constexpr (EARLY) {
    b.issue_hdr(hdr);
    b.load_planes(rows, fd, zeros);
    b.template load_army_narrow<HALF_LAST>(army);
    b.decode_hdr_scalar(hdr);   // SMEM: in flight with the vector loads above
    b.land();
    b.land_scalars();
    b.spread_shared();
    b.load_lists(rows, fd);
    b.load_army_wide_if_flagged(army);
  } else {
    b.load_hdr(hdr);
    load_army(b, army);
    b.template load_planes<false>(rows, fd, zeros);
  }
}

// vector-env auto-reset: this step re-deals the env from the board pool (no Go analogue)
template <int MAXP, int NSLOT, typename BT>
__device__ __forceinline__ void redeal(BT& b, const StepArgs& A, int env, int fd, int row_dw) {
  const uint32_t episode = hdr_get(b, H_EPISODE) + 1u;
  const uint32_t cs = hdr_get(b, H_CNT_STEPS), ca = hdr_get(b, H_CNT_ABORT), cd = hdr_get(b, H_CNT_DONE);
  const uint32_t hk = fmix32(env_key_of(A.pool_seed_base, (uint32_t)env) ^ (episode * 0x9E3779B1u));
  const int j = (int)__umulhi(hk, (uint32_t)A.pool_size);
  load_turn(b, A.pool_hdr + (size_t)j * HDR_DW, A.pool_rows + (size_t)j * row_dw, army_cref<NSLOT>(A.pool_army16, A.pool_army32, j), fd, A.zeros);
  hdr_set(b, H_EPISODE, episode);
  hdr_set(b, H_CNT_STEPS, cs);
  hdr_set(b, H_CNT_ABORT, ca);
  hdr_set(b, H_CNT_DONE, cd);
}

}  // namespace gvec
