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
// The EARLY order in its two halves: everything up to the point where the header words have landed (where the per-turn
// kernel decides what kind of turn this is, PBoard::ordinary_turn), and the tail that depends on the header's flags -
// ORD: of an ordinary turn, which has neither list planes nor wide armies to fetch.
template <bool HALF_LAST, typename BT>
__device__ __forceinline__ void load_turn_issue(BT& b, const uint32_t* hdr, const uint32_t* rows, const ArmyCRef& army, int fd, const uint32_t* zeros) {
  b.issue_hdr(hdr);
  b.load_planes(rows, fd, zeros);
  b.template load_army_narrow<HALF_LAST>(army);
  b.decode_hdr_scalar(hdr);   // SMEM: in flight with the vector loads above
  b.land();
  b.land_scalars();
}
template <int ORD, typename BT>
__device__ __forceinline__ void load_turn_tail(BT& b, const uint32_t* rows, const ArmyCRef& army, int fd) {
  b.spread_shared();
  b.template load_lists<ORD>(rows, fd);
  b.template load_army_wide_if_flagged<ORD>(army);
}
template <bool EARLY = false, bool HALF_LAST = false, typename BT>
__device__ __forceinline__ void load_turn(BT& b, const uint32_t* hdr, const uint32_t* rows, const ArmyCRef& army, int fd, const uint32_t* zeros) {
  if constexpr (EARLY) {  // load_turn_issue + load_turn_tail<0>, statement for statement
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

// =========================================================================================
// register budgets of the kernels that keep a board for many turns (rollout_kernel, search_kernel)
// =========================================================================================
constexpr int waves_for_regs(int need) {  // the waves per SIMD that leave every wave `need` registers (allocated in eights)
  const int alloc = (need + 7) / 8 * 8;
  const int w = 512 / alloc;
  return w > 8 ? 8 : (w < 2 ? 2 : w);
}
// Waves per SIMD to ask of the register allocator for the fused rollout kernel.  With no HBM traffic
// inside the turn loop the kernel is latency / issue bound, and occupancy pays even at the price of
// a few scratch spills; a spill inside the turn loop of the big variants costs far more than a wave.
template <int MAXP, int NSLOT>
constexpr int rollout_waves() {
  return waves_for_regs(Turn<MAXP, NSLOT>::STATE_REGS + (NSLOT >= 16 ? 100 : NSLOT >= 10 ? 68 : 44));
}

// =========================================================================================
// one player's view of a board in the Turn layout, and a gym action decoded against it (the gym step kernels of
// gvec_gym.hip, where the reference's rules are cited phase by phase, and the playout search of gvec_search.hip)
// =========================================================================================
// What the proto shows one player: `own` its tiles, `seen` the tiles it sees (ComputePlayerVisibility,
// visibility_optimized.go:166-195: everything when the fog is off), as replicated flat planes.
struct GymView {
  uint32_t own, seen;
};
// Turn layout: player pl's plane, replicated into every row, is row pl % PPR of register pl / PPR.  pl is wave-uniform (a
// kernel argument or the counter of a loop every lane runs); every lane calls it.
template <typename B>
__device__ __forceinline__ uint32_t player_view(int pl, const uint32_t (&reg)[B::NR]) {
  uint32_t out = 0u;
#pragma unroll
  for (int k = 0; k < B::NR; ++k) {
    const uint32_t g = bperm(player_lane<B::ROWL>(pl, B::col()) << 2, reg[k]);
    out = (pl / B::PPR == k) ? g : out;
  }
  return out;
}
template <typename B>
__device__ __forceinline__ GymView turn_view(const B& b, int pl) {
  const uint32_t own_p = player_view<B>(pl, b.own);
  return GymView{own_p, (b.hflags & HF_FOG) ? player_view<B>(pl, b.vis) : b.valid};
}
// _get_valid_actions_mask's source tiles: a tile the proto shows as ours (visible, owner == player) with army > 1
template <typename BT>
__device__ __forceinline__ uint32_t gym_sources(const BT& b, const GymView& v) {
  return v.own & v.seen & b.gt1;
}

// Every player's stats, player p's in lane p < MAXP.  tile_counts: len(OwnedTiles) of the Turn layout, row totals in the
// rows' last lanes, handed to lane p.  army_counts: lanes H_ARMYCNT + p of the header register hold ArmyCount[p], fetched
// by every lane (a cross-lane read must not sit under a divergent branch: masked-off source lanes read as 0).
template <typename B>
__device__ __forceinline__ uint32_t turn_tile_counts(const B& b) {
  const int lane = lane_id();
  uint32_t tcl = 0u;
#pragma unroll
  for (int k = 0; k < B::NR; ++k) {
    const uint32_t sc = row_scan_add<B::ROWL>((uint32_t)__builtin_popcount(b.lst[k]));
    const uint32_t got = row_result<B::ROWL>(sc, lane % B::PPR);
    tcl = (lane / B::PPR == k) ? got : tcl;
  }
  return tcl;
}
template <int MAXP, typename BT>
__device__ __forceinline__ uint32_t army_counts(const BT& b) {
  return bperm((H_ARMYCNT + (lane_id() & (MAXP - 1))) << 2, b.hv);
}

__device__ __forceinline__ int gym_winner(bool over, int P, uint32_t alive) {   // Engine.GetWinner
  return (over && P > 1 && __builtin_popcount(alive) == 1) ? (31 - __builtin_clz(alive)) : -1;
}

// GeneralsEnv.step's action handling (generals_env.py:226-259, :389-441; gym_actions_kernel does the same from mask bytes):
// Discrete(N*5) action `a` of the player whose source tiles are `src`, decoded against the valid-action mask of the
// resident state (recomputed from the planes in registers - the bytes gym_observe wrote are not read back).
//   valid:    the mask has the action's bit (:226-241)
//   accepted: the move it turns into is legal too.  A half move, index 4, takes the FIRST of up / right / down / left whose
//             target is on the board (mountains are not checked there, :389-441), and the server validates the move it
//             received (action_validator.go:114-139)
//   from, d, tt: source tile, direction, target tile (on the board and legal by construction of the mask when accepted)
// a and src are wave-uniform in value; every lane calls it (the rdlanes sit outside every lane-dependent condition).
struct GymMove {
  bool valid, accepted, half;
  int from, d, tt;
};
template <typename B>
__device__ __forceinline__ GymMove gym_decode(const B& b, uint32_t src, long long a, int stride) {
  GymMove mv;
  const long long n5 = 5ll * stride;
  const bool in_range = a >= 0 && a < n5;
  mv.from = in_range ? (int)(a / 5) : 0;
  const int from = mv.from, info = in_range ? (int)(a % 5) : 0;
  const int fy = (int)(__umul24((uint32_t)from, (uint32_t)b.recipW) >> 16), fx = from - (int)__umul24((uint32_t)fy, (uint32_t)b.W);  // from < 1024
  mv.half = info == 4;
  int d = mv.half ? 3 : info;
  if (mv.half) {
    if (fx - 1 >= 0) d = 3;
    if (fy + 1 < b.H) d = 2;
    if (fx + 1 < b.W) d = 1;
    if (fy - 1 >= 0) d = 0;
  }
  mv.d = d;
  // a tile index beyond the env's own board has no mask bit: the planes are zero there
  const uint32_t wsrc = rdlane(src, from >> 5);
  const uint32_t o0 = rdlane(b.ok[0], from >> 5), o1 = rdlane(b.ok[1], from >> 5), o2 = rdlane(b.ok[2], from >> 5), o3 = rdlane(b.ok[3], from >> 5);
  const uint32_t bit = 1u << (from & 31);
  const bool s_ok = (wsrc & bit) != 0u;
  const bool k0 = s_ok && (o0 & bit), k1 = s_ok && (o1 & bit), k2 = s_ok && (o2 & bit), k3 = s_ok && (o3 & bit);
  const bool kinfo = (info == 0) ? k0 : (info == 1) ? k1 : (info == 2) ? k2 : (info == 3) ? k3 : (k0 || k1 || k2 || k3);
  mv.valid = in_range && kinfo;
  const bool kd = (d == 0) ? k0 : (d == 1) ? k1 : (d == 2) ? k2 : k3;
  mv.accepted = mv.valid && kd;
  mv.tt = from + ((d == 0) ? -b.W : (d == 1) ? 1 : (d == 2) ? b.W : -1);
  return mv;
}

}  // namespace gvec
