// gvec_features.hip — strategic feature planes as a pure function of the 9-plane observation: four capped shortest-path
// distances (own general, shown enemy, cities to take, nearest fog) and the front line (gvec_obs_features in generals_vec.h;
// DESIGN.md §4.13).
//
// One wavefront per observation, four per workgroup, no barrier between them (each wave owns its slice of LDS).
//   load     lane = tile (t = 64 s + lane): the five planes that are read, one compare and one ballot per predicate; the ballot
//            words are the predicate's H*W-bit string, staged in LDS.
//   re-layout lane y of either half-wave picks board row y of a predicate up as a W-bit word: two dwords at bit y*W and a
//            funnel shift.  GVEC_MAX_DIM = 32 is what makes a row one dword.
//   BFS      one level is f<<1 | f>>1 | row_above(f) | row_below(f), masked with the passable tiles not reached yet; the row
//            moves are DPP shifts by one lane.  The row mask keeps column W-1 from reaching column 0 of the next row.  Each lane
//            carries two searches, the two half-waves four.  Distances stay bit-sliced: slice i of a row collects the tiles
//            whose level has bit i set.  Levels run to cap - 1 (a tile first reached at level cap saturates to 1.0 like an
//            unreached one) or to the fixpoint, a wave-wide any.
//   store    reached words and slices go to LDS; lane = tile reads its row's words back, rebuilds d and stores min(d, cap) / cap.
#include "gvec_launch.hpp"
#include "gvec_waves.hpp"

namespace gvec {

namespace {

constexpr int FEAT_SLICES = 10;                  // levels 1 .. cap - 1 <= 1023
constexpr int FEAT_PRED_DW = 34;                 // 1,024 bits, and the dword after the last row's (read, then masked off)
enum { PRED_PASS, PRED_MINE, PRED_SRC0, PRED_SRC1, PRED_SRC2, PRED_SRC3, PRED_COUNT };   // SRC1 = enemy
constexpr int FEAT_OFF_REACHED = PRED_COUNT * FEAT_PRED_DW;            // [4][32]
constexpr int FEAT_OFF_SLICE = FEAT_OFF_REACHED + 4 * 32;              // [4][FEAT_SLICES][32]
constexpr int FEAT_OFF_FRONT = FEAT_OFF_SLICE + 4 * FEAT_SLICES * 32;  // [32]
constexpr int FEAT_WAVE_DW = FEAT_OFF_FRONT + 32;

// the rows above and below, inside one half-wave: row 0 has nothing above it, row 31 nothing below
__device__ __forceinline__ uint32_t dilate(uint32_t f, uint32_t has_above, uint32_t has_below) {
  const uint32_t above = from_prev(f), below = from_next(f);
  return (f << 1) | (f >> 1) | (above & has_above) | (below & has_below);
}

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void obs_features_kernel(gvec_obs_features_args P, int cap_log2) {
  __shared__ uint32_t feat_lds[WAVES_PER_BLOCK * FEAT_WAVE_DW];
  const int lane = lane_id();
  const long long r = wave_item64();
  if (r >= P.rows) return;                       // the whole wave leaves: everything below is wave-uniform control flow
  const int W = P.width, H = P.height, HW = W * H, slots = (HW + 63) >> 6;
  uint32_t* L = feat_lds + block_wave() * FEAT_WAVE_DW;
  const float* __restrict__ o = P.obs + (size_t)r * (size_t)P.obs_row_stride;

  // ---- load: predicates per tile, one ballot each ----
  for (int s = 0; s < slots; ++s) {
    const int t = 64 * s + lane;
    const bool in = t < HW;
    const float v0 = in ? o[t] : 0.0f, v1 = in ? o[HW + t] : 0.0f, v4 = in ? o[4 * HW + t] : 0.0f;
    const float v5 = in ? o[5 * HW + t] : 0.0f, v6 = in ? o[6 * HW + t] : 0.0f;
    const bool mine = v1 == 0.5f, pass = in && !(v4 != 0.0f);
    unsigned long long b[PRED_COUNT];
    b[PRED_PASS] = __builtin_amdgcn_ballot_w64(pass);
    b[PRED_MINE] = __builtin_amdgcn_ballot_w64(mine);
    b[PRED_SRC0] = __builtin_amdgcn_ballot_w64(v6 != 0.0f && mine);
    b[PRED_SRC1] = __builtin_amdgcn_ballot_w64(v1 == 1.0f);
    b[PRED_SRC2] = __builtin_amdgcn_ballot_w64(v5 != 0.0f && !mine);
    b[PRED_SRC3] = __builtin_amdgcn_ballot_w64(in && !(v0 != 0.0f));
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < PRED_COUNT; ++k) {
        L[k * FEAT_PRED_DW + 2 * s] = (uint32_t)b[k];
        L[k * FEAT_PRED_DW + 2 * s + 1] = (uint32_t)(b[k] >> 32);
      }
    }
  }
  wave_lds_fence();

  // ---- re-layout: lane y of each half-wave holds row y ----
  const int y = lane & 31, half = lane >> 5;
  const uint32_t row_mask = y < H ? (W == 32 ? 0xFFFFFFFFu : (1u << W) - 1u) : 0u;
  const uint32_t has_above = y > 0 ? 0xFFFFFFFFu : 0u, has_below = y < 31 ? 0xFFFFFFFFu : 0u;
  const int bit0 = y * W;
  auto row_of = [&](int pred) {
    const uint32_t* p = L + pred * FEAT_PRED_DW + (bit0 >> 5);
    const unsigned long long two = ((unsigned long long)p[1] << 32) | p[0];
    return (uint32_t)(two >> (bit0 & 31)) & row_mask;
  };
  const uint32_t pass = row_of(PRED_PASS), mine = row_of(PRED_MINE), enemy = row_of(PRED_SRC1);
  // the half-waves' searches: planes 0 and 1 in lanes 0-31, planes 2 and 3 in lanes 32-63
  uint32_t fa = row_of(PRED_SRC0 + 2 * half) & pass, fb = row_of(PRED_SRC1 + 2 * half) & pass;
  uint32_t open_a = pass & ~fa, open_b = pass & ~fb;                  // passable and not reached yet
  uint32_t sa[FEAT_SLICES], sb[FEAT_SLICES];
#pragma unroll
  for (int i = 0; i < FEAT_SLICES; ++i) sa[i] = sb[i] = 0u;

  // ---- the level loop ----
  const int cap = 1 << cap_log2;
  for (int level = 1; level < cap; ++level) {
    const uint32_t na = dilate(fa, has_above, has_below) & open_a;
    const uint32_t nb = dilate(fb, has_above, has_below) & open_b;
    if (!wave_any((na | nb) != 0u)) break;
    open_a &= ~na;
    open_b &= ~nb;
#pragma unroll
    for (int i = 0; i < FEAT_SLICES; ++i) {
      const uint32_t m = 0u - (((uint32_t)level >> i) & 1u);           // wave-uniform
      sa[i] |= na & m;
      sb[i] |= nb & m;
    }
    fa = na;
    fb = nb;
  }

  // ---- front line: mine, and a 4-neighbour is enemy ----
  const uint32_t front = mine & dilate(enemy, has_above, has_below);   // mine carries the row mask

  const int pa = 2 * half, pb = 2 * half + 1;
  L[FEAT_OFF_REACHED + pa * 32 + y] = pass & ~open_a;
  L[FEAT_OFF_REACHED + pb * 32 + y] = pass & ~open_b;
#pragma unroll
  for (int i = 0; i < FEAT_SLICES; ++i) {
    L[FEAT_OFF_SLICE + (pa * FEAT_SLICES + i) * 32 + y] = sa[i];
    L[FEAT_OFF_SLICE + (pb * FEAT_SLICES + i) * 32 + y] = sb[i];
  }
  if (half == 0) L[FEAT_OFF_FRONT + y] = front;
  wave_lds_fence();

  // ---- store: lane = tile again ----
  float* __restrict__ out = P.out + (size_t)r * 5u * (size_t)HW;
  const float inv = __builtin_ldexpf(1.0f, -cap_log2);
  const int step_y = 64 / W, step_x = 64 % W;
  int ty = lane / W, tx = lane % W;
  for (int s = 0; s < slots; ++s) {
    const int t = 64 * s + lane;
    if (t < HW) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        uint32_t d = 0u;
        for (int i = 0; i < cap_log2; ++i) d |= ((L[FEAT_OFF_SLICE + (p * FEAT_SLICES + i) * 32 + ty] >> tx) & 1u) << i;
        const bool reached = (L[FEAT_OFF_REACHED + p * 32 + ty] >> tx) & 1u;
        out[p * HW + t] = reached ? (float)d * inv : 1.0f;
      }
      out[4 * HW + t] = ((L[FEAT_OFF_FRONT + ty] >> tx) & 1u) ? 1.0f : 0.0f;
    }
    tx += step_x;
    ty += step_y;
    if (tx >= W) {
      tx -= W;
      ty += 1;
    }
  }
}

}  // namespace

hipError_t launch_obs_features(const gvec_obs_features_args& a, hipStream_t s) {
  int cap_log2 = 0;
  while ((1 << cap_log2) < a.cap) ++cap_log2;
  return launch_waves(obs_features_kernel, a.rows, s, a, cap_log2);
}

}  // namespace gvec
