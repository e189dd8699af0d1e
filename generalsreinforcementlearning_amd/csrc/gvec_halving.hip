// gvec_halving.hip — what a sequential-halving search does between two playout launches, and its policy target
// (gvec_search_halve, gvec_search_improved_policy in generals_vec.h).
//
// One wavefront per row (wave_item), four per workgroup, no LDS and no barrier.
//   halve   lane = column of the round.  The lane scores its column's playouts in float64, replica by replica, onto the running
//           sum and count of the slot the column stands for; the row's largest count is one butterfly; the ranking is a loop
//           over the columns in which every lane reads column j's (live, key, slot) with v_readlane and counts the columns
//           that come before its own.  No atomics, no sort network: the rank IS the output position.
//   policy  lane = action i mod 64: the masked logits of a row live in NJ registers per lane (element 64 j + lane in register
//           j), read from HBM once.  The candidates sit one per lane; their completed scores reach the registers that hold
//           their actions through v_readlane and a compile-time register index.
// Every cross-lane read runs with all 64 lanes active: the lanes beyond k, m or A carry neutral values (count 0, not live,
// -inf) instead of sitting out.  Every reduction is a fixed xor butterfly (gvec_device.hpp): the same input gives the same bits.
#include <math.h>

#include "gvec_launch.hpp"
#include "gvec_playout_score.hpp"
#include "gvec_waves.hpp"

namespace gvec {

namespace {

__device__ __forceinline__ double rdlane_f64(double v, int lane) {
  const uint32_t hi = rdlane((uint32_t)__double2hiint(v), lane), lo = rdlane((uint32_t)__double2loint(v), lane);
  return __hiloint2double((int)hi, (int)lo);
}
// wave_max of gvec_device.hpp for counts: every lane ends with the same value
__device__ __forceinline__ int wave_max_count(int x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(x, off, 64);
    x = o > x ? o : x;
  }
  return x;
}

// ---- gvec_search_halve ----
// the score of a playout: playout_score of gvec_playout_score.hpp
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void search_halve_kernel(gvec_search_halve_args P) {
  const int r = wave_item();
  if (r >= P.n) return;                          // the whole wave leaves: everything below is wave-uniform control flow
  const int lane = lane_id(), m = P.m, k = P.k, R = P.replicas, k_next = P.k_next;
  const size_t row_m = (size_t)r * (size_t)m;
  int s = lane;
  if (P.slot && lane < k) s = P.slot[(size_t)r * (size_t)k + (size_t)lane];
  const bool on = lane < k && s >= 0 && s < m;   // a slot outside the row is never an address
  const int before = lane < m ? P.count[row_m + lane] : 0;   // every slot's count, the untouched ones included
  double sum = 0.0, prior = 0.0;
  int cnt = 0;
  long long cand = GVEC_SEARCH_NONE;
  if (on) {
    sum = P.sum[row_m + s];
    cnt = P.count[row_m + s];
    cand = P.candidates0[row_m + s];
    prior = P.prior_key[row_m + s];
    const int32_t* __restrict__ t = P.terms + ((size_t)r * (size_t)k + (size_t)lane) * (size_t)R * GVEC_SEARCH_TERMS;
    for (int j = 0; j < R; ++j, t += GVEC_SEARCH_TERMS) {
      if (t[0] != 0) {
        sum = sum + playout_score(P, t);
        cnt += 1;
      }
    }
  }
  const int nmax = wave_max_count(cnt > before ? cnt : before);   // counts only grow: the old ones and the new ones together
  const bool live = on && cnt > 0 && cand != GVEC_SEARCH_NONE;
  double key = 0.0;
  if (cnt > 0) {
    const double mean = sum / (double)cnt;
    key = prior + ((P.c_visit + (double)nmax) * P.c_scale) * ((mean - P.q_lo) * P.q_inv_range);
  }
  // rank = the columns that come before this one: live before not, the larger key, the lower slot
  const uint32_t flags = (on ? 2u : 0u) | (live ? 1u : 0u);
  int rank = 0;
  for (int j = 0; j < k; ++j) {
    const uint32_t fj = rdlane(flags, j);
    const int sj = (int)rdlane((uint32_t)s, j);
    const double kj = rdlane_f64(key, j);
    const bool live_j = (fj & 1u) != 0u;
    bool first = sj < s;
    if (live && live_j) first = kj > key || (kj == key && sj < s);
    if (live != live_j) first = live_j;
    rank += ((fj & 2u) != 0u && first) ? 1 : 0;
  }
  if (on) {
    P.sum[row_m + s] = sum;
    P.count[row_m + s] = cnt;
    if (rank < k_next) {
      P.next_slot[(size_t)r * (size_t)k_next + (size_t)rank] = s;
      P.next_candidates[(size_t)r * (size_t)k_next + (size_t)rank] = cand;
    }
  }
}

// ---- gvec_search_improved_policy ----
// NJ registers per lane hold a row of up to 64 * NJ actions
template <int NJ>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void search_policy_kernel(gvec_search_policy_args P) {
  const int r = wave_item();
  if (r >= P.n) return;
  const int lane = lane_id(), A = P.num_actions, m = P.m;
  const size_t row = (size_t)r * (size_t)A, row_m = (size_t)r * (size_t)m;
  const uint8_t* __restrict__ legal = P.mask + row;
  const float* __restrict__ logit = P.logits ? P.logits + row : nullptr;
  float* __restrict__ out = P.target + row;
  // the masked logits x_i = legal_i ? l_i : -inf, the legal entries' logits and no other
  float y[NJ];
  float top = NEG_INF;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = 64 * j + lane;
    float v = NEG_INF;
    if (i < A && legal[i] != 0) v = logit ? logit[i] : 0.0f;
    y[j] = v;
    top = v > top ? v : top;
  }
  const float value = P.value ? P.value[r] : 0.0f;
  if (!wave_any(top > NEG_INF)) {                // no legal action: zeros (wave-uniform: a ballot)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int i = 64 * j + lane;
      if (i < A) out[i] = 0.0f;
    }
    if (lane == 0) P.v_mix[r] = value;
    return;
  }
  // lane = slot: its candidate, and whether it is in V
  long long a = GVEC_SEARCH_NONE;
  int cnt = 0;
  double sum = 0.0;
  if (lane < m) {
    a = P.candidates0[row_m + lane];
    cnt = P.count[row_m + lane];
    sum = P.sum[row_m + lane];
  }
  const int nmax = wave_max_count(cnt);
  const bool in_row = cnt > 0 && a >= 0 && a < (long long)A;   // the action is an index only under this test
  const int ai = in_row ? (int)a : 0;
  float xa = NEG_INF;
  if (in_row && legal[ai] != 0) xa = logit ? logit[ai] : 0.0f;
  const bool visited = xa > NEG_INF;
  const float q = visited ? (float)(sum / (double)cnt) : 0.0f;
  // vq = sum_V pi q / sum_V pi: the prior's normaliser cancels, so the weights are exp(x_a - max_V x)
  const float vtop = wave_max(xa);
  const float w = visited ? expf(xa - vtop) : 0.0f;
  const float den = wave_sum(w), num = wave_sum(w * q);
  const uint32_t visits = wave_sum(visited ? (uint32_t)cnt : 0u);   // N; wave-uniform
  const float scale = (float)((P.c_visit + (double)nmax) * P.c_scale), lo = (float)P.q_lo, inv = (float)P.q_inv_range;
  float vmix = value, shift = 0.0f;              // V empty: v_mix = value and the target is the prior itself
  if (visits != 0u) {
    const float vq = num / den, nv = (float)visits;
    vmix = P.value ? (value + nv * vq) / (1.0f + nv) : vq;
    shift = scale * ((vmix - lo) * inv);
  }
  // completed scores: x_i + sigma(v_mix) everywhere, then x_a + sigma(q(a)) on V
#pragma unroll
  for (int j = 0; j < NJ; ++j) y[j] = y[j] + shift;
  const float ya = xa + scale * ((q - lo) * inv);
  const uint32_t where = visited ? (uint32_t)ai : 0xFFFFFFFFu;
  for (int l = 0; l < m; ++l) {
    const uint32_t al = rdlane(where, l);
    const float yl = rdlane(ya, l);
    if (al != 0xFFFFFFFFu) {                     // scalar: the register index is wave-uniform, the lane is a select
      const int jl = (int)(al >> 6);
      const bool mine = (int)(al & 63u) == lane;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (j == jl) y[j] = mine ? yl : y[j];
    }
  }
  // softmax over S
  float big = NEG_INF;
#pragma unroll
  for (int j = 0; j < NJ; ++j) big = y[j] > big ? y[j] : big;
  big = wave_max(big);
  float z = 0.0f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    y[j] = y[j] > NEG_INF ? expf(y[j] - big) : 0.0f;
    z = z + y[j];
  }
  z = wave_sum(z);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = 64 * j + lane;
    if (i < A) out[i] = y[j] / z;
  }
  if (lane == 0) P.v_mix[r] = vmix;
}

}  // namespace

hipError_t launch_search_halve(const gvec_search_halve_args& a, hipStream_t s) { return launch_waves(search_halve_kernel, a.n, s, a); }

hipError_t launch_search_improved_policy(const gvec_search_policy_args& a, hipStream_t s) {
  static_assert(64 * 80 == SEARCH_POLICY_MAX_ACTIONS, "the widest instantiation holds the largest board's row");
  const int A = a.num_actions;                   // 15x15 is 1,125 actions, 20x20 2,000
  if (A <= 64 * 2) return launch_waves(search_policy_kernel<2>, a.n, s, a);
  if (A <= 64 * 8) return launch_waves(search_policy_kernel<8>, a.n, s, a);
  if (A <= 64 * 18) return launch_waves(search_policy_kernel<18>, a.n, s, a);
  if (A <= 64 * 32) return launch_waves(search_policy_kernel<32>, a.n, s, a);
  if (A <= 64 * 50) return launch_waves(search_policy_kernel<50>, a.n, s, a);
  return launch_waves(search_policy_kernel<80>, a.n, s, a);
}

}  // namespace gvec
