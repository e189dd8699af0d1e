// gvec_collect.hpp — what the kernels that fill the replay ring (gvec_pool_collect, gvec_stream.hip) and the kernels that
// read it back (gvec_nstep_*, gvec_nstep.hip) share: the layout of the collect scratch and the row copy.
#pragma once
#include "gvec_device.hpp"

namespace gvec {

// scratch: flag[B] (bit 0 live: this step was a transition of the worker's episode; bit 1 over: the episode ended with it),
// per 64-worker group the exclusive prefix counts of both bits, the cursors the push works from, what finished episodes report
struct CollectScratch {
  uint8_t* flag;          // [G * 64]
  int32_t* fin_length;    // [B]
  long long* base_live;   // [G + 1]
  long long* base_over;   // [G + 1]
  long long* snap;        // [2]: the ring's cursor and the results held BEFORE this call
  double* fin_reward;     // [B]
};
__host__ __device__ inline int collect_groups(int32_t n) { return (n + 63) >> 6; }
__host__ __device__ inline CollectScratch collect_scratch(void* base, int32_t n) {
  const int g = collect_groups(n);
  CollectScratch c;
  c.base_live = static_cast<long long*>(base);
  c.base_over = c.base_live + g + 1;
  c.snap = c.base_over + g + 1;
  c.flag = reinterpret_cast<uint8_t*>(c.snap + 2);              // 16 * (g + 2) bytes in: read sixteen bytes at a time
  c.fin_reward = reinterpret_cast<double*>(c.flag + (size_t)g * 64);
  c.fin_length = reinterpret_cast<int32_t*>(c.fin_reward + n);
  return c;
}

// A row of n floats from s to d, both only dword-aligned (a row is 9*W*H floats) and not alike: sixteen bytes per lane with
// BOTH the loads and the stores on 16-byte boundaries - a destination quad is cut out of two neighbouring source quads (the
// second load hits the lines the neighbouring lane fetches) - because either side misaligned costs a quarter of the rate
// (4.0-4.2 TB/s against 5.3 on this copy).  The few floats before / after the aligned body go one by one.  `part` of
// 1 << shift wavefronts share the row.
template <int D>
static __device__ __forceinline__ void copy_quads(const float4* __restrict__ sq, float4* __restrict__ dq, int jlo, int jhi, int c, int first, int stride) {
#pragma unroll 4
  for (int j = jlo + first; j < jhi; j += stride) {
    const float4 lo = sq[j + c];
    float4 o;
    if (D == 0) {
      o = lo;
    } else {
      const float4 hi = sq[j + c + 1];
      if (D == 1) o = make_float4(lo.y, lo.z, lo.w, hi.x);
      if (D == 2) o = make_float4(lo.z, lo.w, hi.x, hi.y);
      if (D == 3) o = make_float4(lo.w, hi.x, hi.y, hi.z);
    }
    dq[j] = o;
  }
}
static __device__ __forceinline__ void copy_row(const float* __restrict__ s, float* __restrict__ d, int n, int part, int lane, int shift) {
  const int ks = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(s) & 15u)) & 15u) >> 2);   // floats before s is 16-byte aligned
  const int kd = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) >> 2);
  const int delta = uni((kd - ks) & 3), c = kd >= ks ? 0 : -1;
  // destination quad j = floats [kd + 4j, kd + 4j + 4) = source quads j + c and j + c + 1 (counted from s + ks); all of it inside the row:
  const int jlo = -c;
  const int jhi = (n - 8 - ks < 0) ? jlo : (n - 8 - ks) / 4 - c + 1;          // exclusive
  const float4* sq = reinterpret_cast<const float4*>(s + ks);
  float4* dq = reinterpret_cast<float4*>(d + kd);
  const int first = part * 64 + lane, stride = 64 << shift;
  switch (delta) {
    case 0: copy_quads<0>(sq, dq, jlo, jhi, c, first, stride); break;
    case 1: copy_quads<1>(sq, dq, jlo, jhi, c, first, stride); break;
    case 2: copy_quads<2>(sq, dq, jlo, jhi, c, first, stride); break;
    default: copy_quads<3>(sq, dq, jlo, jhi, c, first, stride); break;
  }
  if (part == 0) {
    const int head = kd + 4 * jlo, tail = kd + 4 * jhi;       // [0, head) and [tail, n): fewer than 16 floats each
    if (lane < head && lane < n) d[lane] = s[lane];
    if (tail + lane < n) d[tail + lane] = s[tail + lane];
  }
}

}  // namespace gvec
