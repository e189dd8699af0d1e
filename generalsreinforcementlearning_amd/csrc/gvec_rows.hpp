// gvec_rows.hpp — the row movers of the kernels that fill the replay ring (gvec_pool_collect, gvec_stream.hip) and of those
// that read a ring or a rollout back (gvec_nstep.hip, gvec_traj.hip): a row of floats or of bytes between two addresses that
// are aligned to nothing wider than an element, shared by the 1 << shift wavefronts of a WaveSplit (gvec_waves.hpp).
#pragma once
#include "gvec_waves.hpp"

namespace gvec {

// A row of n floats from s to d, both only dword-aligned (a row is 9*W*H floats) and not alike: sixteen bytes per lane with
// BOTH the loads and the stores on 16-byte boundaries - a destination quad is cut out of two neighbouring source quads (the
// second load hits the lines the neighbouring lane fetches) - because either side misaligned costs a quarter of the rate
// (4.0-4.2 TB/s against 5.3 on this copy).  The few floats before / after the aligned body go one by one (part 0).
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
static __device__ __forceinline__ void copy_row(const float* __restrict__ s, float* __restrict__ d, int n, const WaveSplit& w) {
  const int ks = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(s) & 15u)) & 15u) >> 2);   // floats before s is 16-byte aligned
  const int kd = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) >> 2);
  const int delta = uni((kd - ks) & 3), c = kd >= ks ? 0 : -1;
  // destination quad j = floats [kd + 4j, kd + 4j + 4) = source quads j + c and j + c + 1 (counted from s + ks); all of it inside the row:
  const int jlo = -c;
  const int jhi = (n - 8 - ks < 0) ? jlo : (n - 8 - ks) / 4 - c + 1;          // exclusive
  const float4* sq = reinterpret_cast<const float4*>(s + ks);
  float4* dq = reinterpret_cast<float4*>(d + kd);
  switch (delta) {
    case 0: copy_quads<0>(sq, dq, jlo, jhi, c, w.first, w.stride); break;
    case 1: copy_quads<1>(sq, dq, jlo, jhi, c, w.first, w.stride); break;
    case 2: copy_quads<2>(sq, dq, jlo, jhi, c, w.first, w.stride); break;
    default: copy_quads<3>(sq, dq, jlo, jhi, c, w.first, w.stride); break;
  }
  if (w.part == 0) {
    const int lane = lane_id();
    const int head = kd + 4 * jlo, tail = kd + 4 * jhi;       // [0, head) and [tail, n): fewer than 16 floats each
    if (lane < head && lane < n) d[lane] = s[lane];
    if (tail + lane < n) d[tail + lane] = s[tail + lane];
  }
}

// copy_row's scheme for a row of n BYTES (a mask row is 5*W*H bytes, aligned to nothing): four bytes per lane, the loads and
// the stores on dword boundaries, a destination dword cut out of two neighbouring source dwords by v_alignbyte.  The range
// is derived from the destination side: a = the bytes s + kd sits into its dword, source dword j = bytes [kd - a + 4j, + 4)
// of the row; j and (a != 0) j + 1 must lie in [0, n).
static __device__ __forceinline__ void move_row_u8(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int n, const WaveSplit& w) {
  const int kd = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 3u)) & 3u);
  const int a = uni((int)(reinterpret_cast<uintptr_t>(s + kd) & 3u));
  const int jlo = a > kd ? 1 : 0;
  const int room = a ? n - 8 - kd + a : n - 4 - kd;
  const int jhi = room < 0 ? jlo : (room / 4 + 1 > jlo ? room / 4 + 1 : jlo);                    // exclusive
  const uint32_t* __restrict__ sw = reinterpret_cast<const uint32_t*>(s + kd - a);
  uint32_t* __restrict__ dw = reinterpret_cast<uint32_t*>(d + kd);
  if (a == 0) {
    for (int j = jlo + w.first; j < jhi; j += w.stride) dw[j] = sw[j];
  } else {
    for (int j = jlo + w.first; j < jhi; j += w.stride) dw[j] = __builtin_amdgcn_alignbyte(sw[j + 1], sw[j], (uint32_t)a);
  }
  if (w.part == 0) {
    int head = kd + 4 * jlo, tail = kd + 4 * jhi;       // [0, head) and [tail, n): a few bytes each (all of a very short row)
    if (jhi == jlo) head = tail = 0;
    for (int k = w.first; k < head && k < n; k += 64) d[k] = s[k];
    for (int k = tail + w.first; k < n; k += 64) d[k] = s[k];
  }
}

}  // namespace gvec
