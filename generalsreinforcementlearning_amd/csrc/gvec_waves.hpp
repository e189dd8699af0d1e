// gvec_waves.hpp — the launch shapes every kernel unit shares, host half and device half side by side: one wavefront per item
// (WAVES_PER_BLOCK items per workgroup), the rule that splits an item over several wavefronts when there are few items, one
// thread per item, and the one-workgroup prefix scan.  Nothing here knows about boards (that is gvec_dispatch.hpp).
#pragma once
#include "gvec_device.hpp"

namespace gvec {

// ---- one wavefront per item ---------------------------------------------------------------
constexpr int WAVES_PER_BLOCK = 4;

// device side of launch_waves: this wave's index in its block, and the item it owns (wave-uniform) - none when it is not
// below the launch's n (the spare waves of the last block), and the kernel leaves.  wave_item64: n may exceed 2^31.
__device__ __forceinline__ int block_wave() { return (int)(threadIdx.x >> 6); }
__device__ __forceinline__ int wave_item() { return uni((int)blockIdx.x * WAVES_PER_BLOCK + block_wave()); }
__device__ __forceinline__ long long wave_item64() { return uni_ll((long long)blockIdx.x * WAVES_PER_BLOCK + block_wave()); }

static inline dim3 wave_grid(long long n) { return dim3((unsigned)((n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)); }

// kernel k with one wavefront per item, n items, lds bytes of dynamic LDS per workgroup
template <typename... P, typename... A>
static hipError_t launch_waves(void (*k)(P...), long long n, size_t lds, hipStream_t s, const A&... a) {
  hipLaunchKernelGGL(k, wave_grid(n), dim3(64 * WAVES_PER_BLOCK), lds, s, a...);
  return hipGetLastError();
}
template <typename... P, typename... A>
static hipError_t launch_waves(void (*k)(P...), long long n, hipStream_t s, const A&... a) {
  return launch_waves(k, n, size_t{0}, s, a...);
}

// ---- few items: 1 << shift wavefronts share one ---------------------------------------------
// enough wavefronts to fill 256 CUs when n is small: at most 8 per item, none once there are 16,384
static inline int split_shift(long long n) {
  int shift = 0;
  while (shift < 3 && (n << shift) < 16384) ++shift;
  return shift;
}
// device side of launch_waves(k, n << shift, ...): wave `part` of the 1 << shift that own `item`; its lanes take elements
// first, first + stride, ...
struct WaveSplit {
  long long item;
  int part, first, stride;
};
__device__ __forceinline__ WaveSplit wave_split(int shift) {
  const long long gw = wave_item64();
  const int part = (int)(gw & ((1 << shift) - 1));
  return WaveSplit{gw >> shift, part, part * 64 + lane_id(), 64 << shift};
}

// ---- one thread per item --------------------------------------------------------------------
constexpr int THREADS_PER_BLOCK = 256;
template <typename... P, typename... A>
static hipError_t launch_threads(void (*k)(P...), long long n, hipStream_t s, const A&... a) {
  hipLaunchKernelGGL(k, dim3((unsigned)((n + THREADS_PER_BLOCK - 1) / THREADS_PER_BLOCK)), dim3(THREADS_PER_BLOCK), 0, s, a...);
  return hipGetLastError();
}

// ---- one workgroup of SCAN_THREADS: the exclusive prefix sums of n items ----------------------
constexpr int SCAN_THREADS = 1024;
// thread tid owns the consecutive items [lo, hi): runs of ceil(n / SCAN_THREADS), the last ones short or empty
struct ScanRun {
  long long lo, hi;
};
__device__ __forceinline__ ScanRun scan_run(long long n) {
  const long long per = (n + SCAN_THREADS - 1) / SCAN_THREADS, at = (long long)threadIdx.x * per;
  const long long lo = at < n ? at : n;
  return ScanRun{lo, lo + per < n ? lo + per : n};
}
// in: sum[k] = the total of count k over this thread's run; out: sum[k] = the total over every run before it (the base of
// the run's first item), part[k][SCAN_THREADS - 1] = the grand total.  K counts ride one Hillis-Steele pass.  Every thread
// of the workgroup calls it.
template <int K>
__device__ __forceinline__ void block_scan(long long (&part)[K][SCAN_THREADS], long long (&sum)[K]) {
  const int tid = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) part[k][tid] = sum[k];
  __syncthreads();
  for (int off = 1; off < SCAN_THREADS; off <<= 1) {
    long long add[K];
#pragma unroll
    for (int k = 0; k < K; ++k) add[k] = tid >= off ? part[k][tid - off] : 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) part[k][tid] += add[k];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) sum[k] = part[k][tid] - sum[k];
}

}  // namespace gvec
