// gvec_collect.hpp — what the kernels that fill the replay ring (gvec_pool_collect, gvec_stream.hip) and the kernels that
// link its rows afterwards (gvec_nstep_link, gvec_nstep.hip) share: the layout of the collect scratch.  The row copy is
// gvec_rows.hpp's.
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

}  // namespace gvec
