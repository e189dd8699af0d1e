// gvec_nstep.hip — n-step returns over the replay ring (gvec_nstep_* in generals_vec.h): the per-slot successor
// links gvec_pool_collect's compacted push cannot express by position, written right after it from what it left in its
// scratch, and the one fused gather that walks them and moves a sample's two rows, which come from two different slots.
#include "gvec_launch.hpp"
#include "gvec_collect.hpp"
#include "gvec_rows.hpp"

namespace gvec {

namespace {

// one thread per worker, one wavefront per 64-worker group of the collect scratch: the rank of a live worker among the live
// ones is the group's prefix count plus the live lanes below it - exactly collect_push_kernel's slot
__global__ __launch_bounds__(256) void nstep_link_kernel(gvec_collect_args A, const long long* before, long long* succ, long long* last) {
  const int w = (int)(blockIdx.x * 256 + threadIdx.x);
  const int padded = collect_groups(A.num_envs) * 64;
  const CollectScratch S = collect_scratch(A.scratch, A.num_envs);
  const uint32_t mine = w < padded ? S.flag[w] : 0u;             // the tail of the last group holds zeros
  const unsigned long long live_m = __ballot(mine & 1);
  if (!(mine & 1) || w >= A.num_envs) return;
  const long long cursor = before[0], pushed = before[2];
  if (cursor < 0 || cursor >= A.capacity) return;                // not a copy of this ring's counters: touch nothing
  const int at = w & 63;
  const long long rank = S.base_live[w >> 6] + __popcll(live_m & ((1ull << at) - 1));
  const long long q = pushed + rank;
  long long s = cursor + rank;                                   // rank < num_envs <= capacity
  if (s >= A.capacity) s -= A.capacity;
  const long long total = A.ring_counters[2];                    // after the push
  const long long pq = last[2 * (size_t)w], ps = last[2 * (size_t)w + 1];
  // the predecessor is still held: by arithmetic alone (its slot may have been rewritten by this very push)
  if (pq >= 0 && ps >= 0 && ps < A.capacity && pq >= total - A.capacity) succ[ps] = s;
  succ[s] = -1;
  const bool over = (mine & 2) != 0;
  last[2 * (size_t)w] = over ? -1 : q;
  last[2 * (size_t)w + 1] = over ? -1 : s;
}

// `1 << shift` wavefronts per sample: each walks the links for itself (wave-uniform: at most n_step - 1 dependent loads), then
// they share the two rows
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void nstep_gather_kernel(gvec_nstep_gather_args A, int shift) {
  const WaveSplit w = wave_split(shift);
  const long long j = w.item;
  if (j >= A.k) return;
  const int n = A.obs_floats;
  float* d0 = A.state + (size_t)j * n;
  float* d1 = A.next_state + (size_t)j * n;
  const long long first = uni_ll(A.idx[j]);
  long long size = uni_ll(A.ring_counters[1]);
  if (size > A.capacity) size = A.capacity;
  if (first < 0 || first >= size) {                              // no such transition: the zero record
    for (int i = w.first; i < n; i += w.stride) {
      d0[i] = 0.0f;
      d1[i] = 0.0f;
    }
    if (w.first == 0) {
      A.action[j] = -1;
      A.ret[j] = 0.0;
      A.discount[j] = 0.0;
      A.done[j] = 0;
      A.steps[j] = 0;
      A.last_idx[j] = -1;
    }
    return;
  }
  long long cur = first;
  double ret = A.ring_reward[cur], disc = 1.0;
  int steps = 1;
  while (steps < A.n_step && !A.ring_done[cur]) {
    const long long nx = uni_ll(A.ring_succ[cur]);
    if (nx < 0 || nx >= A.capacity) break;
    cur = nx;
    disc = disc * A.gamma;
    ret = ret + disc * A.ring_reward[cur];
    ++steps;
  }
  copy_row(A.ring_state + (size_t)first * n, d0, n, w);
  copy_row(A.ring_next_state + (size_t)cur * n, d1, n, w);
  if (w.first == 0) {
    A.action[j] = A.ring_action[first];
    A.ret[j] = ret;
    A.discount[j] = disc * A.gamma;
    A.done[j] = A.ring_done[cur] != 0;
    A.steps[j] = steps;
    A.last_idx[j] = cur;
  }
}

}  // namespace

hipError_t launch_nstep_link(const gvec_collect_args& a, const long long* before, long long* ring_succ, long long* nstep_last, hipStream_t s) {
  return launch_threads(nstep_link_kernel, collect_groups(a.num_envs) * 64, s, a, before, ring_succ, nstep_last);
}
hipError_t launch_nstep_gather(const gvec_nstep_gather_args& a, hipStream_t s) {
  const int shift = split_shift(a.k);
  return launch_waves(nstep_gather_kernel, a.k << shift, s, a, shift);
}

}  // namespace gvec
