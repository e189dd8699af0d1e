// gvec_per.hip — prioritized experience replay (Schaul et al. 2016) over a replay ring in HBM: a radix-64 sum tree, one float32
// leaf per ring slot, maintained and sampled by the kernels below (gvec_per_* in generals_vec.h).
//
// The tree is one float array: a 64-word header, then level 0 (the leaves), level 1, ... up to the one-node root level, every
// level padded with zeros to a multiple of 64 floats.  Node i of level l + 1 covers nodes [64 i, 64 i + 64) of level l.
//
// In-node arithmetic: the SEQUENTIAL left-to-right float32 prefix P[j] = P[j-1] + c[j] over the 64 children, which every lane
// of a wavefront computes for itself over values handed round with v_readlane (seq_prefix).  The stored value of a node is
// P[63].  The descent picks the child j = #{i : P[i] <= r} for a residual r < P[63], so
//   1. a child of value 0 is never picked (c[j] == 0 gives P[j] == P[j-1]: no r lies between them), and
//   2. the pick never leaves the node (r < P[63] = the node's stored value),
// both exactly, in floating point.  The residual handed down, r - P[j-1], is clamped below c[j]: P[j] may have been rounded up.
// A node is only ever recomputed from its children - no differences, no float atomics - so the tree cannot drift and a
// refresh is idempotent (duplicate indices need no deduplication).
#include "gvec_launch.hpp"
#include "gvec_waves.hpp"

namespace gvec {

namespace {

constexpr uint32_t F32_INF = 0x7F800000u;

// Lane j receives P[j] = ((c[0] + c[1]) + ...) + c[j], the additions in exactly this order in every lane (wave-uniform
// control flow: all 64 lanes take part).  Non-negative inputs make P non-decreasing.
__device__ __forceinline__ float seq_prefix(float c) {
  const int me = lane_id();
  float acc = rdlane(c, 0);
  float p = acc;
#pragma unroll
  for (int j = 1; j < 64; ++j) {
    acc = acc + rdlane(c, j);
    p = (me >= j) ? acc : p;
  }
  return p;
}

// one wavefront: node `node` of level `lvl` (>= 1) := the last sequential prefix over its 64 children
__device__ __forceinline__ void refresh_node(float* tree, const PerLayout& Y, int lvl, long long node) {
  const float c = tree[Y.off[lvl - 1] + node * 64 + lane_id()];
  const float p = seq_prefix(c);
  if (lane_id() == 63) tree[Y.off[lvl] + node] = p;
}

__global__ __launch_bounds__(256) void per_init_kernel(float* tree, long long total_floats) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long stride = (long long)gridDim.x * 256;
  uint32_t* w = reinterpret_cast<uint32_t*>(tree);
  for (long long j = i; j < total_floats; j += stride) {
    uint32_t v = 0u;
    if (j == GVEC_PER_HDR_MAX) v = __float_as_uint(1.0f);
    if (j == GVEC_PER_HDR_MIN0 || j == GVEC_PER_HDR_MIN0 + 1) v = F32_INF;
    w[j] = v;
  }
}

// The slots a push covers: [cursor, cursor + count) mod capacity as at most two runs [a0, a1) and [0, b1), from two copies of
// the ring's counters {cursor, size, total pushed} taken before and after the rows were appended.
struct PerRuns {
  long long a0, a1, b1;   // b1 == 0: no second run
};
__device__ __forceinline__ PerRuns push_runs(const long long* before, const long long* after, long long capacity, long long max_count,
                                             uint32_t* hdr, bool report) {
  PerRuns r;
  long long count = after[2] - before[2];
  if (count > capacity) count = capacity;                     // the ring went all the way round: every slot is new
  if (count > max_count) {                                    // more rows than the launch was sized for: the rest keep their leaves
    if (report) atomicAdd(hdr + GVEC_PER_HDR_REJECTED, 1u);
    count = max_count;
  }
  long long cursor = before[0];
  if (count <= 0 || cursor < 0 || cursor >= capacity) {
    r.a0 = r.a1 = r.b1 = 0;
    return r;
  }
  r.a0 = cursor;
  r.a1 = cursor + count < capacity ? cursor + count : capacity;
  r.b1 = cursor + count - r.a1;
  return r;
}
// the w-th node of level `lvl` that the runs touch (first run's nodes, then the second's), or -1
__device__ __forceinline__ long long touched_node(const PerRuns& r, int lvl, long long w) {
  const int sh = 6 * lvl;
  if (r.a1 <= r.a0) return -1;
  const long long na0 = r.a0 >> sh, na = ((r.a1 - 1) >> sh) - na0 + 1;
  if (w < na) return na0 + w;
  w -= na;
  if (r.b1 > 0 && w <= ((r.b1 - 1) >> sh)) return w;
  return -1;
}

// push, level 0 and 1 together: one wavefront per touched level-1 node writes the node's new leaves (the running maximum)
// and the node itself from the 64 leaves it holds in registers - no other wavefront's store is needed
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void per_push_leaves_kernel(float* tree, PerLayout Y, const long long* before, const long long* after,
                                                                         long long max_count) {
  const long long w = wave_item64();
  uint32_t* hdr = reinterpret_cast<uint32_t*>(tree);
  const PerRuns r = push_runs(before, after, Y.capacity, max_count, hdr, w == 0 && lane_id() == 0);
  const long long node = touched_node(r, 1, w);
  if (node < 0) return;
  const long long slot = node * 64 + lane_id();
  const bool hit = (slot >= r.a0 && slot < r.a1) || slot < r.b1;      // both runs: they may meet inside one node
  float* leaf = tree + Y.off[0] + slot;
  const float top = __uint_as_float(hdr[GVEC_PER_HDR_MAX]);
  float c = *leaf;
  if (hit) {
    c = top;
    *leaf = c;
  }
  const float p = seq_prefix(c);
  if (lane_id() == 63) tree[Y.off[1] + node] = p;
}

// one workgroup: levels lvl0 .. root, each level's touched nodes (whole != 0: all of them) before the next level's
__global__ __launch_bounds__(1024) void per_upper_kernel(float* tree, PerLayout Y, int lvl0, int whole, const long long* before, const long long* after,
                                                         long long max_count) {
  const int wv = (int)(threadIdx.x >> 6);
  PerRuns r;
  if (whole) {
    r.a0 = 0;
    r.a1 = Y.capacity;
    r.b1 = 0;
  } else {
    r = push_runs(before, after, Y.capacity, max_count, reinterpret_cast<uint32_t*>(tree), false);
  }
  for (int lvl = lvl0; lvl <= Y.levels; ++lvl) {
    for (long long w = wv;; w += 16) {
      const long long node = touched_node(r, lvl, w);
      if (node < 0) break;
      refresh_node(tree, Y, lvl, node);
    }
    __syncthreads();      // a level's stores before the next level's loads (one workgroup: one CU, one L1)
  }
}

// update, level 0: one thread per (index, td error)
__global__ __launch_bounds__(256) void per_update_leaves_kernel(float* tree, PerLayout Y, const long long* idx, const float* td, long long n, float alpha,
                                                                float eps) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t* hdr = reinterpret_cast<uint32_t*>(tree);
  const long long slot = idx[i];
  const float e = fabsf(td[i]);
  const float v = powf(e + eps, alpha);
  // outside the ring, a NaN / infinite error (tested on the input: pow(NaN, 0) is 1), or a priority that overflows
  if (slot < 0 || slot >= Y.capacity || !(e < __uint_as_float(F32_INF)) || !(v >= 0.0f) || __float_as_uint(v) >= F32_INF) {
    atomicAdd(hdr + GVEC_PER_HDR_REJECTED, 1u);
    return;
  }
  tree[Y.off[0] + slot] = v;
  const uint32_t bits = __float_as_uint(v);          // non-negative floats order like their bit patterns
  if (bits > hdr[GVEC_PER_HDR_MAX]) atomicMax(hdr + GVEC_PER_HDR_MAX, bits);
}
// update, level lvl: one wavefront per index refreshes that slot's ancestor (a duplicate rewrites the same value)
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void per_refresh_touched_kernel(float* tree, PerLayout Y, int lvl, const long long* idx, long long n) {
  const long long w = wave_item64();
  if (w >= n) return;
  const long long slot = uni_ll(idx[w]);
  if (slot < 0 || slot >= Y.capacity) return;
  refresh_node(tree, Y, lvl, slot >> (6 * lvl));
}

// sample, the draws: one wavefront per draw descends from the root
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void per_draw_kernel(float* tree, PerLayout Y, const long long* ring_counters, long long k, const double* u_in,
                                                                  unsigned long long seed, long long* idx, float* weight) {
  const long long j = wave_item64();
  uint32_t* hdr = reinterpret_cast<uint32_t*>(tree);
  const uint32_t call = hdr[GVEC_PER_HDR_DRAWS];               // the RNG's draw counter: a caller may zero it
  const uint32_t seq = hdr[GVEC_PER_HDR_SEQ];                  // the kernels' own call count: picks the minimum word, never reset
  if (j == 0 && lane_id() == 0) {
    hdr[GVEC_PER_HDR_DRAWS + 1] = call;                       // the weights kernel's copies (this kernel only reads the others)
    hdr[GVEC_PER_HDR_SEQ + 1] = seq;
    hdr[GVEC_PER_HDR_MIN0 + ((seq + 1u) & 1u)] = F32_INF;     // the next call's minimum; this call's was reset by the last one
  }
  if (j >= k) return;
  const float total = tree[Y.off[Y.levels]];
  if (!(total > 0.0f) || ring_counters[1] <= 0) {             // nothing to draw from
    if (lane_id() == 0) {
      idx[j] = -1;
      weight[j] = 0.0f;
    }
    return;
  }
  double u;
  if (u_in) {
    u = u_in[j];
  } else {                                                    // 53 bits from two hashes keyed by (seed, call, j)
    const uint32_t key = fmix32((uint32_t)seed ^ 0x9E3779B9u) + (uint32_t)(seed >> 32) * 0x85EBCA77u + call * 0xC2B2AE3Du;
    const uint32_t h1 = fmix32(key + (uint32_t)j * 0x27D4EB2Fu + (uint32_t)((unsigned long long)j >> 32) * 0x165667B1u);
    const uint32_t h2 = fmix32(h1 ^ 0x68E31DA4u ^ key);
    u = ((double)(h1 >> 5) * 67108864.0 + (double)(h2 >> 6)) * (1.0 / 9007199254740992.0);
  }
  u = u < 0.0 ? 0.0 : (u < 1.0 ? u : 1.0 - 1.0 / 9007199254740992.0);
  float r = (float)(((double)j + u) / (double)k * (double)total);
  if (r >= total) r = __uint_as_float(__float_as_uint(total) - 1u);   // the root target stays below the total
  long long node = 0;
  float leaf = 0.0f;
  for (int lvl = Y.levels; lvl >= 1; --lvl) {
    const float c = tree[Y.off[lvl - 1] + node * 64 + lane_id()];
    const float p = seq_prefix(c);
    int child = __popcll(__builtin_amdgcn_ballot_w64(p <= r));        // P is non-decreasing: the lanes that vote are a prefix
    child = child < 63 ? child : 63;                                  // (only a tree that breaks its invariant gets here with 64)
    const float below = child > 0 ? rdlane(p, child - 1) : 0.0f;
    leaf = rdlane(c, child);
    r = r - below;
    if (r >= leaf) r = leaf > 0.0f ? __uint_as_float(__float_as_uint(leaf) - 1u) : 0.0f;   // P[child] was rounded up: stay inside the child
    node = node * 64 + child;
  }
  if (lane_id() == 0) {
    idx[j] = node;
    weight[j] = leaf;                                                 // the weights kernel turns it into the weight
    const uint32_t bits = __float_as_uint(leaf);
    uint32_t* mn = hdr + GVEC_PER_HDR_MIN0 + (seq & 1u);
    if (bits < *mn) atomicMin(mn, bits);
  }
}
// sample, the weights: (size leaf / total)^-beta over the batch's largest = (leaf / the batch's smallest leaf)^-beta
__global__ __launch_bounds__(256) void per_weights_kernel(float* tree, long long k, float beta, float* weight) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  uint32_t* hdr = reinterpret_cast<uint32_t*>(tree);
  const uint32_t seq = hdr[GVEC_PER_HDR_SEQ + 1];             // the draw kernel's copies: this kernel moves the originals on
  if (j == 0) {
    hdr[GVEC_PER_HDR_DRAWS] = hdr[GVEC_PER_HDR_DRAWS + 1] + 1u;
    hdr[GVEC_PER_HDR_SEQ] = seq + 1u;
  }
  if (j >= k) return;
  const float least = __uint_as_float(hdr[GVEC_PER_HDR_MIN0 + (seq & 1u)]);
  const float leaf = weight[j];
  weight[j] = leaf > 0.0f ? powf(leaf / least, -beta) : 0.0f;
}

}  // namespace

PerLayout per_layout(long long capacity) {
  PerLayout y{};
  y.capacity = capacity;
  long long n = capacity, at = GVEC_PER_HEADER_WORDS;
  int l = 0;
  y.off[0] = at;
  do {
    at += (n + 63) / 64 * 64;
    n = (n + 63) / 64;
    y.off[++l] = at;
  } while (n > 1);
  y.levels = l;
  y.total = at + 64;          // the root level: one node and its padding
  return y;
}

hipError_t launch_per_init(float* tree, const PerLayout& y, hipStream_t s) {
  const long long blocks = (y.total + 255) / 256;
  hipLaunchKernelGGL(per_init_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, tree, y.total);
  return hipGetLastError();
}
hipError_t launch_per_push(float* tree, const PerLayout& y, const long long* before, const long long* after, long long max_count, hipStream_t s) {
  if (max_count > y.capacity) max_count = y.capacity;
  const hipError_t e = launch_waves(per_push_leaves_kernel, max_count / 64 + 4, s, tree, y, before, after, max_count);
  if (e != hipSuccess || y.levels < 2) return e;
  hipLaunchKernelGGL(per_upper_kernel, dim3(1), dim3(1024), 0, s, tree, y, 2, 0, before, after, max_count);
  return hipGetLastError();
}
hipError_t launch_per_update(float* tree, const PerLayout& y, const long long* idx, const float* td, long long n, float alpha, float eps, hipStream_t s) {
  hipError_t e = launch_threads(per_update_leaves_kernel, n, s, tree, y, idx, td, n, alpha, eps);
  int lvl = 1;
  // a level of more than 64 nodes: only the touched ones, one launch per level; the few levels above: whole, in one workgroup
  for (long long nodes = (y.capacity + 63) / 64; e == hipSuccess && lvl <= y.levels && nodes > 64; ++lvl, nodes = (nodes + 63) / 64)
    e = launch_waves(per_refresh_touched_kernel, n, s, tree, y, lvl, idx, n);
  if (e != hipSuccess || lvl > y.levels) return e;
  hipLaunchKernelGGL(per_upper_kernel, dim3(1), dim3(1024), 0, s, tree, y, lvl, 1, nullptr, nullptr, 0);
  return hipGetLastError();
}
hipError_t launch_per_sample(float* tree, const PerLayout& y, const long long* ring_counters, long long k, float beta, const double* u,
                             unsigned long long seed, long long* idx, float* weight, hipStream_t s) {
  const hipError_t e = launch_waves(per_draw_kernel, k, s, tree, y, ring_counters, k, u, seed, idx, weight);
  return e != hipSuccess ? e : launch_threads(per_weights_kernel, k, s, tree, k, beta, weight);
}

}  // namespace gvec
