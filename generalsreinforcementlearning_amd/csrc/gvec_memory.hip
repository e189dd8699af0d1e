// gvec_memory.hip — fog-of-war memory planes: per tile, what a learner last saw of it and how long ago (gvec_obs_memory_update
// in generals_vec.h).
//
// Elementwise and bandwidth-bound: a row reads three observation planes and the four planes of its previous state and writes
// four planes, every byte once.  One wavefront per row, four per workgroup, no LDS and no barrier.  lane = tile, plain dword
// loads and stores as in gvec_features.hip's load and store steps: 15x15 and 25x25 planes start on no 16-byte boundary and
// a row may sit at any dword offset.  A lane carries MEM_TILES tiles at a time, so that all of their loads are in flight before
// the first store: prev may be out (in place), which keeps the compiler from moving a load over a store by itself.  A tile's
// result depends on that tile's inputs alone and the lane that stores a tile is the lane that loaded it, so in place is safe.
// The row's reset flag is wave-uniform: a restarted row (and every row when prev is null) skips the four loads of prev.
#include "gvec_launch.hpp"
#include "gvec_waves.hpp"

namespace gvec {

namespace {

constexpr int MEM_TILES = 2;   // tiles per lane and pass

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void obs_memory_kernel(gvec_obs_memory_args P, float capf, float inv) {
  const int lane = lane_id();
  // not wave_item(): with it the 8,192-row shape of scripts/bench_memory.py measured 1-2 % slower than the parent in each
  // of three parent / result / parent runs (profiles/learner_units_ab.json), so the opening keeps its own spelling
  const uint32_t wave = (uint32_t)uni(block_wave());
  const uint32_t r = blockIdx.x * (uint32_t)WAVES_PER_BLOCK + wave;   // rows < 2^31: no wrap
  if (r >= (uint32_t)P.rows) return;                                 // the whole wave leaves
  const int HW = P.width * P.height;
  const bool blank = !P.prev || (P.reset && P.reset[r / (uint32_t)P.rows_per_flag] != 0);   // wave-uniform
  const float* o = P.obs + (size_t)r * (size_t)P.obs_row_stride;
  const uint32_t* o_bits = reinterpret_cast<const uint32_t*>(o);               // planes 1 and 2 are copied, not computed with
  const size_t row = (size_t)r * 4u * (size_t)HW;
  const float* prev = P.prev + row;                                  // not dereferenced when blank
  const uint32_t* prev_bits = reinterpret_cast<const uint32_t*>(prev);
  float* out = P.out + row;
  uint32_t* out_bits = reinterpret_cast<uint32_t*>(out);

  for (int t0 = lane; t0 < HW; t0 += 64 * MEM_TILES) {
    float vis[MEM_TILES], seen[MEM_TILES], age[MEM_TILES];
    uint32_t owner[MEM_TILES], army[MEM_TILES], b_owner[MEM_TILES], b_army[MEM_TILES];
#pragma unroll
    for (int u = 0; u < MEM_TILES; ++u) {
      const int t = min(t0 + 64 * u, HW - 1);                          // a lane past the row's end loads its last tile: no branch
      vis[u] = o[t];
      owner[u] = o_bits[HW + t];
      army[u] = o_bits[2 * HW + t];
    }
    if (!blank) {
#pragma unroll
      for (int u = 0; u < MEM_TILES; ++u) {
        const int t = min(t0 + 64 * u, HW - 1);
        seen[u] = prev[t];
        b_owner[u] = prev_bits[HW + t];
        b_army[u] = prev_bits[2 * HW + t];
        age[u] = prev[3 * HW + t];
      }
    } else {
#pragma unroll
      for (int u = 0; u < MEM_TILES; ++u) {
        seen[u] = 0.0f;
        b_owner[u] = b_army[u] = 0u;
        age[u] = 1.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < MEM_TILES; ++u) {
      const int t = t0 + 64 * u;
      if (t < HW) {
        const bool v = vis[u] != 0.0f;
        const float older = fminf(age[u] * capf + 1.0f, capf) * inv;  // exact: age * cap is an integer <= cap
        out[t] = v ? 1.0f : seen[u];
        out_bits[HW + t] = v ? owner[u] : b_owner[u];
        out_bits[2 * HW + t] = v ? army[u] : b_army[u];
        out[3 * HW + t] = v ? 0.0f : (seen[u] != 0.0f ? older : 1.0f);
      }
    }
  }
}

}  // namespace

hipError_t launch_obs_memory(const gvec_obs_memory_args& a, hipStream_t s) {
  return launch_waves(obs_memory_kernel, a.rows, s, a, (float)a.cap, 1.0f / (float)a.cap);
}

}  // namespace gvec
