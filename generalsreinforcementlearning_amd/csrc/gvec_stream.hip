// gvec_stream.hip — what leaves the device in compacted form: one player's stream deltas with their packing, and the pool
// collector that pushes every worker's transition into the replay ring.
#include "gvec_dispatch.hpp"
#include "gvec_collect.hpp"
#include "gvec_rows.hpp"
#include "gvec_turn.hpp"

namespace gvec {

// =========================================================================================
// gameInstance.createStreamUpdate's delta (internal/grpc/gameserver/server.go:636-777) for one player's stream, every env:
// when 0 < |ChangedTiles| + |VisibilityChangedTiles| < N / 5 (a tile in both sets counts twice, :636-640) the update is a
// GameStateDelta whose tile updates are the tiles of either set with the proto's fog rules applied for that player
// (:664-689 == :556-582); otherwise the server sends the full state.  The handful of tiles a turn touches leave the GPU
// instead of the board: ~10 eight-byte updates per env instead of 4 KB of planes.
// updates[env][k] = tile index | type << 16 | visible << 18 | fog_of_war << 19 | (owner + 1) << 20 | army << 32, the changed
// tiles ascending, then the visibility-only ones ascending (Go ranges over maps: its order is unspecified).
// =========================================================================================
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void stream_delta_kernel(StreamDeltaArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  const int nc = b.count(b.chg), nv = b.count(b.vch);
  const int total = nc + nv;
  const bool delta = total > 0 && total < b.N / 5;       // :640 (integer division)
  const int n_union = b.count(b.chg | b.vch);            // a wave-wide reduction: every lane takes part
  const bool all_tiles = !delta && A.full_tiles != 0;     // the full state's tiles (server.go:556-582) for envs that get no delta
  if (lane == 0) {
    A.kind[env] = (uint8_t)(delta ? 1 : 2);
    A.count[env] = delta ? n_union : (all_tiles ? b.N : 0);
  }
  if (!delta && !all_tiles) return;                       // wave-uniform
  const bool fog_on = (b.hflags & HF_FOG) != 0u;
  uint32_t vis_p = 0u;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) vis_p = (p == A.player) ? b.vis[p] : vis_p;
  unsigned long long* out = A.updates + (size_t)env * A.cap;
  int base = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const uint32_t sel_plane = all_tiles ? (pass == 0 ? b.valid : 0u) : (pass == 0 ? b.chg : (b.vch & ~b.chg));
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      int owner = -1;
#pragma unroll
      for (int p = 0; p < MAXP; ++p) owner = gather(b.own[p], s) ? p : owner;
      const uint32_t is_gen = gather(b.gen, s), is_city = gather(b.city, s), is_mtn = gather(b.mtn, s);
      const uint32_t pv = gather(vis_p, s);
      const bool sel = gather(sel_plane, s) != 0u && t < b.N;
      int type = is_gen ? GVEC_TILE_GENERAL : (is_city ? GVEC_TILE_CITY : (is_mtn ? GVEC_TILE_MOUNTAIN : GVEC_TILE_NORMAL));
      const bool visible = !fog_on || pv != 0u;                        // ComputePlayerVisibility (visibility_optimized.go:166-195)
      const bool fogged = !visible && type != GVEC_TILE_NORMAL;
      int32_t army = b.army[s];
      if (!visible) {                                                  // :676-688: hidden or fogged - the current state is withheld
        owner = -1;
        army = 0;
      }                                                                // (a hidden tile IS a normal tile: its type needs no rewrite)
      const unsigned long long m = __builtin_amdgcn_ballot_w64(sel);
      const int pos = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));
      if (sel && pos < A.cap)
        out[pos] = (unsigned long long)((uint32_t)t | ((uint32_t)type << 16) | ((visible ? 1u : 0u) << 18) | ((fogged ? 1u : 0u) << 19) |
                                        ((uint32_t)(owner + 1) << 20)) |
                   ((unsigned long long)(uint32_t)army << 32);
      base += __builtin_popcountll(m);
    }
  }
}

// gvec_stream_deltas_packed: exclusive prefix sum of the per-env update counts (one workgroup: B is a few hundred thousand
// small integers) and the row-to-stream compaction that follows it.
__global__ __launch_bounds__(SCAN_THREADS) void scan_counts_kernel(const int32_t* count, long long* offset, int32_t n) {
  __shared__ long long part[1][SCAN_THREADS];
  const ScanRun r = scan_run(n);
  long long run[1] = {0};
  for (long long i = r.lo; i < r.hi; ++i) run[0] += count[i];
  block_scan(part, run);
  for (long long i = r.lo; i < r.hi; ++i) {
    offset[i] = run[0];
    run[0] += count[i];
  }
  if (threadIdx.x == SCAN_THREADS - 1) offset[n] = part[0][SCAN_THREADS - 1];
}
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void pack_updates_kernel(const unsigned long long* rows, const int32_t* count, const long long* offset,
                                                                            unsigned long long* packed, int32_t n, int32_t cap, long long capacity) {
  const int env = wave_item();
  if (env >= n) return;
  const long long base = offset[env];
  const int c = count[env];
  for (int k = lane_id(); k < c; k += 64)
    if (base + k < capacity) packed[base + k] = rows[(size_t)env * cap + k];
}

// =========================================================================================
// pool collection: the loop ParallelEnvPool's workers run around GeneralsEnv.step (python/generals_gym/vector_env.py:164-192)
// and ReplayBuffer.push (replay_buffer.py:31-36), for every worker at once and without leaving the device
// =========================================================================================
// one thread per worker: vector_env.py:172-192 without the push
__global__ __launch_bounds__(256) void collect_flags_kernel(gvec_collect_args A) {
  const int w = (int)(blockIdx.x * 256 + threadIdx.x);
  const CollectScratch S = collect_scratch(A.scratch, A.num_envs);
  if (w >= collect_groups(A.num_envs) * 64) return;
  if (w >= A.num_envs) {
    S.flag[w] = 0;          // the tail of the last group
    return;
  }
  const bool live = !A.was_reset[w];
  const bool done = (A.terminated[w] | A.truncated[w]) != 0;
  double er = A.episode_reward[w];
  long long el = A.episode_length[w];
  if (live) {
    er += A.reward[w];      // :186
    el += 1;                // :187
  }
  const bool over = live && (done || el >= A.max_steps_per_episode);   // the while condition of :177 failing
  S.flag[w] = (uint8_t)((live ? 1 : 0) | (over ? 2 : 0));
  if (over) {
    S.fin_reward[w] = er;
    S.fin_length[w] = (int32_t)el;
    er = 0.0;
    el = 0;
    if (!done && A.needs_reset) A.needs_reset[w] = 1;   // cut at the length limit: the next step is the worker's env.reset()
  }
  A.episode_reward[w] = er;
  A.episode_length[w] = el;
}
// run[0] += the live bits, run[1] += the over bits of the 64 flag bytes of group g
__device__ __forceinline__ void add_group_flags(const CollectScratch& S, long long g, long long (&run)[2]) {
  const uint4* f = reinterpret_cast<const uint4*>(S.flag + (size_t)g * 64);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 v = f[q];
    run[0] += __popc(v.x & 0x01010101u) + __popc(v.y & 0x01010101u) + __popc(v.z & 0x01010101u) + __popc(v.w & 0x01010101u);
    run[1] += __popc(v.x & 0x02020202u) + __popc(v.y & 0x02020202u) + __popc(v.z & 0x02020202u) + __popc(v.w & 0x02020202u);
  }
}
// one workgroup: exclusive prefix counts per 64-worker group (a thread owns a run of consecutive groups, 64 flag bytes each),
// then the counters move on - the push works from the snapshot
__global__ __launch_bounds__(SCAN_THREADS) void collect_scan_kernel(gvec_collect_args A) {
  __shared__ long long part[2][SCAN_THREADS];
  const CollectScratch S = collect_scratch(A.scratch, A.num_envs);
  const ScanRun r = scan_run(collect_groups(A.num_envs));
  long long run[2] = {0, 0};                   // live, over: both counts ride one scan
  for (long long g = r.lo; g < r.hi; ++g) add_group_flags(S, g, run);
  block_scan(part, run);
  for (long long g = r.lo; g < r.hi; ++g) {
    S.base_live[g] = run[0];
    S.base_over[g] = run[1];
    add_group_flags(S, g, run);
  }
  if (threadIdx.x == SCAN_THREADS - 1) {
    const long long pushed = part[0][SCAN_THREADS - 1], ended = part[1][SCAN_THREADS - 1];
    long long* R = reinterpret_cast<long long*>(A.ring_counters);
    long long* P = reinterpret_cast<long long*>(A.pool_counters);
    S.snap[0] = R[0];
    S.snap[1] = P[1];
    R[0] = (R[0] + pushed) % A.capacity;
    R[1] = (R[1] + pushed < A.capacity) ? R[1] + pushed : A.capacity;
    R[2] += pushed;
    P[0] += ended;
    const long long room = A.result_capacity - P[1];
    const long long kept = ended < room ? ended : room;
    P[1] += kept;
    P[2] += ended - kept;
  }
}
// `wpe` wavefronts per worker (a power of two): ReplayBuffer.push of its transition, and its episode result
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void collect_push_kernel(gvec_collect_args A, int wpe_shift) {
  const WaveSplit sp = wave_split(wpe_shift);
  if (sp.item >= A.num_envs) return;
  const CollectScratch S = collect_scratch(A.scratch, A.num_envs);
  const int w = (int)sp.item, part = sp.part, lane = lane_id();
  const int g = w >> 6, at = w & 63;
  const uint32_t mine = S.flag[(size_t)g * 64 + lane];
  const unsigned long long below = (1ull << at) - 1;
  const unsigned long long live_m = __ballot(mine & 1), over_m = __ballot(mine & 2);
  if ((live_m >> at) & 1) {
    long long slot = S.snap[0] + S.base_live[g] + __popcll(live_m & below);
    if (slot >= A.capacity) slot -= A.capacity;          // cursor < capacity and fewer than num_envs <= capacity ahead of it
    const float* s0 = A.state + (size_t)w * A.obs_floats;
    const float* s1 = A.next_state + (size_t)w * A.obs_floats;
    float* d0 = A.ring_state + (size_t)slot * A.obs_floats;
    float* d1 = A.ring_next_state + (size_t)slot * A.obs_floats;
    copy_row(s0, d0, A.obs_floats, sp);
    copy_row(s1, d1, A.obs_floats, sp);
    if (part == 0) {
      if (lane == 0) {
        A.ring_action[slot] = A.action[w];
        A.ring_reward[slot] = A.reward[w];
        A.ring_done[slot] = (A.terminated[w] | A.truncated[w]) != 0;
      }
    }
  }
  if (part == 0 && lane == 0 && ((over_m >> at) & 1)) {
    const long long j = S.snap[1] + S.base_over[g] + __popcll(over_m & below);
    if (j < A.result_capacity) {
      A.result_reward[j] = S.fin_reward[w];
      A.result_length[j] = S.fin_length[w];
      A.result_worker[j] = w;
    }
  }
}

// =========================================================================================
// host-side launchers
// =========================================================================================
hipError_t launch_stream_deltas(const Variant& v, const StreamDeltaArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(stream_delta_kernel<P, S>, a.num_envs, s, a); });
}
hipError_t launch_pack_updates(const unsigned long long* rows, const int32_t* count, long long* offset, unsigned long long* packed, int32_t n,
                               int32_t cap, long long capacity, hipStream_t s) {
  hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, count, offset, n);
  return launch_waves(pack_updates_kernel, n, s, rows, count, offset, packed, n, cap, capacity);
}
size_t pool_collect_scratch_bytes(int32_t n) {
  const size_t g = (size_t)collect_groups(n);
  return (2 * (g + 1) + 2) * 8 + (size_t)n * 8 + (size_t)n * 4 + g * 64;
}
hipError_t launch_pool_collect(const gvec_collect_args& a, hipStream_t s) {
  const hipError_t e = launch_threads(collect_flags_kernel, collect_groups(a.num_envs) * 64, s, a);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(collect_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, a);
  const int shift = split_shift(a.num_envs);
  return launch_waves(collect_push_kernel, (long long)a.num_envs << shift, s, a, shift);
}

}  // namespace gvec
