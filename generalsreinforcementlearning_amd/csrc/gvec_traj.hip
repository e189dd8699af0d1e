// gvec_traj.hip — self-play rollouts in HBM: the per-step record, generalized advantage estimation, V-trace targets, the
// compaction of the valid rows and the minibatch gather (gvec_traj_* in generals_vec.h).
//
// A rollout is T rows of N = B * L streams, learner-minor as gvec_gym_step_players emits them; row t, stream n sits at
// position p = t * N + n of every store.  flags[p] carries the episode protocol (GVEC_TRAJ_VALID / _TERMINAL / _CUT), so the
// recurrence and the gather never look at the env's own arrays again.
#include "gvec_launch.hpp"
#include "gvec_rows.hpp"

namespace gvec {

namespace {

constexpr int GAE_ROWS = 32;           // rows a lane has in flight: the loads do not depend on the recurrence
constexpr int VTRACE_ROWS = 8;         // the same for V-trace, whose rows cost eight registers and an exp each: DESIGN.md §4.17
constexpr int COMPACT_BLOCK = 1024;    // positions per workgroup of the compaction (256 threads, four each)

// ---- record: one thread per stream ----
__global__ __launch_bounds__(256) void traj_record_kernel(gvec_traj_record_args A) {
  const long long N = (long long)A.num_envs * A.num_learners;
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const long long b = n / A.num_learners, p = A.t * N + n;
  const bool was_alive = A.alive_state[n] != 0, alive = A.alive[n] != 0;
  const bool reset = A.reset[b] != 0, term = A.terminated[b] != 0, trunc = A.truncated[b] != 0;
  const bool valid = !reset && was_alive;
  uint32_t f = 0;
  if (valid) f = GVEC_TRAJ_VALID | ((term || !alive) ? GVEC_TRAJ_TERMINAL : 0) | ((term || trunc || !alive) ? GVEC_TRAJ_CUT : 0);
  A.action[p] = A.step_action[n];
  A.logp[p] = A.step_logp[n];
  A.value[p] = A.step_value[n];
  A.reward[p] = A.step_reward[n];
  A.flags[p] = (uint8_t)f;
  A.alive_state[n] = alive ? 1 : 0;
}

// ---- GAE: one lane per stream walks t = T-1 .. 0; a wavefront's loads of a row are one coalesced line per array ----
__global__ __launch_bounds__(64) void traj_gae_kernel(gvec_traj_gae_args A) {
  const long long N = A.N, T = A.T;
  const long long n0 = (long long)blockIdx.x * 64 + lane_id();
  const bool act = n0 < N;
  const long long n = act ? n0 : N - 1;             // the tail lanes of the last wavefront read a real stream and store nothing
  const double* __restrict__ reward = A.reward;
  const float* __restrict__ value = A.value;
  const uint8_t* __restrict__ flags = A.flags;
  float* __restrict__ adv = A.adv;
  float* __restrict__ ret = A.ret;
  const double g = A.gamma, gl = A.gamma * A.lambda;
  double carry = 0.0, next_v = (double)value[T * N + n];
  double cnt = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long hi = T; hi > 0; hi -= GAE_ROWS) {  // rows hi-1 .. hi-GAE_ROWS: all their loads first, then the recurrence
    double r[GAE_ROWS];
    float v[GAE_ROWS];
    uint32_t f[GAE_ROWS];
#pragma unroll
    for (int i = 0; i < GAE_ROWS; ++i) {
      const long long t = hi - 1 - i, o = (t < 0 ? 0 : t) * N + n;
      r[i] = reward[o];
      v[i] = value[o];
      f[i] = flags[o];
    }
#pragma unroll
    for (int i = 0; i < GAE_ROWS; ++i) {
      const long long t = hi - 1 - i;
      if (t < 0) continue;                          // the same in every lane
      const double vt = (double)v[i];
      double a = 0.0, rt = vt;
      if (f[i] & GVEC_TRAJ_VALID) {
        const double delta = (r[i] + g * ((f[i] & GVEC_TRAJ_TERMINAL) ? 0.0 : next_v)) - vt;
        a = delta + gl * ((f[i] & GVEC_TRAJ_CUT) ? 0.0 : carry);
        rt = a + vt;
      }
      carry = a;                                    // an invalid row clears it
      next_v = vt;
      const float a32 = (float)a;
      if (act) {
        adv[t * N + n] = a32;
        ret[t * N + n] = (float)rt;
        if (f[i] & GVEC_TRAJ_VALID) {               // the statistics describe adv as stored
          const double x = (double)a32;
          cnt += 1.0;
          s1 += x;
          s2 += x * x;
        }
      }
    }
  }
  cnt = wave_sum(cnt);                              // fixed butterflies: the same bits on every run
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane_id() == 0) {
    double* part = static_cast<double*>(A.scratch) + (size_t)blockIdx.x * 3;
    part[0] = cnt;
    part[1] = s1;
    part[2] = s2;
  }
}
// second stage, one workgroup: thread i adds the K partials of groups i, i + 256, ... in that order, then a fixed tree over
// the 256 threads; the slots of stats[4] past K are zero
template <int K>
__global__ __launch_bounds__(256) void traj_stats_kernel(const double* part, long long groups, double* stats) {
  __shared__ double sh[K][256];
  const int tid = (int)threadIdx.x;
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  for (long long gi = tid; gi < groups; gi += 256) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += part[gi * K + k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][tid] = s[k];
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][tid] += sh[k][tid + off];
    }
    __syncthreads();
  }
  if (tid < 4) stats[tid] = tid < K ? sh[tid < K ? tid : 0][0] : 0.0;
}

// ---- V-trace: the same walk with two more loads per row.  exp and the two min depend on no other row: they are formed
// between the loads and the recurrence, and only delta -> acc -> vs and pg are on the serial chain ----
__global__ __launch_bounds__(64) void traj_vtrace_kernel(gvec_traj_vtrace_args A) {
  const long long N = A.N, T = A.T;
  const long long n0 = (long long)blockIdx.x * 64 + lane_id();
  const bool act = n0 < N;
  const long long n = act ? n0 : N - 1;             // the tail lanes of the last wavefront read a real stream and store nothing
  const double* __restrict__ reward = A.reward;
  const float* __restrict__ value = A.value;
  const uint8_t* __restrict__ flags = A.flags;
  const float* __restrict__ logp_b = A.logp_behaviour;
  const float* __restrict__ logp_t = A.logp_target;
  float* __restrict__ vs = A.vs;
  float* __restrict__ pg = A.pg;
  float* __restrict__ rho_out = A.rho_out;
  const double g = A.gamma, gl = A.gamma * A.lambda, rho_bar = A.rho_bar, c_bar = A.c_bar;
  double acc = 0.0, next_v = (double)value[T * N + n], next_vs = next_v;
  double cnt = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (long long hi = T; hi > 0; hi -= VTRACE_ROWS) {  // rows hi-1 .. hi-VTRACE_ROWS: loads, then the ratios, then the recurrence
    double r[VTRACE_ROWS], rho[VTRACE_ROWS], glc[VTRACE_ROWS];
    float v[VTRACE_ROWS], lt[VTRACE_ROWS], lb[VTRACE_ROWS];
    uint32_t f[VTRACE_ROWS];
#pragma unroll
    for (int i = 0; i < VTRACE_ROWS; ++i) {
      const long long t = hi - 1 - i, o = (t < 0 ? 0 : t) * N + n;
      r[i] = reward[o];
      v[i] = value[o];
      f[i] = flags[o];
      lt[i] = logp_t[o];
      lb[i] = logp_b[o];
    }
#pragma unroll
    for (int i = 0; i < VTRACE_ROWS; ++i) {
      const double w = exp((double)lt[i] - (double)lb[i]);
      rho[i] = fmin(rho_bar, w);
      glc[i] = gl * fmin(c_bar, w);
    }
#pragma unroll
    for (int i = 0; i < VTRACE_ROWS; ++i) {
      const long long t = hi - 1 - i;
      if (t < 0) continue;                          // the same in every lane
      const double vt = (double)v[i];
      const bool valid = f[i] & GVEC_TRAJ_VALID, term = f[i] & GVEC_TRAJ_TERMINAL, cut = f[i] & GVEC_TRAJ_CUT;
      double a = 0.0, p = 0.0, ro = 0.0;
      if (valid) {
        const double nv = term ? 0.0 : next_v, nvs = term ? 0.0 : (cut ? next_v : next_vs);
        const double delta = rho[i] * ((r[i] + g * nv) - vt);
        a = delta + glc[i] * (cut ? 0.0 : acc);
        p = rho[i] * ((r[i] + g * nvs) - vt);
        ro = rho[i];
      }
      acc = a;                                      // an invalid row clears it
      next_vs = vt + a;
      next_v = vt;
      const float p32 = (float)p, ro32 = (float)ro;
      if (act) {
        vs[t * N + n] = (float)next_vs;
        pg[t * N + n] = p32;
        if (rho_out) rho_out[t * N + n] = ro32;
        if (valid) {                                // the statistics describe pg and rho as stored
          const double x = (double)p32;
          cnt += 1.0;
          s1 += x;
          s2 += x * x;
          s3 += (double)ro32;
        }
      }
    }
  }
  cnt = wave_sum(cnt);                              // fixed butterflies: the same bits on every run
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  s3 = wave_sum(s3);
  if (lane_id() == 0) {
    double* part = static_cast<double*>(A.scratch) + (size_t)blockIdx.x * 4;
    part[0] = cnt;
    part[1] = s1;
    part[2] = s2;
    part[3] = s3;
  }
}

// ---- compaction: the ascending positions of the VALID rows ----
// scratch: cnt[G] valid rows per COMPACT_BLOCK positions, base[G] their exclusive prefix
__host__ __device__ inline long long compact_groups(long long total) { return (total + COMPACT_BLOCK - 1) / COMPACT_BLOCK; }
// thread `tid` of workgroup `blk` owns positions blk * 1024 + k * 256 + tid, k < 4: sub-run q = k * 4 + wave is 64 consecutive positions
__device__ __forceinline__ void compact_ballots(const uint8_t* flags, long long total, long long blk, unsigned long long m[4], int* runs) {
  const int tid = (int)threadIdx.x, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long p = blk * COMPACT_BLOCK + k * 256 + tid;
    const bool v = p < total && (flags[p < total ? p : 0] & GVEC_TRAJ_VALID);
    m[k] = __ballot(v);
    if (lane_id() == 0) runs[k * 4 + wave] = __popcll(m[k]);
  }
  __syncthreads();
}
__global__ __launch_bounds__(256) void traj_compact_count_kernel(gvec_traj_compact_args A) {
  __shared__ int runs[16];
  unsigned long long m[4];
  compact_ballots(A.flags, A.T * A.N, blockIdx.x, m, runs);
  if (threadIdx.x == 0) {
    long long c = 0;
    for (int q = 0; q < 16; ++q) c += runs[q];
    static_cast<long long*>(A.scratch)[blockIdx.x] = c;
  }
}
// one workgroup: exclusive prefix of cnt[G] (a thread owns a run of consecutive groups), and the total
__global__ __launch_bounds__(SCAN_THREADS) void traj_compact_scan_kernel(gvec_traj_compact_args A) {
  __shared__ long long part[1][SCAN_THREADS];
  const long long G = compact_groups(A.T * A.N);
  const long long* cnt = static_cast<const long long*>(A.scratch);
  long long* base = static_cast<long long*>(A.scratch) + G;
  const ScanRun r = scan_run(G);
  long long run[1] = {0};
  for (long long gi = r.lo; gi < r.hi; ++gi) run[0] += cnt[gi];
  block_scan(part, run);
  for (long long gi = r.lo; gi < r.hi; ++gi) {
    base[gi] = run[0];
    run[0] += cnt[gi];
  }
  if (threadIdx.x == SCAN_THREADS - 1) *reinterpret_cast<long long*>(A.count) = part[0][SCAN_THREADS - 1];
}
__global__ __launch_bounds__(256) void traj_compact_write_kernel(gvec_traj_compact_args A) {
  __shared__ int runs[16];
  unsigned long long m[4];
  const long long total = A.T * A.N, G = compact_groups(total);
  compact_ballots(A.flags, total, blockIdx.x, m, runs);
  const long long base = (static_cast<const long long*>(A.scratch) + G)[blockIdx.x];
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  long long* idx = reinterpret_cast<long long*>(A.idx);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int before = 0;
    for (int q = 0; q < k * 4 + wave; ++q) before += runs[q];
    if ((m[k] >> lane_id()) & 1) idx[base + before + __popcll(m[k] & ((1ull << lane_id()) - 1))] = blockIdx.x * (long long)COMPACT_BLOCK + k * 256 + tid;
  }
}

// ---- gather: 1 << shift wavefronts per minibatch row (a row is 9 * W * H floats and 5 * W * H mask bytes: 8,100 and 1,125
// bytes at 15x15, aligned to nothing wider than an element - gvec_rows.hpp) ----
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void traj_gather_kernel(gvec_traj_gather_args A, int shift) {
  const WaveSplit w = wave_split(shift);
  const long long i = w.item;
  if (i >= A.M) return;
  const long long p = uni_ll(A.pos[i]);
  float* dobs = A.out_obs + (size_t)i * A.obs_floats;
  uint8_t* dmask = A.out_mask + (size_t)i * A.mask_bytes;
  const int first = w.first, stride = w.stride;
  if (p < 0 || p >= A.T * A.N) {                   // a position the host never saw: a zeroed row that weighs nothing
    for (int k = first; k < A.obs_floats; k += stride) dobs[k] = 0.0f;
    for (int k = first; k < A.mask_bytes; k += stride) dmask[k] = 0;
    if (first == 0) {
      A.out_action[i] = 0;
      A.out_logp[i] = A.out_value[i] = A.out_ret[i] = A.out_adv[i] = A.out_weight[i] = 0.0f;
      atomicAdd(reinterpret_cast<unsigned long long*>(A.rejected), 1ull);
    }
    return;
  }
  copy_row(A.obs + (size_t)p * A.obs_floats, dobs, A.obs_floats, w);
  if (A.mask_bytes > 0) move_row_u8(A.mask + (size_t)p * A.mask_bytes, dmask, A.mask_bytes, w);
  if (first == 0) {
    A.out_action[i] = A.action[p];
    A.out_logp[i] = A.logp[p];
    A.out_value[i] = A.value[p];
    A.out_ret[i] = A.ret[p];
    float a = A.adv[p];
    if (A.stats) {
      const double c = A.stats[0];
      const double mean = c > 0.0 ? A.stats[1] / c : 0.0;
      double var = c > 0.0 ? A.stats[2] / c - mean * mean : 0.0;
      var = var > 0.0 ? var : 0.0;
      a = (float)(((double)a - mean) / sqrt(var + 1e-8));
    }
    A.out_adv[i] = a;
    A.out_weight[i] = (A.flags[p] & GVEC_TRAJ_VALID) ? 1.0f : 0.0f;
  }
}

}  // namespace

size_t traj_scratch_bytes(long long T, long long N) {
  const size_t gae = (size_t)((N + 63) / 64) * 4 * 8;    // V-trace's four partials per wavefront; GAE uses three
  const size_t compact = (size_t)compact_groups(T * N) * 2 * 8;
  return ((gae > compact ? gae : compact) + 255) / 256 * 256;
}
hipError_t launch_traj_record(const gvec_traj_record_args& a, hipStream_t s) {
  return launch_threads(traj_record_kernel, (long long)a.num_envs * a.num_learners, s, a);
}
hipError_t launch_traj_gae(const gvec_traj_gae_args& a, hipStream_t s) {
  const long long groups = (a.N + 63) / 64;
  hipLaunchKernelGGL(traj_gae_kernel, dim3((unsigned)groups), dim3(64), 0, s, a);
  hipLaunchKernelGGL(traj_stats_kernel<3>, dim3(1), dim3(256), 0, s, static_cast<const double*>(a.scratch), groups, a.stats);
  return hipGetLastError();
}
hipError_t launch_traj_vtrace(const gvec_traj_vtrace_args& a, hipStream_t s) {
  const long long groups = (a.N + 63) / 64;
  hipLaunchKernelGGL(traj_vtrace_kernel, dim3((unsigned)groups), dim3(64), 0, s, a);
  hipLaunchKernelGGL(traj_stats_kernel<4>, dim3(1), dim3(256), 0, s, static_cast<const double*>(a.scratch), groups, a.stats);
  return hipGetLastError();
}
hipError_t launch_traj_compact(const gvec_traj_compact_args& a, hipStream_t s) {
  const dim3 grid((unsigned)compact_groups(a.T * a.N));
  hipLaunchKernelGGL(traj_compact_count_kernel, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(traj_compact_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, a);
  hipLaunchKernelGGL(traj_compact_write_kernel, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_traj_gather(const gvec_traj_gather_args& a, hipStream_t s) {
  const int shift = split_shift(a.M);
  return launch_waves(traj_gather_kernel, a.M << shift, s, a, shift);
}

}  // namespace gvec
