// gvec_policy.hip — the masked-categorical policy head of on-device PPO: sample (Gumbel-max or greedy), evaluate and
// backward over rows of A float32 logits + A mask bytes (gvec_policy_* in generals_vec.h), and the
// distillation loss of the same rows against a search's soft target, forward and backward (gvec_policy_distill*; §4.23).
//
// One wavefront per row, one row per workgroup.  A row of A <= POLICY_STAGE_MAX is read from HBM once: the masked logits
// x_i = mask_i ? l_i : -inf go to LDS (16 bytes per lane where the row allows it) and every later pass reads LDS.  S, the set
// the formulas run over, is {i : x_i > -inf}, so the mask needs no second copy.  Every reduction is lane-strided partial
// results in ascending i, then a fixed xor butterfly: the same input gives the same bits, whatever the row's alignment.
#include <math.h>

#include "gvec_launch.hpp"

namespace gvec {

namespace {

constexpr int POLICY_STAGE_MAX = 5 * 32 * 32;   // the largest board the engine deals: 20.5 KB of LDS per row

// ---- the draws (DESIGN.md §6 "Policy head") ----
__host__ __device__ __forceinline__ uint32_t policy_row_key(uint32_t base, long long row) {
  const uint32_t lo = (uint32_t)(unsigned long long)row, hi = (uint32_t)((unsigned long long)row >> 32);
  return fmix32(env_key_of(base, lo) ^ (hi * 0x9E3779B1u) ^ 0x68E31DA4u);
}
// g = -log(-log u), u = (k + 0.5) * 2^-24, k the hash's top 24 bits.  k + 0.5 has 25 significant bits once k >= 2^23: there
// 1 - u = (2^24 - k - 0.5) * 2^-24 is the exact float32 and -log u = -log1p(-(1 - u)), so no draw is rounded before its log.
__device__ __forceinline__ float policy_gumbel(uint32_t row_key, uint32_t i) {
  const uint32_t k = fmix32(row_key + i * 0x9E3779B9u) >> 8;
  float e;
  if (k < (1u << 23)) {
    e = -logf(((float)k + 0.5f) * 0x1p-24f);
  } else {
    e = -log1pf(-(((float)((1u << 24) - k) - 0.5f) * 0x1p-24f));
  }
  return -logf(e);
}

// ---- a row: staged in LDS, or (A > POLICY_STAGE_MAX) read from HBM again by every pass ----
template <bool STAGED>
struct Row {
  const float* x;        // STAGED: the masked logits in LDS
  const float* l;
  const uint8_t* k;
  __device__ __forceinline__ float operator()(int i) const {
    if (STAGED) return x[i];
    return k[i] ? l[i] : NEG_INF;
  }
};

// floats before p is 16-byte aligned (at most n), and the whole quads that follow
__device__ __forceinline__ void quad_split(const float* p, int n, int& head, int& quads) {
  const int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  head = h < n ? h : n;
  quads = (n - head) >> 2;
}

extern __shared__ float4 policy_lds[];

// Element i lands at LDS float i + pad, pad chosen so that the row's first 16-byte-aligned quad in HBM is a 16-byte-aligned
// quad in LDS too.  The mask of a quad is four bytes at any address: one unaligned dword load.
template <bool STAGED>
__device__ __forceinline__ Row<STAGED> open_row(const float* __restrict__ l, const uint8_t* __restrict__ k, int A) {
  Row<STAGED> row{nullptr, l, k};
  if (!STAGED) return row;
  int head, quads;
  quad_split(l, A, head, quads);
  const int pad = (4 - head) & 3;
  float* x = reinterpret_cast<float*>(policy_lds) + pad;
  const float4* __restrict__ lq = reinterpret_cast<const float4*>(l + head);
  float4* xq = reinterpret_cast<float4*>(x + head);
#pragma unroll 4
  for (int j = lane_id(); j < quads; j += 64) {
    float4 v = lq[j];
    uint32_t mb;
    __builtin_memcpy(&mb, k + head + 4 * j, 4);
    v.x = (mb & 0x000000FFu) ? v.x : NEG_INF;
    v.y = (mb & 0x0000FF00u) ? v.y : NEG_INF;
    v.z = (mb & 0x00FF0000u) ? v.z : NEG_INF;
    v.w = (mb & 0xFF000000u) ? v.w : NEG_INF;
    xq[j] = v;
  }
  const int i0 = lane_id();                       // head: at most three floats
  if (i0 < head) x[i0] = k[i0] ? l[i0] : NEG_INF;
  const int i1 = head + 4 * quads + lane_id();    // tail: at most three floats
  if (i1 < A) x[i1] = k[i1] ? l[i1] : NEG_INF;
  __syncthreads();
  row.x = x;
  return row;
}

struct RowStats {
  float m, logz, ent;    // ent = H
  bool dead;
};
// Z = sum exp(x - m), W = sum exp(x - m) * (x - m); log Z and H = log Z - W / Z (both terms >= 0: nothing cancels).
// |S| = 1 gives Z = 1, W = 0: log Z = 0 and H = 0 exactly.
template <bool STAGED>
__device__ __forceinline__ RowStats row_stats(const Row<STAGED>& row, int A, float m) {
  RowStats s{m, 0.0f, 0.0f, !(m > NEG_INF)};
  if (s.dead) return s;
  float z = 0.0f, w = 0.0f;
  for (int i = lane_id(); i < A; i += 64) {
    const float d = row(i) - m;
    if (d > NEG_INF) {
      const float e = expf(d);
      z = z + e;
      w = w + e * d;
    }
  }
  z = wave_sum(z);
  w = wave_sum(w);
  s.logz = logf(z);
  s.ent = s.logz - w / z;
  return s;
}
template <bool STAGED>
__device__ __forceinline__ float row_max(const Row<STAGED>& row, int A) {
  float m = NEG_INF;
  for (int i = lane_id(); i < A; i += 64) {
    const float v = row(i);
    m = v > m ? v : m;
  }
  return wave_max(m);
}
// the action's masked logit, or -inf when it is out of range
template <bool STAGED>
__device__ __forceinline__ float action_logit(const Row<STAGED>& row, int A, long long a) {
  const bool in_range = a >= 0 && a < A;
  const float v = row(in_range ? (int)a : 0);
  return in_range ? v : NEG_INF;
}

template <bool STAGED>
__global__ __launch_bounds__(64) void policy_sample_kernel(gvec_policy_sample_args P, uint32_t key_base) {
  const long long r = blockIdx.x;
  const int A = P.num_actions;
  const Row<STAGED> row = open_row<STAGED>(P.logits + (size_t)r * A, P.mask + (size_t)r * A, A);
  const uint32_t rk = policy_row_key(key_base, P.row_base + r);
  float m = NEG_INF, best = NEG_INF;
  int pick = NO_INDEX;
  for (int i = lane_id(); i < A; i += 64) {
    const float v = row(i);
    if (v > NEG_INF) {                         // i in S: only these cost a draw
      m = v > m ? v : m;
      const float key = P.greedy ? v : v + policy_gumbel(rk, (uint32_t)i);
      if (key > best || pick == NO_INDEX) {
        best = key;
        pick = i;
      }
    }
  }
  m = wave_max(m);
  wave_argmax(best, pick);
  const RowStats s = row_stats(row, A, m);
  if (lane_id() == 0) {
    const float lp = s.dead ? 0.0f : (row(s.dead ? 0 : pick) - m) - s.logz;
    P.action[r] = s.dead ? 0 : pick;
    P.logp[r] = lp;
    P.entropy[r] = s.ent;
  }
}

template <bool STAGED>
__global__ __launch_bounds__(64) void policy_evaluate_kernel(gvec_policy_evaluate_args P) {
  const long long r = blockIdx.x;
  const int A = P.num_actions;
  const Row<STAGED> row = open_row<STAGED>(P.logits + (size_t)r * A, P.mask + (size_t)r * A, A);
  const RowStats s = row_stats(row, A, row_max(row, A));
  if (lane_id() == 0) {
    const float xa = action_logit(row, A, P.action[r]);
    const bool ok = xa > NEG_INF;              // on a dead row no action is legal and none is counted
    P.logp[r] = ok ? (xa - s.m) - s.logz : 0.0f;
    P.entropy[r] = s.ent;
    if (!ok && !s.dead && P.bad_actions) atomicAdd(reinterpret_cast<unsigned long long*>(P.bad_actions), 1ull);
  }
}

template <bool STAGED>
__device__ __forceinline__ float grad_of(const Row<STAGED>& row, const RowStats& s, int i, int a, float gl, float ge) {
  const float v = row(i);
  if (s.dead || !(v > NEG_INF)) return 0.0f;
  const float lp = (v - s.m) - s.logz, p = expf(lp);
  return gl * ((i == a ? 1.0f : 0.0f) - p) - (ge * p) * (lp + s.ent);
}
template <bool STAGED>
__global__ __launch_bounds__(64) void policy_backward_kernel(gvec_policy_backward_args P) {
  const long long r = blockIdx.x;
  const int A = P.num_actions;
  const Row<STAGED> row = open_row<STAGED>(P.logits + (size_t)r * A, P.mask + (size_t)r * A, A);
  const RowStats s = row_stats(row, A, row_max(row, A));
  const long long a64 = P.action[r];
  const bool ok = action_logit(row, A, a64) > NEG_INF;
  const int a = ok ? (int)a64 : -1;            // an action outside S has logp 0: a constant
  const float gl = (ok && P.grad_logp) ? P.grad_logp[r] : 0.0f;
  const float ge = P.grad_entropy ? P.grad_entropy[r] : 0.0f;
  float* __restrict__ g = P.grad_logits + (size_t)r * A;
  int head, quads;
  quad_split(g, A, head, quads);
  float4* gq = reinterpret_cast<float4*>(g + head);
  for (int j = lane_id(); j < quads; j += 64) {
    const int i = head + 4 * j;
    gq[j] = make_float4(grad_of(row, s, i, a, gl, ge), grad_of(row, s, i + 1, a, gl, ge), grad_of(row, s, i + 2, a, gl, ge),
                        grad_of(row, s, i + 3, a, gl, ge));
  }
  const int i0 = lane_id();
  if (i0 < head) g[i0] = grad_of(row, s, i0, a, gl, ge);
  const int i1 = head + 4 * quads + lane_id();
  if (i1 < A) g[i1] = grad_of(row, s, i1, a, gl, ge);
}

inline size_t policy_lds_bytes(int A) { return A <= POLICY_STAGE_MAX ? (size_t)((A + 3 + 3) / 4) * 16 : 0; }

// ---- distillation against a soft target (generals_vec.h "policy distillation") ----
// The target row, raw: staged behind the logits' LDS image (a second image of policy_lds_bytes(A), its own pad: the target's
// alignment need not be the logits'), or read from HBM again by every pass.  tau_i is formed where it is used, from x_i and t_i.
template <bool STAGED>
struct Target {
  const float* t;        // STAGED: LDS
  __device__ __forceinline__ float operator()(int i, float x) const {
    const float v = t[i];
    return (x > NEG_INF && v > 0.0f) ? v : 0.0f;    // NaN > 0 is false: dropped with the negatives
  }
};
// Issues the target's loads; the barrier of the open_row that follows publishes them along with the logits.
template <bool STAGED>
__device__ __forceinline__ Target<STAGED> open_target(const float* __restrict__ t, int A, int lds_quads) {
  if (!STAGED) return Target<STAGED>{t};
  int head, quads;
  quad_split(t, A, head, quads);
  const int pad = (4 - head) & 3;
  float* x = reinterpret_cast<float*>(policy_lds + lds_quads) + pad;
  const float4* __restrict__ tq = reinterpret_cast<const float4*>(t + head);
  float4* xq = reinterpret_cast<float4*>(x + head);
#pragma unroll 4
  for (int j = lane_id(); j < quads; j += 64) xq[j] = tq[j];
  const int i0 = lane_id();
  if (i0 < head) x[i0] = t[i0];
  const int i1 = head + 4 * quads + lane_id();
  if (i1 < A) x[i1] = t[i1];
  return Target<STAGED>{x};
}

template <bool STAGED>
__global__ __launch_bounds__(64) void policy_distill_kernel(gvec_policy_distill_args P, int lds_quads) {
  const long long r = blockIdx.x;
  const int A = P.num_actions;
  const Target<STAGED> tau = open_target<STAGED>(P.target + (size_t)r * A, A, lds_quads);
  const Row<STAGED> row = open_row<STAGED>(P.logits + (size_t)r * A, P.mask + (size_t)r * A, A);
  const RowStats s = row_stats(row, A, row_max(row, A));
  float c = 0.0f, k = 0.0f;
  if (!s.dead) {
    for (int i = lane_id(); i < A; i += 64) {
      const float v = row(i), t = tau(i, v);
      if (t > 0.0f) {
        const float lp = (v - s.m) - s.logz;
        c = c + t * lp;
        k = k + t * (logf(t) - lp);
      }
    }
  }
  c = wave_sum(c);
  k = wave_sum(k);
  if (lane_id() == 0) {
    P.ce[r] = s.dead ? 0.0f : -c;              // one-hot: c is that action's logp, summed with zeros
    P.kl[r] = s.dead ? 0.0f : k;
    P.entropy[r] = s.ent;
  }
}

template <bool STAGED>
__device__ __forceinline__ float distill_grad_of(const Row<STAGED>& row, const Target<STAGED>& tau, const RowStats& s, int i, float g,
                                                 float tsum, float ge) {
  const float v = row(i);
  if (s.dead || !(v > NEG_INF)) return 0.0f;
  const float lp = (v - s.m) - s.logz, p = expf(lp);
  return g * (tsum * p - tau(i, v)) - (ge * p) * (lp + s.ent);
}
template <bool STAGED>
__global__ __launch_bounds__(64) void policy_distill_backward_kernel(gvec_policy_distill_backward_args P, int lds_quads) {
  const long long r = blockIdx.x;
  const int A = P.num_actions;
  const Target<STAGED> tau = open_target<STAGED>(P.target + (size_t)r * A, A, lds_quads);
  const Row<STAGED> row = open_row<STAGED>(P.logits + (size_t)r * A, P.mask + (size_t)r * A, A);
  const RowStats s = row_stats(row, A, row_max(row, A));
  float tsum = 0.0f;
  if (!s.dead) {
    for (int i = lane_id(); i < A; i += 64) tsum = tsum + tau(i, row(i));
  }
  tsum = wave_sum(tsum);
  const float g = (P.grad_ce ? P.grad_ce[r] : 0.0f) + (P.grad_kl ? P.grad_kl[r] : 0.0f);
  const float ge = P.grad_entropy ? P.grad_entropy[r] : 0.0f;
  float* __restrict__ out = P.grad_logits + (size_t)r * A;
  int head, quads;
  quad_split(out, A, head, quads);
  float4* oq = reinterpret_cast<float4*>(out + head);
  for (int j = lane_id(); j < quads; j += 64) {
    const int i = head + 4 * j;
    oq[j] = make_float4(distill_grad_of(row, tau, s, i, g, tsum, ge), distill_grad_of(row, tau, s, i + 1, g, tsum, ge),
                        distill_grad_of(row, tau, s, i + 2, g, tsum, ge), distill_grad_of(row, tau, s, i + 3, g, tsum, ge));
  }
  const int i0 = lane_id();
  if (i0 < head) out[i0] = distill_grad_of(row, tau, s, i0, g, tsum, ge);
  const int i1 = head + 4 * quads + lane_id();
  if (i1 < A) out[i1] = distill_grad_of(row, tau, s, i1, g, tsum, ge);
}

}  // namespace

hipError_t launch_policy_sample(const gvec_policy_sample_args& a, hipStream_t s) {
  const uint32_t base = env_key_base((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  const dim3 grid((unsigned)a.rows);
  if (a.num_actions <= POLICY_STAGE_MAX) {
    hipLaunchKernelGGL(policy_sample_kernel<true>, grid, dim3(64), policy_lds_bytes(a.num_actions), s, a, base);
  } else {
    hipLaunchKernelGGL(policy_sample_kernel<false>, grid, dim3(64), 0, s, a, base);
  }
  return hipGetLastError();
}
hipError_t launch_policy_evaluate(const gvec_policy_evaluate_args& a, hipStream_t s) {
  const dim3 grid((unsigned)a.rows);
  if (a.num_actions <= POLICY_STAGE_MAX) {
    hipLaunchKernelGGL(policy_evaluate_kernel<true>, grid, dim3(64), policy_lds_bytes(a.num_actions), s, a);
  } else {
    hipLaunchKernelGGL(policy_evaluate_kernel<false>, grid, dim3(64), 0, s, a);
  }
  return hipGetLastError();
}
hipError_t launch_policy_backward(const gvec_policy_backward_args& a, hipStream_t s) {
  const dim3 grid((unsigned)a.rows);
  if (a.num_actions <= POLICY_STAGE_MAX) {
    hipLaunchKernelGGL(policy_backward_kernel<true>, grid, dim3(64), policy_lds_bytes(a.num_actions), s, a);
  } else {
    hipLaunchKernelGGL(policy_backward_kernel<false>, grid, dim3(64), 0, s, a);
  }
  return hipGetLastError();
}
// two LDS images per row, logits then target: 41 KB at A = 5120, under the 64 KB a launch may ask for without an attribute
hipError_t launch_policy_distill(const gvec_policy_distill_args& a, hipStream_t s) {
  const dim3 grid((unsigned)a.rows);
  const size_t image = policy_lds_bytes(a.num_actions);
  if (a.num_actions <= POLICY_STAGE_MAX) {
    hipLaunchKernelGGL(policy_distill_kernel<true>, grid, dim3(64), 2 * image, s, a, (int)(image / 16));
  } else {
    hipLaunchKernelGGL(policy_distill_kernel<false>, grid, dim3(64), 0, s, a, 0);
  }
  return hipGetLastError();
}
hipError_t launch_policy_distill_backward(const gvec_policy_distill_backward_args& a, hipStream_t s) {
  const dim3 grid((unsigned)a.rows);
  const size_t image = policy_lds_bytes(a.num_actions);
  if (a.num_actions <= POLICY_STAGE_MAX) {
    hipLaunchKernelGGL(policy_distill_backward_kernel<true>, grid, dim3(64), 2 * image, s, a, (int)(image / 16));
  } else {
    hipLaunchKernelGGL(policy_distill_backward_kernel<false>, grid, dim3(64), 0, s, a, 0);
  }
  return hipGetLastError();
}

}  // namespace gvec
