// gvec_dispatch.hpp — host side of the board-kernel units: the launch shape (one wavefront per board, WAVES_PER_BLOCK boards
// per workgroup), the <MAXP, NSLOT> dispatch, and what their launchers share.  The only device code is the launch shape's
// other half: which wave of its block a kernel is, and which item it owns.
#pragma once
#include "gvec_launch.hpp"

#include <type_traits>

namespace gvec {

constexpr int WAVES_PER_BLOCK = 4;

// f(MAXP, NSLOT) of the handle's variant, both as std::integral_constant: usable as template arguments
template <typename F>
static hipError_t dispatch(const Variant& v, F&& f) {
#define GVEC_CASE(P_, S_) \
  if (v.maxp == P_ && v.nslot == S_) return f(std::integral_constant<int, P_>{}, std::integral_constant<int, S_>{});
#define GVEC_ROW(P_) GVEC_CASE(P_, 1) GVEC_CASE(P_, 2) GVEC_CASE(P_, 4) GVEC_CASE(P_, 7) GVEC_CASE(P_, 10) GVEC_CASE(P_, 16)
  GVEC_ROW(2) GVEC_ROW(4) GVEC_ROW(8)
#undef GVEC_ROW
#undef GVEC_CASE
  return hipErrorInvalidValue;
}

// device side of launch_waves: this wave's index in its block, and the item it owns (wave-uniform) - none when it is not
// below the launch's n (the spare waves of the last block), and the kernel leaves
__device__ __forceinline__ int block_wave() { return (int)(threadIdx.x >> 6); }
__device__ __forceinline__ int wave_item() { return uni((int)blockIdx.x * WAVES_PER_BLOCK + block_wave()); }

static inline dim3 wave_grid(int n) { return dim3((unsigned)((n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)); }

// kernel k with one wavefront per item, n items
template <typename... P, typename... A>
static hipError_t launch_waves(void (*k)(P...), int n, hipStream_t s, const A&... a) {
  hipLaunchKernelGGL(k, wave_grid(n), dim3(64 * WAVES_PER_BLOCK), 0, s, a...);
  return hipGetLastError();
}

// the resident format keeps planes of 2*S-1 or 2*S dwords (gvec_api.hip: set_geometry), and the kernels that take the plane
// stride as a compile-time constant come in both: 1 for the odd form, 0 for the even one, -1 when a is neither of variant <P, S>
template <int P, int S>
static int plane_parity(const StepArgs& a) {
  using Odd = VariantGeom<P, S, true>;
  using Even = VariantGeom<P, S, false>;
  if (a.fd == Odd::FD && a.row_dw == Odd::ROW_DW) return 1;
  return (a.fd == Even::FD && a.row_dw == Even::ROW_DW) ? 0 : -1;
}

// env_key_of(base, env) = fmix32(base + env * C): a handle that is shard [env_base, env_base + B) of a larger batch
// (gvec_create_sharded) folds its offset into the bases, and its env e then draws exactly what env env_base + e of one
// big handle would - agent moves and pool boards alike; the kernels never see the offset.
static inline StepArgs with_seed_bases(const StepArgs& in) {
  StepArgs a = in;
  a.seed_base = env_key_base(a.seed_lo, a.seed_hi) + (uint32_t)a.env_base * 0xC2B2AE3Du;
  a.pool_seed_base = env_key_base(a.pool_seed_lo, a.pool_seed_hi) + (uint32_t)a.env_base * 0xC2B2AE3Du;
  return a;
}

}  // namespace gvec
