// gvec_dispatch.hpp — host side of the board-kernel units: the <MAXP, NSLOT> dispatch and what their launchers share.  The
// launch shape (one wavefront per board, WAVES_PER_BLOCK boards per workgroup) is gvec_waves.hpp's.
#pragma once
#include "gvec_launch.hpp"
#include "gvec_waves.hpp"

#include <type_traits>

namespace gvec {

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
