// gvec_api_obs.hip — the entry points that read a batch of nine-plane observations: the strategic feature planes, the
// fog-of-war memory planes and the masked Q targets.  Handle-free like gvec_api_replay.hip's: they check their arguments,
// which needs no device, and end in ON_DEVICE.  Host only (gvec_handle.hpp); the kernels are in gvec_features.hip,
// gvec_memory.hip and gvec_qtarget.hip.
#include <cmath>

#include "gvec_handle.hpp"

namespace {

// what every argument struct here starts with; each entry point calls these in its own order
template <typename A>
int32_t check_rows_and_board(const char* fn, const A* a) {
  if (a->rows < 0 || a->rows > 0x7FFFFFFFll) {
    set_err("%s: rows %lld outside [0, 2^31)", fn, (long long)a->rows);
    return GVEC_E_INVALID;
  }
  if (a->width < 1 || a->width > GVEC_MAX_DIM || a->height < 1 || a->height > GVEC_MAX_DIM) {
    set_err("%s: width %d or height %d outside [1, %d]", fn, a->width, a->height, GVEC_MAX_DIM);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

template <typename A>
int32_t check_cap(const char* fn, const A* a) {
  if (a->cap < 2 || a->cap > 1024 || (a->cap & (a->cap - 1)) != 0) {
    set_err("%s: cap %d is not a power of two in [2, 1024]", fn, a->cap);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

template <typename A>
int32_t check_row_stride(const char* fn, const A* a) {
  if (a->obs_row_stride < (int64_t)9 * a->width * a->height) {
    set_err("%s: obs_row_stride %lld < 9 * width * height = %d", fn, (long long)a->obs_row_stride, 9 * a->width * a->height);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

}  // namespace

extern "C" {

// ---- strategic feature planes ----
int32_t gvec_obs_features(int32_t device, void* hip_stream, const gvec_obs_features_args* a) {
  if (!a) return null_args("gvec_obs_features");
  RET_IF(check_rows_and_board("gvec_obs_features", a));
  RET_IF(check_cap("gvec_obs_features", a));
  if (a->reserved != 0) {
    set_err("gvec_obs_features: reserved %d must be 0", a->reserved);
    return GVEC_E_INVALID;
  }
  RET_IF(check_row_stride("gvec_obs_features", a));
  if (!a->obs || !a->out) return null_args("gvec_obs_features");
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_obs_features(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

// ---- fog-of-war memory planes ----
int32_t gvec_obs_memory_update(int32_t device, void* hip_stream, const gvec_obs_memory_args* a) {
  if (!a) return null_args("gvec_obs_memory_update");
  RET_IF(check_rows_and_board("gvec_obs_memory_update", a));
  RET_IF(check_cap("gvec_obs_memory_update", a));
  if (a->rows_per_flag < 1 || a->rows % a->rows_per_flag != 0) {
    set_err("gvec_obs_memory_update: rows_per_flag %d is not a divisor >= 1 of rows %lld", a->rows_per_flag, (long long)a->rows);
    return GVEC_E_INVALID;
  }
  RET_IF(check_row_stride("gvec_obs_memory_update", a));
  if (!a->obs || !a->out) return null_args("gvec_obs_memory_update");
  if (a->prev && a->prev != a->out) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a->prev), o = reinterpret_cast<uintptr_t>(a->out);
    const uintptr_t bytes = (uintptr_t)a->rows * 4u * (uintptr_t)(a->width * a->height) * sizeof(float);
    if (p < o + bytes && o < p + bytes) {
      set_err("gvec_obs_memory_update: prev overlaps out without being equal to it (in place means prev == out)");
      return GVEC_E_INVALID;
    }
  }
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_obs_memory(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

// ---- masked Q targets ----
int32_t gvec_obs_valid_mask(int32_t device, void* hip_stream, const gvec_obs_valid_mask_args* a) {
  if (!a) return null_args("gvec_obs_valid_mask");
  RET_IF(check_rows_and_board("gvec_obs_valid_mask", a));
  RET_IF(check_row_stride("gvec_obs_valid_mask", a));
  if (!a->obs || !a->mask) return null_args("gvec_obs_valid_mask");
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_obs_valid_mask(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_q_target(int32_t device, void* hip_stream, const gvec_q_target_args* a) {
  if (!a) return null_args("gvec_q_target");
  RET_IF(check_rows_and_board("gvec_q_target", a));
  RET_IF(check_row_stride("gvec_q_target", a));
  if (a->reserved != 0) {
    set_err("gvec_q_target: reserved %d must be 0", a->reserved);
    return GVEC_E_INVALID;
  }
  if (!a->next_obs || !a->q_eval || !a->reward || !a->done || !a->target || !a->next_action) return null_args("gvec_q_target");
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_q_target(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_categorical_target(int32_t device, void* hip_stream, const gvec_categorical_target_args* a) {
  if (!a) return null_args("gvec_categorical_target");
  RET_IF(check_rows_and_board("gvec_categorical_target", a));
  RET_IF(check_row_stride("gvec_categorical_target", a));
  if (a->num_atoms < 2 || a->num_atoms > 64) {
    set_err("gvec_categorical_target: num_atoms %d outside [2, 64]", a->num_atoms);
    return GVEC_E_INVALID;
  }
  if (!std::isfinite(a->v_min) || !std::isfinite(a->v_max) || !(a->v_min < a->v_max)) {
    set_err("gvec_categorical_target: v_min %g and v_max %g must be finite with v_min < v_max", (double)a->v_min, (double)a->v_max);
    return GVEC_E_INVALID;
  }
  if (!a->next_obs || !a->logits_eval || !a->reward || !a->done || !a->m || !a->next_action) return null_args("gvec_categorical_target");
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_categorical_target(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

}  // extern "C"
