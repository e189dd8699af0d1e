// gvec_api_memory.hip — the entry point of the fog-of-war memory planes.  Handle-free like gvec_api_features.hip's: it checks
// its arguments, which needs no device, and ends in ON_DEVICE.  Host only (gvec_handle.hpp); the kernel is in gvec_memory.hip.
#include "gvec_handle.hpp"

extern "C" {

int32_t gvec_obs_memory_update(int32_t device, void* hip_stream, const gvec_obs_memory_args* a) {
  if (!a) return null_args("gvec_obs_memory_update");
  if (a->rows < 0 || a->rows > 0x7FFFFFFFll) {
    set_err("gvec_obs_memory_update: rows %lld outside [0, 2^31)", (long long)a->rows);
    return GVEC_E_INVALID;
  }
  if (a->width < 1 || a->width > GVEC_MAX_DIM || a->height < 1 || a->height > GVEC_MAX_DIM) {
    set_err("gvec_obs_memory_update: width %d or height %d outside [1, %d]", a->width, a->height, GVEC_MAX_DIM);
    return GVEC_E_INVALID;
  }
  if (a->cap < 2 || a->cap > 1024 || (a->cap & (a->cap - 1)) != 0) {
    set_err("gvec_obs_memory_update: cap %d is not a power of two in [2, 1024]", a->cap);
    return GVEC_E_INVALID;
  }
  if (a->rows_per_flag < 1 || a->rows % a->rows_per_flag != 0) {
    set_err("gvec_obs_memory_update: rows_per_flag %d is not a divisor >= 1 of rows %lld", a->rows_per_flag, (long long)a->rows);
    return GVEC_E_INVALID;
  }
  if (a->obs_row_stride < (int64_t)9 * a->width * a->height) {
    set_err("gvec_obs_memory_update: obs_row_stride %lld < 9 * width * height = %d", (long long)a->obs_row_stride,
            9 * a->width * a->height);
    return GVEC_E_INVALID;
  }
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

}  // extern "C"
