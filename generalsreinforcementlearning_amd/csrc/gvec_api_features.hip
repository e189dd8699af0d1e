// gvec_api_features.hip — the entry point of the strategic feature planes.  Handle-free like gvec_api_replay.hip's: it checks
// its arguments, which needs no device, and ends in ON_DEVICE.  Host only (gvec_handle.hpp); the kernel is in gvec_features.hip.
#include "gvec_handle.hpp"

extern "C" {

int32_t gvec_obs_features(int32_t device, void* hip_stream, const gvec_obs_features_args* a) {
  if (!a) return null_args("gvec_obs_features");
  if (a->rows < 0 || a->rows > 0x7FFFFFFFll) {
    set_err("gvec_obs_features: rows %lld outside [0, 2^31)", (long long)a->rows);
    return GVEC_E_INVALID;
  }
  if (a->width < 1 || a->width > GVEC_MAX_DIM || a->height < 1 || a->height > GVEC_MAX_DIM) {
    set_err("gvec_obs_features: width %d or height %d outside [1, %d]", a->width, a->height, GVEC_MAX_DIM);
    return GVEC_E_INVALID;
  }
  if (a->cap < 2 || a->cap > 1024 || (a->cap & (a->cap - 1)) != 0) {
    set_err("gvec_obs_features: cap %d is not a power of two in [2, 1024]", a->cap);
    return GVEC_E_INVALID;
  }
  if (a->reserved != 0) {
    set_err("gvec_obs_features: reserved %d must be 0", a->reserved);
    return GVEC_E_INVALID;
  }
  if (a->obs_row_stride < (int64_t)9 * a->width * a->height) {
    set_err("gvec_obs_features: obs_row_stride %lld < 9 * width * height = %d", (long long)a->obs_row_stride, 9 * a->width * a->height);
    return GVEC_E_INVALID;
  }
  if (!a->obs || !a->out) return null_args("gvec_obs_features");
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_obs_features(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

}  // extern "C"
