// gvec_api_halving.hip — the entry points of the sequential-halving search (gvec_search_halve, gvec_search_improved_policy;
// generals_vec.h "sequential-halving search").  Handle-free like gvec_api_obs.hip's: they check their arguments, which needs
// no device, and end in ON_DEVICE.  Host only (gvec_handle.hpp); the kernels are in gvec_halving.hip.
#include "gvec_handle.hpp"

namespace {

int32_t check_slots(const char* fn, int32_t n, int32_t m) {
  if (n < 0) {
    set_err("%s: n %d is negative", fn, n);
    return GVEC_E_INVALID;
  }
  if (m < 1 || m > GVEC_SEARCH_MAX_SLOTS) {
    set_err("%s: m %d outside [1, %d]", fn, m, GVEC_SEARCH_MAX_SLOTS);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

}  // namespace

extern "C" {

int32_t gvec_search_halve(int32_t device, void* hip_stream, const gvec_search_halve_args* a) {
  const char* fn = "gvec_search_halve";
  if (!a) return null_args(fn);
  RET_IF(check_slots(fn, a->n, a->m));
  if (a->k < 1 || a->k > a->m || a->k_next < 1 || a->k_next > a->k) {
    set_err("%s: k %d outside [1, m = %d] or k_next %d outside [1, k]", fn, a->k, a->m, a->k_next);
    return GVEC_E_INVALID;
  }
  if (a->replicas < 1) {
    set_err("%s: replicas %d < 1", fn, a->replicas);
    return GVEC_E_INVALID;
  }
  if (a->reserved != 0) {
    set_err("%s: reserved %d must be 0", fn, a->reserved);
    return GVEC_E_INVALID;
  }
  if (!a->slot && a->k != a->m) {
    set_err("%s: slot is NULL (the identity) with k %d != m %d", fn, a->k, a->m);
    return GVEC_E_INVALID;
  }
  if (!a->terms || !a->candidates0 || !a->prior_key || !a->sum || !a->count || !a->next_slot || !a->next_candidates) return null_args(fn);
  if (a->n == 0) return GVEC_OK;
  ON_DEVICE(device, launch_search_halve(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_search_improved_policy(int32_t device, void* hip_stream, const gvec_search_policy_args* a) {
  const char* fn = "gvec_search_improved_policy";
  if (!a) return null_args(fn);
  RET_IF(check_slots(fn, a->n, a->m));
  if (a->num_actions < 1 || a->num_actions > SEARCH_POLICY_MAX_ACTIONS) {
    set_err("%s: num_actions %d outside [1, %d]", fn, a->num_actions, SEARCH_POLICY_MAX_ACTIONS);
    return GVEC_E_INVALID;
  }
  if (a->reserved != 0) {
    set_err("%s: reserved %d must be 0", fn, a->reserved);
    return GVEC_E_INVALID;
  }
  if (!a->mask || !a->candidates0 || !a->sum || !a->count || !a->target || !a->v_mix) return null_args(fn);
  if (a->n == 0) return GVEC_OK;
  ON_DEVICE(device, launch_search_improved_policy(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

}  // extern "C"
