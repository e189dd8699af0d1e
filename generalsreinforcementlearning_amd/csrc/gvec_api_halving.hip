// gvec_api_halving.hip — the entry points of the sequential-halving search (gvec_search_halve, gvec_search_improved_policy;
// generals_vec.h "sequential-halving search") and of the tree below its root (gvec_tree_select, gvec_tree_backup).
// Handle-free like gvec_api_obs.hip's: they check their arguments, which needs no device, and end in ON_DEVICE.  Host only
// (gvec_handle.hpp); the kernels are in gvec_halving.hip and gvec_tree.hip.
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

// ---- the tree below the root (generals_vec.h "tree search below the root"; the kernels are in gvec_tree.hip) ----
static int32_t check_tree(const char* fn, const gvec_tree& t, int32_t k) {
  if (t.n < 0) {
    set_err("%s: n %d is negative", fn, t.n);
    return GVEC_E_INVALID;
  }
  if (t.num_slots < 1 || t.num_slots > GVEC_SEARCH_MAX_SLOTS) {
    set_err("%s: num_slots %d outside [1, %d]", fn, t.num_slots, GVEC_SEARCH_MAX_SLOTS);
    return GVEC_E_INVALID;
  }
  if (k < 1 || k > t.num_slots) {
    set_err("%s: k %d outside [1, num_slots = %d]", fn, k, t.num_slots);
    return GVEC_E_INVALID;
  }
  if (t.nodes < 1 || (long long)t.nodes * t.n >= (1ll << 31) || (long long)t.n * k >= (1ll << 31)) {
    set_err("%s: nodes %d is below 1, or nodes * n or n * k is not below 2^31 (n = %d)", fn, t.nodes, t.n);
    return GVEC_E_INVALID;
  }
  if (t.reserved != 0) {
    set_err("%s: reserved %d must be 0", fn, t.reserved);
    return GVEC_E_INVALID;
  }
  const struct {
    const void* p;
    const char* name;
  } arrays[] = {{t.child_action, "child_action"}, {t.child_logit, "child_logit"}, {t.child_node, "child_node"},
                {t.child_count, "child_count"},   {t.child_sum, "child_sum"},     {t.node_value, "node_value"},
                {t.node_status, "node_status"},   {t.node_parent, "node_parent"}, {t.node_slot, "node_slot"}};
  for (const auto& a : arrays)
    if (!a.p) {
      set_err("%s: %s is NULL", fn, a.name);
      return GVEC_E_INVALID;
    }
  return GVEC_OK;
}

int32_t gvec_tree_select(int32_t device, void* hip_stream, const gvec_tree_select_args* a) {
  const char* fn = "gvec_tree_select";
  if (!a) return null_args(fn);
  RET_IF(check_tree(fn, a->tree, a->k));
  if (a->reserved != 0) {
    set_err("%s: reserved %d must be 0", fn, a->reserved);
    return GVEC_E_INVALID;
  }
  if (!a->slot && a->k != a->tree.num_slots) {
    set_err("%s: slot is NULL (the identity) with k %d != num_slots %d", fn, a->k, a->tree.num_slots);
    return GVEC_E_INVALID;
  }
  if (!a->leaf_node || !a->leaf_slot || !a->leaf_action || !a->leaf_depth) return null_args(fn);
  if (a->tree.n == 0) return GVEC_OK;
  ON_DEVICE(device, launch_tree_select(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_tree_backup(int32_t device, void* hip_stream, const gvec_tree_backup_args* a) {
  const char* fn = "gvec_tree_backup";
  if (!a) return null_args(fn);
  RET_IF(check_tree(fn, a->tree, a->k));
  if (a->replicas < 1) {
    set_err("%s: replicas %d < 1", fn, a->replicas);
    return GVEC_E_INVALID;
  }
  if (!a->leaf_node || !a->leaf_slot || !a->new_node || !a->terms || !a->status) return null_args(fn);
  if (a->tree.n == 0) return GVEC_OK;
  ON_DEVICE(device, launch_tree_backup(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

}  // extern "C"
