// gvec_api_obs.hip — the entry points that read a batch of nine-plane observations: the strategic feature planes, the
// fog-of-war memory planes, the masked Q targets, the board symmetries and the match arena's tally (which reads one when it
// is given one).  Handle-free like gvec_api_replay.hip's: they check their arguments, which needs no device, and end in
// ON_DEVICE.  Host only (gvec_handle.hpp); the kernels are in gvec_features.hip, gvec_memory.hip, gvec_qtarget.hip,
// gvec_symmetry.hip and gvec_arena.hip.
#include <cmath>

#include "gvec_handle.hpp"

namespace {

// what every argument struct here starts with; each entry point calls these in its own order
template <typename A>
int32_t check_rows(const char* fn, const A* a) {
  if (a->rows < 0 || a->rows > 0x7FFFFFFFll) {
    set_err("%s: rows %lld outside [0, 2^31)", fn, (long long)a->rows);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

template <typename A>
int32_t check_rows_and_board(const char* fn, const A* a) {
  RET_IF(check_rows(fn, a));
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

// ---- board symmetries ----
int32_t gvec_obs_symmetry(int32_t device, void* hip_stream, const gvec_obs_symmetry_args* a) {
  const char* fn = "gvec_obs_symmetry";
  if (!a) return null_args(fn);
  RET_IF(check_rows_and_board(fn, a));
  if (a->num_sets < 0 || a->num_sets > GVEC_SYM_MAX_PLANE_SETS) {
    set_err("%s: num_sets %d outside [0, %d]", fn, a->num_sets, GVEC_SYM_MAX_PLANE_SETS);
    return GVEC_E_INVALID;
  }
  if (a->inverse != 0 && a->inverse != 1) {
    set_err("%s: inverse %d is neither 0 nor 1", fn, a->inverse);
    return GVEC_E_INVALID;
  }
  if (a->reserved != 0) {
    set_err("%s: reserved %d must be 0", fn, a->reserved);
    return GVEC_E_INVALID;
  }
  // what the launch reads and what it writes, as byte ranges (empty when rows == 0)
  struct Range {
    uintptr_t lo, hi;
    const char* name;
  };
  Range ins[GVEC_SYM_MAX_PLANE_SETS + 4], outs[GVEC_SYM_MAX_PLANE_SETS + 4];
  int n_in = 0, n_out = 0;
  const uintptr_t rows = (uintptr_t)a->rows, HW = (uintptr_t)(a->width * a->height), A = 5u * HW;
  auto range = [&](const void* p, uintptr_t row_bytes, uintptr_t stride_bytes, const char* name) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return Range{lo, rows ? lo + (rows - 1) * stride_bytes + row_bytes : lo, name};
  };
  static const char* const set_in[] = {"sets[0].in", "sets[1].in", "sets[2].in", "sets[3].in"};
  static const char* const set_out[] = {"sets[0].out", "sets[1].out", "sets[2].out", "sets[3].out"};
  for (int k = 0; k < a->num_sets; ++k) {
    const gvec_sym_plane_set& s = a->sets[k];
    if (s.planes < 1 || s.planes > 64) {
      set_err("%s: sets[%d].planes %d outside [1, 64]", fn, k, s.planes);
      return GVEC_E_INVALID;
    }
    const uintptr_t row = (uintptr_t)s.planes * HW;
    if (s.in_row_stride < (int64_t)row) {
      set_err("%s: sets[%d].in_row_stride %lld < planes * width * height = %lld", fn, k, (long long)s.in_row_stride, (long long)row);
      return GVEC_E_INVALID;
    }
    if (!s.in || !s.out) return null_args(fn);
    ins[n_in++] = range(s.in, row * sizeof(float), (uintptr_t)s.in_row_stride * sizeof(float), set_in[k]);
    outs[n_out++] = range(s.out, row * sizeof(float), row * sizeof(float), set_out[k]);
  }
  if (!a->sym || !a->mask_in != !a->mask_out || !a->values_in != !a->values_out || !a->action_in != !a->action_out) return null_args(fn);
  if (a->num_sets == 0 && !a->mask_in && !a->values_in && !a->action_in) {
    set_err("%s: nothing to transform (no plane set, mask, values or action)", fn);
    return GVEC_E_INVALID;
  }
  ins[n_in++] = range(a->sym, 1, 1, "sym");
  if (a->mask_in) ins[n_in++] = range(a->mask_in, A, A, "mask_in"), outs[n_out++] = range(a->mask_out, A, A, "mask_out");
  if (a->values_in) {
    ins[n_in++] = range(a->values_in, A * sizeof(float), A * sizeof(float), "values_in");
    outs[n_out++] = range(a->values_out, A * sizeof(float), A * sizeof(float), "values_out");
  }
  if (a->action_in) ins[n_in++] = range(a->action_in, 8, 8, "action_in"), outs[n_out++] = range(a->action_out, 8, 8, "action_out");
  if (a->applied) outs[n_out++] = range(a->applied, 1, 1, "applied");
  for (int o = 0; o < n_out; ++o)
    for (int i = 0; i < n_in; ++i)
      if (outs[o].lo < ins[i].hi && ins[i].lo < outs[o].hi) {
        set_err("%s: output %s overlaps input %s (the transform is not in place)", fn, outs[o].name, ins[i].name);
        return GVEC_E_INVALID;
      }
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_obs_symmetry(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

// ---- match arena ----
int32_t gvec_arena_update(int32_t device, void* hip_stream, const gvec_arena_args* a) {
  const char* fn = "gvec_arena_update";
  if (!a) return null_args(fn);
  if (a->obs) {   // the board is read with an observation only
    RET_IF(check_rows_and_board(fn, a));
    RET_IF(check_row_stride(fn, a));
  } else {
    RET_IF(check_rows(fn, a));
  }
  if (a->num_learners < 1 || a->num_learners > GVEC_MAX_PLAYERS) {
    set_err("%s: num_learners %d outside [1, %d]", fn, a->num_learners, GVEC_MAX_PLAYERS);
    return GVEC_E_INVALID;
  }
  if (a->games_cap < 0) {
    set_err("%s: games_cap %d is negative (0 means no cap)", fn, a->games_cap);
    return GVEC_E_INVALID;
  }
  if (!a->terminated || !a->truncated || !a->winner || !a->reward || !a->player_ids) return null_args(fn);
  if (!a->death || !a->ep_len || !a->ep_return || !a->games || !a->wins || !a->eliminated || !a->len_sum || !a->ret_sum || !a->pair2)
    return null_args(fn);
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_arena_update(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

}  // extern "C"
