// gvec_api_replay.hip — the entry points that take no handle, only a device, a stream and device arrays: the replay ring's
// collect, prioritized replay, n-step returns, on-policy rollouts and the policy head.  Each checks its arguments, which
// needs no device, and ends in ON_DEVICE.  Host only (gvec_handle.hpp); the kernels are in gvec_stream.hip and their own units.
#include "gvec_handle.hpp"

// ---- prioritized replay (gvec_per.hip) ----
static constexpr int64_t PER_MAX_CAPACITY = (int64_t)1 << 36;   // six levels above the leaves: PerLayout::off holds them
static int32_t per_check(const char* fn, const void* tree, int64_t capacity) {
  if (!tree) {
    set_err("%s: tree is NULL", fn);
    return GVEC_E_INVALID;
  }
  if (capacity < 1 || capacity > PER_MAX_CAPACITY) {
    set_err("%s: capacity %lld outside [1, 2^36]", fn, (long long)capacity);
    return GVEC_E_INVALID;
  }
  if (reinterpret_cast<uintptr_t>(tree) & 255) {
    set_err("%s: tree must be 256-byte aligned (a node's 64 children are one 256-byte read)", fn);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

// ---- on-policy rollouts (gvec_traj.hip) ----
static int32_t traj_shape(const char* fn, int64_t T, int64_t N) {
  if (T < 1 || N < 1 || T > ((int64_t)1 << 40) / N) {
    set_err("%s: T %lld, N %lld: both must be >= 1 (and T * N <= 2^40)", fn, (long long)T, (long long)N);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

// ---- masked-categorical policy head (gvec_policy.hip) ----
static int32_t policy_shape(const char* fn, int64_t rows, int32_t num_actions, bool null_ptr) {
  if (rows < 0 || rows > 0x7FFFFFFFll || num_actions < 1) {
    set_err("%s: rows %lld outside [0, 2^31) or num_actions %d < 1", fn, (long long)rows, num_actions);
    return GVEC_E_INVALID;
  }
  if (null_ptr) {
    set_err("%s: a required pointer is NULL", fn);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

extern "C" {

uint64_t gvec_pool_collect_scratch_bytes(int32_t num_envs) { return num_envs > 0 ? pool_collect_scratch_bytes(num_envs) : 0; }

int32_t gvec_pool_collect(int32_t device, void* hip_stream, const gvec_collect_args* a) {
  if (!a) return GVEC_E_INVALID;
  if (a->num_envs < 1 || a->obs_floats < 1 || a->max_steps_per_episode < 1 || a->result_capacity < 0 || a->capacity < a->num_envs) {
    set_err("gvec_pool_collect: num_envs %d, obs_floats %d, max_steps_per_episode %d, capacity %lld (a step's transitions must fit: >= num_envs), "
            "result_capacity %lld", a->num_envs, a->obs_floats, a->max_steps_per_episode, (long long)a->capacity, (long long)a->result_capacity);
    return GVEC_E_INVALID;
  }
  if (!a->state || !a->next_state || !a->action || !a->reward || !a->terminated || !a->truncated || !a->was_reset || !a->ring_state ||
      !a->ring_next_state || !a->ring_action || !a->ring_reward || !a->ring_done || !a->ring_counters || !a->episode_reward ||
      !a->episode_length || !a->pool_counters || !a->scratch ||
      (a->result_capacity > 0 && (!a->result_reward || !a->result_length || !a->result_worker))) {
    set_err("gvec_pool_collect: a required pointer is NULL (only needs_reset may be)");
    return GVEC_E_INVALID;
  }
  RET_IF(check_scratch("gvec_pool_collect", a->scratch));
  ON_DEVICE(device, launch_pool_collect(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

uint64_t gvec_per_tree_bytes(int64_t capacity) {
  return capacity >= 1 && capacity <= PER_MAX_CAPACITY ? (uint64_t)per_layout(capacity).total * 4 : 0;
}

int32_t gvec_per_tree_layout(int64_t capacity, int64_t* out10) {
  if (!out10 || capacity < 1 || capacity > PER_MAX_CAPACITY) {
    set_err("gvec_per_tree_layout: capacity %lld outside [1, 2^36] or out is NULL", (long long)capacity);
    return GVEC_E_INVALID;
  }
  const PerLayout y = per_layout(capacity);
  for (int i = 0; i < 10; ++i) out10[i] = 0;
  out10[0] = y.levels;
  out10[1] = y.total;
  for (int l = 0; l <= y.levels; ++l) out10[2 + l] = y.off[l];
  return GVEC_OK;
}

int32_t gvec_per_init(int32_t device, void* hip_stream, void* tree, int64_t capacity) {
  RET_IF(per_check("gvec_per_init", tree, capacity));
  ON_DEVICE(device, launch_per_init(static_cast<float*>(tree), per_layout(capacity), reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_per_push(int32_t device, void* hip_stream, void* tree, int64_t capacity, const int64_t* counters_before,
                      const int64_t* counters_after, int64_t max_count) {
  RET_IF(per_check("gvec_per_push", tree, capacity));
  if (!counters_before || !counters_after || max_count < 1) {
    set_err("gvec_per_push: counters_before / counters_after NULL or max_count %lld < 1", (long long)max_count);
    return GVEC_E_INVALID;
  }
  ON_DEVICE(device, launch_per_push(static_cast<float*>(tree), per_layout(capacity), reinterpret_cast<const long long*>(counters_before),
                                    reinterpret_cast<const long long*>(counters_after), max_count, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_per_update(int32_t device, void* hip_stream, void* tree, int64_t capacity, const int64_t* idx, const float* td_error,
                        int64_t n, float alpha, float eps) {
  RET_IF(per_check("gvec_per_update", tree, capacity));
  if (n < 0 || !(alpha >= 0.0f) || !(eps > 0.0f)) {
    set_err("gvec_per_update: n %lld < 0, alpha %g < 0 or eps %g <= 0", (long long)n, (double)alpha, (double)eps);
    return GVEC_E_INVALID;
  }
  if (n == 0) return GVEC_OK;
  if (!idx || !td_error) {
    set_err("gvec_per_update: idx or td_error is NULL");
    return GVEC_E_INVALID;
  }
  ON_DEVICE(device, launch_per_update(static_cast<float*>(tree), per_layout(capacity), reinterpret_cast<const long long*>(idx), td_error, n, alpha,
                                      eps, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_per_sample(int32_t device, void* hip_stream, void* tree, int64_t capacity, const int64_t* ring_counters, int64_t k,
                        float beta, const double* u, uint64_t seed, int64_t* idx, float* weight) {
  RET_IF(per_check("gvec_per_sample", tree, capacity));
  if (k < 1 || !(beta >= 0.0f)) {
    set_err("gvec_per_sample: k %lld < 1 or beta %g < 0", (long long)k, (double)beta);
    return GVEC_E_INVALID;
  }
  if (!ring_counters || !idx || !weight) {
    set_err("gvec_per_sample: ring_counters, idx or weight is NULL");
    return GVEC_E_INVALID;
  }
  ON_DEVICE(device, launch_per_sample(static_cast<float*>(tree), per_layout(capacity), reinterpret_cast<const long long*>(ring_counters), k, beta,
                                      u, seed, reinterpret_cast<long long*>(idx), weight, reinterpret_cast<hipStream_t>(hip_stream)));
}

// ---- n-step returns over the replay ring (gvec_nstep.hip) ----
int32_t gvec_nstep_link(int32_t device, void* hip_stream, const gvec_collect_args* a, const int64_t* counters_before, int64_t* ring_succ,
                        int64_t* nstep_last) {
  if (!a || !counters_before || !ring_succ || !nstep_last) {
    set_err("gvec_nstep_link: args, counters_before, ring_succ or nstep_last is NULL");
    return GVEC_E_INVALID;
  }
  if (a->capacity < 1 || a->num_envs < 1 || a->num_envs > a->capacity) {
    set_err("gvec_nstep_link: capacity %lld < 1, or num_envs %d outside [1, capacity]", (long long)a->capacity, a->num_envs);
    return GVEC_E_INVALID;
  }
  if (!a->ring_counters || !a->scratch) {
    set_err("gvec_nstep_link: a required pointer of args is NULL (ring_counters, scratch)");
    return GVEC_E_INVALID;
  }
  RET_IF(check_scratch("gvec_nstep_link", a->scratch));
  ON_DEVICE(device, launch_nstep_link(*a, reinterpret_cast<const long long*>(counters_before), reinterpret_cast<long long*>(ring_succ),
                                      reinterpret_cast<long long*>(nstep_last), reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_nstep_gather(int32_t device, void* hip_stream, const gvec_nstep_gather_args* a) {
  if (!a) {
    set_err("gvec_nstep_gather: args is NULL");
    return GVEC_E_INVALID;
  }
  if (a->capacity < 1 || a->k < 0 || a->k > ((int64_t)1 << 28) || a->n_step < 1 || a->obs_floats < 1) {
    set_err("gvec_nstep_gather: capacity %lld < 1, k %lld outside [0, 2^28], n_step %d < 1 or obs_floats %d < 1", (long long)a->capacity,
            (long long)a->k, a->n_step, a->obs_floats);
    return GVEC_E_INVALID;
  }
  if (!(a->gamma >= 0.0) || !(a->gamma <= 1.7976931348623157e308)) {
    set_err("gvec_nstep_gather: gamma %g must be finite and >= 0", a->gamma);
    return GVEC_E_INVALID;
  }
  if (a->n_step > 1 && !a->ring_succ) {
    set_err("gvec_nstep_gather: ring_succ is NULL with n_step %d > 1", a->n_step);
    return GVEC_E_INVALID;
  }
  if (a->k == 0) return GVEC_OK;
  if (!a->idx || !a->ring_state || !a->ring_next_state || !a->ring_action || !a->ring_reward || !a->ring_done || !a->ring_counters ||
      !a->state || !a->next_state || !a->action || !a->ret || !a->discount || !a->done || !a->steps || !a->last_idx) {
    set_err("gvec_nstep_gather: a required pointer is NULL (only ring_succ may be, with n_step == 1)");
    return GVEC_E_INVALID;
  }
  ON_DEVICE(device, launch_nstep_gather(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

uint64_t gvec_traj_scratch_bytes(int64_t T, int64_t N) {
  return traj_shape("gvec_traj_scratch_bytes", T, N) == GVEC_OK ? (uint64_t)traj_scratch_bytes(T, N) : 0;
}

int32_t gvec_traj_record(int32_t device, void* hip_stream, const gvec_traj_record_args* a) {
  if (!a) return null_args("gvec_traj_record");
  if (a->num_envs < 1 || a->num_learners < 1) {
    set_err("gvec_traj_record: num_envs %d, num_learners %d: N = num_envs * num_learners must be >= 1", a->num_envs, a->num_learners);
    return GVEC_E_INVALID;
  }
  RET_IF(traj_shape("gvec_traj_record", a->T, (int64_t)a->num_envs * a->num_learners));
  if (a->t < 0 || a->t >= a->T) {
    set_err("gvec_traj_record: t %lld outside [0, T = %lld)", (long long)a->t, (long long)a->T);
    return GVEC_E_INVALID;
  }
  if (!a->step_action || !a->step_logp || !a->step_value || !a->step_reward || !a->reset || !a->terminated || !a->truncated || !a->alive ||
      !a->alive_state || !a->action || !a->logp || !a->value || !a->reward || !a->flags)
    return null_args("gvec_traj_record");
  ON_DEVICE(device, launch_traj_record(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_traj_gae(int32_t device, void* hip_stream, const gvec_traj_gae_args* a) {
  if (!a) return null_args("gvec_traj_gae");
  RET_IF(traj_shape("gvec_traj_gae", a->T, a->N));
  if (!(a->gamma >= 0.0 && a->gamma <= 1.0) || !(a->lambda >= 0.0 && a->lambda <= 1.0)) {
    set_err("gvec_traj_gae: gamma %g or lambda %g outside [0, 1]", a->gamma, a->lambda);
    return GVEC_E_INVALID;
  }
  if (!a->reward || !a->value || !a->flags || !a->adv || !a->ret || !a->stats || !a->scratch) return null_args("gvec_traj_gae");
  RET_IF(check_scratch("gvec_traj_gae", a->scratch));
  ON_DEVICE(device, launch_traj_gae(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_traj_vtrace(int32_t device, void* hip_stream, const gvec_traj_vtrace_args* a) {
  if (!a) return null_args("gvec_traj_vtrace");
  RET_IF(traj_shape("gvec_traj_vtrace", a->T, a->N));
  if (!(a->gamma >= 0.0 && a->gamma <= 1.0) || !(a->lambda >= 0.0 && a->lambda <= 1.0)) {
    set_err("gvec_traj_vtrace: gamma %g or lambda %g outside [0, 1]", a->gamma, a->lambda);
    return GVEC_E_INVALID;
  }
  if (!(a->rho_bar > 0.0) || !(a->c_bar > 0.0)) {
    set_err("gvec_traj_vtrace: rho_bar %g or c_bar %g not > 0 (+inf means no clipping)", a->rho_bar, a->c_bar);
    return GVEC_E_INVALID;
  }
  if (!a->reward || !a->value || !a->flags || !a->logp_behaviour || !a->logp_target || !a->vs || !a->pg || !a->stats || !a->scratch)
    return null_args("gvec_traj_vtrace");          // rho_out may be NULL
  RET_IF(check_scratch("gvec_traj_vtrace", a->scratch));
  ON_DEVICE(device, launch_traj_vtrace(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_traj_compact(int32_t device, void* hip_stream, const gvec_traj_compact_args* a) {
  if (!a) return null_args("gvec_traj_compact");
  RET_IF(traj_shape("gvec_traj_compact", a->T, a->N));
  if (!a->flags || !a->idx || !a->count || !a->scratch) return null_args("gvec_traj_compact");
  RET_IF(check_scratch("gvec_traj_compact", a->scratch));
  ON_DEVICE(device, launch_traj_compact(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_traj_gather(int32_t device, void* hip_stream, const gvec_traj_gather_args* a) {
  if (!a) return null_args("gvec_traj_gather");
  RET_IF(traj_shape("gvec_traj_gather", a->T, a->N));
  if (a->M < 0 || a->obs_floats < 1 || a->mask_bytes < 0) {
    set_err("gvec_traj_gather: M %lld < 0, obs_floats %d < 1 or mask_bytes %d < 0", (long long)a->M, a->obs_floats, a->mask_bytes);
    return GVEC_E_INVALID;
  }
  if (a->M == 0) return GVEC_OK;
  if (!a->pos || !a->obs || !a->action || !a->logp || !a->value || !a->ret || !a->adv || !a->flags || !a->out_obs || !a->out_action ||
      !a->out_logp || !a->out_value || !a->out_ret || !a->out_adv || !a->out_weight || !a->rejected ||
      (a->mask_bytes > 0 && (!a->mask || !a->out_mask)))
    return null_args("gvec_traj_gather");
  ON_DEVICE(device, launch_traj_gather(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_policy_sample(int32_t device, void* hip_stream, const gvec_policy_sample_args* a) {
  if (!a) return null_args("gvec_policy_sample");
  RET_IF(policy_shape("gvec_policy_sample", a->rows, a->num_actions, !a->logits || !a->mask || !a->action || !a->logp || !a->entropy));
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_policy_sample(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_policy_evaluate(int32_t device, void* hip_stream, const gvec_policy_evaluate_args* a) {
  if (!a) return null_args("gvec_policy_evaluate");
  RET_IF(policy_shape("gvec_policy_evaluate", a->rows, a->num_actions, !a->logits || !a->mask || !a->action || !a->logp || !a->entropy));
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_policy_evaluate(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_policy_backward(int32_t device, void* hip_stream, const gvec_policy_backward_args* a) {
  if (!a) return null_args("gvec_policy_backward");
  RET_IF(policy_shape("gvec_policy_backward", a->rows, a->num_actions, !a->logits || !a->mask || !a->action || !a->grad_logits));
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_policy_backward(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_policy_distill(int32_t device, void* hip_stream, const gvec_policy_distill_args* a) {
  if (!a) return null_args("gvec_policy_distill");
  RET_IF(policy_shape("gvec_policy_distill", a->rows, a->num_actions,
                      a->rows > 0 && (!a->logits || !a->mask || !a->target || !a->ce || !a->kl || !a->entropy)));
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_policy_distill(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_policy_distill_backward(int32_t device, void* hip_stream, const gvec_policy_distill_backward_args* a) {
  if (!a) return null_args("gvec_policy_distill_backward");
  RET_IF(policy_shape("gvec_policy_distill_backward", a->rows, a->num_actions,
                      a->rows > 0 && (!a->logits || !a->mask || !a->target || !a->grad_logits)));
  if (a->rows == 0) return GVEC_OK;
  ON_DEVICE(device, launch_policy_distill_backward(*a, reinterpret_cast<hipStream_t>(hip_stream)));
}

}  // extern "C"
