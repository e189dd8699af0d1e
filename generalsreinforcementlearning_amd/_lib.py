"""ctypes binding of libgvec_hip.so (the C ABI of include/generals_vec.h)."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class GvecError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gvec error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("num_envs", C.c_int32), ("max_width", C.c_int32), ("max_height", C.c_int32),
                ("max_players", C.c_int32), ("device", C.c_int32), ("fog_of_war", C.c_int32), ("prod_general", C.c_int32),
                ("prod_city", C.c_int32), ("prod_normal", C.c_int32), ("normal_growth_interval", C.c_int32),
                ("auto_reset", C.c_int32), ("reserved", C.c_int32 * 4)]


STATE_FIELDS = ["army", "owner", "type", "visible", "listed", "changed", "vis_changed", "turn", "done", "winner", "width",
                "height", "players", "alive", "army_count", "tile_count", "general_idx"]


class StateView(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in STATE_FIELDS]


class RolloutStats(C.Structure):
    _fields_ = [("env_steps", C.c_int64), ("aborted_turns", C.c_int64), ("games_finished", C.c_int64), ("reserved", C.c_int64)]


class CollectArgs(C.Structure):
    """gvec_collect_args (include/generals_vec.h): every pointer is device memory."""
    _fields_ = ([(n, C.c_int32) for n in ("num_envs", "obs_floats", "max_steps_per_episode", "reserved")]
                + [(n, C.c_int64) for n in ("capacity", "result_capacity")]
                + [(n, C.c_void_p) for n in ("state", "next_state", "action", "reward", "terminated", "truncated", "was_reset", "needs_reset",
                                             "ring_state", "ring_next_state", "ring_action", "ring_reward", "ring_done", "ring_counters",
                                             "episode_reward", "episode_length", "result_reward", "result_length", "result_worker",
                                             "pool_counters", "scratch")])


class NstepGatherArgs(C.Structure):
    """gvec_nstep_gather_args (include/generals_vec.h): every pointer is device memory."""
    _fields_ = ([("k", C.c_int64), ("capacity", C.c_int64), ("n_step", C.c_int32), ("obs_floats", C.c_int32), ("gamma", C.c_double)]
                + [(n, C.c_void_p) for n in ("idx", "ring_state", "ring_next_state", "ring_action", "ring_reward", "ring_done",
                                             "ring_counters", "ring_succ", "state", "next_state", "action", "ret", "discount", "done",
                                             "steps", "last_idx")])


class TrajRecordArgs(C.Structure):
    """gvec_traj_record_args (include/generals_vec.h): every pointer is device memory."""
    _fields_ = ([("T", C.c_int64), ("t", C.c_int64), ("num_envs", C.c_int32), ("num_learners", C.c_int32)]
                + [(n, C.c_void_p) for n in ("step_action", "step_logp", "step_value", "step_reward", "reset", "terminated", "truncated",
                                             "alive", "alive_state", "action", "logp", "value", "reward", "flags")])


class TrajGaeArgs(C.Structure):
    _fields_ = ([("T", C.c_int64), ("N", C.c_int64), ("gamma", C.c_double), ("lam", C.c_double)]
                + [(n, C.c_void_p) for n in ("reward", "value", "flags", "adv", "ret", "stats", "scratch")])


class TrajVtraceArgs(C.Structure):
    """gvec_traj_vtrace_args (include/generals_vec.h): every pointer is device memory; rho_out may be None."""
    _fields_ = ([("T", C.c_int64), ("N", C.c_int64), ("gamma", C.c_double), ("lam", C.c_double), ("rho_bar", C.c_double), ("c_bar", C.c_double)]
                + [(n, C.c_void_p) for n in ("reward", "value", "flags", "logp_behaviour", "logp_target", "vs", "pg", "rho_out", "stats",
                                             "scratch")])


class TrajCompactArgs(C.Structure):
    _fields_ = [("T", C.c_int64), ("N", C.c_int64)] + [(n, C.c_void_p) for n in ("flags", "idx", "count", "scratch")]


class TrajGatherArgs(C.Structure):
    _fields_ = ([("T", C.c_int64), ("N", C.c_int64), ("M", C.c_int64), ("obs_floats", C.c_int32), ("mask_bytes", C.c_int32)]
                + [(n, C.c_void_p) for n in ("pos", "obs", "mask", "action", "logp", "value", "ret", "adv", "flags", "stats", "out_obs",
                                             "out_mask", "out_action", "out_logp", "out_value", "out_ret", "out_adv", "out_weight",
                                             "rejected")])


class PolicySampleArgs(C.Structure):
    """gvec_policy_sample_args (include/generals_vec.h): every pointer is device memory."""
    _fields_ = ([("rows", C.c_int64), ("num_actions", C.c_int32), ("greedy", C.c_int32), ("seed", C.c_uint64), ("row_base", C.c_int64)]
                + [(n, C.c_void_p) for n in ("logits", "mask", "action", "logp", "entropy")])


class PolicyEvaluateArgs(C.Structure):
    _fields_ = ([("rows", C.c_int64), ("num_actions", C.c_int32), ("reserved", C.c_int32)]
                + [(n, C.c_void_p) for n in ("logits", "mask", "action", "logp", "entropy", "bad_actions")])


class PolicyBackwardArgs(C.Structure):
    _fields_ = ([("rows", C.c_int64), ("num_actions", C.c_int32), ("reserved", C.c_int32)]
                + [(n, C.c_void_p) for n in ("logits", "mask", "action", "grad_logp", "grad_entropy", "grad_logits")])


class PolicyDistillArgs(C.Structure):
    """gvec_policy_distill_args (include/generals_vec.h): every pointer is device memory."""
    _fields_ = ([("rows", C.c_int64), ("num_actions", C.c_int32), ("reserved", C.c_int32)]
                + [(n, C.c_void_p) for n in ("logits", "mask", "target", "ce", "kl", "entropy")])


class PolicyDistillBackwardArgs(C.Structure):
    """gvec_policy_distill_backward_args: grad_ce, grad_kl and grad_entropy may be None (= zeros)."""
    _fields_ = ([("rows", C.c_int64), ("num_actions", C.c_int32), ("reserved", C.c_int32)]
                + [(n, C.c_void_p) for n in ("logits", "mask", "target", "grad_ce", "grad_kl", "grad_entropy", "grad_logits")])


class ObsFeaturesArgs(C.Structure):
    """gvec_obs_features_args (include/generals_vec.h): obs and out are device memory."""
    _fields_ = ([("rows", C.c_int64)] + [(n, C.c_int32) for n in ("width", "height", "cap", "reserved")]
                + [("obs_row_stride", C.c_int64), ("obs", C.c_void_p), ("out", C.c_void_p)])


class ObsMemoryArgs(C.Structure):
    """gvec_obs_memory_args (include/generals_vec.h): obs, prev, reset and out are device memory; prev and reset may be None."""
    _fields_ = ([("rows", C.c_int64)] + [(n, C.c_int32) for n in ("width", "height", "cap", "rows_per_flag")]
                + [("obs_row_stride", C.c_int64)] + [(n, C.c_void_p) for n in ("obs", "prev", "reset", "out")])


class ObsValidMaskArgs(C.Structure):
    """gvec_obs_valid_mask_args (include/generals_vec.h): obs and mask are device memory."""
    _fields_ = [("rows", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("obs_row_stride", C.c_int64), ("obs", C.c_void_p),
                ("mask", C.c_void_p)]


class QTargetArgs(C.Structure):
    """gvec_q_target_args (include/generals_vec.h): every pointer is device memory; q_select, discount and next_value may be None."""
    _fields_ = ([("rows", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("obs_row_stride", C.c_int64), ("gamma", C.c_float),
                 ("reserved", C.c_int32)]
                + [(n, C.c_void_p) for n in ("next_obs", "q_eval", "q_select", "reward", "discount", "done", "target", "next_action",
                                             "next_value")])


class CategoricalTargetArgs(C.Structure):
    """gvec_categorical_target_args (include/generals_vec.h): every pointer is device memory; logits_select and discount may be None."""
    _fields_ = ([("rows", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("obs_row_stride", C.c_int64), ("num_atoms", C.c_int32),
                 ("gamma", C.c_float), ("v_min", C.c_float), ("v_max", C.c_float)]
                + [(n, C.c_void_p) for n in ("next_obs", "logits_eval", "logits_select", "reward", "discount", "done", "m", "next_action")])


class RewardConfigC(C.Structure):
    """gvec_reward_config (include/generals_vec.h); reward.RewardConfig is the Python form."""
    _fields_ = ([(n, C.c_float) for n in ("win_game", "lose_game", "capture_city", "lose_city", "capture_general", "lose_general",
                                          "territory", "army", "army_advantage", "invalid_action")]
                + [("flags", C.c_uint32), ("reserved", C.c_uint32)])


REWARD_CLIP = 1          # GVEC_REWARD_CLIP

SYM_MAX_PLANE_SETS = 4   # GVEC_SYM_MAX_PLANE_SETS


class SymPlaneSet(C.Structure):
    """gvec_sym_plane_set (include/generals_vec.h): in and out are device memory."""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("planes", C.c_int32), ("in_row_stride", C.c_int64)]


class ObsSymmetryArgs(C.Structure):
    """gvec_obs_symmetry_args (include/generals_vec.h): every pointer is device memory; all but sym may be None."""
    _fields_ = ([("rows", C.c_int64)] + [(n, C.c_int32) for n in ("width", "height", "num_sets", "inverse", "reserved")]
                + [("sets", SymPlaneSet * SYM_MAX_PLANE_SETS)]
                + [(n, C.c_void_p) for n in ("sym", "mask_in", "mask_out", "values_in", "values_out", "action_in", "action_out",
                                             "applied")])


class ArenaArgs(C.Structure):
    """gvec_arena_args (include/generals_vec.h): every pointer is device memory; alive, reset and obs may be None."""
    _fields_ = ([("rows", C.c_int64)] + [(n, C.c_int32) for n in ("width", "height", "num_learners", "games_cap")]
                + [("obs_row_stride", C.c_int64)]
                + [(n, C.c_void_p) for n in ("alive", "terminated", "truncated", "reset", "winner", "reward", "player_ids", "obs",
                                             "death", "ep_len", "ep_return", "games", "wins", "eliminated", "len_sum", "ret_sum",
                                             "pair2")])


class SearchArgs(C.Structure):
    """gvec_search_args (include/generals_vec.h): every pointer is device memory; root_envs may be None."""
    _fields_ = ([(n, C.c_int32) for n in ("num_roots", "num_candidates", "replicas", "depth")]
                + [(n, C.c_void_p) for n in ("root_envs", "root_players", "candidates")]
                + [("seed", C.c_uint64), ("terms", C.c_void_p)])


SEARCH_TERMS, SEARCH_PASS, SEARCH_NONE = 8, -1, -2     # GVEC_SEARCH_* in include/generals_vec.h
SEARCH_MAX_SLOTS = 64                                  # GVEC_SEARCH_MAX_SLOTS


class SearchHalveArgs(C.Structure):
    """gvec_search_halve_args (include/generals_vec.h): every pointer is device memory; slot may be None (the identity)."""
    _fields_ = ([(n, C.c_int32) for n in ("n", "m", "k", "replicas", "k_next", "reserved")]
                + [(n, C.c_void_p) for n in ("terms", "slot", "candidates0", "prior_key")]
                + [(n, C.c_double) for n in ("win", "loss", "land", "army", "q_lo", "q_inv_range", "c_visit", "c_scale")]
                + [(n, C.c_void_p) for n in ("sum", "count", "next_slot", "next_candidates")])


class SearchPolicyArgs(C.Structure):
    """gvec_search_policy_args (include/generals_vec.h): every pointer is device memory; logits and value may be None."""
    _fields_ = ([(n, C.c_int32) for n in ("n", "num_actions", "m", "reserved")]
                + [(n, C.c_void_p) for n in ("logits", "mask", "candidates0", "sum", "count", "value")]
                + [(n, C.c_double) for n in ("q_lo", "q_inv_range", "c_visit", "c_scale")]
                + [(n, C.c_void_p) for n in ("target", "v_mix")])


class Tree(C.Structure):
    """gvec_tree (include/generals_vec.h): the node-major device arrays of n trees of `nodes` nodes with num_slots child slots."""
    _fields_ = ([(n, C.c_int32) for n in ("n", "nodes", "num_slots", "reserved")]
                + [(n, C.c_void_p) for n in ("child_action", "child_logit", "child_node", "child_count", "child_sum", "node_value",
                                             "node_status", "node_parent", "node_slot")])


class TreeSelectArgs(C.Structure):
    """gvec_tree_select_args: slot may be None (the identity)."""
    _fields_ = ([("tree", Tree), ("k", C.c_int32), ("reserved", C.c_int32), ("slot", C.c_void_p)]
                + [(n, C.c_double) for n in ("q_lo", "q_inv_range", "c_visit", "c_scale")]
                + [(n, C.c_void_p) for n in ("leaf_node", "leaf_slot", "leaf_action", "leaf_depth")])


class TreeBackupArgs(C.Structure):
    """gvec_tree_backup_args: net_value may be None."""
    _fields_ = ([("tree", Tree), ("k", C.c_int32), ("replicas", C.c_int32)]
                + [(n, C.c_void_p) for n in ("leaf_node", "leaf_slot", "new_node", "terms", "status", "net_value")]
                + [(n, C.c_double) for n in ("value_weight", "win", "loss", "land", "army")])


TREE_NOT_EXPANDED, TREE_DEAD = -1, -2                  # child_node of an edge without a node
TREE_IN_USE, TREE_TERMINAL = 1, 2                      # node_status bits
EXPAND_STORED, EXPAND_OVER, EXPAND_DEAD = 1, 2, 4      # gvec_search_expand's status bits


# flag bits of a rollout row (GVEC_TRAJ_* in include/generals_vec.h)
TRAJ_VALID, TRAJ_TERMINAL, TRAJ_CUT = 1, 2, 4

# header words of a prioritized-replay tree (GVEC_PER_* in include/generals_vec.h)
PER_HEADER_WORDS, PER_HDR_MAX, PER_HDR_REJECTED, PER_HDR_DRAWS = 64, 0, 1, 2

# every symbol include/generals_vec.h declares: (restype, argtypes)
_vp, _i32, _u64 = C.c_void_p, C.c_int32, C.c_uint64
SYMBOLS = {
    "gvec_abi_version": (_i32, []),
    "gvec_config_default": (_i32, [C.POINTER(Config)]),
    "gvec_create": (_i32, [C.POINTER(Config), C.POINTER(_vp)]),
    "gvec_destroy": (_i32, [_vp]),
    "gvec_create_sharded": (_i32, [C.POINTER(Config), C.POINTER(C.c_int32), _i32, C.POINTER(_vp)]),
    "gvec_num_shards": (_i32, [_vp]),
    "gvec_shard": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gvec_gather_experience_records": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "gvec_set_stream": (_i32, [_vp, _vp]),
    "gvec_synchronize": (_i32, [_vp]),
    "gvec_last_error": (C.c_char_p, []),
    "gvec_host_alloc": (_i32, [_u64, C.POINTER(_vp)]),
    "gvec_host_free": (_i32, [_vp]),
    "gvec_num_envs": (_i32, [_vp]),
    "gvec_tile_stride": (_i32, [_vp]),
    "gvec_mask_bytes": (_i32, [_vp]),
    "gvec_state_bytes_per_env": (C.c_int64, [_vp]),
    "gvec_reset": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "gvec_reset_generated": (_i32, [_vp, _u64, _vp, _vp, _vp]),
    "gvec_reset_go_seeded": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "gvec_build_board_pool": (_i32, [_vp, _i32, _u64, _vp, _vp, _vp]),
    "gvec_step": (_i32, [_vp, _vp, _vp, _vp, _i32]),
    "gvec_legal_mask": (_i32, [_vp, _vp, _i32]),
    "gvec_player_visibility": (_i32, [_vp, _i32, _vp, _vp, _i32]),
    "gvec_read_state": (_i32, [_vp, _i32, _i32, C.POINTER(StateView), _i32]),
    "gvec_write_state": (_i32, [_vp, _i32, _i32, C.POINTER(StateView), _i32]),
    "gvec_rollout": (_i32, [_vp, _i32, _u64, _i32, _i32, C.POINTER(RolloutStats)]),
    "gvec_rollout_range": (_i32, [_vp, _i32, _i32, _i32, _u64, _i32]),
    "gvec_set_agent_mix": (_i32, [_vp, _i32, _i32]),
    "gvec_agent_actions": (_i32, [_vp, _u64, _i32, _vp, _i32]),
    "gvec_bot_actions": (_i32, [_vp, C.c_uint32, _u64, _i32, _vp, _i32]),
    "gvec_search_playouts": (_i32, [_vp, C.POINTER(SearchArgs)]),
    "gvec_search_playouts_bot": (_i32, [_vp, C.POINTER(SearchArgs), C.c_uint32, _i32]),
    "gvec_search_halve": (_i32, [_i32, _vp, C.POINTER(SearchHalveArgs)]),
    "gvec_search_improved_policy": (_i32, [_i32, _vp, C.POINTER(SearchPolicyArgs)]),
    "gvec_search_expand": (_i32, [_vp, C.POINTER(SearchArgs), C.c_uint32, _i32, _vp, _vp, _vp]),
    "gvec_tree_select": (_i32, [_i32, _vp, C.POINTER(TreeSelectArgs)]),
    "gvec_tree_backup": (_i32, [_i32, _vp, C.POINTER(TreeBackupArgs)]),
    "gvec_counters": (_i32, [_vp, C.POINTER(RolloutStats)]),
    "gvec_step_traffic_bytes": (_i32, [_vp, C.POINTER(C.c_int64)]),
    "gvec_experience_begin": (_i32, [_vp]),
    "gvec_experience_begin_range": (_i32, [_vp, _i32, _i32]),
    "gvec_experience_rewards": (_i32, [_vp, _vp, _vp, _i32]),
    "gvec_reward_config_default": (_i32, [C.POINTER(RewardConfigC)]),
    "gvec_experience_begin_rewards": (_i32, [_vp]),
    "gvec_experience_rewards_config": (_i32, [_vp, C.POINTER(RewardConfigC), C.c_uint32, _vp, _vp, _vp, _vp, _i32]),
    "gvec_experience_record_layout": (_i32, [_vp, C.POINTER(C.c_int32)]),
    "gvec_experience_record_bytes": (_i32, [_vp]),
    "gvec_experience_records": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "gvec_record_agent_actions": (_i32, [_vp, _i32]),
    "gvec_expand_experience_records": (_i32, [_i32, _vp, C.POINTER(C.c_int32), _vp, _i32, _vp, _vp, _vp, _vp]),
    "gvec_pool_collect": (_i32, [_i32, _vp, C.POINTER(CollectArgs)]),
    "gvec_pool_collect_scratch_bytes": (_u64, [_i32]),
    "gvec_per_tree_bytes": (_u64, [C.c_int64]),
    "gvec_per_tree_layout": (_i32, [C.c_int64, C.POINTER(C.c_int64)]),
    "gvec_per_init": (_i32, [_i32, _vp, _vp, C.c_int64]),
    "gvec_per_push": (_i32, [_i32, _vp, _vp, C.c_int64, _vp, _vp, C.c_int64]),
    "gvec_per_update": (_i32, [_i32, _vp, _vp, C.c_int64, _vp, _vp, C.c_int64, C.c_float, C.c_float]),
    "gvec_per_sample": (_i32, [_i32, _vp, _vp, C.c_int64, _vp, C.c_int64, C.c_float, _vp, _u64, _vp, _vp]),
    "gvec_nstep_link": (_i32, [_i32, _vp, C.POINTER(CollectArgs), _vp, _vp, _vp]),
    "gvec_nstep_gather": (_i32, [_i32, _vp, C.POINTER(NstepGatherArgs)]),
    "gvec_traj_scratch_bytes": (_u64, [C.c_int64, C.c_int64]),
    "gvec_traj_record": (_i32, [_i32, _vp, C.POINTER(TrajRecordArgs)]),
    "gvec_traj_gae": (_i32, [_i32, _vp, C.POINTER(TrajGaeArgs)]),
    "gvec_traj_vtrace": (_i32, [_i32, _vp, C.POINTER(TrajVtraceArgs)]),
    "gvec_traj_compact": (_i32, [_i32, _vp, C.POINTER(TrajCompactArgs)]),
    "gvec_traj_gather": (_i32, [_i32, _vp, C.POINTER(TrajGatherArgs)]),
    "gvec_policy_sample": (_i32, [_i32, _vp, C.POINTER(PolicySampleArgs)]),
    "gvec_policy_evaluate": (_i32, [_i32, _vp, C.POINTER(PolicyEvaluateArgs)]),
    "gvec_policy_backward": (_i32, [_i32, _vp, C.POINTER(PolicyBackwardArgs)]),
    "gvec_policy_distill": (_i32, [_i32, _vp, C.POINTER(PolicyDistillArgs)]),
    "gvec_policy_distill_backward": (_i32, [_i32, _vp, C.POINTER(PolicyDistillBackwardArgs)]),
    "gvec_obs_features": (_i32, [_i32, _vp, C.POINTER(ObsFeaturesArgs)]),
    "gvec_obs_memory_update": (_i32, [_i32, _vp, C.POINTER(ObsMemoryArgs)]),
    "gvec_obs_valid_mask": (_i32, [_i32, _vp, C.POINTER(ObsValidMaskArgs)]),
    "gvec_q_target": (_i32, [_i32, _vp, C.POINTER(QTargetArgs)]),
    "gvec_categorical_target": (_i32, [_i32, _vp, C.POINTER(CategoricalTargetArgs)]),
    "gvec_obs_symmetry": (_i32, [_i32, _vp, C.POINTER(ObsSymmetryArgs)]),
    "gvec_arena_update": (_i32, [_i32, _vp, C.POINTER(ArenaArgs)]),
    "gvec_gym_observe":(_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "gvec_gym_finish_step": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gvec_gym_actions": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gvec_gym_step": (_i32, [_vp, _i32, _u64] + [_vp] * 3 + [_i32] + [_vp] * 11),
    "gvec_gym_observe_players": (_i32, [_vp, C.c_uint32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "gvec_gym_step_players": (_i32, [_vp, C.c_uint32, _u64] + [_vp] * 3 + [_i32] + [_vp] * 11),
    "gvec_stream_delta_cap": (_i32, [_vp]),
    "gvec_stream_deltas": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32]),
    "gvec_stream_deltas_packed": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "gvec_observe": (_i32, [_vp, _i32, _vp, _i32]),
    "gvec_serializer_mask": (_i32, [_vp, _vp, _i32]),
    "gvec_export_records": (_i32, [_vp, _i32, _i32, _vp]),
    "gvec_import_records": (_i32, [_vp, _i32, _i32, _vp]),
    "gvec_copy_envs": (_i32, [_vp, _vp, _vp, _vp, _i32]),
    "gvec_device_buffer": (_vp, [_vp, _i32]),
    "gvec_read_buffer": (_i32, [_vp, _i32, _u64, _u64, _vp]),
    "gvec_selftest": (_i32, [_i32]),
}


def lib_path():
    """The in-tree build; GVEC_LIB names another build of the same library (A/B measurements of two builds)."""
    return os.environ.get("GVEC_LIB") or os.path.join(_PKG, "libgvec_hip.so")


def load_from(path):
    """Loads one build of the HIP library from `path` (not cached: A/B benchmarking of two builds
    in one process uses this directly)."""
    if not os.path.exists(path):
        raise GvecError(-2, f"{path} not found: build it with `python generalsreinforcementlearning_amd/csrc/build.py` "
                            "(hipcc, gfx950). This package has no CPU fallback.")
    L = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if L.gvec_abi_version() != 2:
        raise GvecError(-1, "ABI version mismatch")
    return L


def load():
    """Loads the HIP library.  Fails loudly if it has not been built: there is no fallback."""
    global _LIB
    if _LIB is None:
        _LIB = load_from(lib_path())
    return _LIB


def lib():
    return load()


def check(rc, what="", L=None):
    if rc < 0:
        msg = (L or load()).gvec_last_error()
        raise GvecError(rc, f"{what}: {msg.decode() if msg else ''}")
    return rc
