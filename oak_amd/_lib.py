"""ctypes loader for liboakgpu.so (the HIP product library).  Fails loudly: there is no CPU
fallback anywhere in oak_amd -- if the library is missing or no HIP device is usable, calls raise."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OAKGPU_LIB") or os.path.join(_HERE, "liboakgpu.so")   # (OAKGPU_LIB: an alternative build of the SAME library, e.g. tools/engine_variants.sh)

# every symbol include/oakgpu.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "oakgpu_create", "oakgpu_destroy", "oakgpu_last_error", "oakgpu_set_stream", "oakgpu_get_stream", "oakgpu_synchronize", "oakgpu_set_kernel_timing", "oakgpu_get_leaf_kernel_ms", "oakgpu_set_playouts_per_lane", "oakgpu_set_regroup", "oakgpu_set_tail_pack", "oakgpu_set_yield_schedule", "oakgpu_set_yield_saturation", "oakgpu_last_launch_yield", "oakgpu_last_launch_parked", "oakgpu_set_queue_order", "oakgpu_queue_order", "oakgpu_set_spread", "oakgpu_set_migration", "oakgpu_set_migration_window", "oakgpu_set_standstill_skip", "oakgpu_set_move_carry", "oakgpu_set_move_carry_dry", "oakgpu_set_lean_rollout", "oakgpu_last_launch_lean", "oakgpu_get_queue_counters",
    "oakgpu_device_count", "oakgpu_rollout_dev", "oakgpu_rollout", "oakgpu_rollout_group_dev", "oakgpu_rollout_group",
    "oakgpu_mt19937_fill", "oakgpu_rollout_draws_dev", "oakgpu_rollout_shared_device", "oakgpu_update_dev", "oakgpu_update",
    "oakgpu_choices_dev", "oakgpu_choices", "oakgpu_init_battles_dev", "oakgpu_init_battles",
    "oakgpu_set_ou_pools", "oakgpu_random_ou_battles_dev",
    "oakgpu_net_load", "oakgpu_net_load_memory", "oakgpu_net_free", "oakgpu_net_shape", "oakgpu_net_set_main_precision", "oakgpu_net_main_precision", "oakgpu_net_policy_form",
    "oakgpu_net_load_discrete", "oakgpu_net_load_discrete_memory", "oakgpu_net_is_discrete", "oakgpu_leaf_eval_discrete_raw_dev",
    "oakgpu_leaf_eval_dev", "oakgpu_leaf_eval", "oakgpu_leaf_eval_cached_dev", "oakgpu_leaf_cache_last_count", "oakgpu_leaf_embed_forms", "oakgpu_leaf_eval_policy_dev", "oakgpu_leaf_eval_policy",
    "oakgpu_heap_create", "oakgpu_heap_destroy", "oakgpu_heap_empty", "oakgpu_heap_clear", "oakgpu_heap_kind", "oakgpu_heap_nodes", "oakgpu_heap_update",
    "oakgpu_heap_root_stats", "oakgpu_heap_child_stats", "oakgpu_search_heap", "oakgpu_search_agent_heap", "oakgpu_heap_check_shards", "oakgpu_heap_selftest",
    "oakgpu_tree_step_dev", "oakgpu_search", "oakgpu_search_many", "oakgpu_search_agent", "oakgpu_agent_networks_clear", "oakgpu_bandit_replay", "oakgpu_bandit_select_run", "oakgpu_solve_matrix",
    "oakgpu_segment_mean_dev", "oakgpu_comm_unique_id", "oakgpu_comm_create", "oakgpu_comm_destroy", "oakgpu_all_gather_dev",
    "oakgpu_root_steps_create", "oakgpu_root_steps_destroy", "oakgpu_root_steps_launch_dev", "oakgpu_root_steps_capacity", "oakgpu_root_steps_reserve",
    "oakgpu_endless_battle_check", "oakgpu_frames_size", "oakgpu_frames_write", "oakgpu_frames_read", "oakgpu_selfplay_game", "oakgpu_selfplay_games", "oakgpu_poke_engine_eval_dev", "oakgpu_poke_engine_eval",
    "oakgpu_replay_index", "oakgpu_replay_records_dev", "oakgpu_replay_records", "oakgpu_engine_switches",
    "oakgpu_corpus_create", "oakgpu_corpus_destroy", "oakgpu_corpus_info", "oakgpu_frames_encode_dev", "oakgpu_frames_sample_dev", "oakgpu_encode_battles_dev",
    "oakgpu_frames_encode", "oakgpu_frames_sample",
    "oakgpu_corpus_frame_bases", "oakgpu_corpus_chunks", "oakgpu_corpus_states_dev", "oakgpu_corpus_states", "oakgpu_corpus_inference_dev", "oakgpu_corpus_loss_dev",
    "oakgpu_corpus_inference", "oakgpu_corpus_evaluate",
    "oakgpu_corpus_window_check", "oakgpu_corpus_create_window", "oakgpu_corpus_append_dev", "oakgpu_corpus_append", "oakgpu_corpus_window_stats",
    "oakgpu_corpus_records", "oakgpu_window_scan_host",
    "oakgpu_party_table_create", "oakgpu_party_table_destroy", "oakgpu_party_table_fill_dev", "oakgpu_party_table_fill", "oakgpu_leaf_eval_table_dev",
    "oakgpu_leaf_eval_policy_table_dev", "oakgpu_party_table_last_misses", "oakgpu_party_table_rows", "oakgpu_party_table_width", "oakgpu_party_key", "oakgpu_party_variant",
    "oakgpu_set_search_party_table", "oakgpu_search_party_table_stats", "oakgpu_leaf_eval_table", "oakgpu_leaf_eval_policy_table",
    "oakgpu_policy_games_dev", "oakgpu_policy_games", "oakgpu_policy_games_last_stats",
    "oakgpu_forest_create", "oakgpu_forest_destroy", "oakgpu_forest_check", "oakgpu_forest_search_dev", "oakgpu_forest_search", "oakgpu_forest_nodes",
    "oakgpu_forest_last_stats", "oakgpu_search_stream", "oakgpu_agent_params",
    "oakgpu_forest_selfplay_check", "oakgpu_forest_selfplay_dev", "oakgpu_forest_selfplay_records", "oakgpu_forest_selfplay", "oakgpu_forest_selfplay_last_stats",
    "oakgpu_selfplay_pick_host",
    "oakgpu_forest_match_check", "oakgpu_forest_match_dev", "oakgpu_forest_match", "oakgpu_forest_match_last_stats", "oakgpu_match_pick_host",
    "oakgpu_forest_match_set_records", "oakgpu_forest_match_records",
    "oakgpu_forest_create_kept", "oakgpu_forest_create_kept_check", "oakgpu_forest_kept_tree_bytes", "oakgpu_forest_advance_dev", "oakgpu_forest_advance",
    "oakgpu_forest_search_kept_dev", "oakgpu_forest_search_kept", "oakgpu_forest_keep_stats", "oakgpu_forest_mismatch", "oakgpu_forest_node_counts",
    "oakgpu_forest_selfplay_nodes_kept", "oakgpu_forest_selfplay_keep_stats",
    "oakgpu_nash_solve_dev", "oakgpu_solve_matrices", "oakgpu_nash_soft_host", "oakgpu_nash_round_host", "oakgpu_nash_width4_max_entry",
    "oakgpu_forest_selfplay_last_traffic",
    "oakgpu_forest_budgets_check", "oakgpu_forest_search_budgets_dev", "oakgpu_forest_search_budgets", "oakgpu_forest_search_budgets_kept_dev",
    "oakgpu_forest_search_budgets_kept", "oakgpu_forest_last_rows", "oakgpu_forest_selfplay_fast_stats", "oakgpu_forest_selfplay_set_partition",
    "oakgpu_selfplay_prelude_host",
    "oakgpu_forest_selfplay_build_dev", "oakgpu_forest_selfplay_build", "oakgpu_forest_selfplay_matchup", "oakgpu_selfplay_skip_host",
    "oakgpu_forest_selfplay_skip_check",
    "oakgpu_frames_symmetries_dev", "oakgpu_trainer_check", "oakgpu_trainer_create", "oakgpu_trainer_destroy", "oakgpu_trainer_shape",
    "oakgpu_trainer_forward_dev", "oakgpu_trainer_gradients_dev", "oakgpu_trainer_adam_dev", "oakgpu_trainer_step_dev", "oakgpu_trainer_report",
    "oakgpu_trainer_read", "oakgpu_trainer_set_gradients", "oakgpu_trainer_net_bytes", "oakgpu_trainer_forward", "oakgpu_trainer_gradients",
    "oakgpu_trainer_step",
    "oakgpu_build_tables", "oakgpu_build_net_check", "oakgpu_build_net_load", "oakgpu_build_net_destroy", "oakgpu_build_net_shape", "oakgpu_build_teams_check",
    "oakgpu_build_provide_check", "oakgpu_build_rollout_dev", "oakgpu_build_provide_dev", "oakgpu_build_records_dev", "oakgpu_build_rollout",
    "oakgpu_build_provide", "oakgpu_build_records", "oakgpu_build_game_records_dev", "oakgpu_build_game_targets_host",
    "oakgpu_build_window_create", "oakgpu_build_window_destroy", "oakgpu_build_window_append_dev", "oakgpu_build_window_append", "oakgpu_build_window_corpus",
    "oakgpu_build_window_records", "oakgpu_build_window_stats",
    "oakgpu_build_traj_check", "oakgpu_build_corpus_create", "oakgpu_build_corpus_destroy", "oakgpu_build_corpus_scan_dev", "oakgpu_build_corpus_info",
    "oakgpu_build_traj_dev", "oakgpu_build_traj_sample_dev", "oakgpu_build_targets_dev", "oakgpu_build_state_dense_dev", "oakgpu_build_traj",
    "oakgpu_build_traj_sample", "oakgpu_build_targets", "oakgpu_build_state_dense",
    "oakgpu_build_trainer_check", "oakgpu_build_trainer_create", "oakgpu_build_trainer_destroy", "oakgpu_build_trainer_shape", "oakgpu_build_trainer_forward_dev",
    "oakgpu_build_trainer_accumulate_dev", "oakgpu_build_trainer_zero_gradients_dev", "oakgpu_build_trainer_adam_dev", "oakgpu_build_trainer_average_dev",
    "oakgpu_build_trainer_report", "oakgpu_build_trainer_read", "oakgpu_build_trainer_set_gradients", "oakgpu_build_trainer_net_bytes",
]


def nash_mode(solve_nash):
    """The C ABI's solve_nash word: 0 none, 1 the host's threads, 2 ("device") the device solver -- the same bits either way."""
    if isinstance(solve_nash, str):
        if solve_nash not in ("host", "device"):
            raise ValueError("solve_nash: True / False, \"host\", \"device\" or 0 / 1 / 2")
        return 2 if solve_nash == "device" else 1
    return 2 if (not isinstance(solve_nash, bool) and solve_nash == 2) else int(bool(solve_nash))


class RolloutBatch(C.Structure):      # oakgpu_rollout_batch (include/oakgpu.h)
    _fields_ = [("battles", C.c_void_p), ("durations", C.c_void_p), ("results_in", C.c_void_p), ("prng_state", C.c_void_p),
                ("n", C.c_uint32), ("results_out", C.c_void_p), ("steps_out", C.c_void_p), ("values_out", C.c_void_p),
                ("battles_out", C.c_void_p), ("durations_out", C.c_void_p)]


class SearchParams(C.Structure):      # oakgpu_search_params (include/oakgpu.h)
    _fields_ = [("iterations", C.c_uint64), ("batch", C.c_uint32), ("ucb_c", C.c_float), ("bandit", C.c_int32),
                ("eval", C.c_int32), ("max_depth", C.c_uint32), ("root_rolls", C.c_uint32), ("other_rolls", C.c_uint32),
                ("seed", C.c_uint64), ("matrix_ucb", C.c_int32), ("mucb_delay", C.c_uint32), ("mucb_minimum", C.c_uint32),
                ("mucb_c", C.c_float), ("exp3_alpha", C.c_float), ("duration_us", C.c_uint64)]


class Agent(C.Structure):             # oakgpu_agent
    _fields_ = [("budget", C.c_char_p), ("bandit", C.c_char_p), ("eval", C.c_char_p), ("matrix_ucb", C.c_char_p),
                ("discrete", C.c_int), ("table", C.c_int)]


class SearchOutput(C.Structure):      # oakgpu_search_output
    _fields_ = [("m", C.c_uint8), ("n", C.c_uint8), ("p1_choices", C.c_uint8 * 9), ("p2_choices", C.c_uint8 * 9),
                ("visit_matrix", C.c_uint64 * 81), ("value_matrix", C.c_double * 81), ("iterations", C.c_uint64),
                ("empirical_value", C.c_double), ("initial_value", C.c_double), ("p1_empirical", C.c_double * 9),
                ("p2_empirical", C.c_double * 9), ("nodes", C.c_uint64), ("total_depth", C.c_uint64),
                ("duration_us", C.c_double), ("nash_value", C.c_double), ("p1_nash", C.c_double * 9), ("p2_nash", C.c_double * 9),
                ("p1_logit", C.c_double * 9), ("p2_logit", C.c_double * 9), ("p1_prior", C.c_double * 9), ("p2_prior", C.c_double * 9)]

class FrameUpdate(C.Structure):       # oakgpu_frame_update
    _fields_ = [("m", C.c_uint8), ("n", C.c_uint8), ("c1", C.c_uint8), ("c2", C.c_uint8), ("iterations", C.c_uint32),
                ("empirical_value", C.c_double), ("nash_value", C.c_double), ("p1_empirical", C.c_double * 9),
                ("p1_nash", C.c_double * 9), ("p2_empirical", C.c_double * 9), ("p2_nash", C.c_double * 9)]


class SelfplayParams(C.Structure):    # oakgpu_selfplay_params
    _fields_ = [("search", SearchParams), ("policy_mode", C.c_char * 16), ("policy_temp", C.c_double), ("policy_min", C.c_double),
                ("max_battle_length", C.c_uint32), ("seed", C.c_uint64), ("keep_node", C.c_int32), ("nodes_kept", C.c_uint32),
                ("fast_budget", C.c_uint32), ("fast_search_prob", C.c_double), ("fast_policy_mode", C.c_char * 16)]


class SelfplaySkip(C.Structure):      # oakgpu_selfplay_skip
    _fields_ = [("t1_budget", C.c_uint32), ("battle_skip_prob", C.c_double)]


class EncodedFrames(C.Structure):     # oakgpu_encoded_frames: one pointer per tensor, device or host as the call says
    _fields_ = [(name, C.c_void_p) for name in ("pokemon", "active", "hp", "choice_indices", "k", "choice", "iterations", "empirical_policies",
                                                "nash_policies", "empirical_value", "nash_value", "score", "status", "where")]


class CorpusStats(C.Structure):       # oakgpu_corpus_stats
    _fields_ = [("records", C.c_uint32), ("malformed", C.c_uint32), ("frames", C.c_uint64), ("stopped_at", C.c_size_t)]


class CorpusEval(C.Structure):        # oakgpu_corpus_eval: one nullable pointer per tensor, device or host as the call says
    _fields_ = [(name, C.c_void_p) for name in ("value", "policy_logit", "policy", "k", "choices", "status", "where")]


class LossParams(C.Structure):        # oakgpu_loss_params
    _fields_ = [("wn", C.c_float), ("we", C.c_float), ("ws", C.c_float), ("pn", C.c_float), ("min_iterations", C.c_uint32)]


class CorpusTerms(C.Structure):       # oakgpu_corpus_terms
    _fields_ = [(name, C.c_void_p) for name in ("sq_err", "ce", "excluded", "record_sums", "record_counts")]


class CorpusLosses(C.Structure):      # oakgpu_corpus_losses
    _fields_ = [("sq_err", C.c_double), ("ce1", C.c_double), ("ce2", C.c_double), ("rows", C.c_uint64), ("excluded", C.c_uint64), ("failed", C.c_uint64),
                ("mse", C.c_double), ("ce_p1", C.c_double), ("ce_p2", C.c_double)]


class TrainLoss(C.Structure):         # oakgpu_train_loss
    _fields_ = [(name, C.c_float) for name in ("wn", "we", "ws", "pn", "value_weight", "policy_weight")]


class TrainReport(C.Structure):       # oakgpu_train_report
    _fields_ = [("loss", C.c_double), ("mse", C.c_double), ("ce_p1", C.c_double), ("ce_p2", C.c_double), ("rows", C.c_uint64)]


class TrainOutputs(C.Structure):      # oakgpu_train_outputs: one nullable pointer per tensor, device or host as the call says
    _fields_ = [(name, C.c_void_p) for name in ("value", "logits", "sq_err", "ce")]


class BuildOutputs(C.Structure):      # oakgpu_build_outputs: one pointer per array, device or host as the call says
    _fields_ = [(name, C.c_void_p) for name in ("teams_out", "n_updates", "action", "index", "n_legal", "prob", "trace_legal", "trace_logits",
                                                "trace_policy", "teams_init", "sizes_out", "team_index")]


class BuildSeatArrays(C.Structure):   # oakgpu_build_seat_arrays
    _fields_ = [(name, C.c_void_p) for name in ("teams_init", "sizes", "n_updates", "action", "prob")]


class BuildProvider(C.Structure):     # oakgpu_build_provider
    _fields_ = [("max_pokemon", C.c_int32), ("input_update", C.c_int32), ("pokemon_delete_prob", C.c_double), ("move_delete_prob", C.c_double),
                ("team_modify_prob", C.c_double)]


class BuildCorpusStats(C.Structure):  # oakgpu_build_corpus_stats
    _fields_ = [("records", C.c_uint32), ("files", C.c_uint32), ("status_count", C.c_uint32 * 6)]


class BuildTrajParams(C.Structure):   # oakgpu_build_traj_params
    _fields_ = [("mask_dtype", C.c_int32), ("no_score", C.c_int32)]


class BuildTrajectories(C.Structure):  # oakgpu_build_trajectories: one nullable pointer per array, device or host as the call says
    _fields_ = [(name, C.c_void_p) for name in ("action", "mask", "n_legal", "policy", "value", "score", "start", "end", "status", "t_max")]


class BuildTargetOutputs(C.Structure):  # oakgpu_build_target_outputs
    _fields_ = [(name, C.c_void_p) for name in ("valid", "n_valid", "rows", "state_cells", "state_n", "old_logp", "rewards")]


class BuildChunk(C.Structure):        # oakgpu_build_chunk
    _fields_ = [("mask", C.c_void_p), ("mask_dtype", C.c_int32), ("n", C.c_uint32), ("n_legal", C.c_void_p), ("valid", C.c_void_p), ("rewards", C.c_void_p),
                ("n_valid", C.c_uint32), ("rows", C.c_void_p), ("state_cells", C.c_void_p), ("state_n", C.c_void_p), ("keep", C.c_void_p),
                ("gamma", C.c_double), ("gamma_lam", C.c_double), ("policy_loss_weight", C.c_float), ("value_loss_weight", C.c_float),
                ("entropy_loss_weight", C.c_float), ("total", C.c_uint32), ("remaining", C.c_uint32)]


class BuildTrainOutputs(C.Structure):  # oakgpu_build_train_outputs
    _fields_ = [(name, C.c_void_p) for name in ("logits", "value", "logp", "gae", "returns", "forced", "selected", "du")]


class BuildTrainReport(C.Structure):  # oakgpu_build_train_report
    _fields_ = [("rows", C.c_uint32), ("kept", C.c_uint32), ("n_cap", C.c_uint32), ("reserved", C.c_uint32), ("policy_loss", C.c_double),
                ("value_loss", C.c_double), ("entropy", C.c_double), ("loss", C.c_double), ("steps", C.c_uint64)]


class Seat(C.Structure):              # oakgpu_seat
    _fields_ = [("kind", C.c_int32), ("net", C.c_void_p), ("temp", C.c_double), ("min", C.c_double)]


class PolicyGamesParams(C.Structure):  # oakgpu_policy_games_params
    _fields_ = [("p1", Seat), ("p2", Seat), ("max_turns", C.c_uint32), ("poll", C.c_uint32), ("compact_below", C.c_float),
                ("log_turns", C.c_uint32)]


class MatchSeat(C.Structure):         # oakgpu_match_seat
    _fields_ = [("search", SearchParams), ("net", C.c_void_p), ("policy_mode", C.c_char * 16), ("policy_temp", C.c_double), ("policy_min", C.c_double)]


class ForestMatchParams(C.Structure):  # oakgpu_forest_match_params
    _fields_ = [("p1", MatchSeat), ("p2", MatchSeat), ("max_turns", C.c_uint32), ("early_stop", C.c_double), ("log_turns", C.c_uint32),
                ("solve_nash", C.c_int32)]


class MatchTurn(C.Structure):         # oakgpu_match_turn
    _fields_ = [("c1", C.c_uint8), ("c2", C.c_uint8), ("m", C.c_uint8), ("n", C.c_uint8), ("zero", C.c_uint32), ("ev_p1", C.c_double),
                ("ev_p2", C.c_double)]


class ForestOutputs(C.Structure):     # oakgpu_forest_outputs: one device pointer per array
    _fields_ = [(name, C.c_void_p) for name in ("m", "n", "p1_choices", "p2_choices", "visit_matrix", "value_matrix", "iterations", "nodes",
                                                "total_depth", "initial_value", "p1_logit", "p2_logit", "p1_prior", "p2_prior", "stream")]


class ForestBandit(C.Structure):      # oakgpu_forest_bandit
    _fields_ = [("scores", C.c_float * 9), ("priors", C.c_float * 9), ("visits", C.c_uint32 * 9), ("k", C.c_uint8), ("pad", C.c_uint8 * 3)]


class ForestNode(C.Structure):        # oakgpu_forest_node
    _fields_ = [("p1", ForestBandit), ("p2", ForestBandit)]


class ForestTraceHead(C.Structure):   # oakgpu_forest_trace_head
    _fields_ = [("levels", C.c_uint32), ("leaf", C.c_uint32), ("initialised", C.c_uint8), ("result_type", C.c_uint8), ("pad", C.c_uint8 * 2),
                ("value", C.c_float), ("logits", C.c_float * 18)]


class ForestTraceLevel(C.Structure):  # oakgpu_forest_trace_level
    _fields_ = [("node", C.c_uint32), ("i", C.c_uint8), ("j", C.c_uint8), ("pad", C.c_uint8 * 2)]


# include/pkmn.h: the libpkmn-named single-battle ABI (batch-of-one wrappers, pkmn_shim.hip)
PKMN_SYMBOLS = [
    "pkmn_gen1_battle_update", "pkmn_gen1_battle_choices", "pkmn_gen1_battle_options_set",
    "pkmn_gen1_battle_options_chance_actions", "pkmn_gen1_battle_options_chance_durations",
    "pkmn_result_type", "pkmn_result_p1", "pkmn_result_p2",
]

_lib = None


class OakGpuError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OakGpuError("liboakgpu.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    lib.oakgpu_create.argtypes = [C.POINTER(vp), i32]
    lib.oakgpu_destroy.argtypes = [vp]
    lib.oakgpu_destroy.restype = None
    lib.oakgpu_last_error.restype = C.c_char_p
    lib.oakgpu_set_stream.argtypes = [vp, vp]
    lib.oakgpu_get_stream.argtypes = [vp]
    lib.oakgpu_get_stream.restype = vp
    lib.oakgpu_synchronize.argtypes = [vp]
    lib.oakgpu_set_kernel_timing.argtypes = [vp, i32]
    lib.oakgpu_get_leaf_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.oakgpu_set_playouts_per_lane.argtypes = [vp, i32]
    lib.oakgpu_set_regroup.argtypes = [vp, i32, i32, i32]
    lib.oakgpu_set_tail_pack.argtypes = [vp, i32, i32, i32]
    lib.oakgpu_set_yield_schedule.argtypes = [vp, i32, i32, i32, i32]
    lib.oakgpu_set_yield_saturation.argtypes = [vp, i32]
    lib.oakgpu_last_launch_yield.argtypes = [vp]
    lib.oakgpu_last_launch_parked.argtypes = [vp, C.POINTER(u32)]
    lib.oakgpu_set_queue_order.argtypes = [vp, i32]
    lib.oakgpu_queue_order.argtypes = [vp, C.POINTER(RolloutBatch), u32, vp, C.POINTER(u32)]
    lib.oakgpu_set_spread.argtypes = [vp, i32]
    lib.oakgpu_set_migration.argtypes = [vp, i32, i32, i32]
    lib.oakgpu_set_migration_window.argtypes = [vp, i32]
    lib.oakgpu_set_standstill_skip.argtypes = [vp, i32]
    lib.oakgpu_set_move_carry.argtypes = [vp, i32]
    lib.oakgpu_set_move_carry_dry.argtypes = [vp, i32]
    lib.oakgpu_set_lean_rollout.argtypes = [vp, i32]
    lib.oakgpu_last_launch_lean.argtypes = [vp]
    lib.oakgpu_get_queue_counters.argtypes = [vp, vp]
    lib.oakgpu_rollout_dev.argtypes = [vp, vp, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp, vp]
    lib.oakgpu_rollout.argtypes = [vp, vp, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp, vp]
    lib.oakgpu_rollout_group_dev.argtypes = [vp, C.POINTER(RolloutBatch), u32, u32, i32]
    lib.oakgpu_rollout_group.argtypes = [vp, C.POINTER(RolloutBatch), u32, u32, i32]
    lib.oakgpu_mt19937_fill.argtypes = [u32, u64, vp, C.c_size_t]
    lib.oakgpu_rollout_draws_dev.argtypes = [vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, u32, i32, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_rollout_shared_device.argtypes = [vp, vp, vp, C.c_uint8, vp, u32, u32, u32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_poke_engine_eval_dev.argtypes = [vp, vp, u32, C.c_float, vp, vp]
    lib.oakgpu_poke_engine_eval.argtypes = [vp, vp, u32, C.c_float, vp, vp]
    lib.oakgpu_tree_step_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp]
    lib.oakgpu_search.argtypes = [vp, vp, vp, vp, C.c_uint8, C.POINTER(SearchParams), C.POINTER(SearchOutput)]
    lib.oakgpu_heap_create.argtypes = [C.POINTER(vp)]
    lib.oakgpu_heap_destroy.argtypes = [vp]
    lib.oakgpu_heap_destroy.restype = None
    lib.oakgpu_heap_empty.argtypes = [vp]
    lib.oakgpu_heap_clear.argtypes = [vp]
    lib.oakgpu_heap_clear.restype = None
    lib.oakgpu_heap_kind.argtypes = [vp]
    lib.oakgpu_heap_nodes.argtypes = [vp]
    lib.oakgpu_heap_nodes.restype = u64
    lib.oakgpu_heap_update.argtypes = [vp, C.c_uint8, C.c_uint8, vp]
    lib.oakgpu_heap_root_stats.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.oakgpu_heap_check_shards.argtypes = [vp]
    lib.oakgpu_heap_check_shards.restype = u64
    lib.oakgpu_heap_selftest.argtypes = [u32, u32, u64, i32, C.POINTER(u64 * 4)]
    lib.oakgpu_heap_child_stats.argtypes = [vp, C.c_uint8, C.c_uint8, vp, i32, vp, vp, vp, vp]
    lib.oakgpu_search_heap.argtypes = [vp, vp, vp, vp, vp, C.c_uint8, C.POINTER(SearchParams), C.POINTER(SearchOutput), C.POINTER(SearchOutput)]
    lib.oakgpu_search_many.argtypes = [C.POINTER(vp), vp, C.POINTER(vp), vp, vp, vp, C.POINTER(SearchParams), u32, i32, C.POINTER(SearchOutput)]
    lib.oakgpu_search_agent_heap.argtypes = [vp, vp, vp, vp, C.c_uint8, C.POINTER(Agent), u32, u64, C.POINTER(SearchOutput), C.POINTER(SearchOutput)]
    lib.oakgpu_segment_mean_dev.argtypes = [vp, vp, u32, u32, vp]
    lib.oakgpu_root_steps_create.argtypes = [vp, u32, u32, u32, u32, C.POINTER(vp)]
    lib.oakgpu_root_steps_destroy.argtypes = [vp]
    lib.oakgpu_root_steps_destroy.restype = None
    lib.oakgpu_root_steps_launch_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp]
    lib.oakgpu_root_steps_capacity.argtypes = [vp, C.POINTER(u32)]
    lib.oakgpu_root_steps_reserve.argtypes = [vp, u64]
    lib.oakgpu_comm_unique_id.argtypes = [vp]
    lib.oakgpu_comm_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    lib.oakgpu_comm_destroy.argtypes = [vp]
    lib.oakgpu_comm_destroy.restype = None
    lib.oakgpu_all_gather_dev.argtypes = [vp, vp, vp, vp, C.c_size_t]
    lib.oakgpu_endless_battle_check.argtypes = [vp]
    lib.oakgpu_frames_size.restype = C.c_size_t
    lib.oakgpu_frames_size.argtypes = [C.POINTER(FrameUpdate), u32]
    lib.oakgpu_frames_write.argtypes = [vp, C.c_uint8, C.POINTER(FrameUpdate), u32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.oakgpu_frames_read.argtypes = [vp, C.c_size_t, vp, C.POINTER(C.c_uint8), C.POINTER(FrameUpdate), u32, C.POINTER(u32), C.POINTER(C.c_size_t)]
    lib.oakgpu_replay_index.argtypes = [vp, C.c_size_t, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(C.c_size_t)]
    lib.oakgpu_replay_records_dev.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp]
    lib.oakgpu_replay_records.argtypes = [vp, vp, C.c_size_t, vp, u32, C.POINTER(u32), C.POINTER(C.c_size_t), vp, vp]
    lib.oakgpu_engine_switches.argtypes = [C.POINTER(C.c_int * 4)]
    lib.oakgpu_corpus_create.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    lib.oakgpu_corpus_destroy.argtypes = [vp]
    lib.oakgpu_corpus_destroy.restype = None
    lib.oakgpu_corpus_info.argtypes = [vp, C.POINTER(CorpusStats)]
    lib.oakgpu_corpus_window_check.argtypes = [u32, C.c_size_t]
    lib.oakgpu_corpus_create_window.argtypes = [vp, u32, C.c_size_t, C.POINTER(vp)]
    lib.oakgpu_corpus_append_dev.argtypes = [vp, vp, vp, vp, u32]
    lib.oakgpu_corpus_append.argtypes = [vp, vp, vp, C.c_size_t]
    lib.oakgpu_corpus_window_stats.argtypes = [vp, C.POINTER(C.c_uint64 * 6)]
    lib.oakgpu_corpus_records.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), i32]
    lib.oakgpu_window_scan_host.argtypes = [vp, vp, u32, vp, vp]
    lib.oakgpu_frames_encode_dev.argtypes = [vp, vp, vp, u32, C.POINTER(EncodedFrames)]
    lib.oakgpu_frames_sample_dev.argtypes = [vp, vp, u32, u64, u32, u32, vp, C.POINTER(EncodedFrames)]
    lib.oakgpu_encode_battles_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    lib.oakgpu_frames_encode.argtypes = [vp, vp, vp, u32, C.POINTER(EncodedFrames), C.POINTER(u32)]
    lib.oakgpu_frames_sample.argtypes = [vp, vp, u32, u64, u32, u32, vp, C.POINTER(EncodedFrames), C.POINTER(u32)]
    lib.oakgpu_corpus_frame_bases.argtypes = [vp, vp]
    lib.oakgpu_corpus_chunks.argtypes = [vp, vp, u32, u32, vp, u32, C.POINTER(u32)]
    lib.oakgpu_corpus_states_dev.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_corpus_states.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_corpus_inference_dev.argtypes = [vp, vp, vp, u32, u32, u32, C.POINTER(CorpusEval)]
    lib.oakgpu_corpus_loss_dev.argtypes = [vp, vp, vp, u32, u32, u32, C.POINTER(LossParams), C.POINTER(CorpusEval), C.POINTER(CorpusTerms)]
    lib.oakgpu_corpus_inference.argtypes = [vp, vp, vp, u32, u32, u32, C.POINTER(CorpusEval)]
    lib.oakgpu_corpus_evaluate.argtypes = [vp, vp, vp, C.POINTER(LossParams), u32, C.POINTER(CorpusLosses), C.POINTER(CorpusLosses)]
    lib.oakgpu_selfplay_game.argtypes = [vp, vp, vp, u64, C.POINTER(SelfplayParams), vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(u32),
                                         C.POINTER(C.c_uint8)]
    lib.oakgpu_selfplay_games.argtypes = [C.POINTER(vp), vp, vp, C.POINTER(u64), C.POINTER(SelfplayParams), u32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(u32), C.POINTER(C.c_uint8)]
    lib.oakgpu_search_agent.argtypes = [vp, vp, vp, C.c_uint8, C.POINTER(Agent), u32, u64, C.POINTER(SearchOutput)]
    lib.oakgpu_agent_networks_clear.argtypes = [vp]
    lib.oakgpu_agent_networks_clear.restype = None
    lib.oakgpu_solve_matrix.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.oakgpu_nash_solve_dev.argtypes = [vp, vp, u32, vp]
    lib.oakgpu_solve_matrices.argtypes = [vp, vp, vp, vp, u32, i32, vp, vp, vp]
    lib.oakgpu_nash_soft_host.argtypes = [vp, vp, vp, u32, i32, vp, vp, vp, vp]
    lib.oakgpu_nash_round_host.argtypes = [vp, vp, vp, u32, vp, vp]
    lib.oakgpu_nash_width4_max_entry.argtypes = []
    lib.oakgpu_bandit_select_run.argtypes = [i32, C.c_float, C.c_float, u32, vp, vp, vp, u32, vp, vp, vp, vp]
    lib.oakgpu_bandit_replay.argtypes = [i32, C.c_float, C.c_float, u32, vp, u32, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_update_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, vp]
    lib.oakgpu_update.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, vp]
    lib.oakgpu_choices_dev.argtypes = [vp, vp, vp, i32, vp, vp, u32]
    lib.oakgpu_choices.argtypes = [vp, vp, vp, i32, vp, vp, u32]
    lib.oakgpu_init_battles_dev.argtypes = [vp, vp, vp, u32, i32, vp, vp, vp]
    lib.oakgpu_init_battles.argtypes = [vp, vp, vp, u32, i32, vp, vp, vp]
    lib.oakgpu_set_ou_pools.argtypes = [vp, vp, i32, vp, vp]
    lib.oakgpu_random_ou_battles_dev.argtypes = [vp, u64, u32, vp, vp, vp, vp]
    lib.oakgpu_net_load.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    lib.oakgpu_net_load_memory.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    lib.oakgpu_net_free.argtypes = [vp, vp]
    lib.oakgpu_net_free.restype = None
    lib.oakgpu_net_shape.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.oakgpu_net_set_main_precision.argtypes = [vp, C.c_int]
    lib.oakgpu_net_main_precision.argtypes = [vp, C.POINTER(C.c_int)]
    lib.oakgpu_net_policy_form.argtypes = [vp]
    lib.oakgpu_net_load_discrete.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    lib.oakgpu_net_load_discrete_memory.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    lib.oakgpu_net_is_discrete.argtypes = [vp]
    lib.oakgpu_leaf_eval_discrete_raw_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    lib.oakgpu_leaf_eval_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    lib.oakgpu_leaf_eval.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    lib.oakgpu_leaf_eval_cached_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp]
    lib.oakgpu_leaf_cache_last_count.argtypes = [vp, C.POINTER(u32)]
    lib.oakgpu_leaf_embed_forms.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.oakgpu_leaf_eval_policy_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_leaf_eval_policy.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_party_table_create.argtypes = [vp, vp, u32, C.POINTER(vp)]
    lib.oakgpu_party_table_destroy.argtypes = [vp, vp]
    lib.oakgpu_party_table_destroy.restype = None
    lib.oakgpu_party_table_fill_dev.argtypes = [vp, vp, vp, u32]
    lib.oakgpu_party_table_fill.argtypes = [vp, vp, vp, u32]
    lib.oakgpu_leaf_eval_table_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp]
    lib.oakgpu_leaf_eval_policy_table_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_party_table_last_misses.argtypes = [vp, vp, C.POINTER(u32)]
    lib.oakgpu_party_table_rows.argtypes = [vp, vp, u32, i32, i32, vp]
    lib.oakgpu_party_table_width.argtypes = [vp]
    lib.oakgpu_party_key.argtypes = [vp, C.c_uint8]
    lib.oakgpu_party_key.restype = C.c_uint8
    lib.oakgpu_party_variant.argtypes = [vp, C.c_uint8, vp, C.POINTER(C.c_uint8)]
    lib.oakgpu_set_search_party_table.argtypes = [vp, i32]
    lib.oakgpu_search_party_table_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.oakgpu_leaf_eval_table.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp]
    lib.oakgpu_leaf_eval_policy_table.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_policy_games_dev.argtypes = [vp, C.POINTER(PolicyGamesParams), vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_policy_games.argtypes = [vp, C.POINTER(PolicyGamesParams), vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.oakgpu_policy_games_last_stats.argtypes = [vp]
    lib.oakgpu_forest_create.argtypes = [vp, u32, u32, i32, C.POINTER(vp)]
    lib.oakgpu_forest_destroy.argtypes = [vp, vp]
    lib.oakgpu_forest_destroy.restype = None
    lib.oakgpu_forest_check.argtypes = [u32, u32, i32, C.POINTER(SearchParams), i32, u32, vp, i32, u32]
    lib.oakgpu_forest_search_dev.argtypes = [vp, vp, C.POINTER(SearchParams), vp, vp, vp, vp, u32, C.POINTER(ForestOutputs), vp, u32]
    lib.oakgpu_forest_search.argtypes = [vp, vp, C.POINTER(SearchParams), vp, vp, vp, vp, u32, C.POINTER(SearchOutput), i32, vp, vp, u32]
    lib.oakgpu_forest_nodes.argtypes = [vp, u32, u32, u32, C.POINTER(ForestNode)]
    lib.oakgpu_forest_last_stats.argtypes = [vp, C.POINTER(u64 * 4)]
    lib.oakgpu_forest_create_kept.argtypes = [vp, u32, u32, i32, u32, C.POINTER(vp)]
    lib.oakgpu_forest_create_kept_check.argtypes = [u32, u32, u32]
    lib.oakgpu_forest_kept_tree_bytes.argtypes = [u32, u32]
    lib.oakgpu_forest_kept_tree_bytes.restype = u64
    lib.oakgpu_forest_advance_dev.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    lib.oakgpu_forest_advance.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    lib.oakgpu_forest_search_kept_dev.argtypes = lib.oakgpu_forest_search_dev.argtypes
    lib.oakgpu_forest_search_kept.argtypes = lib.oakgpu_forest_search.argtypes
    lib.oakgpu_forest_keep_stats.argtypes = [vp, C.POINTER(u64 * 4)]
    lib.oakgpu_forest_budgets_check.argtypes = [vp, u32, u64]
    lib.oakgpu_forest_search_budgets_dev.argtypes = [vp, vp, C.POINTER(SearchParams), vp, vp, vp, vp, vp, u32, C.POINTER(ForestOutputs), vp, u32]
    lib.oakgpu_forest_search_budgets.argtypes = [vp, vp, C.POINTER(SearchParams), vp, vp, vp, vp, vp, u32, C.POINTER(SearchOutput), i32, vp, vp, u32]
    lib.oakgpu_forest_search_budgets_kept_dev.argtypes = lib.oakgpu_forest_search_budgets_dev.argtypes
    lib.oakgpu_forest_search_budgets_kept.argtypes = lib.oakgpu_forest_search_budgets.argtypes
    lib.oakgpu_forest_last_rows.argtypes = [vp, C.POINTER(u64 * 2)]
    lib.oakgpu_forest_mismatch.argtypes = [vp, vp, u32, i32]
    lib.oakgpu_forest_node_counts.argtypes = [vp, vp, u32, i32]
    lib.oakgpu_search_stream.argtypes = [vp, C.POINTER(u64)]
    lib.oakgpu_agent_params.argtypes = [vp, C.POINTER(Agent), u32, u64, C.POINTER(SearchParams), C.POINTER(vp)]
    lib.oakgpu_forest_selfplay_check.argtypes = [u32, u32, i32, C.POINTER(SelfplayParams), i32, u32, vp, i32]
    lib.oakgpu_forest_selfplay_dev.argtypes = [vp, vp, C.POINTER(SelfplayParams), vp, vp, vp, u32, i32]
    lib.oakgpu_forest_selfplay_records.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, vp, vp, i32]
    lib.oakgpu_forest_selfplay.argtypes = [vp, vp, C.POINTER(SelfplayParams), vp, vp, vp, u32, i32]
    lib.oakgpu_forest_selfplay_last_stats.argtypes = [vp, C.POINTER(u64 * 4)]
    lib.oakgpu_forest_selfplay_last_traffic.argtypes = [vp, C.POINTER(u64 * 2)]
    lib.oakgpu_forest_selfplay_nodes_kept.argtypes = [vp, vp, i32]
    lib.oakgpu_forest_selfplay_keep_stats.argtypes = [vp, C.POINTER(u64 * 4)]
    lib.oakgpu_forest_selfplay_fast_stats.argtypes = [vp, C.POINTER(u64 * 4)]
    lib.oakgpu_forest_selfplay_set_partition.argtypes = [vp, i32]
    lib.oakgpu_selfplay_prelude_host.argtypes = [C.POINTER(u64), C.c_double, C.POINTER(i32), C.POINTER(u64)]
    lib.oakgpu_forest_selfplay_build_dev.argtypes = [vp, vp, C.POINTER(SelfplayParams), C.POINTER(SelfplaySkip), vp, vp, vp, vp, u32, i32]
    lib.oakgpu_forest_selfplay_build.argtypes = [vp, vp, C.POINTER(SelfplayParams), C.POINTER(SelfplaySkip), vp, vp, vp, vp, u32, i32]
    lib.oakgpu_forest_selfplay_skip_check.argtypes = [u32, C.POINTER(SelfplaySkip)]
    lib.oakgpu_forest_selfplay_matchup.argtypes = [vp, vp, i32]
    lib.oakgpu_selfplay_skip_host.argtypes = [u64, C.c_double, i32]
    lib.oakgpu_selfplay_pick_host.argtypes = [u32, u32, vp, vp, u64, vp, vp, C.c_double, vp, vp, vp, vp, C.c_char_p, C.c_double, C.c_double, C.POINTER(u64),
                                              C.POINTER(C.c_double), vp, vp, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.POINTER(u32)]
    lib.oakgpu_forest_match_check.argtypes = [u32, u32, i32, C.POINTER(ForestMatchParams), u32]
    lib.oakgpu_forest_match_dev.argtypes = [vp, C.POINTER(ForestMatchParams), vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    lib.oakgpu_forest_match.argtypes = [vp, C.POINTER(ForestMatchParams), vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    lib.oakgpu_forest_match_last_stats.argtypes = [vp, C.POINTER(u64 * 4)]
    lib.oakgpu_forest_match_set_records.argtypes = [vp, i32]
    lib.oakgpu_forest_match_records.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, vp, vp, vp, i32]
    lib.oakgpu_match_pick_host.argtypes = [i32, u32, u32, vp, vp, u64, vp, vp, C.c_char_p, C.c_double, C.c_double, C.c_double, C.POINTER(u64), vp,
                                           C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    f32, sz = C.c_float, C.c_size_t
    rows_p, loss_p, outs_p = C.POINTER(EncodedFrames), C.POINTER(TrainLoss), C.POINTER(TrainOutputs)
    lib.oakgpu_frames_symmetries_dev.argtypes = [vp, rows_p, u32, u64, i32, i32]
    lib.oakgpu_trainer_check.argtypes = [vp, sz, u32, u32, loss_p]
    lib.oakgpu_trainer_create.argtypes = [vp, vp, sz, u32, C.POINTER(vp)]
    lib.oakgpu_trainer_destroy.argtypes = [vp]
    lib.oakgpu_trainer_destroy.restype = None
    lib.oakgpu_trainer_shape.argtypes = [vp, C.POINTER(u32 * 24), C.POINTER(sz), C.POINTER(u32)]
    lib.oakgpu_trainer_forward_dev.argtypes = [vp, vp, rows_p, u32, loss_p, outs_p]
    lib.oakgpu_trainer_forward.argtypes = lib.oakgpu_trainer_forward_dev.argtypes
    lib.oakgpu_trainer_gradients_dev.argtypes = [vp, vp, rows_p, u32, loss_p]
    lib.oakgpu_trainer_gradients.argtypes = lib.oakgpu_trainer_gradients_dev.argtypes
    lib.oakgpu_trainer_adam_dev.argtypes = [vp, vp, f32, i32, u32]
    lib.oakgpu_trainer_step_dev.argtypes = [vp, vp, rows_p, u32, loss_p, f32, i32]
    lib.oakgpu_trainer_step.argtypes = lib.oakgpu_trainer_step_dev.argtypes
    lib.oakgpu_trainer_report.argtypes = [vp, vp, C.POINTER(TrainReport), C.POINTER(u64 * 3)]
    lib.oakgpu_trainer_read.argtypes = [vp, vp, i32, vp, sz]
    lib.oakgpu_trainer_set_gradients.argtypes = [vp, vp, vp, sz]
    lib.oakgpu_trainer_net_bytes.argtypes = [vp, vp, vp, sz, C.POINTER(sz)]
    f64, outs_b = C.c_double, C.POINTER(BuildOutputs)
    lib.oakgpu_build_tables.argtypes = [vp, vp, vp]
    lib.oakgpu_build_net_check.argtypes = [vp, sz]
    lib.oakgpu_build_net_load.argtypes = [vp, vp, sz, C.POINTER(vp)]
    lib.oakgpu_build_net_destroy.argtypes = [vp]
    lib.oakgpu_build_net_destroy.restype = None
    lib.oakgpu_build_net_shape.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    lib.oakgpu_build_teams_check.argtypes = [vp, vp, u32, i32]
    lib.oakgpu_build_provide_check.argtypes = [vp, u32, u32, i32, f64, f64, f64]
    lib.oakgpu_build_rollout_dev.argtypes = [vp, vp, vp, vp, vp, u32, i32, outs_b]
    lib.oakgpu_build_rollout.argtypes = lib.oakgpu_build_rollout_dev.argtypes
    lib.oakgpu_build_provide_dev.argtypes = [vp, vp, vp, u32, vp, u32, C.POINTER(BuildProvider), outs_b]
    lib.oakgpu_build_provide.argtypes = lib.oakgpu_build_provide_dev.argtypes
    lib.oakgpu_build_records_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
    lib.oakgpu_build_records.argtypes = lib.oakgpu_build_records_dev.argtypes
    lib.oakgpu_build_game_records_dev.argtypes = [vp, C.POINTER(BuildSeatArrays), C.POINTER(BuildSeatArrays), vp, vp, vp, u32, vp, vp]
    lib.oakgpu_build_window_create.argtypes = [vp, u32, C.POINTER(vp)]
    lib.oakgpu_build_window_destroy.argtypes = [vp]
    lib.oakgpu_build_window_destroy.restype = None
    lib.oakgpu_build_window_append_dev.argtypes = [vp, vp, vp, vp, u32]
    lib.oakgpu_build_window_append.argtypes = [vp, vp, vp, sz]
    lib.oakgpu_build_window_corpus.argtypes = [vp]
    lib.oakgpu_build_window_corpus.restype = vp
    lib.oakgpu_build_window_records.argtypes = [vp, vp, sz, C.POINTER(sz)]
    lib.oakgpu_build_window_stats.argtypes = [vp, C.POINTER(u64 * 4)]
    lib.oakgpu_build_game_targets_host.argtypes = [i32, C.c_uint8, C.c_double, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    traj_p, prm_t = C.POINTER(BuildTrajectories), C.POINTER(BuildTrajParams)
    lib.oakgpu_build_traj_check.argtypes = [vp, sz, vp]
    lib.oakgpu_build_corpus_create.argtypes = [vp, vp, sz, C.POINTER(sz), u32, C.POINTER(vp)]
    lib.oakgpu_build_corpus_destroy.argtypes = [vp]
    lib.oakgpu_build_corpus_destroy.restype = None
    lib.oakgpu_build_corpus_scan_dev.argtypes = [vp, vp]
    lib.oakgpu_build_corpus_info.argtypes = [vp, C.POINTER(BuildCorpusStats)]
    lib.oakgpu_build_traj_dev.argtypes = [vp, vp, vp, u32, prm_t, traj_p]
    lib.oakgpu_build_traj.argtypes = lib.oakgpu_build_traj_dev.argtypes
    lib.oakgpu_build_traj_sample_dev.argtypes = [vp, vp, u32, u64, prm_t, vp, traj_p]
    lib.oakgpu_build_traj_sample.argtypes = lib.oakgpu_build_traj_sample_dev.argtypes
    lib.oakgpu_build_targets_dev.argtypes = [vp, traj_p, u32, f64, C.POINTER(BuildTargetOutputs)]
    lib.oakgpu_build_targets.argtypes = lib.oakgpu_build_targets_dev.argtypes
    lib.oakgpu_build_state_dense_dev.argtypes = [vp, vp, vp, u32, u32, vp]
    lib.oakgpu_build_state_dense.argtypes = lib.oakgpu_build_state_dense_dev.argtypes
    chunk_p = C.POINTER(BuildChunk)
    lib.oakgpu_build_trainer_check.argtypes = [vp, sz, u32]
    lib.oakgpu_build_trainer_create.argtypes = [vp, vp, sz, u32, C.POINTER(vp)]
    lib.oakgpu_build_trainer_destroy.argtypes = [vp]
    lib.oakgpu_build_trainer_destroy.restype = None
    lib.oakgpu_build_trainer_shape.argtypes = [vp, C.POINTER(u32 * 12), C.POINTER(sz), C.POINTER(u32)]
    lib.oakgpu_build_trainer_forward_dev.argtypes = [vp, vp, chunk_p, C.POINTER(BuildTrainOutputs)]
    lib.oakgpu_build_trainer_accumulate_dev.argtypes = [vp, vp, chunk_p]
    lib.oakgpu_build_trainer_zero_gradients_dev.argtypes = [vp, vp]
    lib.oakgpu_build_trainer_adam_dev.argtypes = [vp, vp, C.c_float]
    lib.oakgpu_build_trainer_average_dev.argtypes = [vp, vp, f64]
    lib.oakgpu_build_trainer_report.argtypes = [vp, vp, C.POINTER(BuildTrainReport)]
    lib.oakgpu_build_trainer_read.argtypes = [vp, vp, i32, vp, sz]
    lib.oakgpu_build_trainer_set_gradients.argtypes = [vp, vp, vp, sz]
    lib.oakgpu_build_trainer_net_bytes.argtypes = [vp, vp, i32, vp, sz, C.POINTER(sz)]
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise OakGpuError("liboakgpu: %s (code %d)" % (load().oakgpu_last_error().decode(), rc))
