"""ctypes binding of libnavenv.so (include/navenv.h) — the only way this package computes.

Loaded after `import torch` so the library binds torch's already-loaded HIP runtime
(libamdhip64.so.7, same SONAME as /opt/rocm's). There is no fallback: if the library is missing or
a call fails, an exception is raised.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must be loaded first: provides the HIP runtime)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnavenv.so")
_lib_path = LIB_PATH
NAV_EINVAL = -100000
ABI_VERSION = 11

_dp = C.POINTER(C.c_double)
_vp = C.c_void_p


class NavParams(C.Structure):
    _fields_ = [
        ("world_size", C.c_double), ("max_action", C.c_double), ("init_region_size", C.c_double),
        ("goal_threshold", C.c_double), ("goal_reward", C.c_double),
        ("stuck_threshold", C.c_double), ("stuck_penalty", C.c_double),
        ("demo_factor", C.c_double), ("noise_decay", C.c_double),
        ("path_length0", C.c_int32), ("path_increase", C.c_int32),
        ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("max_goal_draws", C.c_int32),
    ]


class NavEnvSoa(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("state", _vp), ("goal", _vp), ("region", _vp), ("hist", _vp),
        ("meta", _vp), ("plan_index", _vp), ("path_length", _vp), ("episodes", _vp),
        ("noise_scale", _vp),
    ]


class NavStepOut(C.Structure):
    _fields_ = [("next_state", _vp), ("goal_term", _vp), ("flags", _vp), ("block_stats", _vp)]


class NavReplay(C.Structure):
    _fields_ = [("rows", _vp), ("capacity", C.c_int64)]


class NavPer(C.Structure):
    """nav_per: the priority store beside a replay ring (prioritised replay)."""
    _fields_ = [("pri", _vp), ("sums", _vp), ("stat", _vp), ("capacity", C.c_int64)]


class NavMlp(C.Structure):
    _fields_ = [
        ("d_in", C.c_int32), ("d_out", C.c_int32), ("hidden", C.c_int32),
        ("hidden_pad", C.c_int32), ("n_hidden", C.c_int32), ("params", _vp), ("packed", _vp),
    ]


class NavTestOut(C.Structure):
    _fields_ = [("reached", _vp), ("steps", _vp), ("best_distance", _vp), ("final_state", _vp),
                ("traj", _vp)]


class NavPopScore(C.Structure):
    """nav_pop_score: one member's reduction of a population test rollout."""
    _fields_ = [("reached", C.c_int64), ("steps_reached", C.c_int64), ("sum_best", C.c_double),
                ("max_best", C.c_double)]


class NavTd3Member(C.Structure):
    """nav_td3_member: one member of the population learner (its networks, ring, moments,
    hyper-parameters, injected samples and workspace)."""
    _fields_ = [
        ("actor", NavMlp), ("critics", NavMlp * 2), ("target_actor", NavMlp),
        ("target_critics", NavMlp * 2), ("replay", NavReplay),
        ("m_actor", _vp), ("v_actor", _vp), ("m_critic", _vp * 2), ("v_critic", _vp * 2),
        ("actor_lr", C.c_double), ("critic_lr", C.c_double),
        ("policy_noise", C.c_float), ("noise_clip", C.c_float), ("max_action", C.c_float),
        ("gamma", C.c_float), ("tau", C.c_float),
        ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
        ("idx_critic", _vp), ("idx_actor", _vp), ("eps", _vp),
        ("batch", _vp), ("batch_actor", _vp), ("dq", _vp * 2), ("loss_part", _vp * 2),
        ("edge_slabs", _vp * 2), ("edge_slabs_actor", _vp), ("acts", _vp * 2),
        ("acts_actor", _vp), ("dz", _vp * 2), ("dz_actor", _vp), ("masks", _vp * 2),
        ("masks_actor", _vp), ("q", _vp), ("da", _vp), ("hidden_slabs", _vp * 2),
        ("grad_critic", _vp * 2), ("grad_actor", _vp),
    ]


class NavTd3MemberBc(C.Structure):
    """nav_td3_member_bc: one member's demonstration mix and BC term beside its nav_td3_member."""
    _fields_ = [("B_demo", C.c_int64), ("n_demo", C.c_int64), ("q_weight", C.c_float),
                ("bc_weight", C.c_float), ("idx_critic", _vp), ("idx_actor", _vp),
                ("bc_part", _vp)]


# (name, restype, argtypes) for every entry point of include/navenv.h
_P = C.POINTER
SIGNATURES = [
    ("nav_abi_version", C.c_int, []),
    ("nav_default_params", None, [_P(NavParams)]),
    ("nav_mlp_param_count", C.c_int64, [C.c_int32] * 4),
    ("nav_mlp_packed_count", C.c_int64, [C.c_int32] * 2),
    ("nav_mlp_layer_offsets", C.c_int, [_P(NavMlp), C.c_int32, _P(C.c_int64), _P(C.c_int64)]),
    ("nav_env_init", C.c_int, [_P(NavParams), _P(NavEnvSoa), C.c_int32, C.c_int32, _vp, _vp]),
    ("nav_env_reset", C.c_int, [_P(NavParams), _P(NavEnvSoa), _vp, _vp, _vp]),
    ("nav_env_step", C.c_int, [_P(NavParams), _P(NavEnvSoa), _vp, _vp, _vp, _vp]),
    ("nav_dynamics", C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _vp]),
    ("nav_env_step_k", C.c_int, [_P(NavParams), _P(NavEnvSoa), _vp, _vp, C.c_int32, _vp, _vp]),
    ("nav_agent_step", C.c_int, [_P(NavParams), _P(NavEnvSoa), _vp, _vp, _P(NavReplay),
                                 C.c_int64, _P(NavStepOut), C.c_int32, _vp]),
    ("nav_demo_reward", C.c_int, [_P(NavParams), C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int64,
                                  C.c_int32, _P(NavReplay), C.c_int64, _vp, _vp, _vp]),
    ("nav_transition", C.c_int, [_P(NavParams), _P(NavEnvSoa), _vp, _vp, _vp, _P(NavReplay),
                                 C.c_int64, _P(NavStepOut), C.c_int32, _vp]),
    ("nav_check_if_stuck", C.c_int, [_P(NavParams), _P(NavEnvSoa), _vp, _vp, _vp]),
    ("nav_rollout", C.c_int, [_vp, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("nav_cem_rollout", C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("nav_cem_elite", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp,
                                _vp, _vp]),
    ("nav_replay_push", C.c_int, [_P(NavReplay), C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp,
                                  _vp]),
    ("nav_demo_index_plan", C.c_int, [_vp, _vp, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    ("nav_demo_index_scan", C.c_int, [_vp, C.c_int32, _vp, _vp]),
    ("nav_demo_index_fill", C.c_int, [_vp, _vp, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp]),
    ("nav_demo_index_res", C.c_int32, []),
    ("nav_fields_generate", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("nav_demo_augment", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp,
                                   _vp]),
    ("nav_demo_index_subplan", C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    ("nav_demo_index_subscan", C.c_int, [_vp, C.c_int32, _vp, _vp]),
    ("nav_demo_index_subfill", C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("nav_demo_reward_indexed", C.c_int, [_P(NavParams), C.c_int64, _vp, _vp, _vp, _vp, _vp,
                                          C.c_int32, _vp, _vp, _P(NavReplay), C.c_int64, _vp,
                                          _vp, _vp]),
    ("nav_agent_step_indexed", C.c_int, [_P(NavParams), _P(NavEnvSoa), _vp, _vp, _P(NavReplay),
                                         C.c_int64, _P(NavStepOut), _vp, _vp, C.c_int32, _vp,
                                         _vp, _vp, _vp]),
    ("nav_demo_min", C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _vp, _vp]),
    ("nav_compute_reward", C.c_int, [_P(NavParams), C.c_int64, _vp, _vp, _vp, C.c_int64,
                                     C.c_int32, _vp, _vp, _vp]),
    ("nav_act", C.c_int, [_P(NavParams), _P(NavMlp), C.c_int64, _vp, _vp, _vp, _vp, C.c_uint32,
                          C.c_int32, _vp, _vp, _vp]),
    ("nav_act_tick", C.c_int, [_P(NavParams), _P(NavMlp), _P(NavEnvSoa), _vp, _vp, C.c_uint32,
                               C.c_int32, _P(NavReplay), C.c_int64, _P(NavStepOut), _vp, _vp,
                               C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    ("nav_test_rollout", C.c_int, [_P(NavParams), _P(NavMlp), _P(NavEnvSoa), _vp, _vp,
                                   C.c_uint32, C.c_int32, _P(NavTestOut), _vp]),
    ("nav_pop_table_bytes", C.c_int64, [C.c_int32]),
    ("nav_pop_table_build", C.c_int, [_P(NavParams), _P(NavMlp), _P(NavReplay), C.c_int32,
                                      C.c_int32, _vp, _vp]),
    ("nav_act_tick_pop", C.c_int, [_P(NavParams), _P(NavMlp), _P(NavReplay), C.c_int32,
                                   C.c_int32, _vp, _P(NavEnvSoa), _vp, _vp, C.c_uint32,
                                   C.c_int32, C.c_int64, _P(NavStepOut), _vp, _vp, C.c_int32,
                                   _vp, _vp, _vp, _vp, _vp]),
    ("nav_test_rollout_pop", C.c_int, [_P(NavParams), _P(NavMlp), C.c_int32, C.c_int32, _vp,
                                       _P(NavEnvSoa), _vp, _vp, C.c_uint32, C.c_int32,
                                       _P(NavTestOut), _vp]),
    ("nav_pop_test_summary", C.c_int, [_P(NavTestOut), C.c_int32, C.c_int32, _vp, _vp]),
    ("nav_mlp_forward", C.c_int, [_P(NavMlp), C.c_int32, C.c_int64, _vp, C.c_int32, C.c_int32,
                                  _P(_vp), C.c_int32, C.c_int32, C.c_int32, _vp, C.c_float,
                                  C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32,
                                  _P(_vp), C.c_uint32, _P(_vp), _vp]),
    ("nav_td3_critic_rows", C.c_int, [_P(NavMlp), _P(NavMlp), _P(NavMlp), _P(NavReplay),
                                      C.c_int64, C.c_int64, _vp, C.c_uint32, C.c_uint32,
                                      C.c_uint32, _vp, C.c_float, C.c_float, C.c_float, C.c_float,
                                      _vp, _P(_vp), _P(_vp), _P(_vp), _P(_vp), C.c_uint32,
                                      _P(_vp), C.c_int32, _P(_vp), C.c_uint32, C.c_int32,
                                      _vp]),
    ("nav_td3_critic_rows_w", C.c_int, [_P(NavMlp), _P(NavMlp), _P(NavMlp), _P(NavReplay),
                                        C.c_int64, C.c_int64, _vp, C.c_uint32, C.c_uint32,
                                        C.c_uint32, _vp, C.c_float, C.c_float, C.c_float,
                                        C.c_float, _vp, _P(_vp), _P(_vp), _P(_vp), _P(_vp),
                                        C.c_uint32, _P(_vp), C.c_int32, _P(_vp), C.c_uint32,
                                        C.c_int32, _vp, _P(_vp), _vp]),
    ("nav_td3_actor_rows", C.c_int, [_P(NavMlp), _P(NavMlp), _P(NavReplay), C.c_int64,
                                     C.c_int64, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp,
                                     _vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp,
                                     _vp]),
    ("nav_td3_actor_rows_bc", C.c_int, [_P(NavMlp), _P(NavMlp), _P(NavReplay), C.c_int64,
                                        C.c_int64, _vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp, _vp, _vp,
                                        C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp, _vp]),
    ("nav_td3_actor_rows_bcq", C.c_int, [_P(NavMlp), _P(NavMlp), _P(NavReplay), C.c_int64,
                                         C.c_int64, _vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp,
                                         _vp]),
    ("nav_td3_mix_idx", C.c_int, [C.c_int64] * 5 + [C.c_uint32] * 3 + [_vp, _vp, _vp]),
    ("nav_demo_transitions", C.c_int, [_P(NavParams), C.c_int32, C.c_int32, _vp, _vp, _vp,
                                       C.c_int32, _vp, _vp]),
    ("nav_per_sums_count", C.c_int64, [C.c_int64]),
    ("nav_per_init", C.c_int, [_P(NavPer), _vp]),
    ("nav_per_stamp", C.c_int, [_P(NavPer), C.c_int64, C.c_int64, _vp]),
    ("nav_per_sums", C.c_int, [_P(NavPer), C.c_int64, _vp]),
    ("nav_per_sample", C.c_int, [_P(NavPer), C.c_int64, C.c_int64, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_float, _vp, _vp, _vp, _vp]),
    ("nav_per_update", C.c_int, [_P(NavPer), C.c_int64, _vp, _vp, _vp, C.c_float, C.c_float,
                                 _vp]),
    ("nav_nstep_stamp", C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp]),
    ("nav_nstep_rows", C.c_int, [_P(NavReplay), _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                 C.c_float, C.c_int64, _vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                 _vp, _vp, _vp]),
    ("nav_demo_reset", C.c_int, [_P(NavEnvSoa), _vp, C.c_uint32, C.c_uint32, _vp, _vp, C.c_int32,
                                 C.c_int32, C.c_int32, C.c_double, _vp, _vp, _vp]),
    ("nav_mlp_mask_count", C.c_int64, [C.c_int32, C.c_int32, C.c_int64]),
    ("nav_mlp_row_blocks", C.c_int64, [C.c_int64]),
    ("nav_mlp_edge_count", C.c_int64, [C.c_int32] * 4),
    ("nav_mlp_hidden_count", C.c_int64, [C.c_int32] * 2),
    ("nav_td3_critic_forward", C.c_int, [_P(NavMlp), C.c_int64, _vp, C.c_int32, C.c_int32, _vp,
                                         _vp, _vp, C.c_float, _P(_vp), _P(_vp), _P(_vp),
                                         _P(_vp), C.c_uint32, _P(_vp), _vp]),
    ("nav_mlp_backward", C.c_int, [_P(NavMlp), C.c_int32, C.c_int64, _P(_vp), C.c_int32, _P(_vp),
                                   _vp, C.c_int32, C.c_int32, _P(_vp), _P(_vp), C.c_uint32,
                                   _P(_vp), _P(_vp), _vp]),
    ("nav_mlp_wgrad", C.c_int, [_P(NavMlp), C.c_int32, C.c_int64, _vp, C.c_int32, C.c_int32,
                                _P(_vp), _P(_vp), _P(_vp), C.c_int32, _P(_vp), _P(_vp), C.c_int32,
                                _vp]),
    ("nav_mlp_wgrad_splits", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int64]),
    ("nav_grad_reduce", C.c_int, [_P(NavMlp), _vp, C.c_int32, _vp, C.c_int64, _vp, _vp]),
    ("nav_grad_reduce_adam", C.c_int, [_P(NavMlp), C.c_int32, _P(_vp), C.c_int32, _P(_vp),
                                       C.c_int64, _P(_vp), _P(_vp), _P(_vp), C.c_float, C.c_float,
                                       C.c_float, _P(C.c_float), _P(C.c_float), _vp]),
    ("nav_grad_reduce_adam_polyak", C.c_int,
     [_P(NavMlp), C.c_int32, _P(_vp), C.c_int32, _P(_vp), C.c_int64, _P(_vp), _P(_vp), _P(_vp),
      C.c_float, C.c_float, C.c_float, _P(C.c_float), _P(C.c_float), _P(NavMlp), _P(NavMlp),
      _P(NavMlp), C.c_int32, C.c_float, _vp]),
    ("nav_grad_reduce_multi", C.c_int, [_P(NavMlp), C.c_int32, _P(_vp), C.c_int32, _P(_vp),
                                        C.c_int64, _P(_vp), _vp]),
    ("nav_adam_multi", C.c_int, [_P(NavMlp), C.c_int32, _P(_vp), _P(_vp), _P(_vp), C.c_float,
                                 C.c_float, C.c_float, _P(C.c_float), _P(C.c_float), C.c_float,
                                 _vp]),
    ("nav_adam_polyak_multi", C.c_int, [_P(NavMlp), C.c_int32, _P(_vp), _P(_vp), _P(_vp),
                                        C.c_float, C.c_float, C.c_float, _P(C.c_float),
                                        _P(C.c_float), C.c_float, _P(NavMlp), _P(NavMlp),
                                        _P(NavMlp), C.c_int32, C.c_float, _vp]),
    ("nav_adam", C.c_int, [_P(NavMlp), _vp, _vp, _vp, C.c_float, C.c_float, C.c_float,
                           C.c_float, C.c_float, _vp]),
    ("nav_polyak", C.c_int, [_P(NavMlp), _P(NavMlp), C.c_float, _vp]),
    ("nav_polyak_multi", C.c_int, [_P(NavMlp), _P(NavMlp), C.c_int32, C.c_float, _vp]),
    ("nav_mlp_pack", C.c_int, [_P(NavMlp), _vp]),
    ("nav_replay_sample", C.c_int, [_P(NavReplay), C.c_int64, C.c_int64, _vp, C.c_uint32,
                                    C.c_uint32, C.c_uint32, _vp, _vp]),
    ("nav_fill", C.c_int, [_vp, C.c_int64, C.c_float, _vp]),
    ("nav_strided_copy", C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32,
                                   C.c_int64, C.c_int32, _vp]),
    ("nav_td3_pop_table_bytes", C.c_int64, [C.c_int32]),
    ("nav_td3_pop_table_build", C.c_int, [_P(NavTd3Member), C.c_int32, C.c_int64, C.c_int32,
                                          C.c_int32, _vp, _vp]),
    ("nav_td3_critic_rows_pop", C.c_int, [_P(NavTd3Member), C.c_int32, C.c_int64, _vp, C.c_int64,
                                          C.c_uint32, C.c_int32, _vp]),
    ("nav_td3_actor_rows_pop", C.c_int, [_P(NavTd3Member), C.c_int32, C.c_int64, _vp, C.c_int64,
                                         C.c_uint32, _vp]),
    ("nav_td3_pop_bc_table_bytes", C.c_int64, [C.c_int32]),
    ("nav_td3_pop_bc_table_build", C.c_int, [_P(NavTd3Member), _P(NavTd3MemberBc), C.c_int32,
                                             C.c_int64, _vp, _vp]),
    ("nav_td3_mix_idx_pop", C.c_int, [_P(NavTd3Member), _P(NavTd3MemberBc), C.c_int32, C.c_int64,
                                      _vp, C.c_int64, C.c_uint32, C.c_int32, _vp]),
    ("nav_td3_actor_rows_bc_pop", C.c_int, [_P(NavTd3Member), _P(NavTd3MemberBc), C.c_int32,
                                            C.c_int64, _vp, C.c_int64, C.c_uint32, _vp]),
    ("nav_mlp_wgrad_splits_pop", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_int64]),
    ("nav_mlp_wgrad_pop", C.c_int, [_P(NavTd3Member), C.c_int32, C.c_int64, _vp, C.c_int32,
                                    C.c_int32, _vp]),
    ("nav_grad_reduce_adam_pop", C.c_int, [_P(NavTd3Member), C.c_int32, C.c_int64, _vp,
                                           C.c_int32, C.c_float, C.c_float, C.c_float,
                                           C.c_double, C.c_float, C.c_int32, _vp]),
    ("nav_td3_pop_state_bytes", C.c_int64, [C.c_int32]),
    ("nav_td3_pop_state_build", C.c_int, [_P(NavTd3Member), C.c_int32, _vp, _vp]),
    ("nav_td3_pop_exploit", C.c_int, [_P(NavTd3Member), C.c_int32, _vp, _P(C.c_int32),
                                      _P(C.c_int32), C.c_int32, C.c_int64, _vp]),
    ("nav_event_create", C.c_int, [_P(_vp)]),
    ("nav_event_destroy", C.c_int, [_vp]),
    ("nav_event_record", C.c_int, [_vp, _vp]),
    ("nav_event_elapsed_ms", C.c_int, [_vp, _vp, _P(C.c_float)]),
]

# Entry points that return int64 counts (negative = error) rather than a status code.
_COUNT_FNS = {"nav_mlp_param_count", "nav_mlp_packed_count", "nav_mlp_mask_count",
              "nav_mlp_row_blocks", "nav_mlp_edge_count", "nav_mlp_hidden_count",
              "nav_mlp_wgrad_splits", "nav_demo_index_res", "nav_pop_table_bytes",
              "nav_td3_pop_table_bytes", "nav_mlp_wgrad_splits_pop",
              "nav_td3_pop_state_bytes", "nav_td3_pop_bc_table_bytes",
              "nav_per_sums_count"}


class NavError(RuntimeError):
    pass


class _Checked:
    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __call__(self, *args):
        r = self.fn(*args)
        if self.name in _COUNT_FNS:
            if r < 0:
                raise NavError(f"{self.name}: invalid argument")
        elif self.fn.restype is C.c_int and r != 0 and self.name != "nav_abi_version":
            what = "invalid argument" if r == NAV_EINVAL else f"HIP error {-r}"
            raise NavError(f"{self.name} failed: {what}")
        return r


class _Lib:
    def __init__(self, path):
        if not os.path.exists(path):
            raise NavError(f"{path} is missing: build it with `make -C "
                           f"residual-td3-robot-navigation_amd` (or __graft_entry__.build())")
        self.raw = C.CDLL(path)
        for name, res, args in SIGNATURES:
            fn = getattr(self.raw, name)
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, _Checked(name, fn))
        v = self.nav_abi_version()
        if v != ABI_VERSION:
            raise NavError(f"libnavenv ABI {v} != {ABI_VERSION}")


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _Lib(_lib_path)
    return _lib


def lib_path():
    """The library this process binds (libnavenv.so next to this file unless a tuning tool chose
    another build through use_library)."""
    return _lib_path


def use_library(path):
    """Bind another build of the same ABI instead of the in-tree libnavenv.so. For the A/B timing
    tools only (tools/withlib.py); must run before the first call into the library."""
    global _lib_path
    path = os.path.abspath(path)
    if _lib is not None and path != _lib_path:
        raise NavError(f"libnavenv is already loaded from {_lib_path}")
    _lib_path = path


def require_gpu():
    if not torch.cuda.is_available():
        raise NavError("nav needs a ROCm GPU (MI355X); no HIP device is visible")


def ptr(t):
    """Device pointer of a contiguous tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "nav tensors must be contiguous"
    return C.c_void_p(t.data_ptr())


def parr(*tensors):
    """C array of device pointers (None entries allowed) for the pointer-array parameters."""
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def descs(*nets):
    """C array of nav_mlp descriptors."""
    return (NavMlp * len(nets))(*[n.desc() for n in nets])


def stream_handle(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def params_struct(**kw):
    p = NavParams()
    lib().nav_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p
