"""ctypes binding of ``libgridpf.so`` (C ABI: ``include/gridpf.h``).

There is NO fallback: if the shared library is missing or no HIP device is available the engine
cannot be created and every call raises `GridPFError`.  (The CPU oracle under ``oracle/`` is test
infrastructure only and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

__all__ = ["lib", "GridPFError", "GpfGridDesc", "GpfLayout", "GpfStepOpts", "GpfOpponentDesc", "GpfAlertDesc", "GpfRewardSlot", "GpfEpisodeDesc", "GpfCursorDesc", "GpfCombinedDesc", "library_path", "SIGNATURES", "EXPORTED_SYMBOLS"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libgridpf.so"
ABI_VERSION = 326          # include/gridpf.h GPF_ABI_VERSION
N_ALERT_POINTERS = 3       # include/gridpf.h GPF_N_ALERT_POINTERS
N_REWARD_POINTERS = 1      # include/gridpf.h GPF_N_REWARD_POINTERS
N_EPISODE_POINTERS = 8     # include/gridpf.h GPF_N_EPISODE_POINTERS
N_N1_POINTERS = 4          # include/gridpf.h GPF_N_N1_POINTERS
N_LOOKAHEAD_POINTERS = 6   # include/gridpf.h GPF_N_LOOKAHEAD_POINTERS
N_LOOKAHEAD_CHAIN_POINTERS = 5   # include/gridpf.h GPF_N_LOOKAHEAD_CHAIN_POINTERS
N_CURSOR_POINTERS = 3      # include/gridpf.h GPF_N_CURSOR_POINTERS
N_COMBINED_POINTERS = 1    # include/gridpf.h GPF_N_COMBINED_POINTERS
N_DEVICE_POINTERS = 34     # include/gridpf.h GPF_N_DEVICE_POINTERS
GRAPH_N_SECTIONS = 8       # include/gridpf.h GPF_GRAPH_N_SECTIONS
GRAPH_N_FEATURES = 4       # include/gridpf.h GPF_GRAPH_N_FEATURES
GRAPH_MAX_BUS = 1024       # include/gridpf.h GPF_GRAPH_MAX_BUS


class GridPFError(RuntimeError):
    pass


def library_path() -> str:
    return os.environ.get("GRIDPF_LIB", os.path.join(_HERE, _LIB_NAME))


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)
_bp = C.POINTER(C.c_uint8)
_vpp = C.POINTER(C.c_void_p)


class GpfGridDesc(C.Structure):
    _fields_ = [
        ("n_sub", C.c_int32), ("n_busbar", C.c_int32),
        ("n_line", C.c_int32), ("n_gen", C.c_int32), ("n_load", C.c_int32), ("n_storage", C.c_int32),
        ("n_shunt", C.c_int32), ("dim_topo", C.c_int32),
        ("sn_mva", C.c_double),
        ("sub_vn_kv", _dp),
        ("line_or_sub", _ip), ("line_ex_sub", _ip), ("line_or_pos_topo_vect", _ip), ("line_ex_pos_topo_vect", _ip),
        ("br_y", _dp), ("br_bdc", _dp),
        ("gen_sub", _ip), ("gen_pos_topo_vect", _ip), ("gen_min_q", _dp), ("gen_max_q", _dp), ("gen_slack", _bp),
        ("load_sub", _ip), ("load_pos_topo_vect", _ip),
        ("storage_sub", _ip), ("storage_pos_topo_vect", _ip),
        ("shunt_sub", _ip), ("shunt_fact", _dp),
        ("init_inj", _dp), ("init_topo", _ip), ("init_shunt_bus", _ip),
    ]


class GpfOpponentDesc(C.Structure):
    """include/gridpf.h gpf_opponent_desc"""
    _fields_ = [
        ("kind", C.c_int32), ("n_lines", C.c_int32), ("line_ids", _ip), ("rho_normalization", _dp), ("attack_period", C.c_int32),
        ("attack_hazard_rate", C.c_double), ("recovery_rate", C.c_double), ("recovery_minimum_duration", C.c_int32),
        ("pmax_pmin_ratio", C.c_double), ("episode_max_time", C.c_int32), ("init_budget", C.c_float), ("budget_per_ts", C.c_float),
        ("attack_duration", C.c_int32), ("attack_cooldown", C.c_int32), ("draw_source", C.c_int32), ("seed_lo", C.c_uint32),
        ("seed_hi", C.c_uint32), ("lane_base", C.c_int32), ("schedule_cap", C.c_int32),
    ]


class GpfRewardSlot(C.Structure):
    """include/gridpf.h gpf_reward_slot"""
    _fields_ = [("kind", C.c_int32), ("p", C.c_double * 6)]


class GpfEpisodeDesc(C.Structure):
    """include/gridpf.h gpf_episode_desc"""
    _fields_ = [("max_steps", C.c_int32), ("lane_max_steps", _ip), ("per_timestep", C.c_float), ("alert_end_bonus", C.c_float)]


class GpfCursorDesc(C.Structure):
    """include/gridpf.h gpf_cursor_desc"""
    _fields_ = [("n_order", C.c_int32), ("order", _ip), ("policy", C.c_int32), ("cdf", _dp), ("first_row", C.c_int32), ("lane_first_row", _ip),
                ("next_pos", C.c_int32), ("lane_next_pos", _ip), ("draw_source", C.c_int32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
                ("lane_base", C.c_int32)]


class GpfCombinedDesc(C.Structure):
    """include/gridpf.h gpf_combined_desc"""
    _fields_ = [("on", C.c_int32), ("check_values", C.c_int32), ("storage_max_p_prod", _fp), ("storage_max_p_absorb", _fp)]


class GpfAlertDesc(C.Structure):
    """include/gridpf.h gpf_alert_desc"""
    _fields_ = [("time_window", C.c_int32), ("reward_min_no_blackout", C.c_float), ("reward_min_blackout", C.c_float),
                ("reward_max_no_blackout", C.c_float), ("reward_max_blackout", C.c_float)]


class GpfLayout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_inj", "inj_gen_p", "inj_gen_vm", "inj_load_p", "inj_load_q", "inj_storage_p", "inj_storage_q",
        "inj_shunt_p", "inj_shunt_q",
        "n_out", "out_p_or", "out_q_or", "out_v_or", "out_a_or", "out_theta_or",
        "out_p_ex", "out_q_ex", "out_v_ex", "out_a_ex", "out_theta_ex",
        "out_gen_p", "out_gen_q", "out_gen_v", "out_gen_theta",
        "out_load_p", "out_load_q", "out_load_v", "out_load_theta",
        "out_storage_p", "out_storage_q", "out_storage_v", "out_storage_theta",
        "out_shunt_p", "out_shunt_q", "out_shunt_v",
        "n_chron", "chron_load_p", "chron_load_q", "chron_prod_p", "chron_prod_v", "nb_total")]


class GpfStepOpts(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("tol_mva", C.c_double), ("rebalance", C.c_double), ("cascade", C.c_int32),
                ("hard_overflow", C.c_float), ("soft_overflow", C.c_float), ("nb_ts_allowed", C.c_int32), ("max_rounds", C.c_int32),
                ("is_dc", C.c_int32), ("auto_reset", C.c_int32), ("warm_start", C.c_int32), ("track_cooldown", C.c_int32), ("nb_ts_reco", C.c_int32)]


def _sig(*argtypes, res=C.c_int):
    return list(argtypes), res


h, i32, i64, u32, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_double
# The ONE statement of the C ABI on this side: symbol -> (argtypes, restype), in the order of include/gridpf.h's features.  `lib` binds
# every row, EXPORTED_SYMBOLS is its keys, and tests/test_capi_symbols.py holds every row to the header's prototype.
SIGNATURES = {
    "gpf_last_error": _sig(res=C.c_char_p),
    "gpf_version": _sig(),
    "gpf_set_deterministic": _sig(h, i32),
    "gpf_device_count": _sig(_ip),
    "gpf_create": _sig(C.POINTER(GpfGridDesc), i32, i32, _vpp),
    "gpf_destroy": _sig(h),
    "gpf_get_layout": _sig(h, C.POINTER(GpfLayout)),
    "gpf_n_lanes": _sig(h),
    "gpf_set_injections": _sig(h, i32, i32, _dp),
    "gpf_set_topology": _sig(h, i32, i32, _ip, _ip),
    "gpf_get_injections": _sig(h, i32, i32, _dp),
    "gpf_get_topology": _sig(h, i32, i32, _ip, _ip),
    "gpf_disconnect_line": _sig(h, i32, i32),
    "gpf_reset_lanes": _sig(h, i32, i32),
    "gpf_copy_lanes": _sig(h, i32, i32, i32),
    "gpf_fanout_n1": _sig(h, i32, i32, i32, _ip),
    "gpf_runpf": _sig(h, i32, i32, i32, i32, f64),
    "gpf_solve_lane": _sig(h, i32, _dp, _ip, _ip, i32, i32, f64, _fp, _ip, _ip, _bp, _ip, _dp, _dp),
    "gpf_get_results": _sig(h, i32, i32, _fp, _ip, _ip, _bp, _ip, _dp, _dp),
    "gpf_upload_chronics": _sig(h, i32, i32, _fp),
    "gpf_upload_maintenance": _sig(h, i32, i32, _bp),
    "gpf_upload_hazards": _sig(h, i32, i32, _bp),
    "gpf_set_lane_chronics": _sig(h, _ip, _ip, _fp),
    "gpf_set_thermal_limits": _sig(h, _fp),
    "gpf_step": _sig(h, i32, i32, f64, f64, i32, f32, f32, i32, i32, i32),
    "gpf_step_n": _sig(h, i32, i32, C.POINTER(GpfStepOpts)),
    "gpf_set_lane_redispatch": _sig(h, _fp),
    "gpf_set_gen_limits": _sig(h, _dp, _dp, _dp, _dp, _bp, f64),
    "gpf_redispatch": _sig(h, i32, i32, _dp, _dp, _dp, _dp, _bp, _dp, i32, _bp, _fp),
    "gpf_set_trajectory": _sig(h, i32, i32),
    "gpf_get_trajectory": _sig(h, i32, i32, i32, i32, _fp, C.POINTER(C.c_int8)),
    "gpf_get_trajectory_obs": _sig(h, i32, i32, i32, i32, _fp, _ip, _ip, _bp),
    "gpf_upload_forecasts": _sig(h, i32, i32, i32, _fp),
    "gpf_simulate_batch": _sig(h, i32, i32, i32, _ip, i32, _ip, _ip, _ip, i32, C.POINTER(GpfStepOpts)),
    "gpf_set_overflow_count": _sig(h, i32, i32, _ip),
    "gpf_set_storage_params": _sig(h, _dp, _dp, _dp, _dp, _dp, _fp, f64, i32),
    "gpf_set_env_dynamics": _sig(h, i32, f64),
    "gpf_set_lane_actions": _sig(h, _fp, _fp, i32),
    "gpf_lane_actions_on_device": _sig(h, i32, i32, i32, i32),
    "gpf_get_env_state": _sig(h, i32, i32, _fp, _fp, _fp, _bp, _fp, _fp, _fp, _fp),
    "gpf_get_env_illegal": _sig(h, i32, i32, _ip),
    "gpf_set_env_illegal": _sig(h, i32, i32, _ip),
    "gpf_set_env_state": _sig(h, i32, i32, _fp, _fp, _fp, _bp, _fp, _fp, _fp, _fp),
    "gpf_set_gen_renewable": _sig(h, _bp),
    "gpf_set_lane_curtailment": _sig(h, _fp),
    "gpf_get_episode": _sig(h, i32, i32, _bp, _ip),
    "gpf_lane_capacity": _sig(h),
    "gpf_get_step_outputs": _sig(h, i32, i32, _fp, _ip, _ip),
    "gpf_sync": _sig(h),
    "gpf_get_results_pinned": _sig(h, i32, i32, i32, _vpp),
    "gpf_set_profiling": _sig(h, i32),
    "gpf_get_kernel_time": _sig(h, _dp, C.POINTER(i64)),
    "gpf_get_plan": _sig(h, _ip),
    "gpf_device_pointers": _sig(h, _vpp, _vpp),
    "gpf_device_pointers_n": _sig(h, _vpp, i32, _vpp),
    "gpf_get_counters": _sig(h, C.POINTER(i64)),
    "gpf_upload_outage_durations": _sig(h, i32, i32, C.POINTER(C.c_uint16)),
    "gpf_get_cooldown": _sig(h, i32, i32, _ip),
    "gpf_set_cooldown": _sig(h, i32, i32, _ip),
    "gpf_get_trajectory_cooldown": _sig(h, i32, i32, i32, i32, C.POINTER(C.c_int16)),
    "gpf_ptdf_build": _sig(h, i32),
    "gpf_ptdf_build_batch": _sig(h, i32, i32, i32, _ip),
    "gpf_ptdf_batch_info": _sig(h, _ip, _ip, _ip, _dp),
    "gpf_ptdf_batch_get": _sig(h, i32, _dp, _dp),
    "gpf_ptdf_get": _sig(h, _dp),
    "gpf_ptdf_flows": _sig(h, i32, i32),
    "gpf_get_ptdf_flows": _sig(h, i32, i32, _fp),
    "gpf_ptdf_flows_rows": _sig(h, i32, i32, f64),
    "gpf_get_ptdf_flows_rows": _sig(h, i32, i32, i32, i32, _fp),
    "gpf_lodf_screen": _sig(h, i32, i32, _fp, _fp),
    "gpf_jit_enable": _sig(h, C.c_char_p, C.c_char_p),
    "gpf_jit_disable": _sig(h),
    "gpf_jit_info": _sig(h, C.POINTER(i64), _dp, C.c_char_p, C.c_size_t),
    "gpf_jit_source": _sig(h, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)),
    "gpf_jit_features": _sig(h, i32),
    "gpf_jit_feature_word": _sig(h, i32, C.POINTER(GpfStepOpts), u32, C.POINTER(u32)),
    "gpf_set_topo_rules": _sig(h, i32, i32, i32, i32, i32),
    "gpf_upload_topo_actions": _sig(h, i32, _ip, _ip, _bp),
    "gpf_set_lane_topo_actions": _sig(h, _ip),
    "gpf_topo_actions_on_device": _sig(h, i32),
    "gpf_get_sub_cooldown": _sig(h, i32, i32, _ip),
    "gpf_set_sub_cooldown": _sig(h, i32, i32, _ip),
    "gpf_get_last_bus": _sig(h, i32, i32, _ip),
    "gpf_set_last_bus": _sig(h, i32, i32, _ip),
    "gpf_get_topo_flags": _sig(h, i32, i32, _bp),
    "gpf_topo_action_mask": _sig(h, i32, i32, _bp, i64),
    "gpf_get_topo_action_mask": _sig(h, i32, i32, _bp),
    "gpf_set_topo_areas": _sig(h, i32, _ip),
    "gpf_set_topo_slots": _sig(h, i32),
    "gpf_get_topo_action_areas": _sig(h, C.POINTER(u32)),
    "gpf_set_obs_clock": _sig(h, i32, C.POINTER(i64), i32, i32),
    "gpf_set_obs_spec": _sig(h, i32, _ip, i32, _fp, _fp, i32),
    "gpf_obs_vector": _sig(h, i32, i32, _fp, i64),
    "gpf_obs_vector_trajectory": _sig(h, i32, i32, i32, i32, _fp),
    "gpf_get_obs_vector": _sig(h, i32, i32, _fp),
    "gpf_set_graph_obs": _sig(h, i32, i32),
    "gpf_graph_layout": _sig(h, _ip, _ip, _ip, _ip),
    "gpf_graph_obs": _sig(h, i32, i32, _ip, _fp, _fp),
    "gpf_graph_obs_host": _sig(h, i32, i32, _ip, _fp, _fp),
    "gpf_set_opponent": _sig(h, C.POINTER(GpfOpponentDesc)),
    "gpf_upload_opponent_draws": _sig(h, i32, _dp),
    "gpf_upload_opponent_schedule": _sig(h, _ip, _ip),
    "gpf_get_opponent_state": _sig(h, i32, i32, _dp, _ip),
    "gpf_set_opponent_state": _sig(h, i32, i32, _dp, _ip),
    "gpf_set_opponent_areas": _sig(h, i32, _ip),
    "gpf_upload_opponent_area_schedule": _sig(h, _ip, _ip),
    "gpf_get_opponent_area_state": _sig(h, i32, i32, _ip),
    "gpf_set_opponent_area_state": _sig(h, i32, i32, _ip),
    "gpf_get_opponent_attack_lines": _sig(h, i32, i32, _bp),
    "gpf_set_alerts": _sig(h, C.POINTER(GpfAlertDesc)),
    "gpf_set_lane_alerts": _sig(h, C.POINTER(C.c_uint64)),
    "gpf_alerts_on_device": _sig(h, i32),
    "gpf_alert_state_ints": _sig(h, _ip),
    "gpf_get_alert_state": _sig(h, i32, i32, _ip),
    "gpf_set_alert_state": _sig(h, i32, i32, _ip),
    "gpf_get_alert_reward": _sig(h, i32, i32, _fp),
    "gpf_alert_device_pointers": _sig(h, _vpp, i32),
    "gpf_set_rewards": _sig(h, i32, C.POINTER(GpfRewardSlot), _fp),
    "gpf_get_rewards": _sig(h, i32, i32, _fp),
    "gpf_rewards_eval": _sig(h, i32, i32, _bp, _fp, i64),
    "gpf_reward_device_pointers": _sig(h, _vpp, i32),
    "gpf_set_episode_limit": _sig(h, C.POINTER(GpfEpisodeDesc)),
    "gpf_get_episode_ends": _sig(h, i32, i32, _bp, _bp, _ip, _fp),
    "gpf_get_episode_stats": _sig(h, i32, i32, _dp, _dp, _ip, _ip),
    "gpf_episode_device_pointers": _sig(h, _vpp, i32),
    "gpf_set_n1_screen": _sig(h, i32, _ip, i32),
    "gpf_get_n1_values": _sig(h, i32, i32, _fp),
    "gpf_get_n1_summary": _sig(h, i32, i32, _fp, _ip, _ip, _ip),
    "gpf_n1_device_pointers": _sig(h, _vpp, i32),
    "gpf_set_lookahead": _sig(h, i32, i32),
    "gpf_lookahead": _sig(h, i32, i32, _ip, C.POINTER(GpfStepOpts)),
    "gpf_get_lookahead": _sig(h, i32, i32, _fp, _bp, _ip, _fp, _ip),
    "gpf_lookahead_device_pointers": _sig(h, _vpp, i32),
    "gpf_set_lookahead_chain": _sig(h, i32),
    "gpf_lookahead_chain": _sig(h, i32, i32, _ip, i32, C.POINTER(GpfStepOpts)),
    "gpf_get_lookahead_chain": _sig(h, i32, i32, _ip, _fp, _fp, _ip, _ip),
    "gpf_lookahead_chain_device_pointers": _sig(h, _vpp, i32),
    "gpf_set_chronics_cursor": _sig(h, C.POINTER(GpfCursorDesc)),
    "gpf_upload_cursor_draws": _sig(h, i32, _dp),
    "gpf_get_cursor_state": _sig(h, i32, i32, _ip),
    "gpf_set_cursor_state": _sig(h, i32, i32, _ip),
    "gpf_cursor_device_pointers": _sig(h, _vpp, i32),
    "gpf_set_combined_actions": _sig(h, C.POINTER(GpfCombinedDesc)),
    "gpf_get_action_flags": _sig(h, i32, i32, _bp),
    "gpf_combined_device_pointers": _sig(h, _vpp, i32),
}
EXPORTED_SYMBOLS = list(SIGNATURES)
del h, i32, i64, u32, f32, f64

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load ``libgridpf.so`` (built in-tree by ``__graft_entry__.build()``); fail loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise GridPFError(
            f"{path} not found: the HIP engine is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(there is no CPU fallback).")
    # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  Two HIP runtimes cannot share a process: whichever
    # is loaded first serves both (same SONAME), and torch finds no GPU when it is the system one (measured on the MI355X box:
    # "No HIP GPUs are available" as soon as libgridpf.so was loaded before ``import torch``).  So when torch is installed it is
    # imported first and libgridpf.so binds to the runtime torch ships -- zero-copy views (PowerFlowEngine.device_views),
    # torch.distributed / RCCL and the engine then live on the same runtime.  GRIDPF_NO_TORCH_PRELOAD=1 skips this.
    if os.environ.get("GRIDPF_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    try:
        L = C.CDLL(path)
    except OSError as exc:
        raise GridPFError(f"cannot load {path}: {exc}") from exc
    for name, (argtypes, restype) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    got = L.gpf_version()
    if got != ABI_VERSION:               # a stale GRIDPF_LIB / an old build next to new Python: struct layouts and argument lists differ
        raise GridPFError(f"{path} has ABI version {got}, this binding needs {ABI_VERSION} (include/gridpf.h GPF_ABI_VERSION): rebuild "
                          f"with `python -c 'import __graft_entry__ as g; g.build(force=True)'`")
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().gpf_last_error()
        raise GridPFError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def ptr(a: Optional[np.ndarray], ctype):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ctype))
