"""ctypes binding of libwfstep.so (C ABI: include/wfstep.h).

This is the binding a maintainer of the reference would add next to wfcrl/interface.py to replace
the `floris.tools.FlorisInterface` calls (INTEGRATION.md shows it in place).  There is no fallback:
a missing or unloadable library raises, and wf_create raises without a HIP device.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libwfstep.so"

WF_OK = 0
WF_RISK_OVERLAP = 1     # a deficit within the guard band of the overlap threshold (include/wfstep.h)
WF_RISK_POWER_KNEE = 2  # a turbine on a steep segment (cut-in / cut-out) of the power table
WF_RISK_THRUST_RAMP = 4  # a turbine on the cut-in ramp / cut-out drop of the thrust table (v |dCt/dv| > 5)
WF_RISK_THRUST_UNITY = 8  # a thrust coefficient above 0.995 (user tables): always re-solved in float64, only seen in the raw flags
WF_RISK_NEGATIVE_SPEED = 16  # a rotor-grid speed that is not positive (an unphysically tight farm)
WF_E = {-1: "WF_E_INVALID", -2: "WF_E_UNSUPPORTED", -3: "WF_E_NODEVICE", -4: "WF_E_HIP", -5: "WF_E_NOMEM"}

_MODEL_DOUBLES = (
    "air_density", "ambient_ti", "shear", "veer",
    "rotor_diameter", "hub_height", "tsr", "pP", "pT", "gen_eff", "ref_density",
    "alpha", "beta", "ka", "kb", "ad", "bd", "dm",
    "ch_initial", "ch_constant", "ch_ai", "ch_downstream",
    "eps_gain", "num_eps", "kappa", "gch_gain", "overlap_thresh", "near_wake_c",
    "defl_alpha", "defl_beta", "defl_ka", "defl_kb",
)
_MODEL_SWITCHES = ("enable_secondary_steering", "enable_yaw_added_recovery", "enable_transverse_velocities")


class ModelParams(C.Structure):
    """Mirror of `struct wf_model_params`."""

    _fields_ = [(n, C.c_double) for n in _MODEL_DOUBLES] + [
        ("n_table", C.c_int),
        ("table_ws", C.POINTER(C.c_double)),
        ("table_ct", C.POINTER(C.c_double)),
        ("table_cp", C.POINTER(C.c_double)),
    ] + [(n, C.c_int) for n in _MODEL_SWITCHES]


class TurbineDef(C.Structure):
    """Mirror of `struct wf_turbine_def`."""

    _fields_ = [("n_table", C.c_int), ("table_ws", C.POINTER(C.c_double)), ("table_ct", C.POINTER(C.c_double)),
                ("table_cp", C.POINTER(C.c_double))] + [(n, C.c_double) for n in ("tsr", "pP", "gen_eff", "ref_density")]


class EnvParams(C.Structure):
    """Mirror of `struct wf_env_params`."""

    _fields_ = [(n, C.c_float) for n in ("yaw_lo", "yaw_hi", "yaw_step", "actuator_rate", "dt", "budget", "load_coef")] + [
        ("discrete", C.c_int)]


class WindDist(C.Structure):
    """Mirror of `struct wf_wind_dist`."""

    _fields_ = [(n, C.c_double) for n in ("ws_scale", "ws_shape", "ws_lo", "ws_hi", "wd_mean", "wd_std", "wd_lo", "wd_hi")]


class WindProcess(C.Structure):
    """Mirror of `struct wf_wind_process` (include/wfwindgen.h)."""

    _fields_ = [(n, C.c_double) for n in ("ws_revert", "ws_sigma", "wd_revert", "wd_sigma", "wd_ramp")]


class KernelInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "lanes_per_env", "slots_per_lane", "envs_per_block", "threads_per_block", "grid_blocks",
        "vgprs", "lds_bytes", "scratch_bytes", "pair_table", "direction_groups", "mixed_main_farms", "one_block_kernel")]


class KernelChoice(C.Structure):
    """Mirror of `struct wf_kernel_choice`."""

    _fields_ = [(n, C.c_int) for n in ("slot_G", "slot_S", "one_block", "ll_G", "ll_S", "pair_table", "fly_one_block", "far_skip", "calibrate", "mixed")]


# every symbol include/wfstep.h declares: name -> (restype, argtypes)
_P = C.c_void_p
ABI = {
    "wf_version": (C.c_int, []),
    "wf_default_model": (C.c_int, [C.POINTER(ModelParams)]),
    "wf_turbine_table": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_double)),
                                   C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_double))]),
    "wf_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "wf_destroy": (C.c_int, [_P]),
    "wf_set_stream": (C.c_int, [_P, _P, C.c_int]),
    "wf_get_stream": (_P, [_P]),
    "wf_set_model": (C.c_int, [_P, C.POINTER(ModelParams)]),
    "wf_set_turbine_types": (C.c_int, [_P, C.c_int, C.POINTER(TurbineDef), C.POINTER(C.c_int)]),
    "wf_get_turbine_types": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_set_layout": (C.c_int, [_P, C.c_int, _P, _P]),
    "wf_set_batch": (C.c_int, [_P, C.c_int]),
    "wf_set_layouts": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "wf_set_layouts_counts": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "wf_set_wind": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "wf_set_wind_counts": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int]),
    "wf_wind_sample_binned": (C.c_int, [_P, C.c_ulonglong, C.POINTER(WindDist), C.c_double]),
    "wf_step": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_sync": (C.c_int, [_P]),
    "wf_set_risk_guard": (C.c_int, [_P, C.c_double]),
    "wf_get_risk_flags": (C.c_int, [_P, _P, C.c_int]),
    "wf_set_risk_resolve": (C.c_int, [_P, C.c_int]),
    "wf_get_risk_resolve": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_get_resolve_stats": (C.c_int, [_P, C.POINTER(C.c_int), _P, C.c_int]),
    "wf_wind_sample": (C.c_int, [_P, C.c_ulonglong, C.POINTER(WindDist)]),
    "wf_wind_series": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_ulonglong]),
    "wf_wind_series_step": (C.c_int, [_P]),
    "wf_get_wind": (C.c_int, [_P, _P, _P, C.c_int]),
    "wf_env_config": (C.c_int, [_P, C.POINTER(EnvParams)]),
    "wf_env_set_power_unit": (C.c_int, [_P, C.c_int]),
    "wf_env_reset": (C.c_int, [_P]),
    "wf_env_state": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int]),
    "wf_env_set_prev_wind": (C.c_int, [_P, _P, C.c_int]),
    "wf_env_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_timing_begin": (C.c_int, [_P]),
    "wf_timing_end": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "wf_get_kernel_info": (C.c_int, [_P, C.POINTER(KernelInfo)]),
    "wf_set_kernel_choice": (C.c_int, [_P, C.POINTER(KernelChoice)]),
    "wf_get_kernel_choice": (C.c_int, [_P, C.POINTER(KernelChoice)]),
    "wf_set_own_stage": (C.c_int, [_P, C.c_int]),
    "wf_get_own_stage": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "wf_get_calibration": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "wf_get_fly_calibration": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "wf_get_mixed_launch": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "wf_calibrate": (C.c_int, [_P]),
    "wf_set_calibration": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfprobe.h declares (flow sampling at arbitrary points): a table of its own — `ABI` stays exactly the
# surface of include/wfstep.h
PROBE_ABI = {
    "wf_probe_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_probe_destroy": (C.c_int, [_P]),
    "wf_probe_set_points": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int]),
    "wf_probe_sample": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int]),
    "wf_probe_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_probe_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_probe_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfyawopt.h declares (batched yaw optimisation on the device): again a table of its own
YAWOPT_ABI = {
    "wf_yawopt_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_yawopt_destroy": (C.c_int, [_P]),
    "wf_yawopt_config": (C.c_int, [_P, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int]),
    "wf_yawopt_run": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.c_int]),
    "wf_yawopt_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_yawopt_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_yawopt_evaluator": (_P, [_P]),
    "wf_yawopt_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfrose.h declares (expected power over a wind rose, yaw look-up-table controller): a table of its own
ROSE_ABI = {
    "wf_rose_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_rose_destroy": (C.c_int, [_P]),
    "wf_rose_set_table": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_int, C.c_int]),
    "wf_rose_set_rose": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.c_double, C.c_double]),
    "wf_rose_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_rose_evaluate": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_rose_policy": (C.c_int, [_P, C.c_int, _P, _P, C.c_int]),
    "wf_rose_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_rose_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_rose_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfrobust.h declares (expected power under wind-direction uncertainty, robust yaw search): its own table
ROBUST_ABI = {
    "wf_robust_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_robust_destroy": (C.c_int, [_P]),
    "wf_robust_set_members": (C.c_int, [_P, C.c_int, _P, _P, C.c_int]),
    "wf_robust_config": (C.c_int, [_P, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int]),
    "wf_robust_evaluate": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.c_int]),
    "wf_robust_optimize": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.c_int]),
    "wf_robust_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_robust_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_robust_evaluator": (_P, [_P]),
    "wf_robust_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_robust_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfgrad.h declares (yaw sensitivities: power Jacobian and vector-Jacobian product): its own table
GRAD_ABI = {
    "wf_grad_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_grad_destroy": (C.c_int, [_P]),
    "wf_grad_config": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]),
    "wf_grad_run": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, _P, C.c_int]),
    "wf_grad_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_grad_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_grad_evaluator": (_P, [_P]),
    "wf_grad_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_grad_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfcredit.h declares (per-agent counterfactual rewards: difference rewards, COMA rows): its own table
CREDIT_ABI = {
    "wf_credit_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_credit_destroy": (C.c_int, [_P]),
    "wf_credit_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_credit_run": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int]),
    "wf_credit_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_credit_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_credit_evaluator": (_P, [_P]),
    "wf_credit_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_credit_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wflookahead.h declares (multi-step look-ahead returns of action sequences): its own table
LOOKAHEAD_ABI = {
    "wf_lookahead_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_lookahead_destroy": (C.c_int, [_P]),
    "wf_lookahead_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_lookahead_run": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_double, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_lookahead_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_lookahead_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_lookahead_evaluator": (_P, [_P]),
    "wf_lookahead_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_lookahead_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfplan.h declares (the receding-horizon planner: CEM over action sequences): its own table
PLAN_ABI = {
    "wf_plan_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_plan_destroy": (C.c_int, [_P]),
    "wf_plan_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_plan_run": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_ulonglong, C.c_double, _P, _P, C.c_int, _P,
                              _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_plan_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_plan_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_plan_evaluator": (_P, [_P]),
    "wf_plan_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_plan_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfseries.h declares (time-series episodes: the window of the coming rows, the cursor, the series-ahead mode
# of lookahead, plan and credit): its own table
SERIES_ABI = {
    "wf_series_window": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(C.c_int), C.c_int]),
    "wf_series_get": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P, C.POINTER(C.c_int)]),
    "wf_series_seek": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_lookahead_set_series": (C.c_int, [_P, C.c_int]),
    "wf_plan_set_series": (C.c_int, [_P, C.c_int]),
    "wf_credit_set_series": (C.c_int, [_P, C.c_int]),
    "wf_series_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
}

# every symbol include/wfrollout.h declares (closed-loop rollouts of yaw-table controllers): its own table
ROLLOUT_ABI = {
    "wf_rollout_create": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "wf_rollout_destroy": (C.c_int, [_P]),
    "wf_rollout_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_rollout_set_series": (C.c_int, [_P, C.c_int]),
    "wf_rollout_run": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, _P, _P, C.c_double, C.c_int, _P,
                                 _P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_rollout_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_rollout_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_rollout_evaluator": (_P, [_P]),
    "wf_rollout_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_rollout_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfretgrad.h declares (the gradient of look-ahead returns w.r.t. the action sequences): its own table
RETGRAD_ABI = {
    "wf_retgrad_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_retgrad_destroy": (C.c_int, [_P]),
    "wf_retgrad_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_retgrad_set_series": (C.c_int, [_P, C.c_int]),
    "wf_retgrad_run": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_double, C.c_double, _P, C.c_int, _P,
                                 _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_retgrad_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_retgrad_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_retgrad_evaluator": (_P, [_P]),
    "wf_retgrad_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_retgrad_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfwindgen.h declares (synthetic wind episodes: a stochastic wind series per farm, generated and played on
# the device; the wind source of the five row extensions' series-ahead mode): its own table
WINDGEN_ABI = {
    "wf_windgen_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_windgen_destroy": (C.c_int, [_P]),
    "wf_windgen_generate": (C.c_int, [_P, C.c_int, C.c_ulonglong, C.POINTER(WindDist), C.POINTER(WindProcess), _P, _P]),
    "wf_windgen_set_kernel": (C.c_int, [_P, C.c_int]),
    "wf_windgen_step": (C.c_int, [_P]),
    "wf_windgen_get": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong),
                                 C.POINTER(WindDist), C.POINTER(WindProcess)]),
    "wf_windgen_seek": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_windgen_window": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.POINTER(C.c_int), C.c_int]),
    "wf_windgen_read": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "wf_credit_set_wind_source": (C.c_int, [_P, _P]),
    "wf_lookahead_set_wind_source": (C.c_int, [_P, _P]),
    "wf_plan_set_wind_source": (C.c_int, [_P, _P]),
    "wf_rollout_set_wind_source": (C.c_int, [_P, _P]),
    "wf_retgrad_set_wind_source": (C.c_int, [_P, _P]),
    "wf_windgen_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_windgen_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfscenario.h declares (scenario look-ahead: returns of action sequences over a wind ensemble drawn on the
# device, their mean, tail mean and a choice): its own table
SCENARIO_ABI = {
    "wf_scenario_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_scenario_destroy": (C.c_int, [_P]),
    "wf_scenario_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_scenario_run": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(WindProcess), C.c_double, C.c_double, C.c_ulonglong,
                                  C.c_double, C.c_int, C.c_double, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_scenario_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_scenario_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_scenario_evaluator": (_P, [_P]),
    "wf_scenario_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_scenario_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfscenplan.h declares (the scenario planner: CEM over action sequences scored over a wind ensemble): its own
# table
SCENPLAN_ABI = {
    "wf_scenplan_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_scenplan_destroy": (C.c_int, [_P]),
    "wf_scenplan_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_scenplan_run": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_ulonglong, C.c_double, C.c_int, C.POINTER(WindProcess),
                                  C.c_double, C.c_double, C.c_ulonglong, C.c_int, C.c_double, _P, _P, C.c_int, _P,
                                  _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_scenplan_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_scenplan_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_scenplan_evaluator": (_P, [_P]),
    "wf_scenplan_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_scenplan_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfrollscen.h declares (scenario rollouts: yaw-table controllers in closed loop over a wind ensemble): its
# own table
ROLLSCEN_ABI = {
    "wf_rollscen_create": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "wf_rollscen_destroy": (C.c_int, [_P]),
    "wf_rollscen_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_rollscen_run": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(WindProcess), C.c_double, C.c_double,
                                  C.c_ulonglong, C.c_double, C.c_int, C.c_double, _P, _P, C.c_int, _P,
                                  _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_rollscen_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_rollscen_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_rollscen_evaluator": (_P, [_P]),
    "wf_rollscen_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_rollscen_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfmodelset.h declares (wake-model parameter sets per farm): its own table
_MODEL_SET_FIELDS = ("ambient_ti", "shear", "veer", "alpha", "beta", "ka", "kb", "ad", "bd", "dm",
                     "ch_initial", "ch_constant", "ch_ai", "ch_downstream", "defl_alpha", "defl_beta", "defl_ka", "defl_kb")


class ModelSet(C.Structure):
    """Mirror of `struct wf_model_set` (include/wfmodelset.h)."""

    _fields_ = [(n, C.c_double) for n in _MODEL_SET_FIELDS]


MODELSET_ABI = {
    "wf_set_model_sets": (C.c_int, [_P, C.c_int, C.POINTER(ModelSet), C.POINTER(C.c_int)]),
    "wf_get_model_sets": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(ModelSet), C.POINTER(C.c_int)]),
    "wf_model_set_from_model": (C.c_int, [_P, C.POINTER(ModelSet)]),
    "wf_model_sets_last_kernel": (C.c_int, [_P, C.POINTER(C.c_int)]),
}

# every symbol include/wfcalib.h declares (wake-model calibration: parameter sets scored against and fitted to measured powers): its
# own table
CALIB_ABI = {
    "wf_calib_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_calib_destroy": (C.c_int, [_P]),
    "wf_calib_config": (C.c_int, [_P, C.c_int]),
    "wf_calib_score": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(ModelSet), C.c_int, _P, _P, _P, _P, _P, C.c_double, _P, _P, _P,
                                 C.c_int]),
    "wf_calib_fit": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_ulonglong, _P, _P, C.POINTER(ModelSet), C.c_int,
                               _P, _P, _P, _P, _P, C.c_double, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_calib_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_calib_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_calib_evaluator": (_P, [_P]),
    "wf_calib_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_calib_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfpolicy.h declares (closed-loop rollouts of MLP policies): its own table
POLICY_ABI = {
    "wf_policy_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_policy_destroy": (C.c_int, [_P]),
    "wf_policy_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_policy_set_network": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P]),
    "wf_policy_run": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_double, C.c_int, _P,
                                _P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_policy_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_policy_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_policy_evaluator": (_P, [_P]),
    "wf_policy_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_policy_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfpolscen.h declares (policy rollouts over a wind ensemble): its own table
POLSCEN_ABI = {
    "wf_polscen_create": (C.c_int, [_P, C.POINTER(_P)]),
    "wf_polscen_destroy": (C.c_int, [_P]),
    "wf_polscen_config": (C.c_int, [_P, C.c_int, C.c_int]),
    "wf_polscen_set_network": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P]),
    "wf_polscen_run": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WindProcess), C.c_double, C.c_double,
                                 C.c_ulonglong, C.c_double, C.c_int, C.c_double, _P, C.c_int, _P,
                                 _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_polscen_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_polscen_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_polscen_evaluator": (_P, [_P]),
    "wf_polscen_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_polscen_last_error": (C.c_char_p, [_P]),
}

# every symbol include/wfpolsearch.h declares (policy search: CEM over MLP weights): its own table
POLSEARCH_ABI = {
    "wf_polsearch_create": (C.c_int, [_P, _P, _P, C.POINTER(_P)]),
    "wf_polsearch_destroy": (C.c_int, [_P]),
    "wf_polsearch_run": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_ulonglong, C.c_int, C.c_double, _P,
                                   C.c_int, C.POINTER(WindProcess), C.c_double, C.c_double, C.c_ulonglong, C.c_int, C.c_double, _P,
                                   C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int]),
    "wf_polsearch_set_timing": (C.c_int, [_P, C.c_int]),
    "wf_polsearch_last_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wf_polsearch_kernel_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "wf_polsearch_last_error": (C.c_char_p, [_P]),
}

_lib = None


def build(force: bool = False) -> Path:
    """Compile csrc/ into libwfstep.so with hipcc for gfx950 (cross-compiles without a GPU)."""
    srcs = []
    for d in ("", "ext", "modelset", "probe", "yawopt", "rose", "robust", "grad", "credit", "lookahead", "plan", "series", "rollout", "retgrad", "windgen", "scenario", "scenplan", "calib", "policy", "polscen", "polsearch", "rollscen"):  # csrc/ itself, the extensions' shared layer, the extensions
        srcs += sorted((PKG_DIR / "csrc" / d).glob("*.hip")) + sorted((PKG_DIR / "csrc" / d).glob("*.h"))
    srcs += [PKG_DIR.parent / "include" / h for h in ("wfstep.h", "wfmodelset.h", "wfprobe.h", "wfyawopt.h", "wfrose.h", "wfrobust.h", "wfgrad.h", "wfcredit.h", "wflookahead.h", "wfplan.h", "wfseries.h", "wfrollout.h", "wfretgrad.h", "wfwindgen.h", "wfscenario.h", "wfscenplan.h", "wfcalib.h", "wfpolicy.h", "wfpolscen.h", "wfpolsearch.h", "wfrollscen.h")]
    stale = (not LIB_PATH.exists()) or any(s.stat().st_mtime > LIB_PATH.stat().st_mtime for s in srcs)
    if force or stale:
        subprocess.run(["make", "-j4", "-C", str(PKG_DIR / "csrc")] + (["-B"] if force else []), check=True)
    return LIB_PATH


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (SONAME libamdhip64.so.7).  If libwfstep.so were
    loaded first it would bind /opt/rocm's copy and torch would then load a SECOND runtime (its NEEDED
    entry is the unversioned file name), leaving two HIP runtimes in one process: torch fails to see
    the GPU and torch device pointers are meaningless to our kernels.  Importing torch first makes the
    dynamic loader resolve our `libamdhip64.so.7` to the copy torch already mapped."""
    import importlib.util
    import sys

    if os.environ.get("WFSTEP_NO_TORCH"):
        return
    if "torch" in sys.modules or importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            if os.environ.get("WFSTEP_NO_AUTOBUILD"):
                raise OSError(f"{LIB_PATH} is missing; run __graft_entry__.build() (there is no CPU fallback)")
            build()
        _share_hip_runtime_with_torch()
        lib = C.CDLL(str(LIB_PATH))
        for table in (ABI, MODELSET_ABI, PROBE_ABI, YAWOPT_ABI, ROSE_ABI, ROBUST_ABI, GRAD_ABI, CREDIT_ABI, LOOKAHEAD_ABI, PLAN_ABI, SERIES_ABI, ROLLOUT_ABI, RETGRAD_ABI, WINDGEN_ABI, SCENARIO_ABI, SCENPLAN_ABI, CALIB_ABI, POLICY_ABI, POLSCEN_ABI, POLSEARCH_ABI, ROLLSCEN_ABI):
            for name, (res, args) in table.items():
                fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
                fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


class WfError(RuntimeError):
    pass


def check_ext(rc: int, obj, last_error_name: str):
    """`check` for an extension object: the text comes from the extension's own wf_*_last_error."""
    if rc != WF_OK:
        msg = getattr(load(), last_error_name)(obj)
        text = f"{WF_E.get(rc, rc)}: {msg.decode() if msg else ''}"
        if rc in (-1, -2):
            raise ValueError(text)
        raise WfError(text)


def check_probe(rc: int, probe):
    check_ext(rc, probe, "wf_probe_last_error")


def check_yawopt(rc: int, opt):
    check_ext(rc, opt, "wf_yawopt_last_error")


def check_rose(rc: int, rose):
    check_ext(rc, rose, "wf_rose_last_error")


def check_robust(rc: int, rob):
    check_ext(rc, rob, "wf_robust_last_error")


def check_grad(rc: int, grad):
    check_ext(rc, grad, "wf_grad_last_error")


def check(rc: int, handle=None):
    check_ext(rc, handle, "wf_last_error")
