"""ctypes binding of the C ABI in ``include/mppi_rocm.h`` (libmppi_rocm.so).

The library is built in-tree by ``mppi_robotarm_amd.build.build_native()``
(``hipcc --offload-arch=gfx950``).  There is no fallback: if the shared object
is missing or does not load, importing the engine raises, loudly.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPPI_LIB_PATH") or os.path.join(HERE, "_lib", "libmppi_rocm.so")

MPPI_MAX_T = 128
MPPI_SEARCH_LEN = 30
MPPI_OK = 0
MPPI_E_ARG = -1
MPPI_E_HIP = -2
MPPI_E_SINGULAR = -3
MPPI_E_PATH_END = -4
MPPI_E_EXCHANGE = -5
MPPI_E_RETRY = -6
MPPI_FLAG_FUSED_UPDATE = 1
MPPI_FLAG_EXCHANGE = 2
MPPI_FLAG_HOST_OUT = 4
MPPI_FLAG_INLINE_MERGE = 8
DP = C.POINTER(C.c_double)
MPPI_IPC_HANDLE_BYTES = 64
MPPI_MAX_WORLD = 8
MPPI_MAX_OBSTACLES = 8

# every symbol the header declares (tests check the library exports all of them)
EXPORTS = (
    "mppi_ctx_create", "mppi_ctx_destroy", "mppi_last_error", "mppi_set_stream", "mppi_ctx_info", "mppi_ctx_handoff",
    "mppi_set_step_inputs", "mppi_rollout", "mppi_merge_partials", "mppi_exchange_handle", "mppi_exchange_attach",
    "mppi_get_weighted_noise",
    "mppi_get_nominal", "mppi_rollout_traj", "mppi_optimal_traj", "mppi_get_step_outputs", "mppi_step_dropin",
    "mppi_optimal_traj_host", "mppi_wait_outputs", "mppi_dropin_bind", "mppi_dropin_tick",
    "mppi_dropin_tick_launch", "mppi_dropin_tick_wait",
    "mppi_noise_philox",
    "mppi_sync", "mppi_debug_set_buffer", "mppi_debug_pending",
    "mppi_debug_nearest", "mppi_debug_dropin_times", "mppi_set_obstacles", "mppi_set_moving_obstacles",
    "mppi_debug_obstacle_hits",
    "mppi_chain_ctx_create", "mppi_chain_ctx_destroy", "mppi_chain_set_stream", "mppi_chain_ctx_info",
    "mppi_chain_set_step_inputs", "mppi_chain_rollout", "mppi_chain_merge_partials", "mppi_chain_exchange_handle",
    "mppi_chain_exchange_attach",
    "mppi_chain_get_weighted_noise", "mppi_chain_get_nominal", "mppi_chain_rollout_traj",
    "mppi_chain_noise_philox", "mppi_chain_sync", "mppi_chain_debug_set_buffer", "mppi_chain_debug_slots",
    "mppi_chain_wait_outputs", "mppi_chain_optimal_traj_host", "mppi_chain_last_eta",
    "mppi_chain_set_obstacles", "mppi_chain_set_moving_obstacles", "mppi_chain_debug_obstacle_hits",
    "mppi_chain_set_self_collision", "mppi_chain_debug_self_hits",
    "mppi_config_init", "mppi_chain_config_init",
    "mppi_np_ctx_create", "mppi_np_ctx_destroy", "mppi_np_plan", "mppi_np_set_jumps", "mppi_np_draw",
    "mppi_np_draw_result", "mppi_readback_create", "mppi_readback_destroy", "mppi_readback_run",
)


class DropinBindingC(C.Structure):
    _fields_ = [("path", C.c_void_p), ("rows", C.c_int), ("stride", C.c_int), ("fk_l1", C.c_double),
                ("fk_l2", C.c_double), ("x0", C.c_void_p), ("idx", C.c_void_p), ("u", C.c_void_p),
                ("traj", C.c_void_p), ("noise_dev", C.c_void_p), ("next_noise_dev", C.c_void_p),
                ("S_dev", C.c_void_p), ("seed", C.c_ulonglong)]


NP_MAX_DU = 8
NP_LOG_DATA = 274
NP_POLY_WORDS = 312


class NpStateC(C.Structure):
    """mppi_np_state: NumPy's RandomState.get_state()[1:5]."""
    _fields_ = [("key", C.c_uint * 624), ("pos", C.c_int), ("has_gauss", C.c_int), ("gauss", C.c_double)]


class NpTargetC(C.Structure):
    _fields_ = [("out_dev", C.c_void_p), ("K", C.c_longlong), ("T", C.c_longlong), ("du", C.c_int),
                ("k_offset", C.c_longlong), ("K_local", C.c_longlong), ("stride_t", C.c_longlong),
                ("stride_k", C.c_longlong), ("stride_d", C.c_longlong), ("src", C.c_int * NP_MAX_DU),
                ("scale", C.c_double * NP_MAX_DU), ("mean", C.c_double * NP_MAX_DU), ("dot2", C.c_int),
                ("mat", C.c_double * 4)]


class ArmParamsC(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("m1", "m2", "l1", "l2", "lc1", "lc2", "g", "fk_l1", "fk_l2")]


class ConfigC(C.Structure):
    _fields_ = [
        ("K_local", C.c_int), ("T", C.c_int), ("K_total", C.c_int), ("k_offset", C.c_int),
        ("delta_t", C.c_double), ("param_lambda", C.c_double), ("param_alpha", C.c_double),
        ("param_exploration", C.c_double), ("sigma", C.c_double * 4),
        ("stage_cost_weight", C.c_double * 4), ("terminal_cost_weight", C.c_double * 4),
        ("arm", ArmParamsC), ("lanes_per_sample", C.c_int), ("param_gamma", C.c_double),
        # torque limits (_g, control.py:166-172): 0 off, 1 sampled controls, 2 also the updated nominal
        ("clamp_mode", C.c_int), ("u_min", C.c_double * 2), ("u_max", C.c_double * 2),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "param_gamma" not in kw and len(args) <= [f for f, _ in self._fields_].index("param_gamma"):
            self.param_gamma = float("nan")   # gamma = lambda (1 - alpha), control.py:45


CHAIN_MAX_DOF = 8


class ChainParamsC(C.Structure):
    _fields_ = [("n", C.c_int)] + [(f, C.c_double * CHAIN_MAX_DOF) for f in ("m", "l", "lc", "I", "fk", "J", "b")] + \
               [("g", C.c_double)]


class ChainConfigC(C.Structure):
    _fields_ = [
        ("K_local", C.c_int), ("T", C.c_int), ("K_total", C.c_int), ("k_offset", C.c_int),
        ("delta_t", C.c_double), ("param_lambda", C.c_double), ("param_alpha", C.c_double),
        ("param_exploration", C.c_double), ("sigma", C.c_double * (CHAIN_MAX_DOF * CHAIN_MAX_DOF)),
        ("stage_cost_weight", C.c_double * 4), ("terminal_cost_weight", C.c_double * 4),
        ("chain", ChainParamsC), ("precision", C.c_int), ("lanes_per_sample", C.c_int),
        ("param_gamma", C.c_double),
        # torque limits per joint (_g, control.py:166-172): 0 off, 1 sampled controls, 2 also the updated nominal
        ("clamp_mode", C.c_int), ("u_min", C.c_double * CHAIN_MAX_DOF), ("u_max", C.c_double * CHAIN_MAX_DOF),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if "param_gamma" not in kw and len(args) <= [f for f, _ in self._fields_].index("param_gamma"):
            self.param_gamma = float("nan")   # gamma = lambda (1 - alpha), control.py:45


class MPPIError(RuntimeError):
    """A failed C-ABI call (message from mppi_last_error)."""


class ExchangeError(MPPIError):
    """MPPI_E_EXCHANGE: the in-launch multi-GPU exchange of a step missed its poll bound on some rank.  Every
    rank of that step raises it and none applied the update (the controllers then run the step again over
    the collective fallback)."""


_lib = None


def open_library(path: str):
    """dlopen one build of the C ABI with every entry point's signature set
    (``load`` uses it for the product library; tools open variants with it)."""
    if not os.path.exists(path):
        raise OSError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(path)
    vp, dp, fp, ip = C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int)
    sig = {
        "mppi_ctx_create": ([C.POINTER(ConfigC), C.c_int, vp, C.POINTER(vp)], C.c_int),
        "mppi_ctx_destroy": ([vp], None),
        "mppi_last_error": ([], C.c_char_p),
        "mppi_set_stream": ([vp, vp], C.c_int),
        "mppi_ctx_info": ([vp, ip, ip, ip], C.c_int),
        "mppi_ctx_handoff": ([vp, ip], C.c_int),
        "mppi_debug_pending": ([vp, ip], C.c_int),
        "mppi_set_step_inputs": ([vp, dp, dp, C.c_int, dp], C.c_int),
        "mppi_rollout": ([vp, fp, vp, vp, C.c_uint], C.c_int),
        "mppi_merge_partials": ([vp, vp, C.c_int, C.c_uint], C.c_int),
        "mppi_exchange_handle": ([vp, C.c_int, vp], C.c_int),
        "mppi_exchange_attach": ([vp, C.c_int, C.c_int, vp], C.c_int),
        "mppi_get_weighted_noise": ([vp, dp], C.c_int),
        "mppi_get_nominal": ([vp, dp], C.c_int),
        "mppi_rollout_traj": ([vp, dp, fp, C.c_int, fp], C.c_int),
        "mppi_optimal_traj": ([vp, fp], C.c_int),
        "mppi_get_step_outputs": ([vp, dp, fp, fp], C.c_int),
        "mppi_optimal_traj_host": ([vp, dp, dp, dp], C.c_int),
        "mppi_wait_outputs": ([vp, dp, dp, dp], C.c_int),
        # raw addresses (ints) for every pointer: the per-step hot call skips ctypes pointer objects
        "mppi_step_dropin": ([vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_ulonglong, C.c_ulonglong, vp, vp], C.c_int),
        "mppi_noise_philox": ([vp, C.c_ulonglong, C.c_ulonglong, fp], C.c_int),
        "mppi_dropin_bind": ([vp, C.POINTER(DropinBindingC)], C.c_int),
        "mppi_dropin_tick": ([vp, C.c_ulonglong], C.c_int),
        "mppi_dropin_tick_launch": ([vp, C.c_ulonglong], C.c_int),
        "mppi_dropin_tick_wait": ([vp], C.c_int),
        "mppi_sync": ([vp], C.c_int),
        "mppi_debug_set_buffer": ([vp, vp], C.c_int),
        "mppi_debug_dropin_times": ([vp, dp], C.c_int),
        "mppi_debug_nearest": ([vp, fp, C.c_int, vp, fp], C.c_int),
        "mppi_set_obstacles": ([vp, C.c_int, dp, C.c_double], C.c_int),
        "mppi_set_moving_obstacles": ([vp, C.c_int, dp, dp, C.c_double], C.c_int),
        "mppi_debug_obstacle_hits": ([vp, fp, C.c_int, vp, fp], C.c_int),
        "mppi_chain_ctx_create": ([C.POINTER(ChainConfigC), C.c_int, vp, C.POINTER(vp)], C.c_int),
        "mppi_chain_ctx_destroy": ([vp], None),
        "mppi_chain_set_stream": ([vp, vp], C.c_int),
        "mppi_chain_ctx_info": ([vp, ip, ip, ip, ip], C.c_int),
        "mppi_chain_set_step_inputs": ([vp, dp, dp, C.c_int, dp], C.c_int),
        "mppi_chain_rollout": ([vp, fp, vp, vp, C.c_uint], C.c_int),
        "mppi_chain_merge_partials": ([vp, vp, C.c_int, C.c_uint], C.c_int),
        "mppi_chain_exchange_handle": ([vp, C.c_int, vp], C.c_int),
        "mppi_chain_exchange_attach": ([vp, C.c_int, C.c_int, vp], C.c_int),
        "mppi_chain_get_weighted_noise": ([vp, dp], C.c_int),
        "mppi_chain_get_nominal": ([vp, dp], C.c_int),
        "mppi_chain_rollout_traj": ([vp, dp, fp, C.c_int, fp], C.c_int),
        "mppi_chain_noise_philox": ([vp, C.c_ulonglong, C.c_ulonglong, fp], C.c_int),
        "mppi_chain_sync": ([vp], C.c_int),
        "mppi_chain_debug_set_buffer": ([vp, vp], C.c_int),
        "mppi_chain_debug_slots": ([vp, fp, vp, vp], C.c_int),
        "mppi_chain_wait_outputs": ([vp, dp, dp, dp], C.c_int),
        "mppi_chain_optimal_traj_host": ([vp, dp, dp, dp], C.c_int),
        "mppi_chain_last_eta": ([vp, dp], C.c_int),
        "mppi_chain_set_obstacles": ([vp, C.c_int, dp, C.c_double], C.c_int),
        "mppi_chain_set_moving_obstacles": ([vp, C.c_int, dp, dp, C.c_double], C.c_int),
        "mppi_chain_debug_obstacle_hits": ([vp, fp, C.c_int, vp, fp], C.c_int),
        "mppi_chain_set_self_collision": ([vp, C.c_int, C.c_double, C.c_double], C.c_int),
        "mppi_chain_debug_self_hits": ([vp, fp, C.c_int, vp, fp], C.c_int),
        "mppi_config_init": ([C.POINTER(ConfigC)], None),
        "mppi_np_ctx_create": ([C.c_int, vp, C.POINTER(vp)], C.c_int),
        "mppi_np_ctx_destroy": ([vp], None),
        "mppi_np_plan": ([vp, C.c_longlong, C.c_int, C.c_int, ip, ip], C.c_int),
        "mppi_np_set_jumps": ([vp, C.c_int, C.c_int, vp, C.c_int], C.c_int),
        "mppi_np_draw": ([vp, vp, C.POINTER(NpStateC), C.c_longlong, C.POINTER(NpTargetC)], C.c_int),
        "mppi_np_draw_result": ([vp, C.POINTER(NpStateC)], C.c_int),
        "mppi_chain_config_init": ([C.POINTER(ChainConfigC)], None),
        "mppi_readback_create": ([C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.POINTER(vp)], C.c_int),
        "mppi_readback_destroy": ([vp], None),
        "mppi_readback_run": ([vp, vp, vp, vp, C.c_longlong], C.c_int),
    }
    for name, (args, res) in sig.items():
        if not hasattr(L, name):   # an older diagnostic build (tools/ab.py); load() checks the product's exports
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    return L


def load():
    """Load libmppi_rocm.so (raises OSError if it is missing — no fallback)."""
    global _lib
    if _lib is None:
        L = open_library(LIB_PATH)
        missing = [n for n in EXPORTS if not hasattr(L, n)]
        if missing:
            raise OSError(f"{LIB_PATH} is stale (missing {', '.join(missing)}): rebuild it")
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != MPPI_OK:
        msg = load().mppi_last_error().decode(errors="replace")
        if rc == MPPI_E_SINGULAR:
            import numpy as np
            raise np.linalg.LinAlgError(msg)
        if rc == MPPI_E_ARG:
            raise ValueError(f"{what}: {msg}")
        if rc == MPPI_E_EXCHANGE:
            raise ExchangeError(f"{what}: {msg}")
        raise MPPIError(f"{what} failed ({rc}): {msg}")
