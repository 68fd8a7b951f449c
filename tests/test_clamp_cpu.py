"""CPU: torque limits (the reference's clamp hook _g, control.py:166-172, switched on).

  * oracle/mppi_oracle.py with limits (lo / hi), the NumPy restatement the GPU tests use as their yardstick, is
    pinned to every clamp_step_* / clamp_loop_* fixture captured from the reference itself (make_golden_clamp.py);
  * the drop-in's constructor validation, its _g, and the engine key;
  * the C ABI: mppi_config_init leaves the clamp off, mppi_ctx_create rejects bad limits before any device
    call (so these run without a GPU) and names the field in mppi_last_error.
"""
import ctypes as C
import os

import numpy as np
import pytest

import mppi_oracle as O
from conftest import GOLDEN
from helpers import CLAMP_STEPS, load_clamp_loop, load_clamp_step
from mppi_robotarm_amd.controller import MPPIControllerForPathTracking


def ref_step(g, path):
    return O.step(g["x0"], g["u_prev"], g["eps"].astype(np.float64), path, int(g["prev_idx_after"]),
                  float(g["delta_t"]), float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"],
                  g["stage_cost_weight"], g["terminal_cost_weight"], lo=g["u_min"], hi=g["u_max"],
                  expl=float(g["param_exploration"]), visualize_optimal_traj=bool(g["visualize_optimal_traj"]),
                  sampled=bool(g["sampled"]))


def test_the_fixtures_are_all_here():
    assert CLAMP_STEPS == ["a_k128_t20", "b_novis_k128_t20", "c_dense_k256_t24", "d_expl_k128_t20",
                           "e_runpy_k100_t30"]
    assert os.path.exists(os.path.join(GOLDEN, "clamp_loop_k64_t20.npz"))
    # tests/conftest.py globs step_* and loop_* into the unclamped parity tests: none of ours may match
    assert not [f for f in os.listdir(GOLDEN) if "clamp" in f and f.startswith(("step_", "loop_"))]


@pytest.mark.parametrize("name", CLAMP_STEPS)
def test_clamp_ref_matches_the_reference(name, paths):
    g = load_clamp_step(name)
    r = ref_step(g, paths[str(g["path"])])
    assert int(np.argmin(r["S"])) == int(np.argmin(g["S"]))
    assert float(np.max(np.abs(r["S"] - g["S"]) / np.abs(g["S"]))) < 1e-12
    np.testing.assert_allclose(r["w_eps_filt"], g["w_eps_filt"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["u_seq"], g["u_seq"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["u0"], g["u0"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["optimal_traj"], g["optimal_traj"], rtol=1e-10, atol=1e-10)
    if "sampled_traj" in g:
        np.testing.assert_allclose(r["sampled_traj"], g["sampled_traj"], rtol=1e-10, atol=1e-10)
    inside = bool(np.all((g["u_seq"] >= g["u_min"]) & (g["u_seq"] <= g["u_max"])))
    assert inside == bool(g["visualize_optimal_traj"])     # case b: the nominal is left unclamped


def test_clamp_ref_matches_the_reference_closed_loop(paths):
    g = load_clamp_loop("k64_t20")
    from mppi_robotarm_amd.params import runpy_config
    kw = runpy_config()
    T = int(g["T"])
    u_prev = np.array([[10.0, -2.0]] * T)
    for i in range(int(g["ticks"])):
        r = O.step(g["states"][i], u_prev, g["eps"][i].astype(np.float64), paths["xydq_circle"],
                   int(g["prev_idx"][i]), 0.006, kw["param_lambda"], kw["param_alpha"], kw["sigma"],
                   kw["stage_cost_weight"], kw["terminal_cost_weight"], lo=g["u_min"], hi=g["u_max"])
        assert float(np.max(np.abs(r["S"] - g["S"][i]) / np.abs(g["S"][i]))) < 1e-12, i
        np.testing.assert_allclose(r["u_seq"], g["u_seq"][i], rtol=1e-10, atol=1e-10)
        u_prev = g["u_seq"][i].copy()


def _ctrl(paths, **kw):
    return MPPIControllerForPathTracking(delta_t=0.006, ref_path=paths["xydq_circle"], horizon_step_T=8,
                                         number_of_samples_K=16, verbose=False, sigma=np.eye(2) * 20.0, **kw)


def test_constructor_validation(paths):
    with pytest.raises(ValueError, match="u_min"):
        _ctrl(paths, u_min=[0.0, float("nan")], u_max=[1.0, 1.0])
    with pytest.raises(ValueError, match="u_max"):
        _ctrl(paths, u_min=-1.0, u_max=float("nan"))
    with pytest.raises(ValueError, match="exceeds"):
        _ctrl(paths, u_min=[0.0, 2.0], u_max=[1.0, 1.0])
    with pytest.raises(ValueError, match="u_max"):
        _ctrl(paths, u_min=[0.0, 0.0], u_max=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="u_min"):
        _ctrl(paths, u_min=np.zeros((2, 2)), u_max=1.0)
    c = _ctrl(paths, u_min=-0.8, u_max=0.8)                   # the reference's own commented-out values
    assert c.u_min.tolist() == [-0.8, -0.8] and c.u_max.tolist() == [0.8, 0.8]
    assert c.u_min.dtype == np.float64 and c.u_min.shape == (2,)
    c = _ctrl(paths, u_min=[4, -6], u_max=(14, 2))
    assert c.u_min.tolist() == [4.0, -6.0] and c.u_max.tolist() == [14.0, 2.0]
    c = _ctrl(paths, u_max=[14.0, float("inf")])             # one-sided
    assert c.u_min is None and c._limits()[0].tolist() == [-np.inf, -np.inf]
    c = _ctrl(paths)
    assert c.u_min is None and c.u_max is None and c._limits() is None


def test_positional_arguments_are_the_references(paths):
    """u_min / u_max are keyword-only: the twelve positional arguments stay control.py:21-35's."""
    with pytest.raises(TypeError):
        MPPIControllerForPathTracking(0.006, paths["xydq_circle"], 8, 16, 0.0, 100.0, 0.98, np.eye(2), np.ones(4),
                                      np.ones(4), True, False, -1.0, 1.0)


def test_g_clips_in_place_with_limits_and_is_the_identity_without(paths):
    c = _ctrl(paths, u_min=[4.0, -6.0], u_max=[14.0, 2.0])
    v = np.array([20.0, -7.0])
    assert c._g(v) is v and v.tolist() == [14.0, -6.0]
    rows = np.array([[3.0, 0.0], [5.0, 3.0], [10.0, -2.0]])
    row = rows[1]                                            # a view, as u[t-1] is in control.py:133
    c._g(row)
    assert rows.tolist() == [[3.0, 0.0], [5.0, 2.0], [10.0, -2.0]]
    c._g(rows)
    assert rows.tolist() == [[4.0, 0.0], [5.0, 2.0], [10.0, -2.0]]
    d = _ctrl(paths)
    w = np.array([1e9, -1e9])
    assert d._g(w) is w and w.tolist() == [1e9, -1e9]


def test_limits_and_the_trajectory_switch_enter_the_engine_key(paths):
    c = _ctrl(paths, u_min=[4.0, -6.0], u_max=[14.0, 2.0])
    k0, f0 = c._engine_key(), c._fast_scalars()
    assert c._clamp_key()[0] == 2
    c.u_max = [13.0, 2.0]
    assert c._engine_key() != k0 and c._fast_scalars() != f0
    c.u_max = [14.0, 2.0]
    assert c._engine_key() == k0
    c.visualize_optimal_traj = False                          # the nominal's clamp lives in that loop (control.py:130)
    assert c._clamp_key()[0] == 1 and c._engine_key() != k0
    c.u_min = c.u_max = None
    assert c._clamp_key() == (0,)
    assert _ctrl(paths)._engine_key()[-1] == (0,)
    c.u_min = [20.0, 0.0]
    c.u_max = [14.0, 2.0]
    with pytest.raises(ValueError, match="exceeds"):
        c._engine_key()
    with pytest.raises(ValueError):
        c.u_min[0] = 1.0                                      # read-only: rebind to change


# ---------------------------------------------------------------- C ABI (host-only calls)

def _lib():
    from mppi_robotarm_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        from mppi_robotarm_amd.build import build_native
        build_native()
    return N, N.load()


def test_config_init_leaves_the_clamp_off():
    N, lib = _lib()
    cfg = N.ConfigC()
    cfg.clamp_mode, cfg.u_min[0], cfg.u_max[1] = 2, -3.0, 5.0
    lib.mppi_config_init(C.byref(cfg))
    assert cfg.clamp_mode == 0 and list(cfg.u_min) == [0.0, 0.0] and list(cfg.u_max) == [0.0, 0.0]
    assert N.ConfigC().clamp_mode == 0
    # appended after param_gamma: the fields before them keep their offsets
    assert N.ConfigC.clamp_mode.offset > N.ConfigC.param_gamma.offset
    assert N.ConfigC.u_min.offset < N.ConfigC.u_max.offset == C.sizeof(N.ConfigC) - 16


def _valid_cfg(N, lib):
    cfg = N.ConfigC()
    lib.mppi_config_init(C.byref(cfg))
    cfg.K_local = cfg.K_total = 64
    cfg.T, cfg.delta_t, cfg.param_lambda, cfg.param_alpha = 8, 0.006, 100.0, 0.98
    cfg.sigma[0] = cfg.sigma[3] = 20.0
    return cfg


@pytest.mark.parametrize("mode,lo,hi,field", [
    (3, (0.0, 0.0), (1.0, 1.0), "clamp_mode"), (-1, (0.0, 0.0), (1.0, 1.0), "clamp_mode"),
    (1, (float("nan"), 0.0), (1.0, 1.0), "u_min"), (2, (0.0, 0.0), (1.0, float("nan")), "u_max"),
    (1, (0.0, 2.0), (1.0, 1.0), "u_min[d] > u_max[d]"), (2, (float("inf"), 0.0), (1.0, 1.0), "u_min[d] > u_max[d]"),
])
def test_ctx_create_rejects_bad_limits_before_any_device_call(mode, lo, hi, field):
    N, lib = _lib()
    cfg = _valid_cfg(N, lib)
    cfg.clamp_mode = mode
    for d in range(2):
        cfg.u_min[d], cfg.u_max[d] = lo[d], hi[d]
    ctx = C.c_void_p()
    rc = lib.mppi_ctx_create(C.byref(cfg), 0, None, C.byref(ctx))
    assert rc == N.MPPI_E_ARG and not ctx.value
    assert field in lib.mppi_last_error().decode()
    with pytest.raises(ValueError, match="mppi_ctx_create"):
        N.check(rc, "mppi_ctx_create")
