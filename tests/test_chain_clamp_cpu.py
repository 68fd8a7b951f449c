"""CPU: torque limits of the n-link chain (mppi_chain_config.clamp_mode / u_min / u_max).

  * oracle/chain_oracle.py with limits (lo / hi), the NumPy restatement the GPU tests use as their yardstick,
    reproduces at n = 2 (ChainParams.from_arm2()) every clamp_step_* fixture captured from the reference itself;
  * the C ABI: the three new fields' layout against the header (a gcc probe, as test_abi.py), the fields before
    them where they were, mppi_chain_config_init leaves the clamp off, mppi_chain_ctx_create rejects bad limits
    before any device call (so these run without a GPU) and names the field in mppi_last_error;
  * ChainMPPIController's constructor validation and engine key.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chain_oracle as CO
from conftest import ROOT
from helpers import CLAMP_STEPS, load_clamp_step
from mppi_robotarm_amd.chain import CHAIN7_SIGMA, ChainMPPIController, ChainParams

HEADER = os.path.join(ROOT, "include", "mppi_rocm.h")


@pytest.mark.parametrize("name", CLAMP_STEPS)
def test_chain_clamp_ref_at_n2_matches_the_reference(name, paths):
    g = load_clamp_step(name)
    r = CO.step(g["x0"], g["u_prev"], g["eps"].astype(np.float64), paths[str(g["path"])], int(g["prev_idx_after"]),
                float(g["delta_t"]), float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"],
                g["stage_cost_weight"], g["terminal_cost_weight"], lo=g["u_min"], hi=g["u_max"],
                expl=float(g["param_exploration"]), visualize_optimal_traj=bool(g["visualize_optimal_traj"]),
                sampled=bool(g["sampled"]), P=CO.ChainParams.from_arm2())
    assert int(np.argmin(r["S"])) == int(np.argmin(g["S"]))
    assert float(np.max(np.abs(r["S"] - g["S"]) / np.abs(g["S"]))) < 1e-12
    np.testing.assert_allclose(r["w_eps_filt"], g["w_eps_filt"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["u_seq"], g["u_seq"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["optimal_traj"], g["optimal_traj"], rtol=1e-10, atol=1e-10)
    if "sampled_traj" in g:
        np.testing.assert_allclose(r["sampled_traj"], g["sampled_traj"], rtol=1e-10, atol=1e-10)
    inside = bool(np.all((r["u_seq"] >= g["u_min"]) & (r["u_seq"] <= g["u_max"])))
    assert inside == bool(g["visualize_optimal_traj"])     # case b: the nominal is left unclamped


# ---------------------------------------------------------------- C ABI (host-only calls)

def _lib():
    from mppi_robotarm_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        from mppi_robotarm_amd.build import build_native
        build_native()
    return N, N.load()


def test_chain_clamp_fields_layout_matches_header(tmp_path):
    from mppi_robotarm_amd import _native as N
    probe = tmp_path / "probe.c"
    probe.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "mppi_rocm.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mppi_chain_config), offsetof(mppi_chain_config, precision),
         offsetof(mppi_chain_config, lanes_per_sample), offsetof(mppi_chain_config, param_gamma),
         offsetof(mppi_chain_config, clamp_mode), offsetof(mppi_chain_config, u_min),
         offsetof(mppi_chain_config, u_max), sizeof(((mppi_chain_config *)0)->u_max));
  return 0;
}
''')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(probe), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Cc = N.ChainConfigC
    assert vals == [C.sizeof(Cc), Cc.precision.offset, Cc.lanes_per_sample.offset, Cc.param_gamma.offset,
                    Cc.clamp_mode.offset, Cc.u_min.offset, Cc.u_max.offset, 8 * N.CHAIN_MAX_DOF]
    # appended after param_gamma, in this order, the last field of the struct
    assert Cc.param_gamma.offset < Cc.clamp_mode.offset < Cc.u_min.offset < Cc.u_max.offset
    assert Cc.u_max.offset + 8 * N.CHAIN_MAX_DOF == C.sizeof(Cc)
    assert [f for f, _ in Cc._fields_][-4:] == ["param_gamma", "clamp_mode", "u_min", "u_max"]


def test_chain_config_init_leaves_the_clamp_off():
    N, lib = _lib()
    cfg = N.ChainConfigC()
    cfg.clamp_mode, cfg.u_min[0], cfg.u_max[6] = 2, -3.0, 5.0
    lib.mppi_chain_config_init(C.byref(cfg))
    assert cfg.clamp_mode == 0 and list(cfg.u_min) == [0.0] * 8 and list(cfg.u_max) == [0.0] * 8
    assert np.isnan(cfg.param_gamma) and cfg.chain.g == 9.81
    assert N.ChainConfigC().clamp_mode == 0 and np.isnan(N.ChainConfigC().param_gamma)


def _valid_cfg(N, lib, n=3):
    cfg = N.ChainConfigC()
    lib.mppi_chain_config_init(C.byref(cfg))
    cfg.K_local = cfg.K_total = 64
    cfg.T, cfg.delta_t, cfg.param_lambda, cfg.param_alpha = 8, 0.006, 100.0, 0.98
    cfg.chain.n = n
    for a in range(n):
        cfg.sigma[a * n + a] = 4.0
        cfg.chain.m[a] = cfg.chain.l[a] = cfg.chain.fk[a] = cfg.chain.I[a] = 1.0
        cfg.chain.lc[a] = 0.5
    return cfg


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("mode,lo,hi,field", [
    (3, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), "clamp_mode"), (-1, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), "clamp_mode"),
    (1, (0.0, 0.0, NAN), (1.0, 1.0, 1.0), "u_min"), (2, (0.0, 0.0, 0.0), (1.0, NAN, 1.0), "u_max"),
    (1, (0.0, 0.0, 2.0), (1.0, 1.0, 1.0), "u_min[d] > u_max[d]"), (2, (INF, 0.0, 0.0), (1.0, 1.0, 1.0), "u_min[d] > u_max[d]"),
])
def test_chain_ctx_create_rejects_bad_limits_before_any_device_call(mode, lo, hi, field):
    N, lib = _lib()
    cfg = _valid_cfg(N, lib)
    cfg.clamp_mode = mode
    for d in range(3):
        cfg.u_min[d], cfg.u_max[d] = lo[d], hi[d]
    ctx = C.c_void_p()
    rc = lib.mppi_chain_ctx_create(C.byref(cfg), 0, None, C.byref(ctx))
    assert rc == N.MPPI_E_ARG and not ctx.value
    assert field in lib.mppi_last_error().decode()
    with pytest.raises(ValueError, match="mppi_chain_ctx_create"):
        N.check(rc, "mppi_chain_ctx_create")


# ---------------------------------------------------------------- the drop-in

def _ctrl(paths, n=7, **kw):
    sig = CHAIN7_SIGMA if n == 7 else np.eye(n) * 4.0
    chain = ChainParams() if n == 7 else ChainParams.from_arm2()
    return ChainMPPIController(0.006, paths["xydq_circle"], 8, 16, sigma=sig, chain=chain, **kw)


def test_chain_constructor_validation(paths):
    with pytest.raises(ValueError, match="u_min"):
        _ctrl(paths, u_min=[0.0] * 6 + [NAN], u_max=1.0)
    with pytest.raises(ValueError, match="u_max"):
        _ctrl(paths, u_min=-1.0, u_max=NAN)
    with pytest.raises(ValueError, match="exceeds"):
        _ctrl(paths, u_min=[0.0] * 6 + [2.0], u_max=1.0)
    with pytest.raises(ValueError, match=r"u_max.*\(7\)"):
        _ctrl(paths, u_min=0.0, u_max=[1.0, 1.0])                    # the arm's two values on a 7-link chain
    with pytest.raises(ValueError, match=r"u_min.*\(2\)"):
        _ctrl(paths, n=2, u_min=[0.0] * 7, u_max=1.0)
    with pytest.raises(ValueError, match="u_min"):
        _ctrl(paths, u_min=np.zeros((7, 7)), u_max=1.0)
    c = _ctrl(paths, u_min=-0.8, u_max=0.8)
    assert c.u_min.tolist() == [-0.8] * 7 and c.u_max.tolist() == [0.8] * 7
    assert c.u_min.dtype == np.float64 and c.u_min.shape == (7,)
    c = _ctrl(paths, u_max=[14.0] * 6 + [INF])                     # one-sided
    assert c.u_min is None and c._limits()[0].tolist() == [-np.inf] * 7
    c = _ctrl(paths)
    assert c.u_min is None and c.u_max is None and c._limits() is None
    with pytest.raises(TypeError):                                  # keyword-only, as every extra argument
        ChainMPPIController(0.006, paths["xydq_circle"], 8, 16, 0.0, 100.0, 0.98, CHAIN7_SIGMA, np.ones(4), np.ones(4),
                            True, False, -1.0, 1.0)


def test_chain_limits_and_the_trajectory_switch_enter_the_engine_key(paths):
    lo, hi = np.arange(7.0) - 3.0, np.arange(7.0) + 2.0
    c = _ctrl(paths, u_min=lo, u_max=hi)
    c._activate("f32")
    k0 = c._engine_key()
    assert c._clamp_key()[0] == 2 and k0[-1] == c._clamp_key()
    c.u_max = hi + 1.0
    assert c._engine_key() != k0
    c.u_max = hi
    assert c._engine_key() == k0
    c._activate("f64")                                               # the other engine of precision="auto"
    k64 = c._engine_key()
    assert k64 != k0 and k64[-1] == k0[-1]
    c._activate("f32")
    c.visualize_optimal_traj = False                                 # the nominal's clamp lives in that loop
    assert c._clamp_key()[0] == 1 and c._engine_key() != k0
    c.u_min = c.u_max = None
    assert c._clamp_key() == (0,)
    assert _ctrl(paths)._clamp_key() == (0,)
    c.u_min, c.u_max = hi, lo
    with pytest.raises(ValueError, match="exceeds"):
        c._engine_key()
    with pytest.raises(ValueError):
        c.u_min[0] = 1.0                                             # read-only: rebind to change
    v = np.array([[9.0] * 7, [-9.0] * 7])
    d = _ctrl(paths, u_min=lo, u_max=hi)
    assert d._g(v) is v and v[0].tolist() == hi.tolist() and v[1].tolist() == lo.tolist()
