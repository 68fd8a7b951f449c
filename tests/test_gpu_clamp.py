"""GPU: torque limits (the reference's clamp hook _g, control.py:166-172, switched on) through every layer.

The fixtures are the reference's own outputs with _g clipping in place (tests/golden/make_golden_clamp.py);
oracle/mppi_oracle.py with limits, pinned to them on the CPU (test_clamp_cpu.py), is the yardstick at the other shapes.
Tolerances are the suite's (test_gpu_parity.py): u 1e-4, S 5e-5 with the same argmin, trajectories 1e-4.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mppi_oracle as O  # noqa: E402
from helpers import (CLAMP_STEPS, RUNPY, X0, _ctrl, _engine, _gpu, _inside, _urel, _window,  # noqa: E402, F401
                     load_clamp_loop, load_clamp_step)

U_TOL = 1e-4
S_TOL = 5e-5

LO, HI = np.array([6.0, -5.0]), np.array([12.0, 1.0])
LPS = (1, 2, 4, 8, 16)


# ---------------------------------------------------------------- 1, 2: the reference's own outputs

@pytest.mark.parametrize("how", ["general", "host_update", "device_noise"])
@pytest.mark.parametrize("name", CLAMP_STEPS)
def test_clamped_step_matches_reference(name, how, paths):
    """Each fixture through the drop-in: the general path, the host update, and the device-noise path (the
    native tick; the fused step with sampled trajectories where the fixture has them) fed the fixture's noise."""
    g = load_clamp_step(name)
    eps = g["eps"].astype(np.float64)
    if how == "device_noise":
        c = _ctrl(g, paths, noise="device", seed=3)
        eng = c._get_engine()
        eng.upload_noise(eps, out=c._noise_dev)              # in place of the Philox draw of (seed, step 0)
        c._noise_ready = (c.seed, c._step_count)
    else:
        c = _ctrl(g, paths, host_update=(how == "host_update"))
        c._calc_epsilon = lambda *a, **k: eps
    c.keep_costs = True
    u_prev = c.u_prev
    u0, u_seq, opt, samp = c.calc_control_input(g["x0"])
    if how == "device_noise" and not bool(g["sampled"]):
        assert c._bound is not None                          # the native tick really ran
    S = c.last_S
    print(f"{name}/{how}: S rel {float(np.max(np.abs(S - g['S']) / np.abs(g['S']))):.2e} "
          f"u rel {_urel(u_seq, g['u_seq']):.2e}")
    assert int(np.argmin(S)) == int(np.argmin(g["S"]))
    assert float(np.max(np.abs(S - g["S"]) / np.abs(g["S"]))) < S_TOL
    assert _urel(u_seq, g["u_seq"]) < U_TOL                  # case b: the fixture's nominal is the unclamped one
    assert _urel(u0, g["u0"]) < U_TOL
    assert u_seq is u_prev and np.shares_memory(u0, u_prev)
    assert c.prev_waypoints_idx == int(g["prev_idx_after"])
    if bool(g["visualize_optimal_traj"]):
        assert _inside(u_seq, g["u_min"], g["u_max"])        # exactly: the clamp is a selection
    else:
        assert not _inside(u_seq, g["u_min"], g["u_max"])
    np.testing.assert_allclose(opt, g["optimal_traj"], rtol=1e-4, atol=1e-4)
    if "sampled_traj" in g:
        np.testing.assert_allclose(samp, g["sampled_traj"], rtol=1e-4, atol=1e-4)
    else:
        assert not np.any(samp)
    c.close()


def test_clamped_closed_loop_ticks(paths):
    """Each tick of run.py's loop with limits, from the reference's own state / u_prev / index."""
    from mppi_robotarm_amd.controller import MPPIControllerForPathTracking
    g = load_clamp_loop("k64_t20")
    T, K = int(g["T"]), int(g["K"])
    c = MPPIControllerForPathTracking(delta_t=0.006, ref_path=paths["xydq_circle"], horizon_step_T=T,
                                      number_of_samples_K=K, verbose=False,
                                      visualize_optimal_traj=bool(g["visualize_optimal_traj"]),
                                      u_min=g["u_min"], u_max=g["u_max"], **RUNPY)
    u_prev = np.array([[10.0, -2.0]] * T)
    prev = 0
    for i in range(int(g["ticks"])):
        c.u_prev = u_prev.copy()
        c.prev_waypoints_idx = prev
        eps = g["eps"][i].astype(np.float64)
        c._calc_epsilon = lambda *a, e=eps, **k: e
        u, u_seq, _, _ = c.calc_control_input(g["states"][i])
        assert _urel(u_seq, g["u_seq"][i]) < U_TOL, i
        assert _inside(u_seq, g["u_min"], g["u_max"]), i
        assert c.prev_waypoints_idx == int(g["prev_idx"][i])
        u_prev, prev = g["u_seq"][i].copy(), int(g["prev_idx"][i])
    c.close()


# ---------------------------------------------------------------- 3: every kernel variant against the oracle

K3, T3 = 1000, 9          # ragged K; T no multiple of the 4-deep ring and >= 5 for the device median
_ref3 = {}


def _u3():
    return np.array([[10.0, -2.0]] * T3) + np.random.default_rng(1).normal(0, 0.5, (T3, 2))


def _reference3(lam, eps_tk, paths):
    """The oracle's clamped step on the read-back Philox noise of (seed 42, step 3), computed once per lambda and shared."""
    if lam not in _ref3:
        _ref3[lam] = (eps_tk.copy(), O.step(X0, _u3(), eps_tk.transpose(1, 0, 2).astype(np.float64),
                                            paths["xydq_circle"], 0, 0.006, lam, 0.98, RUNPY["sigma"],
                                            RUNPY["stage_cost_weight"], RUNPY["terminal_cost_weight"],
                                            lo=LO, hi=HI))
    assert np.array_equal(_ref3[lam][0], eps_tk)
    return _ref3[lam][1]


@pytest.mark.parametrize("lam", [100.0, 3.0e6])
@pytest.mark.parametrize("handoff", ["default", "counter"])
@pytest.mark.parametrize("lps", LPS)
def test_every_clamp_kernel_variant_against_clamp_ref(lps, handoff, lam, paths, monkeypatch):
    if handoff == "counter":
        monkeypatch.setenv("MPPI_HANDOFF", "counter")
    eng = _engine(K3, T3, lps=lps, param_lambda=lam, u_min=LO, u_max=HI)
    assert eng.lanes_per_sample == lps and eng.handoff == ("counter" if handoff == "counter" else "poll")
    eng.set_step_inputs(X0, _window(paths), _u3())
    noise = eng.philox_noise(42, 3)
    S_dev = torch.empty(K3, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S_dev)
    w_eps = eng.weighted_noise()
    S = S_dev.cpu().numpy()
    r = _reference3(lam, noise.cpu().numpy(), paths)
    v = O.sampled_controls(_u3(), noise.cpu().numpy().transpose(1, 0, 2), LO, HI)
    assert np.mean((v == LO) | (v == HI)) > 0.10             # the clamp is live at these limits
    print(f"lps {lps} {handoff} lam {lam}: S rel {float(np.max(np.abs(S - r['S']) / np.abs(r['S']))):.2e} "
          f"w_eps rel {_urel(w_eps, r['w_eps_raw']):.2e}")
    assert float(np.max(np.abs(S - r["S"]) / np.abs(r["S"]))) < S_TOL
    j, j_ref = int(np.argmin(S)), int(np.argmin(r["S"]))     # or a near-tie at fp32 resolution, as the suite's sweep
    assert j == j_ref or abs(r["S"][j] - r["S"][j_ref]) <= 1e-6 * abs(r["S"][j_ref])
    assert _urel(w_eps, r["w_eps_raw"]) < U_TOL
    eng.rollout(noise, fused_update=True)
    u = eng.nominal()
    assert _urel(u, r["u_seq"]) < U_TOL
    assert _inside(u, LO, HI)                                # fp64 comparison, no tolerance
    eng.close()


# ---------------------------------------------------------------- 4: wide limits are the identity, bit for bit

@pytest.mark.parametrize("lps", LPS)
def test_wide_limits_are_the_identity_bit_for_bit(lps, paths):
    """The CLAMP kernels with limits no control reaches against the kernels without: the same arithmetic."""
    outs = []
    for lim, nominal in ((None, True), (1e30, True), (1e30, False)):
        kw = {} if lim is None else dict(u_min=-lim, u_max=lim, clamp_nominal=nominal)
        eng = _engine(K3, T3, lps=lps, **kw)
        eng.set_step_inputs(X0, _window(paths, 3), _u3())
        S_dev = torch.empty(K3, dtype=torch.float64, device="cuda")
        got = []
        for step in range(3):
            noise = eng.philox_noise(7, step)
            eng.rollout(noise, S_out=S_dev, fused_update=True)
            got += [S_dev.cpu().numpy(), eng.weighted_noise(), eng.nominal(),
                    eng.trajectories().cpu().numpy(), eng.trajectories(noise=noise).cpu().numpy(),
                    eng.optimal_traj().cpu().numpy()]
        outs.append(got)
        eng.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------- 5: mode 1 against mode 2 at the engine

def test_nominal_clamp_is_mode_2_only_and_feeds_the_next_launch(paths):
    K, T = 512, 8
    lo, hi = np.array([9.5, -2.5]), np.array([10.5, -1.5])
    res = {}
    for mode2 in (False, True):
        eng = _engine(K, T, u_min=lo, u_max=hi, clamp_nominal=mode2)
        eng.set_step_inputs(X0, _window(paths), np.array([[10.0, -2.0]] * T))
        S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
        eng.rollout(eng.philox_noise(5, 0), S_out=S_dev, fused_update=True)
        S0, u1 = S_dev.cpu().numpy(), eng.nominal()
        eng.rollout(eng.philox_noise(5, 1), S_out=S_dev)
        res[mode2] = (S0, u1, S_dev.cpu().numpy())
        eng.close()
    assert np.array_equal(res[False][0], res[True][0])        # the first launch is the same
    assert not _inside(res[False][1], lo, hi)                 # mode 1 leaves the nominal as updated
    assert np.array_equal(res[True][1], np.clip(res[False][1], lo, hi))   # to the last bit
    assert not np.array_equal(res[False][2], res[True][2])    # a_t of the next launch follows the clipped nominal


# ---------------------------------------------------------------- 6: merge path

@pytest.mark.parametrize("lam", [100.0, 3.0e6])
def test_merge_kernel_clamps_the_nominal(lam, paths):
    one = _engine(K3, T3, param_lambda=lam, u_min=LO, u_max=HI)
    one.set_step_inputs(X0, _window(paths), _u3())
    noise = one.philox_noise(42, 3)
    one.rollout(noise, fused_update=True)
    want = one.nominal()
    r = _reference3(lam, noise.cpu().numpy(), paths)
    assert _urel(want, r["u_seq"]) < U_TOL
    Kl = K3 // 2
    parts = torch.empty(2 * one.partial_len, dtype=torch.float64, device="cuda")
    engs = []
    for s in range(2):
        e = _engine(Kl, T3, K_total=K3, k_offset=s * Kl, param_lambda=lam, u_min=LO, u_max=HI)
        e.set_step_inputs(X0, _window(paths), _u3())
        nz = e.philox_noise(42, 3)
        assert torch.equal(nz, noise[:, s * Kl:(s + 1) * Kl])
        e.rollout(nz, partial_out=parts[s * e.partial_len:(s + 1) * e.partial_len])
        engs.append(e)
    engs[0].merge(parts, 2, fused_update=True)
    got = engs[0].nominal()
    assert _urel(got, want) < U_TOL
    assert _inside(got, LO, HI)
    for e in engs + [one]:
        e.close()


# ---------------------------------------------------------------- 7: bound tick and fast path

def test_bound_tick_with_limits_equals_general_dropin_and_follows_new_limits(paths):
    from mppi_robotarm_amd.controller import MPPIControllerForPathTracking
    lo, hi = np.array([4.0, -6.0]), np.array([14.0, 2.0])
    base = paths["xydq_circle"][:400].copy()
    kw = dict(delta_t=0.006, horizon_step_T=12, number_of_samples_K=256, verbose=False, noise="device", seed=3,
              device=0, u_min=lo, u_max=hi, **RUNPY)
    fast = MPPIControllerForPathTracking(ref_path=base[:, 0:4], **kw)
    slow = MPPIControllerForPathTracking(ref_path=base[:, 0:4].copy(order="F"), **kw)   # column-major: no tick
    for c in (fast, slow):
        c.Sigma = np.array(c.Sigma, dtype=np.float64)
        c.stage_cost_weight = np.array(c.stage_cost_weight, dtype=np.float64)
        c.terminal_cost_weight = np.array(c.terminal_cost_weight, dtype=np.float64)
    fast_hits = []
    tick_bound = fast._tick_bound
    fast._tick_bound = lambda x: (fast_hits.append(fast._fast is not None), tick_bound(x))[1]
    for call in range(5):
        ua = fast.calc_control_input(X0)
        ub = slow.calc_control_input(X0)
        assert np.array_equal(ua[1], ub[1]) and np.array_equal(ua[2], ub[2]), call
        assert _inside(ua[1], lo, hi), call
    assert fast._bound is not None and slow._bound is None
    assert len(fast_hits) == 4 and any(fast_hits)            # bound ticks, and the fast test was taken
    eng = fast._engine
    new_hi = np.array([9.0, -3.0])                           # below the nominal of (10, -2): they must act
    fast.u_max = slow.u_max = new_hi
    ua = fast.calc_control_input(X0)
    ub = slow.calc_control_input(X0)
    assert fast._engine is not eng                           # rebuilt with the new limits
    assert _inside(ua[1], lo, new_hi) and np.array_equal(ua[1], ub[1])
    assert np.any(ua[1] == new_hi)
    fast.close()
    slow.close()


# ---------------------------------------------------------------- 8: ctx_create error paths through the engine

def test_engine_rejects_bad_limits(monkeypatch):
    from mppi_robotarm_amd import _native as N
    from mppi_robotarm_amd.engine import RolloutEngine
    with pytest.raises(ValueError, match="u_min"):
        _engine(64, 8, u_min=[float("nan"), 0.0], u_max=[1.0, 1.0])
    assert "u_min" in N.load().mppi_last_error().decode()
    with pytest.raises(ValueError, match="u_max"):
        _engine(64, 8, u_min=[0.0, 0.0], u_max=[1.0, float("nan")])
    with pytest.raises(ValueError, match=r"u_min\[d\] > u_max\[d\]"):
        _engine(64, 8, u_min=[0.0, 2.0], u_max=[1.0, 1.0])
    monkeypatch.setattr(RolloutEngine, "clamp_mode", staticmethod(lambda *a: 3))
    with pytest.raises(ValueError, match="clamp_mode"):
        _engine(64, 8, u_min=0.0, u_max=1.0)
    assert "clamp_mode" in N.load().mppi_last_error().decode()
    monkeypatch.undo()
    eng = _engine(64, 8, u_min=[-np.inf, 0.0], u_max=[1.0, np.inf])   # one-sided limits are fine
    eng.close()
