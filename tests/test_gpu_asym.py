"""GPU: the 2-link arm's kernels away from the reference's one, symmetric parameter point.

Every other GPU test runs ArmParams() (m1 = m2, l1 = l2, lc1 = lc2, fk_l1 = fk_l2), cost weights whose pairs have
equal halves, delta_t = 0.006 and a start pose within 0.05 rad of run.py's: there an exchange of two constants, of
the halves of a register pair or of two weights changes no output bit.  Here the same comparisons run at the two
asymmetric parameter sets of tests/golden/make_golden_asym.py (the reference itself run with its constants
reassigned), whose inputs tests/test_asym_cpu.py shows to move the fp64 cost by >= 1e-3 under each such exchange,
with discs that tell the two link lengths apart, and, at the default parameters, over the arm's state space:
every quadrant, both elbows, stretched and folded, fast joints, whole turns.

Tolerances are the suite's, unchanged (test_gpu_parity.py): S 5e-5 relative with the same argmin (or an fp32
near-tie, as test_random_configs_against_c_oracle allows), w_eps / u 1e-4 of max(1, |.|), trajectories 1e-4.
"""
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import coracle  # noqa: E402
import mppi_oracle as O  # noqa: E402
from conftest import record  # noqa: E402
from helpers import (ASYM_CASES, ASYM_STEPS, RUNPY, X0, _ctrl, _engine, _gpu, _urel, arm_of, asym_cfg,  # noqa: E402, F401
                     asym_engine, asym_obstacle_problem, asym_problem, asym_rollout, load_asym_loop, load_asym_step)
from tieflip import waypoint_pick_delta  # noqa: E402

U_TOL = 1e-4
S_TOL = 5e-5
EDGE = 4e-6                 # test_gpu_obstacles.py's: the clearance within which a flag may fall on either side
EDGE_CAP = 0.005
LPS = (1, 2, 4, 8, 16)


def _near_tie_argmin(S, ref_S):
    j, j_ref = int(np.argmin(S)), int(np.argmin(ref_S))
    return j == j_ref or abs(ref_S[j] - ref_S[j_ref]) <= 1e-6 * abs(ref_S[j_ref])


def _c_oracle(g, cfg, x0, win, u, eps_tk, K):
    ref_S = coracle.rollout_costs(x0, u, eps_tk, win, cfg["delta_t"], cfg["param_lambda"], cfg["param_alpha"],
                                  cfg["sigma"], cfg["stage_cost_weight"], cfg["terminal_cost_weight"],
                                  arm_of(g, O.ArmParams), k_exploit=math.ceil((1.0 - cfg["param_exploration"]) * K),
                                  layout="TK")
    return ref_S, coracle.weighted_noise(ref_S, eps_tk, cfg["param_lambda"], layout="TK")[1]


# ---------------------------------------------------------------- 1: the rollout in every form

_forms = {}


def _all_forms(name, K, T, paths):
    """S and w_eps of one case at every lanes-per-sample split and in both hand-off forms, on the Philox noise of
    (seed 42, step 3), with the C oracle's: computed once per case and shared."""
    if (name, K, T) not in _forms:
        g, cfg, x0, prev, u = asym_problem(name, T)
        win = paths["xydq_circle"][prev:prev + 30]
        runs, eps_tk = {}, None
        saved = os.environ.get("MPPI_HANDOFF")
        try:
            for form in ("poll", "counter"):
                if form == "counter":
                    os.environ["MPPI_HANDOFF"] = "counter"
                else:
                    os.environ.pop("MPPI_HANDOFF", None)
                for lps in LPS:
                    eng = asym_engine(g, K, T, lps=lps)
                    assert eng.lanes_per_sample == lps and eng.handoff == form
                    eng.set_step_inputs(x0, win, u)
                    noise = eng.philox_noise(42, 3)
                    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
                    eng.rollout(noise, S_out=S_dev)
                    runs[(lps, form)] = (S_dev.cpu().numpy(), eng.weighted_noise())
                    if eps_tk is None:
                        eps_tk = noise.cpu().numpy()
                    else:
                        assert np.array_equal(noise.cpu().numpy(), eps_tk)
                    eng.close()
        finally:
            os.environ.pop("MPPI_HANDOFF", None)
            if saved is not None:
                os.environ["MPPI_HANDOFF"] = saved
        _forms[(name, K, T)] = (runs, _c_oracle(g, cfg, x0, win, u, eps_tk, K), cfg)
    return _forms[(name, K, T)]


@pytest.mark.parametrize("name,K,T", ASYM_CASES)
def test_rollout_against_c_oracle_in_every_form(name, K, T, paths):
    runs, (ref_S, ref_weps), cfg = _all_forms(name, K, T, paths)
    worst_S = worst_w = 0.0
    for form, (S, weps) in runs.items():
        rel = float(np.max(np.abs(S - ref_S) / np.abs(ref_S)))
        worst_S, worst_w = max(worst_S, rel), max(worst_w, _urel(weps, ref_weps))
    print(f"{name} K {K} T {T}: S max rel {worst_S:.2e}, w_eps {worst_w:.2e} over {len(runs)} forms")
    record("asym_rollout", case=name, K=K, T=T, S_max_rel_err=worst_S, w_eps_rel_err=worst_w)
    for form, (S, weps) in runs.items():
        assert np.all(np.isfinite(S)), form
        assert float(np.max(np.abs(S - ref_S) / np.abs(ref_S))) < S_TOL, form
        assert _near_tie_argmin(S, ref_S), form
        assert _urel(weps, ref_weps) < U_TOL, form


@pytest.mark.parametrize("name,K,T", ASYM_CASES)
def test_forms_are_bit_identical(name, K, T, paths):
    """S: the same bits at every lanes-per-sample split and in both hand-off forms.  w_eps: the same bits across
    the hand-off forms of one split, and across splits where one sample carries all the weight; 1e-10 where
    several do (the workgroups sum other groups of samples): test_deterministic_and_lanes_per_sample_invariant's
    property."""
    runs, _, cfg = _all_forms(name, K, T, paths)
    S0, w0 = runs[(LPS[0], "poll")]
    one_hot = np.count_nonzero(np.exp(-(S0 - S0.min()) / cfg["param_lambda"])) == 1
    for (lps, form), (S, w) in runs.items():
        assert np.array_equal(S, S0), (lps, form)
        assert np.array_equal(w, runs[(lps, "poll")][1]), (lps, form)
        if one_hot:
            assert np.array_equal(w, w0), (lps, form)
        else:
            np.testing.assert_allclose(w, w0, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("T", [5, 9, 20])
def test_fused_update_equals_host_update(T, paths):
    """Set a: the fused median filter, u += w_eps and shift against SciPy and the fp64 add on the host, bit for
    bit, over three launches; the launch after an update runs on the device-written nominal."""
    from scipy.ndimage import median_filter
    K = 1000
    g, cfg, x0, prev, u = asym_problem("a_k128_t20", T)
    eng = asym_engine(g, K, T, param_lambda=1.0e4)
    eng.set_step_inputs(x0, paths["xydq_circle"][prev:prev + 30], u)
    for step in range(3):
        eng.rollout(eng.philox_noise(5, step), fused_update=True)
        w = eng.weighted_noise()
        assert np.any(w != 0.0)
        un = u + np.stack([median_filter(w[:, d], size=10, mode="reflect") for d in range(2)], 1)
        expect = np.concatenate([un[1:], un[-1:]], 0)
        got = eng.nominal()
        np.testing.assert_array_equal(got, expect)
        u = got
    eng.close()


# ---------------------------------------------------------------- 2: trajectories

@pytest.mark.parametrize("limits", [False, True], ids=["free", "clamped"])
def test_trajectories_match_oracle(limits, paths):
    """Set a, traj_kernel with and without NOISE and CLAMP: the sampled re-roll, the nominal's re-roll and the
    optimal trajectory of a fused update against O.rollout_trajectory; limits distinct per joint."""
    K, T = 64, 20
    g, cfg, x0, prev, u = asym_problem("a_k128_t20", T)
    arm = arm_of(g, O.ArmParams)
    lo, hi = (u[0] + np.array([-3.0, -2.0]), u[0] + np.array([3.5, 2.5])) if limits else (None, None)
    eng = asym_engine(g, K, T, u_min=lo, u_max=hi)
    eng.set_step_inputs(x0, paths["xydq_circle"][prev:prev + 30], u)
    noise = eng.philox_noise(2, 0)
    eps = noise.cpu().numpy().transpose(1, 0, 2).astype(np.float64)
    v = O.sampled_controls(u, eps, lo, hi, expl=cfg["param_exploration"])
    if limits:
        assert 0.2 < float(np.mean(v != O.sampled_controls(u, eps, expl=cfg["param_exploration"]))) < 0.8
    want = O.rollout_trajectory(x0, np.roll(v, 1, axis=1), cfg["delta_t"], arm)
    worst = {}
    for key, tr in (("noise, given base", eng.trajectories(base_u=u, noise=noise)),
                    ("noise, staged base", eng.trajectories(noise=noise))):
        tr = tr.double().cpu().numpy()
        worst[key] = float(np.max(np.abs(tr - want)))
        np.testing.assert_allclose(tr, want, rtol=1e-4, atol=1e-4)
    un = u + np.random.default_rng(3).normal(0, 2.0, u.shape)
    if limits:
        assert not np.all((un >= lo) & (un <= hi))
    want0 = O.rollout_trajectory(x0, np.roll(un if lo is None else np.clip(un, lo, hi), 1, axis=0), cfg["delta_t"], arm)
    tr0 = eng.trajectories(base_u=un, K=1).double().cpu().numpy()[0]
    np.testing.assert_allclose(tr0, want0, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(eng.optimal_traj_host(x0, un), want0, rtol=1e-10, atol=1e-10)
    # the optimal trajectory of a fused update, from the update's own controls before their shift
    from scipy.ndimage import median_filter
    eng.rollout(noise, fused_update=True)
    w = eng.weighted_noise()
    u_new = u + np.stack([median_filter(w[:, d], size=10, mode="reflect") for d in range(2)], 1)
    if limits:
        u_new = np.clip(u_new, lo, hi)
    opt = eng.optimal_traj().double().cpu().numpy()
    want_opt = O.rollout_trajectory(x0, np.roll(u_new, 1, axis=0), cfg["delta_t"], arm)
    np.testing.assert_allclose(opt, want_opt, rtol=1e-4, atol=1e-4)
    worst.update(nominal=float(np.max(np.abs(tr0 - want0))), optimal=float(np.max(np.abs(opt - want_opt))))
    print(f"trajectories ({'clamped' if limits else 'free'}): max abs err {worst}")
    record("asym_traj", limits=limits, **worst)
    eng.close()


# ---------------------------------------------------------------- 3: the fixtures through the drop-ins

def _feed(c, eps, how):
    if how == "tick":
        eng = c._get_engine()
        eng.upload_noise(eps, out=c._noise_dev)              # in place of the Philox draw of (seed, step)
        c._noise_ready = (c.seed, c._step_count)
    else:
        c._calc_epsilon = lambda *a, **k: eps


@pytest.mark.parametrize("how", ["general", "tick"])
@pytest.mark.parametrize("name", ASYM_STEPS)
def test_step_matches_reference(name, how, paths):
    """Each asym_step_* fixture through MPPIControllerForPathTracking(arm=...), fed through the general call and
    through the bound native tick (whose nearest-waypoint update runs on the host from fk_l1, fk_l2)."""
    from mppi_robotarm_amd.params import ArmParams
    g = load_asym_step(name)
    eps = g["eps"].astype(np.float64)
    sampled = bool(g["sampled"]) and how != "tick"   # the tick has no sampled trajectories: the general call has them
    g["sampled"] = np.bool_(sampled)
    c = _ctrl(g, paths, arm=arm_of(g, ArmParams), **(dict(noise="device", seed=3) if how == "tick" else {}))
    _feed(c, eps, how)
    c.keep_costs = True
    u_prev = c.u_prev
    u0, u_seq, opt, samp = c.calc_control_input(g["x0"])
    if how == "tick":
        assert c._bound is not None                          # the native tick really ran
    S = c.last_S
    assert u_seq is u_prev and np.shares_memory(u0, u_prev)
    assert c.prev_waypoints_idx == int(g["prev_idx_after"])
    if "obstacles" not in g:
        rel = float(np.max(np.abs(S - g["S"]) / np.abs(g["S"])))
        print(f"{name}/{how}: S rel {rel:.2e}, u rel {_urel(u_seq, g['u_seq']):.2e}")
        record("asym_step", fixture=name, how=how, S_max_rel_err=rel, u_rel_err=_urel(u_seq, g["u_seq"]))
        assert int(np.argmin(S)) == int(np.argmin(g["S"]))
        assert rel < S_TOL
        assert _urel(u_seq, g["u_seq"]) < U_TOL and _urel(u0, g["u0"]) < U_TOL
        np.testing.assert_allclose(opt, g["optimal_traj"], rtol=1e-4, atol=1e-4)
        if sampled:
            np.testing.assert_allclose(samp[g["sampled_idx"]], g["sampled_traj"], rtol=1e-4, atol=1e-4)
        else:
            assert not np.any(samp)
    else:
        # as test_gpu_obstacles.test_obstructed_step_matches_reference: S on the samples that keep 1e-4 m from
        # every boundary (at least 80 %), and the update with the device's own hit counts in the yardstick, so a
        # state within rounding of a boundary cannot move a weight
        clean = g["clearance"].min(1) >= 1e-4
        assert float(np.mean(clean)) >= 0.80
        w = float(g["obstacle_cost"])
        r = O.rollout_costs(g["x0"], g["u_prev"], eps, paths["xydq_circle"], int(g["prev_idx_after"]),
                            float(g["delta_t"]), float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"],
                            g["stage_cost_weight"], g["terminal_cost_weight"], float(g["param_exploration"]),
                            arm_of(g, O.ArmParams), lo=g["u_min"], hi=g["u_max"], discs=g["obstacles"],
                            obstacle_cost=w, details=True)
        # The cost's other discontinuity, as test_gpu_obstacles.test_obstructed_closed_loop_ticks meets it: this
        # fixture's end effector sweeps 1 mm a step along the path's start, whose waypoints lie 6e-5 m apart, and in
        # fp64 260 of its 2560 (sample, step) pairs lie within 4e-6 m of the bisector of two of them, where the
        # device may take the neighbour.  The fp64 cost takes the device's OWN picks (mppi_debug_nearest); nothing is
        # excluded, and every differing pick must itself be such a tie, on at most 0.5 % of the pairs.
        window = paths["xydq_circle"][c.prev_waypoints_idx:c.prev_waypoints_idx + 30]
        c._engine.set_step_inputs(g["x0"], window, g["u_prev"])     # (the launch above moved the nominal on)
        slots, _ = c._engine.nearest_slots(c._engine.upload_noise(eps))
        delta, gap, differ = waypoint_pick_delta(r, slots, window, g["stage_cost_weight"], g["terminal_cost_weight"])
        ref = g["S"] + delta
        plain = float(np.max(np.abs(S[clean] - g["S"][clean]) / np.abs(g["S"][clean])))
        rel = float(np.max(np.abs(S[clean] - ref[clean]) / np.abs(ref[clean])))
        print(f"{name}/{how}: {int(differ.sum())} picks differ from fp64, largest gap {float(gap.max()):.1e} m; "
              f"S rel {plain:.2e} with the fp64 picks")
        assert float(gap.max()) <= EDGE and float(np.mean(differ)) <= EDGE_CAP
        hits = np.rint((S - r["S_track"] - delta) / w)
        same = float(np.mean(hits == r["hits"]))
        up = O.update(r["S_track"] + delta + w * hits, g["u_prev"], eps, float(g["param_lambda"]), g["x0"],
                      float(g["delta_t"]), g["u_min"], g["u_max"], p=arm_of(g, O.ArmParams))
        print(f"{name}/{how}: S rel {rel:.2e} on {int(clean.sum())}/{clean.size} samples, hit counts equal on "
              f"{same:.1%}, u rel {_urel(u_seq, up['u_seq']):.2e}")
        record("asym_step", fixture=name, how=how, S_max_rel_err=rel, u_rel_err=_urel(u_seq, up["u_seq"]))
        assert rel < S_TOL and same >= 0.99
        assert 0.10 <= float(np.mean(hits > 0)) <= 0.90
        assert _urel(u_seq, up["u_seq"]) < U_TOL
        np.testing.assert_allclose(opt, up["optimal_traj"], rtol=1e-4, atol=1e-4)
        assert bool(np.all((u_seq >= g["u_min"]) & (u_seq <= g["u_max"])))
        if same == 1.0 and clean[np.argsort(g["S"])[:2]].all():
            assert int(np.argmin(S)) == int(np.argmin(g["S"]))
            assert _urel(u_seq, g["u_seq"]) < U_TOL
    c.close()


# Fixture d sweeps the dense start of the path (see test_step_matches_reference) and the chain has no read-back of
# its picks at n = 2 to account for the ties with: measured, its fp32 rollout is 7.3e-4 off on one sample, the
# size of one neighbour pick.  The fp64 rollout has no such ties, so "auto" keeps every fixture.
@pytest.mark.parametrize("name,precision", [(n, "auto") for n in ASYM_STEPS] +
                         [(n, "f32") for n in ASYM_STEPS if "clamp" not in n])
def test_chain_at_n2_reproduces_reference_steps(name, precision, paths):
    """The fixtures through the chain kernels at n = 2 with ChainParams.from_arm2(arm): test_gpu_chain.py's check.
    The chain has no discs: the fixture with discs is compared on the cost without them (S_free).  These fixtures
    spread their weights over several samples, so the default precision ("auto") ends in the fp64 rollout;
    "f32" holds the fp32 one to the same bounds."""
    from mppi_robotarm_amd.chain import ChainMPPIController, ChainParams
    from mppi_robotarm_amd.params import ArmParams
    g = load_asym_step(name)
    lim = dict(u_min=g["u_min"], u_max=g["u_max"]) if "u_min" in g else {}
    c = ChainMPPIController(float(g["delta_t"]), paths["xydq_circle"], int(g["T"]), int(g["K"]),
                            float(g["param_exploration"]), float(g["param_lambda"]), float(g["param_alpha"]),
                            g["sigma"], g["stage_cost_weight"], g["terminal_cost_weight"],
                            visualze_sampled_trajs="sampled_traj" in g,
                            chain=ChainParams.from_arm2(arm_of(g, ArmParams)), u_init=g["u_prev"],
                            precision=precision, **lim)
    c.prev_waypoints_idx = int(g["prev_idx"])
    eps = g["eps"].astype(np.float64)
    c._calc_epsilon = lambda *a, **k: eps
    c.keep_costs = True
    u0, u_seq, opt, samp = c.calc_control_input(g["x0"])
    S, want = c.last_S, g["S_free"] if "obstacles" in g else g["S"]
    rel = float(np.max(np.abs(S - want) / np.abs(want)))
    print(f"{name}: chain n=2 {precision} ({c.last_precision}) S rel {rel:.2e}")
    record("asym_chain_n2", fixture=name, precision=precision, ran=c.last_precision, S_max_rel_err=rel)
    assert rel < S_TOL
    assert c.prev_waypoints_idx == int(g["prev_idx_after"])
    if "obstacles" not in g:
        assert int(np.argmin(S)) == int(np.argmin(g["S"]))
        assert _urel(u_seq, g["u_seq"]) < U_TOL
        np.testing.assert_allclose(opt, g["optimal_traj"], rtol=1e-4, atol=1e-4)
        if "sampled_traj" in g:
            np.testing.assert_allclose(samp[g["sampled_idx"]], g["sampled_traj"], rtol=1e-4, atol=1e-4)
    c.close()


def test_closed_loop_ticks(paths):
    """Each tick of run.py's loop at set a, from the reference's own state / u_prev / index: u and the index as
    test_gpu_parity.test_closed_loop_ticks checks them, and S.  The loop runs along the path, so a few of each
    tick's 1280 (sample, step) pairs lie within fp32 resolution of the bisector of two waypoints (fp64 gaps from
    8e-9 m): S takes the device's own picks, as in test_gpu_obstacles.test_obstructed_closed_loop_ticks."""
    from mppi_robotarm_amd.controller import MPPIControllerForPathTracking
    from mppi_robotarm_amd.params import ArmParams
    g = load_asym_loop("k64_t20")
    T, K = int(g["T"]), int(g["K"])
    c = MPPIControllerForPathTracking(ref_path=paths["xydq_circle"], horizon_step_T=T, number_of_samples_K=K,
                                      verbose=False, arm=arm_of(g, ArmParams), **asym_cfg(g))
    c.keep_costs = True
    cfg, worst_S = asym_cfg(g), 0.0
    u_prev, prev, worst = g["u_init"].copy(), int(g["prev_idx0"]), 0.0
    for i in range(int(g["ticks"])):
        c.u_prev = u_prev.copy()
        c.prev_waypoints_idx = prev
        eps = g["eps"][i].astype(np.float64)
        c._calc_epsilon = lambda *a, e=eps, **k: e
        u, u_seq, _, _ = c.calc_control_input(g["states"][i])
        u_seq, S = np.array(u_seq), c.last_S.copy()
        worst = max(worst, _urel(u_seq, g["u_seq"][i]))
        window = paths["xydq_circle"][c.prev_waypoints_idx:c.prev_waypoints_idx + 30]
        c._engine.set_step_inputs(g["states"][i], window, u_prev)       # (the launch above moved the nominal on)
        slots, _ = c._engine.nearest_slots(c._noise_dev)
        r = asym_rollout(g, cfg, g["states"][i], c.prev_waypoints_idx, u_prev, eps, paths)
        delta, gap, differ = waypoint_pick_delta(r, slots, window, cfg["stage_cost_weight"], cfg["terminal_cost_weight"])
        ref = g["S"][i] + delta
        rel = float(np.max(np.abs(S - ref) / np.abs(ref)))
        print(f"tick {i}: S rel {rel:.2e} with the device's picks ({int(differ.sum())} differ, largest gap "
              f"{float(gap.max()):.1e} m), {float(np.max(np.abs(S - g['S'][i]) / np.abs(g['S'][i]))):.2e} with the fp64 picks")
        worst_S = max(worst_S, rel)
        assert float(gap.max()) <= EDGE and float(np.mean(differ)) <= EDGE_CAP, i
        assert rel < S_TOL, i
        assert _urel(u_seq, g["u_seq"][i]) < U_TOL, i
        assert c.prev_waypoints_idx == int(g["prev_idx"][i])
        u_prev, prev = g["u_seq"][i].copy(), int(g["prev_idx"][i])
    record("asym_loop", u_rel_err=worst, S_max_rel_err=worst_S)
    c.close()


def test_two_shards_merge_to_the_unsharded_launch(paths):
    """Set b (dense weights, an exploration split that falls inside the second shard)."""
    K, T, Ka = 1000, 9, 600
    g, cfg, x0, prev, u = asym_problem("b_dense_k256_t24", T)
    win = paths["xydq_circle"][prev:prev + 30]
    one = asym_engine(g, K, T)
    one.set_step_inputs(x0, win, u)
    noise = one.philox_noise(42, 3)
    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
    one.rollout(noise, S_out=S_dev)
    want, S = one.weighted_noise(), S_dev.cpu().numpy()
    one.close()
    wt = np.exp(-(S - S.min()) / cfg["param_lambda"])
    assert wt.sum() ** 2 / (wt ** 2).sum() > 10                  # the weights really are spread over the shards
    engines, parts = [], []
    for off, Kl in ((0, Ka), (Ka, K - Ka)):
        e = asym_engine(g, Kl, T, K_total=K, k_offset=off)
        e.set_step_inputs(x0, win, u)
        nz = e.philox_noise(42, 3)
        assert torch.equal(nz, noise[:, off:off + Kl])
        part = e.new_partial()
        Sl = torch.empty(Kl, dtype=torch.float64, device="cuda")
        e.rollout(nz, S_out=Sl, partial_out=part)
        e.synchronize()
        assert np.array_equal(Sl.cpu().numpy(), S[off:off + Kl])     # a shard is an exact slice
        engines.append(e)
        parts.append(part)
    engines[1].merge(torch.cat(parts).contiguous(), 2)
    got = engines[1].weighted_noise()
    for e in engines:
        e.close()
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)
    assert np.any(want != 0.0)


# ---------------------------------------------------------------- 4: discs where the two links differ

_obst = {}


def _obstacle_case(K, T, paths):
    """Set a's case of this shape, its Philox noise read back, and helpers.asym_obstacle_problem's discs from the
    yardstick's own rollout on it: computed once per shape and shared."""
    if (K, T) not in _obst:
        g, cfg, x0, prev, u = asym_problem("a_k128_t20", T)
        eng = asym_engine(g, K, T)
        eps = eng.philox_noise(42, 3).cpu().numpy().transpose(1, 0, 2).astype(np.float64)
        eng.close()
        p = asym_obstacle_problem(g, cfg, x0, prev, u, eps, paths)
        _obst[(K, T)] = dict(g=g, cfg=cfg, x0=x0, prev=prev, u=u, eps=eps, **p)
    return _obst[(K, T)]


def _staged(p, K, T, paths, lps=0):
    eng = asym_engine(p["g"], K, T, lps=lps)
    eng.set_step_inputs(p["x0"], paths["xydq_circle"][p["prev"]:p["prev"] + 30], p["u"])
    return eng, eng.philox_noise(42, 3)


@pytest.mark.parametrize("K,T", [(1000, 9), (300, 20)])
def test_flag_parity_with_unequal_links(K, T, paths):
    """The device's masks against the fp64 predicate on the device's OWN directions with fk_l1 = 1.1, fk_l2 = 0.9:
    a kernel that took either length for the other would miss the disc beside link 1's end and the one at the
    elbow, and run link 2 through the disc past its tip."""
    p = _obstacle_case(K, T, paths)
    discs, fk1, fk2 = p["discs"], float(p["g"]["fk_l1"]), float(p["g"]["fk_l2"])
    eng, noise = _staged(p, K, T, paths)
    eng.set_obstacles(discs, 1.0e10)
    mask, d = eng.obstacle_hits(noise)
    eng.close()
    q = p["free"]["q"]
    want_d = np.stack([np.cos(q[..., 0]), np.sin(q[..., 0]), np.cos(q.sum(-1)), np.sin(q.sum(-1))], -1)
    assert float(np.max(np.abs(d - want_d))) < 1e-4
    dist, _ = O.segment_test(d[..., 0], d[..., 1], d[..., 2], d[..., 3], discs, fk1, fk2)
    want = O.touch_mask(dist, discs)
    n = discs.shape[0]
    per_bit_clear = np.abs(dist - discs[:, 2][:, None])
    bits = (np.uint32(1) << np.arange(2 * n, dtype=np.uint32)).reshape(n, 2)
    differ = ((mask[..., None, None] ^ want[..., None, None]) & bits) != 0
    assert not np.any(differ & (per_bit_clear > EDGE)), \
        f"a bit differs at clearance {float(per_bit_clear[differ].max()):.2e} m"
    edge_pairs = float(np.mean(np.any(differ, axis=(-1, -2))))
    share = float(np.mean((mask != 0).any(1)))
    swapped = O.touch_mask(O.segment_test(d[..., 0], d[..., 1], d[..., 2], d[..., 3], discs, fk2, fk1)[0], discs)
    moved = float(np.mean((swapped != want).any(1)))
    print(f"K {K} T {T}: {share:.1%} of the samples collide, {int(differ.sum())} bits differ ({edge_pairs:.3%} of the "
          f"pairs, all within {EDGE} m); with the lengths exchanged the masks differ on {moved:.1%} of the samples")
    record("asym_obstacle_flags", K=K, T=T, share=share, edge_pairs=edge_pairs, swapped_differ=moved)
    assert edge_pairs <= EDGE_CAP
    assert 0.10 <= share <= 0.90 and moved >= 0.10
    assert np.any(mask & 1) and np.any(mask & (3 << 4)) and not np.any(mask & ((3 << 2) | (3 << 6)))


@pytest.mark.parametrize("lps", [1, 4])
@pytest.mark.parametrize("K,T", [(1000, 9), (300, 20)])
def test_S_is_the_free_S_plus_w_hits_bit_for_bit(K, T, lps, paths):
    p = _obstacle_case(K, T, paths)
    eng, noise = _staged(p, K, T, paths, lps=lps)
    assert eng.lanes_per_sample == lps
    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S_dev)
    S_free = S_dev.cpu().numpy()
    assert float(np.max(np.abs(S_free - p["free"]["S"]) / np.abs(p["free"]["S"]))) < S_TOL
    for n, w in ((4, 1.0e10), (3, 3.0e6), (1, 7.0)):       # integer-valued: w * hits is exact
        eng.set_obstacles(p["discs"][:n], w)
        eng.rollout(noise, S_out=S_dev)
        mask, _ = eng.obstacle_hits(noise)
        anyb = mask != 0
        hits = anyb.sum(1) + anyb[:, -1]
        assert hits.max() <= T + 1 and 0.10 <= float(np.mean(hits > 0)) <= 0.90
        assert np.array_equal(S_dev.cpu().numpy(), S_free + w * hits.astype(np.float64)), (n, w)
    eng.close()


# ---------------------------------------------------------------- 5: the state space at the default parameters

def _poses():
    two_pi = 2.0 * np.pi
    out = []
    for i, q1 in enumerate((0.6, 2.2, -2.2, -0.6)):                  # one per quadrant of q1
        for q2 in (-1.2, 1.2):                                      # elbow-down, elbow-up
            out.append((f"quadrant{i + 1}-{'down' if q2 < 0 else 'up'}", [q1, q2, 0.3, -0.2]))
    for tag, q2 in (("stretched+", 0.015), ("stretched-", -0.015), ("folded+", np.pi - 0.015), ("folded-", -np.pi + 0.015)):
        out.append((tag, [1.0, q2, -0.2, 0.3]))
    for tag, dq in (("fast+-", (6.0, -6.0)), ("fast-+", (-6.0, 6.0)), ("fast++", (5.0, 3.0))):
        out.append((tag, [X0[0], X0[1], *dq]))
    for k in (1, -1, 3, -3):
        out.append((f"turn-q1{k:+d}", [X0[0] + k * two_pi, X0[1], 0.0, 0.0]))
        out.append((f"turn-q2{k:+d}", [X0[0], X0[1] + k * two_pi, 0.0, 0.0]))
        out.append((f"turn-both{k:+d}", [X0[0] + k * two_pi, X0[1] - k * two_pi, 0.0, 0.0]))
    return out


@pytest.mark.parametrize("tag,x0", _poses(), ids=[t for t, _ in _poses()])
def test_state_space_against_c_oracle(tag, x0, paths):
    """ArmParams() and run.py's constants away from run.py's start pose: the window is the path slice nearest the
    pose's end effector.  Both sides take the fp32-rounded start state (the device's input format), so a pose
    several turns away is the same pose for both."""
    K, T, lam = 300, 20, 100.0
    x0 = np.asarray(x0, dtype=np.float64).astype(np.float32).astype(np.float64)
    path = paths["xydq_circle"]
    ex = math.cos(x0[0]) + math.cos(x0[0] + x0[1])
    ey = math.sin(x0[0]) + math.sin(x0[0] + x0[1])
    near = int(np.argmin((path[:, 0] - ex) ** 2 + (path[:, 1] - ey) ** 2))
    prev = max(0, min(near - 5, path.shape[0] - 30))
    win = path[prev:prev + 30]
    u = np.array([[10.0, -2.0]] * T) + np.random.default_rng(1).normal(0, 0.5, (T, 2))
    eng = _engine(K, T, param_lambda=lam)
    eng.set_step_inputs(x0, win, u)
    noise = eng.philox_noise(42, 3)
    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S_dev)
    w_eps, S, eps_tk = eng.weighted_noise(), S_dev.cpu().numpy(), noise.cpu().numpy()
    eng.close()
    ref_S = coracle.rollout_costs(x0, u, eps_tk, win, 0.006, lam, 0.98, RUNPY["sigma"], RUNPY["stage_cost_weight"],
                                  RUNPY["terminal_cost_weight"], O.ArmParams(), layout="TK")
    _, ref_weps = coracle.weighted_noise(ref_S, eps_tk, lam, layout="TK")
    rel = np.abs(S - ref_S) / np.abs(ref_S)
    print(f"{tag}: window {prev}, S rel max {rel.max():.2e} p50 {np.median(rel):.2e}, w_eps {_urel(w_eps, ref_weps):.2e}")
    record("state_space", pose=tag, S_max_rel_err=float(rel.max()), w_eps_rel_err=_urel(w_eps, ref_weps))
    assert np.all(np.isfinite(S))
    assert float(rel.max()) < S_TOL
    assert _near_tie_argmin(S, ref_S)
    assert _urel(w_eps, ref_weps) < U_TOL
