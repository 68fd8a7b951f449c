"""GPU: torque limits of the n-link chain (mppi_chain_config.clamp_mode; the CLAMP instantiations of
chain_rollout_kernel, chain_traj_kernel and chain_merge_kernel, chain_update_block's nominal clamp).

Shapes: K = 1000 at one lane per sample (ragged last workgroup) and K = 300 with a quad per sample (1200 lanes:
more than one workgroup, ragged tail); T = 9 (no multiple of the 4-step unroll or of either ring depth, >= 5 for
the device median); n in {2, 3, 7} (n = 3 and 7 have a pad link in the quad form).

  1. exact: a clamped launch on (u, eps) gives the S bits of an unclamped launch on (u, eps'), eps' built on the
     host so that the unclamped kernel forms exactly the clipped control; the weights still take the unclamped eps;
  2. limits of +-1e30 against no limits: bit-equal;
  3. the reference's own clamp_step_* fixtures through ChainMPPIController at n = 2;
  4. n = 7 against oracle/chain_oracle.py with limits at the existing n = 7 bounds;
  5. mode 2 through the fused update and the merge;
  6. the trajectory re-rolls and the host trajectory;
  7. the drop-in.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chain_oracle as CO  # noqa: E402
import mppi_oracle as O  # noqa: E402
from helpers import CLAMP_STEPS, _chains, _gpu, _inside, _sigma, _urel, load_clamp_step  # noqa: E402, F401

U_TOL = 1e-4
S_TOL = 5e-5
W, TW = [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0]
DT, ALPHA, T = 0.006, 0.98, 9
# (precision, lanes per sample, K): every horizon form of chain_rollout_kernel
FORMS = [("f32", 1, 1000), ("f32", 4, 300), ("f64", 1, 1000)]
FORM_IDS = ["f32-lps1", "f32-lps4", "f64"]


def _x0(n, rng):
    q = np.array([1.4] + [-2.2 / (n - 1)] * (n - 1))
    return np.concatenate([q, rng.normal(0, 0.2, n)])


def _engine(n, K, lam, precision="f32", lps=0, expl=0.0, **kw):
    from mppi_robotarm_amd.chain import ChainEngine
    P, _ = _chains(n)
    eng = ChainEngine(K, T, DT, lam, ALPHA, _sigma(n), W, TW, expl, P, device=0, precision=precision,
                      lanes_per_sample=lps, **kw)
    assert eng.lanes_per_sample == (lps or eng.lanes_per_sample)
    return eng


def _rollout(eng, x0, win, u, eps, fused=False):
    """One launch on host noise eps (K, T, n): S (K,) and w_eps (T, n)."""
    eng.set_step_inputs(x0, win, u)
    noise = eng.upload_noise(eps)
    S = torch.empty(eng.K_local, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S, fused_update=fused)
    return S.cpu().numpy(), eng.weighted_noise(), noise


# ---------------------------------------------------------------- 1: exact

def grid_case(n, K, expl, seed=0):
    """Inputs on a grid of 1 / 4 with |values| < 64: a start state, a nominal around one noise standard deviation
    per joint, limits at (0.5, 1.5) standard deviations (every limit positive) and fp32 noise N(0, Sigma)."""
    rng = np.random.default_rng(1000 * n + K + seed)
    sd = np.sqrt(np.diag(_sigma(n)))
    grid = lambda a: np.round(np.asarray(a) * 4.0) / 4.0   # noqa: E731
    u = grid(sd * (1.0 + 0.5 * rng.normal(size=(T, n))))
    lo, hi = np.maximum(grid(0.5 * sd), 0.25), grid(1.5 * sd) + 0.25
    eps = (rng.normal(size=(K, T, n)) * sd).astype(np.float32)
    exploit = ((np.arange(K)) < (1.0 - expl) * K)[:, None, None]
    assert np.all(np.abs(u) < 64) and np.all(lo > 0) and np.all(lo < hi) and np.all(hi < 64)
    return _x0(n, rng), u, lo, hi, eps, exploit


def eps_prime(u, eps, lo, hi, exploit, f64):
    """eps' with fl(u + eps') == clip(fl(u + eps)) in the rollout's own arithmetic (fp32 fma with a factor of
    one, or the fp64 add): lim - u where the control is clipped (exact on the grid), eps elsewhere.  Returns
    (eps', clipped (K, T, n))."""
    ft = np.float64 if f64 else np.float32
    e, un = eps.astype(ft), u.astype(ft)[None]
    assert np.array_equal(un.astype(np.float64), u[None])
    lo_, hi_ = lo.astype(ft), hi.astype(ft)
    form = lambda x: np.where(exploit, un + x, x)   # noqa: E731
    v = form(e)
    assert v.dtype == ft
    vc = np.clip(v, lo_, hi_)
    clipped = vc != v
    ep = np.where(clipped, np.where(exploit, vc - un, vc), e)
    ep32 = ep.astype(np.float32)
    assert np.array_equal(ep32.astype(ft), ep)                      # exact in fp32
    assert np.array_equal(form(ep32.astype(ft)), vc)                # fl(u + eps') == clip(fl(u + eps)), elementwise
    return ep32, clipped


@pytest.mark.parametrize("expl", [0.0, 0.25])
@pytest.mark.parametrize("n", [2, 3, 7])
@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_clamped_launch_equals_unclamped_launch_on_the_clipped_controls(precision, lps, K, n, expl, paths):
    """No tolerance: the CLAMP instantiation does the unclamped one's operations on the clipped control (the pad
    link of an odd chain included: every limit is positive, and a lifted pad link would move S), and its weights
    and weighted sums take the unclamped eps from memory."""
    lam = 1.0e4
    x0, u, lo, hi, eps, exploit = grid_case(n, K, expl)
    ep, clipped = eps_prime(u, eps, lo, hi, exploit, precision == "f64")
    share = clipped.mean(axis=(0, 1))
    print(f"n={n} {precision} lps={lps} expl={expl}: clipped share per joint {np.round(share, 2)}")
    assert np.all(share > 0.2) and np.all(share < 0.8)
    win = paths["xydq_circle"][40:70]
    plain = _engine(n, K, lam, precision, lps, expl)
    S_plain, _, _ = _rollout(plain, x0, win, u, ep)
    plain.close()
    cl = _engine(n, K, lam, precision, lps, expl, u_min=lo, u_max=hi)
    assert cl.lanes_per_sample == lps
    S_cl, w_cl, _ = _rollout(cl, x0, win, u, eps)
    cl.close()
    assert np.all(np.isfinite(S_cl))
    assert np.array_equal(S_cl, S_plain)
    # the weighted noise from the device's own S and the UNCLAMPED eps, in fp64 on the host
    wk = np.exp(-(S_cl - S_cl.min()) / lam)
    w_ref = np.einsum("k,ktd->td", wk / wk.sum(), eps.astype(np.float64))
    w_wrong = np.einsum("k,ktd->td", wk / wk.sum(), ep.astype(np.float64))
    assert _urel(w_wrong, w_ref) > 1e-3                              # eps' would show
    assert _urel(w_cl, w_ref) < 1e-10


# ---------------------------------------------------------------- 2: wide limits are the identity

def _case7(n, K, seed=5):
    """A gravity-holding nominal plus noise, limits around it per joint from Sigma's diagonal, host noise."""
    from mppi_robotarm_amd.chain import gravity_torque
    rng = np.random.default_rng(100 * n + seed)
    P, Po = _chains(n)
    x0 = _x0(n, rng)
    sd = np.sqrt(np.diag(_sigma(n)))
    ug = gravity_torque(x0[:n], P)
    u = np.tile(ug, (T, 1)) + rng.normal(0, 0.3, (T, n))
    lo, hi = ug - 0.5 * sd, ug + 0.8 * sd
    eps = (rng.normal(size=(K, T, n)) * sd).astype(np.float32)
    return Po, x0, u, lo, hi, eps


@pytest.mark.parametrize("handoff", ["poll", "counter"])
@pytest.mark.parametrize("n", [2, 3, 7])
@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_wide_limits_are_the_identity_bit_for_bit(precision, lps, K, n, handoff, paths, monkeypatch):
    if handoff == "counter":
        monkeypatch.setenv("MPPI_HANDOFF", "counter")
    _, x0, u, _, _, eps = _case7(n, K)
    win = paths["xydq_circle"][40:70]
    out = []
    for lim in (None, 1e30):
        kw = {} if lim is None else dict(u_min=-lim, u_max=lim)
        eng = _engine(n, K, 1.0e4, precision, lps, **kw)
        assert eng.handoff == handoff
        S, w, noise = _rollout(eng, x0, win, u, eps, fused=True)
        nom = eng.nominal()
        tr = eng.trajectories(base_u=u, noise=noise, K=64).cpu().numpy()
        tr0 = eng.trajectories(base_u=u, K=1).cpu().numpy()
        out.append((S, w, nom, tr, tr0))
        eng.close()
    for a, b in zip(*out):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)


# ---------------------------------------------------------------- 3: the reference's fixtures at n = 2

@pytest.mark.parametrize("name", CLAMP_STEPS)
def test_chain_at_n2_reproduces_the_clamped_reference_steps(name, paths):
    """The suite's tolerances (same argmin, S 5e-5, u 1e-4 of max(|u|, 1), trajectories 1e-4).  Measured on
    MI355X: S within 4.1e-7 to 7.7e-7 of the reference's and u_seq equal (one-hot weights) on four fixtures;
    c_dense (spread weights: precision="auto" reruns it in fp64) S 4.7e-16, u 1.8e-16."""
    from mppi_robotarm_amd.chain import ChainMPPIController, ChainParams
    g = load_clamp_step(name)
    c = ChainMPPIController(float(g["delta_t"]), paths[str(g["path"])], int(g["T"]), int(g["K"]),
                            float(g["param_exploration"]), float(g["param_lambda"]), float(g["param_alpha"]),
                            g["sigma"], g["stage_cost_weight"], g["terminal_cost_weight"],
                            visualize_optimal_traj=bool(g["visualize_optimal_traj"]),
                            visualze_sampled_trajs=bool(g["sampled"]), chain=ChainParams.from_arm2(),
                            u_init=g["u_prev"], u_min=g["u_min"], u_max=g["u_max"])
    c.prev_waypoints_idx = int(g["prev_idx"])
    eps = g["eps"].astype(np.float64)
    c._calc_epsilon = lambda *a, **k: eps
    c.keep_costs = True
    u0, u_seq, opt, samp = c.calc_control_input(g["x0"])
    S = c.last_S
    print(f"{name}: S rel {float(np.max(np.abs(S - g['S']) / np.abs(g['S']))):.2e} u rel {_urel(u_seq, g['u_seq']):.2e}")
    assert int(np.argmin(S)) == int(np.argmin(g["S"]))
    assert float(np.max(np.abs(S - g["S"]) / np.abs(g["S"]))) < S_TOL
    assert _urel(u_seq, g["u_seq"]) < U_TOL
    assert c.prev_waypoints_idx == int(g["prev_idx_after"])
    assert _inside(u_seq, g["u_min"], g["u_max"]) == bool(g["visualize_optimal_traj"])   # outside for b_novis
    np.testing.assert_allclose(opt, g["optimal_traj"], rtol=1e-4, atol=1e-4)
    if "sampled_traj" in g:
        np.testing.assert_allclose(samp, g["sampled_traj"], rtol=1e-4, atol=1e-4)
    c.close()


# ---------------------------------------------------------------- 4: n = 7 against the chain oracle with limits

_REF7 = {}


def _ref7(paths, lam):
    """The n = 7 case (K = 1000) and its fp64 yardstick, computed once per lambda and left unchanged."""
    if lam not in _REF7:
        Po, x0, u, lo, hi, eps = _case7(7, 1000)
        win = paths["xydq_circle"][40:70]
        Sr = CO.chain_rollout_costs(x0, u, eps, win, 0, DT, lam, ALPHA, _sigma(7), W, TW, lo=lo, hi=hi, P=Po)
        wk = np.exp(-(Sr - Sr.min()) / lam)
        wr = np.einsum("k,ktd->td", wk / wk.sum(), eps.astype(np.float64))
        clipped = O.sampled_controls(u, eps, lo, hi) != (u[None] + eps.astype(np.float64))
        assert 0.2 < clipped.mean() < 0.8
        for a in (x0, u, lo, hi, eps, Sr, wr):
            a.setflags(write=False)
        _REF7[lam] = (Po, x0, u, lo, hi, eps, win, Sr, wr)
    return _REF7[lam]


@pytest.mark.parametrize("precision,lps", [("f32", 1), ("f32", 4), ("f64", 1)], ids=FORM_IDS)
def test_chain_n7_clamped_against_chain_clamp_ref(precision, lps, paths):
    """n = 7, K = 1000, T = 9, window xydq_circle[40:70], lambda = 1e8 (test_gpu_chain.py's case of this shape):
    the fp64 rollout at the fp64 chain bounds (S 1e-11, w_eps 1e-10), the fp32 ones at the n = 7 bounds (p99
    2e-4, at most 0.2 % of the samples beyond 1e-3, w_eps 1e-4).  The yardstick fed fp32-rounded inputs instead
    of these leaves no sample of this seed within 1e-5 m of a waypoint tie at any step (checked with NumPy)."""
    lam = 1.0e8
    Po, x0, u, lo, hi, eps, win, Sr, wr = _ref7(paths, lam)
    eng = _engine(7, 1000, lam, precision, lps, u_min=lo, u_max=hi)
    S, w, _ = _rollout(eng, x0, win, u, eps)
    eng.close()
    rel = np.abs(S - Sr) / np.abs(Sr)
    print(f"n=7 clamped {precision} lps={lps}: S rel p99 {np.percentile(rel, 99):.2e} max {rel.max():.2e} "
          f"beyond 1e-3 {np.mean(rel > 1e-3):.2e} w_eps {_urel(w, wr):.2e}")
    assert np.all(np.isfinite(S)) and int(np.argmin(S)) == int(np.argmin(Sr))
    if precision == "f64":
        assert float(rel.max()) < 1e-11 and _urel(w, wr) < 1e-10
    else:
        assert float(np.percentile(rel, 99)) < 2e-4
        assert float(np.mean(rel > 1e-3)) <= 2e-3
        assert _urel(w, wr) < U_TOL


# ---------------------------------------------------------------- 5: mode 2, the fused update and the merge

@pytest.mark.parametrize("precision,lps,K", [("f32", 1, 1000), ("f32", 4, 1000), ("f64", 1, 1000)], ids=FORM_IDS)
def test_mode_2_clips_the_fused_nominal_and_feeds_the_next_launch(precision, lps, K, paths):
    lam = 100.0   # one-hot weights: the update moves the nominal by a whole noise sample, well past the limits
    Po, x0, u, lo, hi, eps = _case7(7, K)
    eps2 = np.ascontiguousarray(eps[::-1])
    win = paths["xydq_circle"][40:70]
    m1 = _engine(7, K, lam, precision, lps, u_min=lo, u_max=hi, clamp_nominal=False)
    _rollout(m1, x0, win, u, eps, fused=True)
    nom1 = m1.nominal()
    m1.close()
    m2 = _engine(7, K, lam, precision, lps, u_min=lo, u_max=hi)
    _rollout(m2, x0, win, u, eps, fused=True)
    nom2 = m2.nominal()
    n_clipped = int(np.count_nonzero(np.clip(nom1, lo, hi) != nom1))
    print(f"{precision} lps={lps}: {n_clipped} of {nom1.size} nominal entries clipped")
    assert n_clipped >= 5 and not _inside(nom1, lo, hi)
    assert np.array_equal(nom2, np.clip(nom1, lo, hi)) and _inside(nom2, lo, hi)
    # a second fused launch straight from the device-written clipped nominal: a_t and the fp32 rows were
    # rebuilt from the clipped values
    noise2 = m2.upload_noise(eps2)
    S2 = torch.empty(K, dtype=torch.float64, device="cuda")
    m2.rollout(noise2, S_out=S2, fused_update=True)
    S2 = S2.cpu().numpy()
    Sr = CO.chain_rollout_costs(x0, nom2, eps2, win, 0, DT, lam, ALPHA, _sigma(7), W, TW, lo=lo, hi=hi, P=Po)
    rel = np.abs(S2 - Sr) / np.abs(Sr)
    S_wrong = CO.chain_rollout_costs(x0, nom1, eps2, win, 0, DT, lam, ALPHA, _sigma(7), W, TW, lo=lo, hi=hi, P=Po)
    assert float(np.median(np.abs(S_wrong - Sr) / np.abs(Sr))) > 1e-3   # the unclipped nominal would show
    assert float(rel.max()) < 1e-11 if precision == "f64" else float(np.percentile(rel, 99)) < 2e-4
    assert _inside(m2.nominal(), lo, hi)
    # two shards (500 + 500) merged on the device, with the fused update, against the unsharded launch
    from mppi_robotarm_amd.chain import ChainEngine
    P, _ = _chains(7)
    parts = torch.empty(2 * m2.partial_len, dtype=torch.float64, device="cuda")
    shards = []
    for s in range(2):
        e = ChainEngine(K // 2, T, DT, lam, ALPHA, _sigma(7), W, TW, 0.0, P, K_total=K, k_offset=s * (K // 2), device=0,
                        precision=precision, lanes_per_sample=lps, u_min=lo, u_max=hi)
        e.set_step_inputs(x0, win, u)
        e.rollout(e.upload_noise(eps[s * (K // 2):(s + 1) * (K // 2)]),
                  partial_out=parts[s * e.partial_len:(s + 1) * e.partial_len])
        shards.append(e)
    shards[0].merge(parts, 2, fused_update=True)
    nom_m = shards[0].nominal()
    np.testing.assert_allclose(nom_m, nom2, rtol=1e-10, atol=1e-10)
    assert _inside(nom_m, lo, hi)
    for e in shards + [m2]:
        e.close()


# ---------------------------------------------------------------- 6: trajectories

def test_clamped_trajectories_match_chain_clamp_ref(paths):
    K = 64
    Po, x0, u, lo, hi, eps = _case7(7, K)
    un = u + np.random.default_rng(3).normal(0, 2.0, u.shape)       # an update with entries outside the limits
    assert not _inside(un, lo, hi)
    eng = _engine(7, K, 100.0, "f32", 1, expl=0.25, u_min=lo, u_max=hi)
    eng.set_step_inputs(x0, paths["xydq_circle"][40:70], u)
    noise = eng.upload_noise(eps)
    tr = eng.trajectories(base_u=u, noise=noise).double().cpu().numpy()
    v = O.sampled_controls(u, eps, lo, hi, expl=0.25)
    np.testing.assert_allclose(tr, CO.chain_rollout_trajectory(x0, np.roll(v, 1, axis=1), DT, Po), rtol=1e-4, atol=1e-4)
    tr0 = eng.trajectories(base_u=un, K=1).double().cpu().numpy()
    ref0 = CO.chain_rollout_trajectory(x0, np.roll(np.clip(un, lo, hi), 1, axis=0), DT, Po)
    np.testing.assert_allclose(tr0[0], ref0, rtol=1e-4, atol=1e-4)
    assert float(np.max(np.abs(CO.chain_rollout_trajectory(x0, np.roll(un, 1, axis=0), DT, Po) - ref0))) > 1e-2
    np.testing.assert_allclose(eng.optimal_traj_host(x0, un), ref0, rtol=1e-4, atol=1e-4)
    eng.close()


# ---------------------------------------------------------------- 7: the drop-in

def _dropin(paths, lo, hi, ug, **kw):
    from mppi_robotarm_amd.chain import CHAIN7_SIGMA, ChainMPPIController
    kw.setdefault("precision", "f32")
    kw.setdefault("param_lambda", 100.0)
    return ChainMPPIController(DT, paths["xydq_circle"], T, 512, 0.0, kw.pop("param_lambda"), ALPHA, CHAIN7_SIGMA,
                               np.array(W), np.array(TW), u_init=ug, noise="device", seed=7, device=0,
                               u_min=lo, u_max=hi, **kw)


def _limits7():
    from mppi_robotarm_amd.chain import CHAIN7_SIGMA, CHAIN7_X0, gravity_torque
    ug = gravity_torque(CHAIN7_X0[:7])
    sd = np.sqrt(np.diag(CHAIN7_SIGMA))
    return CHAIN7_X0.copy(), ug, ug - 0.5 * sd, ug + 0.5 * sd


def test_dropin_closed_loop_stays_inside_the_limits_and_follows_rebinding(paths):
    x, ug, lo, hi = _limits7()
    a = _dropin(paths, lo, hi, ug)
    b = _dropin(paths, lo, hi, ug, visualze_sampled_trajs=True)     # the host-update path
    Po = CO.ChainParams()
    top, prev_seq = hi, None
    for tick in range(5):
        if tick == 3:
            # rebinding: the next call runs with the new limit, which the nominal so far exceeds
            top = np.maximum(lo + 0.05 * (hi - lo), prev_seq.max(axis=0) - 0.1 * (hi - lo))
            assert np.all(top <= hi) and not _inside(prev_seq, lo, top)
            a.u_max = top
            b.u_max = top
        u0, u_seq, opt, _ = a.calc_control_input(x)
        u0b, u_seqb, optb, sampb = b.calc_control_input(x)
        assert _inside(u_seq, lo, top), tick
        assert np.array_equal(a._engine.u_max, top)
        np.testing.assert_allclose(u_seq, u_seqb, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(opt, optb, rtol=1e-10, atol=1e-10)
        assert np.any(sampb) and not np.any(np.isnan(sampb))
        prev_seq = u_seq.copy()
        q, dq = CO.chain_forward_dynamics(x[:7], x[7:], np.asarray(u0, dtype=np.float64), DT, Po)
        x = np.concatenate([q, dq])
    a.close()
    b.close()


def test_dropin_auto_precision_carries_the_limits_into_its_fp64_engine(paths):
    x, ug, lo, hi = _limits7()
    c = _dropin(paths, lo, hi, ug, precision="auto", param_lambda=3.0e5)
    _, u_seq, _, _ = c.calc_control_input(x)
    assert c.last_precision == "f64" and c._engine.precision == "f64"
    assert np.array_equal(c._engine.u_min, lo) and np.array_equal(c._engine.u_max, hi)
    assert np.array_equal(c._slots["f32"]["_engine"].u_max, hi)     # and the fp32 engine that ran first
    assert _inside(u_seq, lo, hi)
    c.close()


def test_debug_slots_on_a_clamped_engine_raises(paths):
    _, x0, u, lo, hi, eps = _case7(7, 256)
    eng = _engine(7, 256, 100.0, "f32", 1, u_min=lo, u_max=hi)
    eng.set_step_inputs(x0, paths["xydq_circle"][40:70], u)
    with pytest.raises(ValueError, match="torque limits"):
        eng.debug_slots(eng.upload_noise(eps))
    eng.close()
