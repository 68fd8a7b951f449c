"""GPU: workspace obstacles for the n-link chain (mppi_chain_set_obstacles; the OBST instantiations of
chain_rollout_kernel in its three forms: fp32 with one lane per sample, fp32 with a quad per sample, fp64).

Yardstick: oracle/chain_oracle.py (O.collision_costs on chain_model with chain_collides), pinned to the arm's
oracle and the reference's own fixtures at n = 2 by test_chain_obstacle_cpu.py.

Shapes, the smallest at which each form can go wrong: n in {2, 3, 7} (even; odd, with the quad's pad link; config
5's); T = 7 (one 4-step body plus a 3-step tail of the one-lane loop, >= 5 for the device median); K = 300 at one lane
per sample (two workgroups of 256, the second ragged) and K = 100 with a quad per sample (64 samples per workgroup:
two, the second ragged).  The time step is 0.03 s and the noise the chain tests' Sigma, so over the 7 steps the joint
angles spread by ~0.1 rad; the discs are sized from the fp64 reference's own states (_problem).

The collision flag is a discontinuity: a device state within rounding of a disc's boundary may fall on either side.
Nothing is excluded for that.  The masks are compared with the fp64 predicate on the device's OWN directions, a bit
allowed to differ only within EDGE of a boundary; the penalty is checked exactly through S = S_free + w hits with the
device's own hit counts; and the yardstick takes the device's hit counts where a weight depends on them.

EDGE, from the device forms' rounding count (not from what the kernels give).  seg_hits rounds five times on the way to
the squared distance (two in the projection, one in each offset component, two in the sum of squares), and r^2 is
rounded once; the walk of the pair's centres to link a's base adds one fma per link and component before link a, in
every form at most 2 n roundings (one lane per sample: exactly that; the quad's prefix sum of fk (cos, sin) rounds more
often but at the magnitude of a link pair, <= reach / 2 against |centre| + reach: fewer in these units; the fp64 form
rounds at 2^-53 and is compared on directions returned in fp32, an error of at most 2^-25 per component and link, half
a rounding).  Each counts as 2^-24 at magnitude <= |centre| + reach: EDGE(n) = (6 + 2 n) 2^-24 (max |centre| + reach),
5e-6 m at n = 7: the arm test's 4e-6 m at its 16 roundings.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chain_oracle as CO  # noqa: E402
import mppi_oracle as O  # noqa: E402
from chain_oracle import chain_collides, chain_segment_test, chain_touch_mask  # noqa: E402
from helpers import OBST_STEPS, _chains, _gpu, _inside, _sigma, _urel, load_obst_step  # noqa: E402, F401

U_TOL = 1e-4
S_TOL = 5e-5
W_TOL = 1e-10
EDGE_CAP = 0.05            # at most 5 % of the reference's entries may lie within EDGE of a boundary
W, TW = [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0]
DT, ALPHA, T = 0.03, 0.98, 7
REACH = 2.0
NS = [2, 3, 7]
# (precision, lanes per sample, K): every horizon form of chain_rollout_kernel
FORMS = [("f32", 1, 300), ("f32", 4, 100), ("f64", 1, 300)]
FORM_IDS = ["f32-lps1", "f32-lps4", "f64"]
COSTS = ((8, 1.0e10), (3, 3.0e6), (1, 7.0))   # (discs, cost): integer-valued costs, w * hits is exact


def edge(n, discs):
    return (6 + 2 * n) * 2.0 ** -24 * (float(np.max(np.hypot(discs[:, 0], discs[:, 1]))) + REACH)


# ---------------------------------------------------------------- the shared problem of (n, K)

_prob = {}


def _ref(n, K, paths, discs, w, lam=100.0, lo=None, hi=None):
    p = _prob[(n, K)]
    return CO.chain_rollout_costs(p["x0"], p["u"], p["eps"], paths["xydq_circle"], 40, DT, lam, ALPHA, _sigma(n), W, TW,
                                  0.0, _chains(n)[1], lo=lo, hi=hi, discs=discs, obstacle_cost=w, details=True)


def place_discs(free, Po):
    """Eight discs from the unobstructed fp64 rollout's own states (over 7 steps a link moves centimetres: a disc
    anywhere else is touched by every sample or by none).  A disc of radius r = 3 s is put beside a point of the
    chain along a direction d, s being the spread of the point's final positions along d, its centre r + y off the
    point's median final position: y is the 83rd percentile of the final positions' offsets along d, or the
    largest offset of the first two steps where that is more, so the first steps, when the samples are still
    together, all miss, and of the final states about one in six touches.
      0. ahead of the tip of the last link, 45 degrees off the link towards its swing: reached with the tip
         (projection clipped to the end);
      1. on the outer side of the last joint, off the bisector of the two links' outward directions towards the
         joint's own spread: link n-2 touches it past its end, link n-1 before its base;
      2 .. : beside the midpoint of link a = 0, 1, ... (as many as fit) along its normal, on the side it swings
         to: touched in the interior;
      the rest: shifted, shrunk copies of the first ones.
    Returned in the order of the share of samples that touch each."""
    n = Po.n
    fk = np.asarray(Po.fk)
    th = np.cumsum(free["q"], -1)                                          # (K, T, n)
    z = np.zeros(th.shape[:2] + (1,))
    jt = np.stack([np.concatenate([z, np.cumsum(fk * np.cos(th), -1)], -1),
                   np.concatenate([z, np.cumsum(fk * np.sin(th), -1)], -1)], -1)   # (K, T, n + 1, 2): b_{-1} .. b_{n-1}
    med = np.median(th[:, -1], 0)
    unit = lambda a: np.array([np.cos(a), np.sin(a)])           # noqa: E731
    normal = lambda a: np.array([-np.sin(a), np.cos(a)])        # noqa: E731

    def beside(pt, d, flip):
        """pt (K, T, 2): the point's positions."""
        m = np.median(pt[:, -1], 0)
        if flip and float((m - np.median(pt[:, 0], 0)) @ d) < 0.0:
            d = -d
        y = (pt - m) @ d                                                   # (K, T)
        s = max(float(np.std(y[:, -1])), 1e-5)
        off = max(float(np.quantile(y[:, -1], 0.83)), float(y[:, :2].max()) + 0.1 * s)
        return np.append(m + (3.0 * s + off) * d, 3.0 * s)

    out = unit(med[-2]) - unit(med[-1])                         # past link n-2's end and before link n-1's base
    out = out / np.linalg.norm(out)
    # ... leaning towards the direction in which the joint's final positions spread most, as far as it stays there
    lead = np.linalg.svd(jt[:, -1, n - 1] - np.median(jt[:, -1, n - 1], 0), full_matrices=False)[2][0]
    lead = lead if float(lead @ out) >= 0.0 else -lead
    for lean in (4.0, 2.0, 1.0, 0.5, 0.0):
        d = (out + lean * lead) / np.linalg.norm(out + lean * lead)
        if float(d @ unit(med[-2])) > 0.2 and float(d @ unit(med[-1])) < -0.2:
            out = d
            break
    tip = jt[:, :, n]
    swing = normal(med[-1])
    if float((np.median(tip[:, -1], 0) - np.median(tip[:, 0], 0)) @ swing) < 0.0:
        swing = -swing
    discs = [beside(tip, (unit(med[-1]) + swing) / np.sqrt(2.0), False), beside(jt[:, :, n - 1], out, False)]
    for a in range(n):
        if len(discs) == 8:
            break
        discs.append(beside(0.5 * (jt[:, :, a] + jt[:, :, a + 1]), normal(med[a]), True))
    i = 0
    while len(discs) < 8:
        d = discs[i]
        discs.append(np.array([d[0] + 0.3 * d[2], d[1] - 0.2 * d[2], 0.8 * d[2]]))
        i += 1
    discs = np.array(discs)
    # the most-touched first (by the share of samples that touch a disc at any step), so that the runs with one and
    # three discs see collisions too
    dist, _ = chain_segment_test(np.cos(th), np.sin(th), discs, fk)
    share = (dist < discs[:, 2][:, None]).any(axis=(1, 3)).mean(0)
    return discs[np.argsort(-share, kind="stable")]


def _problem(n, K, paths):
    """Start state, a gravity-holding nominal plus noise, host noise N(0, Sigma) in fp32, the yardstick's unobstructed
    rollout on it and the discs placed from it: computed once per (n, K) and shared, never modified.  The
    precondition of every comparison below is asserted here, on the reference: a test that cannot fail must not pass."""
    if (n, K) not in _prob:
        from mppi_robotarm_amd.chain import gravity_torque
        rng = np.random.default_rng(100 * n + K)
        P, Po = _chains(n)
        q = np.array([1.4] + [-2.2 / (n - 1)] * (n - 1))
        x0 = np.concatenate([q, rng.normal(0, 0.2, n)])
        sd = np.sqrt(np.diag(_sigma(n)))
        u = np.tile(gravity_torque(q, P), (T, 1)) + rng.normal(0, 0.3, (T, n))
        eps = (rng.normal(size=(K, T, n)) * sd).astype(np.float32).astype(np.float64)
        _prob[(n, K)] = dict(x0=x0, u=u, eps=eps)
        free = _ref(n, K, paths, np.zeros((0, 3)), 0.0)
        discs = place_discs(free, Po)
        full = _ref(n, K, paths, discs, 1.0)
        r = discs[:, 2]
        hit = full["dist"] < r[:, None]                                    # (K, T, nd, n)
        touched = hit.any(axis=(1, 2))                                     # (K, n): at any step, by any disc
        for a in range(n):
            assert touched[:, a].any(), f"n {n}: no sample touches link {a}"
            assert not touched[:, a].all(), f"n {n}: every sample touches link {a}"
        for end in (-1, 0, 1):
            assert (hit & (full["clipped"] == end)).any(), f"n {n}: no touch with its projection at {end}"
        near = np.abs(full["dist"] - r[:, None]) <= edge(n, discs)
        assert float(np.mean(near)) <= EDGE_CAP
        share = float(np.mean(full["flag"].any(1)))
        assert 0.10 <= share <= 0.90, share
        spread = float(np.max(np.std(np.cumsum(free["q"][:, -1], -1), 0)))
        assert spread > 0.02, spread                                       # the joint angles spread visibly
        _prob[(n, K)].update(discs=discs, free=free, full=full)
    return _prob[(n, K)]


def _engine(n, K, lam=100.0, precision="f32", lps=0, **kw):
    from mppi_robotarm_amd.chain import ChainEngine
    eng = ChainEngine(K, T, DT, lam, ALPHA, _sigma(n), W, TW, 0.0, _chains(n)[0], device=0, precision=precision,
                      lanes_per_sample=lps, **kw)
    assert eng.lanes_per_sample == (lps or eng.lanes_per_sample)
    return eng


def _stage(eng, p, paths):
    eng.set_step_inputs(p["x0"], paths["xydq_circle"][40:70], p["u"])
    return eng.upload_noise(p["eps"])


def _S(eng, noise, **kw):
    S = torch.empty(eng.K_local, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S, **kw)
    return S.cpu().numpy()


def _hits_from_masks(mask):
    anyb = mask != 0
    return anyb.sum(1) + anyb[:, -1]


def _bits(nd, n):
    return np.uint64(1) << (np.uint64(8) * np.arange(nd, dtype=np.uint64)[:, None] + np.arange(n, dtype=np.uint64))


# ---------------------------------------------------------------- 1: flag parity on the device's own directions

@pytest.mark.parametrize("nd", [1, 3, 8])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_flag_parity_on_the_devices_own_directions(precision, lps, K, n, nd, paths):
    p = _problem(n, K, paths)
    discs = p["discs"][:nd]
    eng = _engine(n, K, precision=precision, lps=lps)
    noise = _stage(eng, p, paths)
    eng.set_obstacles(discs, 1.0e10)
    mask, d = eng.obstacle_hits(noise)
    eng.close()
    assert mask.shape == (K, T) and mask.dtype == np.uint64 and d.shape == (K, T, 2 * n)
    th = np.cumsum(p["free"]["q"], -1)
    assert float(np.max(np.abs(d - np.concatenate([np.cos(th), np.sin(th)], -1)))) < 1e-4
    dist, _ = chain_segment_test(d[..., :n], d[..., n:], discs, _chains(n)[1].fk)
    want = chain_touch_mask(dist, discs)
    clear = np.abs(dist - discs[:, 2][:, None])                                  # (K, T, nd, n)
    differ = ((mask[..., None, None] ^ want[..., None, None]) & _bits(nd, n)) != 0
    E = edge(n, p["discs"])
    worst = float(clear[differ].max()) if differ.any() else 0.0
    print(f"{precision} lps {lps} n {n} discs {nd}: {float(np.mean(mask != 0)):.1%} of the states collide, "
          f"{int(differ.sum())} bits differ (largest clearance {worst:.2e} m, EDGE {E:.2e} m)")
    assert not np.any(differ & (clear > E)), f"a bit differs at clearance {worst:.2e} m"
    assert float(np.mean(differ)) <= EDGE_CAP
    # bits of links a >= n (the quad's pad link, lanes past the chain) and of discs j >= nd are never set
    allowed = np.bitwise_or.reduce(_bits(nd, n).ravel())
    assert not np.any(mask & ~allowed)
    if nd == 8:
        touched = ((mask[..., None, None] & _bits(nd, n)) != 0).any(axis=(1, 2))    # (K, n), as in _problem
        assert np.all(touched.any(0)) and not np.any(touched.all(0))                # every link is exercised


# ---------------------------------------------------------------- 2: the decomposition, bit for bit

@pytest.mark.parametrize("lam", [100.0, 3.0e6])
@pytest.mark.parametrize("handoff", ["poll", "counter"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_S_is_the_no_disc_S_plus_w_hits_bit_for_bit(precision, lps, K, n, handoff, lam, paths, monkeypatch):
    """S of a launch with discs is the S of the same context's launch without them, through the CLAMP kernel on
    +-1e30 limits, plus w * hits with the hits rebuilt from the debug masks: one fp64 rounding, w * hits exact."""
    if handoff == "counter":
        monkeypatch.setenv("MPPI_HANDOFF", "counter")
    else:
        monkeypatch.delenv("MPPI_HANDOFF", raising=False)
    p = _problem(n, K, paths)
    eng = _engine(n, K, lam, precision, lps, u_min=-1e30, u_max=1e30)
    assert eng.handoff == handoff
    noise = _stage(eng, p, paths)
    S_free = _S(eng, noise)
    w_free = eng.weighted_noise()
    assert np.all(np.isfinite(S_free))
    for nd, w in COSTS:
        eng.set_obstacles(p["discs"][:nd], w)
        S = _S(eng, noise)
        mask, _ = eng.obstacle_hits(noise)
        hits = _hits_from_masks(mask)
        assert hits.max() <= T + 1 and hits.any()
        if nd == 8:
            assert 0.10 <= float(np.mean(hits > 0)) <= 0.90
        assert np.array_equal(S, S_free + w * hits.astype(np.float64)), (nd, w)
        wk = np.exp(-(S - S.min()) / lam)
        np.testing.assert_allclose(eng.weighted_noise(), np.einsum("k,ktd->td", wk / wk.sum(), p["eps"]),
                                   rtol=W_TOL, atol=W_TOL)
    eng.set_obstacles(None)
    assert np.array_equal(_S(eng, noise), S_free) and np.array_equal(eng.weighted_noise(), w_free)
    eng.close()


# ---------------------------------------------------------------- 3: no limits is wide limits

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_no_limits_is_wide_limits_bit_for_bit(precision, lps, K, n, paths):
    """The OBST kernels are built with the clamp only: without torque limits they run on -+inf limits, which must
    give the bits of +-1e30 limits in S, w_eps and the fused update's nominal."""
    p = _problem(n, K, paths)
    got = []
    for lim in (None, 1e30):
        eng = _engine(n, K, 3.0e6, precision, lps, **({} if lim is None else dict(u_min=-lim, u_max=lim)))
        noise = _stage(eng, p, paths)
        eng.set_obstacles(p["discs"], 3.0e6)
        S = _S(eng, noise, fused_update=True)
        got.append((S, eng.weighted_noise(), eng.nominal()))
        eng.close()
    for a, b in zip(*got):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    assert np.any(got[0][0] >= 3.0e6)


# ---------------------------------------------------------------- 4: weighted noise and the nominal

def _with_device_hits(n, K, paths, discs, w, lam, hits, lo=None, hi=None):
    """The yardstick's step with the device's hit counts in place of its own: a boundary tie cannot move a weight."""
    p = _prob[(n, K)]
    return CO.step(p["x0"], p["u"], p["eps"], paths["xydq_circle"], 40, DT, lam, ALPHA, _sigma(n), W, TW,
                   0.0, _chains(n)[1], lo=lo, hi=hi, discs=discs, obstacle_cost=w, hits=hits)


@pytest.mark.parametrize("lam,w", [(100.0, 1.0e10), (3.0e6, 3.0e6)])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_weighted_noise_and_nominal(precision, lps, K, n, lam, w, paths):
    p = _problem(n, K, paths)
    eng = _engine(n, K, lam, precision, lps)
    noise = _stage(eng, p, paths)
    seen = []
    for discs in (p["discs"][:4], p["discs"][4:] + np.array([2e-3, -1e-3, 0.0])):   # moved between two launches
        eng.set_step_inputs(p["x0"], paths["xydq_circle"][40:70], p["u"])
        eng.set_obstacles(discs, w)
        S, weps = _S(eng, noise), eng.weighted_noise()
        mask, _ = eng.obstacle_hits(noise)
        hits = _hits_from_masks(mask)
        seen.append(hits)
        r = _with_device_hits(n, K, paths, discs, w, lam, hits)
        assert float(np.mean(hits == r["hits"])) >= 0.99
        host = O.weighted_noise(O.compute_weights(S, lam), p["eps"])
        srel = float(np.max(np.abs(S - r["S"]) / np.abs(r["S"])))
        print(f"{precision} lps {lps} n {n} lam {lam}: S rel {srel:.2e}, w_eps vs host sum "
              f"{float(np.max(np.abs(weps - host))):.2e}, vs yardstick {_urel(weps, r['w_eps_raw']):.2e}")
        assert srel < S_TOL
        np.testing.assert_allclose(weps, host, rtol=W_TOL, atol=W_TOL)
        assert _urel(weps, r["w_eps_raw"]) < U_TOL
        eng.rollout(noise, fused_update=True)                 # the fused update, from the same nominal
        assert _urel(eng.nominal(), r["u_seq"]) < U_TOL
    assert not np.array_equal(seen[0], seen[1])               # the second launch saw the move
    eng.close()


# ---------------------------------------------------------------- 5: n = 2 against the reference's fixtures

@pytest.mark.parametrize("name", OBST_STEPS)
def test_chain_at_n2_reproduces_the_obstructed_reference_steps(name, paths):
    """test_gpu_obstacles.py's rules: S at 5e-5 on the samples whose stored clearance is >= 1e-4 m on every step,
    the same argmin and the nominal at 1e-4 where one sample carries the weight; where several do, the update from
    the device's own hit counts."""
    from mppi_robotarm_amd.chain import ChainMPPIController, ChainParams
    g = load_obst_step(name)
    kw = dict(u_min=g["u_min"], u_max=g["u_max"]) if "u_min" in g else {}
    c = ChainMPPIController(float(g["delta_t"]), paths[str(g["path"])], int(g["T"]), int(g["K"]),
                            float(g["param_exploration"]), float(g["param_lambda"]), float(g["param_alpha"]),
                            g["sigma"], g["stage_cost_weight"], g["terminal_cost_weight"],
                            visualize_optimal_traj=bool(g["visualize_optimal_traj"]), chain=ChainParams.from_arm2(),
                            u_init=g["u_prev"], obstacles=g["obstacles"], obstacle_cost=float(g["obstacle_cost"]), **kw)
    c.prev_waypoints_idx = int(g["prev_idx"])
    eps = g["eps"].astype(np.float64)
    c._calc_epsilon = lambda *a, **k: eps
    c.keep_costs = True
    u0, u_seq, opt, _ = c.calc_control_input(g["x0"])
    S = c.last_S
    assert c._engine.obstacles.shape == g["obstacles"].shape
    clean = g["clearance"].min(1) >= 1e-4
    assert float(np.mean(clean)) >= 0.80
    rel = float(np.max(np.abs(S[clean] - g["S"][clean]) / np.abs(g["S"][clean])))
    print(f"{name}: S rel {rel:.2e} on {int(clean.sum())}/{clean.size} samples, precision {c.last_precision}")
    assert rel < S_TOL
    assert c.prev_waypoints_idx == int(g["prev_idx_after"])
    if bool(g["one_hot"]):
        assert int(np.argmin(S)) == int(np.argmin(g["S"])) != int(np.argmin(g["S_free"]))
        assert _urel(u_seq, g["u_seq"]) < U_TOL and _urel(u0, g["u0"]) < U_TOL
    else:
        w = float(g["obstacle_cost"])
        r = CO.chain_rollout_costs(g["x0"], g["u_prev"], eps, paths[str(g["path"])], int(g["prev_idx_after"]),
                                   float(g["delta_t"]), float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"],
                                   g["stage_cost_weight"], g["terminal_cost_weight"], float(g["param_exploration"]),
                                   CO.ChainParams.from_arm2(), lo=g.get("u_min"), hi=g.get("u_max"),
                                   discs=g["obstacles"], obstacle_cost=w, details=True)
        hits = np.rint((S - r["S_track"]) / w)
        assert float(np.mean(hits == r["hits"])) >= 0.99
        up = O.update(r["S_track"] + w * hits, g["u_prev"], eps, float(g["param_lambda"]), g["x0"],
                      float(g["delta_t"]), g.get("u_min"), g.get("u_max"))
        assert _urel(u_seq, up["u_seq"]) < U_TOL
    c.close()


# ---------------------------------------------------------------- 6: with torque limits

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_decomposition_with_torque_limits(precision, lps, K, n, paths):
    """Real limits (clamp_mode 2): the decomposition against the same context's clamped launch without discs, the
    hit counts against the yardstick's with limits, and the fused update's nominal inside the limits."""
    p = _problem(n, K, paths)
    sd = np.sqrt(np.diag(_sigma(n)))
    lo, hi = p["u"][0] - 0.5 * sd, p["u"][0] + 0.8 * sd
    w = 1.0e10
    eng = _engine(n, K, 100.0, precision, lps, u_min=lo, u_max=hi)
    noise = _stage(eng, p, paths)
    S_free = _S(eng, noise)
    free = _ref(n, K, paths, np.zeros((0, 3)), 0.0, lo=lo, hi=hi)
    assert float(np.max(np.abs(S_free - free["S"]) / np.abs(free["S"]))) < S_TOL
    discs = place_discs(free, _chains(n)[1])[:3]              # the clipped controls move the chain elsewhere
    eng.set_obstacles(discs, w)
    S = _S(eng, noise)
    mask, _ = eng.obstacle_hits(noise)
    hits = _hits_from_masks(mask)
    assert 0.10 <= float(np.mean(hits > 0)) <= 0.90
    assert np.array_equal(S, S_free + w * hits.astype(np.float64))
    r = _with_device_hits(n, K, paths, discs, w, 100.0, hits, lo, hi)
    assert float(np.mean(hits == r["hits"])) >= 0.99
    eng.rollout(noise, fused_update=True)
    u = eng.nominal()
    assert _inside(u, lo, hi)                                 # the nominal's clamp still runs (mode 2)
    assert _urel(u, r["u_seq"]) < U_TOL
    eng.close()


# ---------------------------------------------------------------- 7: two shards

@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_two_shards_merge_to_the_unsharded_launch(precision, lps, K, paths):
    n = 7
    p = _problem(n, K, paths)
    lam, w = 3.0e6, 3.0e6
    one = _engine(n, K, lam, precision, lps)
    noise = _stage(one, p, paths)
    one.set_obstacles(p["discs"], w)
    one.rollout(noise)
    want = one.weighted_noise()
    one.close()
    Ka = K // 2 + 7
    engines, parts = [], []
    for off, Kl in ((0, Ka), (Ka, K - Ka)):
        e = _engine(n, Kl, lam, precision, lps, K_total=K, k_offset=off)
        e.set_step_inputs(p["x0"], paths["xydq_circle"][40:70], p["u"])
        e.set_obstacles(p["discs"], w)
        nz = e.new_noise()
        nz.copy_(noise[:, off:off + Kl])
        part = e.new_partial()
        e.rollout(nz, partial_out=part)
        e.synchronize()
        engines.append(e)
        parts.append(part)
    engines[1].merge(torch.cat(parts).contiguous(), 2)
    got = engines[1].weighted_noise()
    for e in engines:
        e.close()
    np.testing.assert_allclose(got, want, rtol=W_TOL, atol=W_TOL)
    assert np.any(want != 0.0)


# ---------------------------------------------------------------- 8: removal

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("precision,lps,K", FORMS, ids=FORM_IDS)
def test_removed_discs_leave_no_trace(precision, lps, K, n, paths):
    p = _problem(n, K, paths)
    out = []
    for had in (False, True):
        eng = _engine(n, K, 3.0e6, precision, lps)
        noise = _stage(eng, p, paths)
        if had:
            eng.set_obstacles(p["discs"], 1.0e10)
            assert np.any(_S(eng, noise) >= 1.0e10)
            eng.set_obstacles(None)
            assert eng.obstacles.shape == (0, 3)
        S = _S(eng, noise, fused_update=True)
        out.append((S, eng.weighted_noise(), eng.nominal()))
        eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 9: bad arguments

def test_set_obstacles_rejects_bad_arguments(paths):
    from mppi_robotarm_amd import _native as N
    n, K = 7, 300
    p = _problem(n, K, paths)
    eng = _engine(n, K, lps=1)
    noise = _stage(eng, p, paths)
    eng.set_obstacles(p["discs"][:2], 1.0e10)
    S = _S(eng, noise)
    lib, dp = eng._lib, C.POINTER(C.c_double)

    def rc(nd, rows, cost):
        a = np.ascontiguousarray(rows, dtype=np.float64)
        return lib.mppi_chain_set_obstacles(eng._ctx, nd, a.ctypes.data_as(dp), cost)

    ok = [[0.0, 0.0, 0.1]]
    nan, inf = float("nan"), float("inf")
    for nd, rows, cost in ((-1, ok, 1.0), (9, np.zeros((9, 3)), 1.0), (1, [[0.0, 0.0, nan]], 1.0),
                           (1, [[0.0, 0.0, -0.1]], 1.0), (1, [[inf, 0.0, 0.1]], 1.0), (1, [[0.0, nan, 0.1]], 1.0),
                           (1, [[0.0, -inf, 0.1]], 1.0), (1, ok, nan), (1, ok, -1.0), (1, ok, inf), (0, ok, -1.0)):
        assert rc(nd, rows, cost) == N.MPPI_E_ARG, (nd, rows, cost)
        assert b"obstacles" in lib.mppi_last_error()
    assert lib.mppi_chain_set_obstacles(eng._ctx, 1, None, 1.0) == N.MPPI_E_ARG
    for bad in ([[0.0, 0.0]], np.zeros((9, 3)), [[0.0, 0.0, -1.0]]):
        with pytest.raises(ValueError):
            eng.set_obstacles(bad, 1.0)
    with pytest.raises(ValueError):
        eng.set_obstacles(ok, -1.0)
    assert np.array_equal(_S(eng, noise), S)                  # a rejected call keeps the discs in effect
    with pytest.raises(ValueError):
        eng.debug_slots(noise)                                # the slot-recording instances have no discs
    for K_bad in (0, K + 1):
        with pytest.raises(ValueError):
            eng.obstacle_hits(noise, K=K_bad)
    assert rc(1, [[0.0, 0.0, inf]], 0.0) == N.MPPI_OK         # an infinite radius and a zero cost are allowed
    assert np.all(eng.obstacle_hits(noise, K=5)[0] == np.uint64(0x7F))   # ... and every link touches it
    eng.set_obstacles(None)
    assert eng.debug_slots(noise).shape == (K, T)
    eng.close()


# ---------------------------------------------------------------- 10: the drop-in

@pytest.mark.parametrize("precision", ["f32", "f64", "auto"])
def test_dropin_avoids_the_disc(precision, paths):
    """ChainMPPIController at n = 7 over a short closed loop on the fp64 plant: with obstacle_cost dominating and a
    clear start no executed state collides; an in-place edit and a rebind of `obstacles` are seen on the next call;
    a bad value raises ValueError with the RNG state and u_prev untouched.  With precision="auto" two steps are
    made to take the fp64 engine (_spread, the flag the weights' spread sets for the next step): the third of the
    loop, which builds that engine, and the one after the in-place edit, which finds it parked with the old disc."""
    from mppi_robotarm_amd.chain import CHAIN7_SIGMA, CHAIN7_X0, ChainMPPIController, ChainParams, gravity_torque
    P, Po = ChainParams(), CO.ChainParams()
    path = paths["xydq_circle"]
    ex, ey = CO.chain_fk(CHAIN7_X0[:7], Po)
    # over 16 steps of 6 ms the tip moves millimetres: a 1 cm disc beside the last link's tip, 1.5 mm clear of it,
    # on the side of the path's waypoints ahead (a third of the first step's rollouts touch it, by the yardstick)
    th = float(np.sum(CHAIN7_X0[:7]))
    side = np.array([-np.sin(th), np.cos(th)])
    side = side * np.sign(float((path[25, :2] - np.array([ex, ey])) @ side))
    discs = np.array([[ex + 0.0115 * side[0], ey + 0.0115 * side[1], 0.01]])
    assert not chain_collides(CHAIN7_X0[:7], discs, Po)[0]
    np.random.seed(5)
    c = ChainMPPIController(0.006, path, 16, 2048, 0.0, 100.0, 0.98, CHAIN7_SIGMA, chain=P, precision=precision,
                            u_init=gravity_torque(CHAIN7_X0[:7], P), obstacles=discs, obstacle_cost=1.0e10)
    c.keep_costs = True
    x = CHAIN7_X0.copy()
    paid = 0
    auto = precision == "auto"
    for i in range(6):
        if auto and i == 2:
            c._spread = True
        u0, _, _, _ = c.calc_control_input(x)
        u0 = np.array(u0)
        if not auto:
            assert c.last_precision == precision
        elif i == 2:
            assert c.last_precision == "f64"                  # (auto's other steps: fp32, then fp64 if the weights spread)
        assert np.array_equal(c._engine.obstacles, discs) and c._engine.obstacle_cost == 1.0e10
        paid += int(np.sum(c.last_S >= 1.0e10))
        q, dq = CO.chain_forward_dynamics(x[None, :7], x[None, 7:], u0[None, :], 0.006, Po)
        x = np.concatenate([q[0], dq[0]])
        assert not chain_collides(x[:7], discs, Po)[0]
    assert paid > 0                                           # the disc was in reach of the sampled rollouts
    # an in-place edit: the disc swallows the whole chain, every sample pays at every step
    discs[0] = [0.0, 0.0, 5.0]
    if auto:
        assert "f64" in set(c._slots) | {c._active}         # the fp64 engine exists, holding the small disc
        c._spread = True
    c.calc_control_input(x)
    assert np.all(c.last_S >= 17 * 1.0e10)
    assert np.array_equal(c._engine.obstacles, discs)
    if auto:
        assert c.last_precision == "f64" and c._active == "f64"
    c.obstacles = None                                        # a rebind: no discs
    c.calc_control_input(x)
    assert np.all(c.last_S < 1.0e10) and c._engine.obstacles.shape == (0, 3)
    c.obstacles = [[0.0, 0.0, -1.0]]
    u_before, state = c.u_prev.copy(), np.random.get_state()
    with pytest.raises(ValueError):
        c.calc_control_input(x)
    assert np.array_equal(c.u_prev, u_before)
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))
    c.close()


# ---------------------------------------------------------------- 11: lifetime

LIFE_K, LIFE_T, LIFE_N = 65536, 128, 7


def test_contexts_with_discs_return_their_memory(paths):
    """32 create / set-discs / launch / close cycles leave the device's free memory where it was, by
    test_gpu_lifetime.py's measure: the drop over the cycles stays below one cycle's live footprint F, and F > 0.
    The cycle is sized so that F shows: what a chain context allocates grows with the hand-off rows only,
    workgroups x (2 + T n) values, so the three forms are built at n = 7, T = 128, K = 65536 (256, 1024 and 256
    workgroups: about 3.7 + 7.4 + 3.7 MB), not at the kernels' smallest shapes.  The noise, the one large tensor,
    exists before anything is measured, and F is taken on the second cycle, so neither the allocator's cache nor the
    loaded code objects count into it."""
    from mppi_robotarm_amd.chain import CHAIN7_SIGMA, CHAIN7_X0, ChainEngine, ChainParams, gravity_torque
    n, K, T_ = LIFE_N, LIFE_K, LIFE_T
    discs = _problem(n, 300, paths)["discs"]
    P = ChainParams()
    u = np.tile(gravity_torque(CHAIN7_X0[:n], P), (T_, 1))
    noise = torch.empty((T_, K, n), dtype=torch.float32, device="cuda")

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle(probe=None):
        engines = [ChainEngine(K, T_, 0.006, 100.0, ALPHA, CHAIN7_SIGMA, W, TW, 0.0, P, device=0, precision=pr,
                               lanes_per_sample=lps) for pr, lps, _ in FORMS]
        for eng in engines:
            eng.set_step_inputs(CHAIN7_X0, paths["xydq_circle"][40:70], u)
            eng.set_obstacles(discs, 1.0e10)
            eng.rollout(noise, fused_update=True)
            eng.obstacle_hits(noise, K=16)
            eng.synchronize()
        if probe is not None:
            probe()
        for eng in engines:
            eng.close()

    first = ChainEngine(K, T_, 0.006, 100.0, ALPHA, CHAIN7_SIGMA, W, TW, 0.0, P, device=0)
    first.philox_noise(3, 0, out=noise)
    first.synchronize()
    first.close()
    cycle()
    alive = []
    before = free()
    cycle(probe=lambda: alive.append(free()))
    F = before - alive[0]
    for _ in range(2):
        cycle()
    start = free()
    for _ in range(32):
        cycle()
    drop = start - free()
    print(f"lifetime: F = {F} B with one cycle's contexts alive, drop over 32 cycles = {drop} B")
    assert F > 0
    assert drop < F
