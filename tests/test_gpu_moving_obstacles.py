"""GPU: moving obstacles (mppi_set_moving_obstacles) on the 2-link arm, through every layer.

The yardstick is oracle/mppi_oracle.py with vel= (the fp64 oracle with the discs at c + v (t + 1) dt), pinned on the CPU
to the move_* fixtures captured from the reference (test_moving_obstacle_cpu.py).  Tolerances and the treatment of
the collision flag's discontinuity are test_gpu_obstacles.py's: masks are compared with the fp64 predicate on the
device's OWN recorded directions (bits may differ only within 4e-6 m of a boundary, on at most 0.5 % of the pairs),
the penalty is checked exactly through S = S_free + w * hits with the device's own hit counts, and the yardstick
takes the device's hit counts where a weight depends on them.  The shared problem of a shape (noise, unobstructed
yardstick run, discs) is test_gpu_obstacles.py's own, computed once for both files.
"""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mppi_oracle as O  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from helpers import RUNPY, X0, _ctrl, _engine, _gpu, _urel, _window  # noqa: E402, F401
from test_gpu_obstacles import (EDGE, EDGE_CAP, LPS, S_TOL, SHAPES, U_TOL, W_TOL, _check_S, _feed,  # noqa: E402
                                _hits_from_masks, _problem, _stage, _u)
from tieflip import waypoint_pick_delta  # noqa: E402

DT = 0.006
MOVE_STEPS = ["a_k128_t20", "b_dense_k256_t24", "c_expl_k128_t20", "d_clamp_k128_t20"]


def _vel(p, T, n=8):
    """Velocities for the shared problem's discs: each disc crosses about its own radius over the horizon (so the
    share of colliding samples stays what the static layout gives, while the step index matters), in directions
    spread round the circle; the far discs and one other stay at rest (a mixed table)."""
    d = p["discs"][:n]
    ang = 2.0 * np.pi * np.arange(n) / 8.0 + 0.4
    v = (d[:, 2] / (T * DT))[:, None] * np.stack([np.cos(ang), np.sin(ang)], -1)
    v[d[:, 2] >= 0.05] = 0.0                     # the discs that are never touched
    if n > 5:
        v[5] = 0.0
    return v


def _arrive(p, T, n=8):
    """(discs, vel): the discs set back so that each is where the static layout has it at the END of the horizon."""
    v = _vel(p, T, n)
    d = p["discs"][:n].copy()
    d[:, :2] -= v * (T * DT)
    return d, v


def _mref(K, T, paths, discs, vel, w, lam=100.0, shift=0, eps=None):
    p = _problem(K, T, paths)
    return O.rollout_costs(X0, _u(T), p["eps"] if eps is None else eps, paths["xydq_circle"], 0, DT, lam, 0.98,
                           RUNPY["sigma"], RUNPY["stage_cost_weight"], RUNPY["terminal_cost_weight"], discs=discs,
                           vel=vel, obstacle_cost=w, shift=shift, details=True)


def _set_moving_raw(eng, discs, vel, cost):
    """The C entry point itself (vel may be None: NULL)."""
    dp = C.POINTER(C.c_double)
    a = np.ascontiguousarray(discs, dtype=np.float64)
    v = None if vel is None else np.ascontiguousarray(vel, dtype=np.float64)
    return eng._lib.mppi_set_moving_obstacles(eng._ctx, a.shape[0], a.ctypes.data_as(dp),
                                              None if v is None else v.ctypes.data_as(dp), cost)


def _fused(eng, noise, K, merge="auto"):
    """One fused step from the staged inputs: (S, w_eps, nominal, the trajectory of the unshifted update)."""
    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S_dev, fused_update=True, merge=merge)
    return S_dev.cpu().numpy(), eng.weighted_noise(), eng.nominal(), eng.optimal_traj().cpu().numpy()


# ---------------------------------------------------------------- 1: at rest equals static

@pytest.mark.parametrize("handoff", ["default", "counter"])
@pytest.mark.parametrize("lps", LPS)
def test_at_rest_is_the_static_feature_bit_for_bit(lps, handoff, paths, monkeypatch):
    """vel = NULL and vel = 0 launch what mppi_set_obstacles launches: S, w_eps, the nominal and upd (through its
    trajectory) are bit-equal, in both hand-off forms, in the in-launch and in the deferred form."""
    from mppi_robotarm_amd import _native as N
    if handoff == "counter":
        monkeypatch.setenv("MPPI_HANDOFF", "counter")
    else:
        monkeypatch.delenv("MPPI_HANDOFF", raising=False)
    K, T = SHAPES[0]
    p = _problem(K, T, paths)
    discs, w = p["discs"], 3.0e6
    got = []
    for how in ("static", "null", "zeros"):
        eng = _engine(K, T, lps=lps, param_lambda=3.0e6)
        noise = _stage(eng, K, T, paths)
        if how == "static":
            eng.set_obstacles(discs, w)
        elif how == "null":
            assert _set_moving_raw(eng, discs, None, w) == N.MPPI_OK
        else:
            eng.set_obstacles(discs, w, velocities=np.zeros((8, 2)))
            assert eng.obstacle_velocities.shape == (8, 2)
        out = _fused(eng, noise, K, merge="inline")
        mask, _ = eng.obstacle_hits(noise)
        # the deferred form: two chained fused steps with nothing read in between, then the result
        eng.set_step_inputs(X0, _window(paths), _u(T))
        eng.rollout(noise, fused_update=True)
        eng.rollout(noise, fused_update=True)
        assert eng.pending()
        got.append(out + (mask, eng.weighted_noise(), eng.nominal(), eng.optimal_traj().cpu().numpy()))
        eng.close()
    assert 0.10 <= float(np.mean(_hits_from_masks(got[0][4]) > 0)) <= 0.90
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------- 2: masks on the device's own directions

def _compare_masks(mask, d, discs, vel, what):
    n = discs.shape[0]
    want, gap = O.moving_masks(d, discs, vel, DT)
    bits = (np.uint32(1) << np.arange(2 * n, dtype=np.uint32)).reshape(n, 2)
    differ = ((mask[..., None, None] ^ want[..., None, None]) & bits) != 0
    assert not np.any(differ & (gap > EDGE)), f"{what}: a bit differs at clearance {float(gap[differ].max()):.2e} m"
    edge_pairs = float(np.mean(differ))
    print(f"{what}: {float(np.mean((mask != 0).any(1))):.1%} of the samples collide, {int(differ.sum())} bits differ "
          f"({edge_pairs:.4%} of the (sample, step, link, disc) pairs, all within {EDGE} m)")
    assert edge_pairs <= EDGE_CAP
    assert mask.max() < (1 << (2 * n))
    return want


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("K,T", SHAPES)
def test_masks_on_the_devices_own_directions(K, T, n, paths):
    p = _problem(K, T, paths)
    discs, vel = _arrive(p, T, n)
    # the inputs, by the fp64 yardstick alone: >= 99.5 % of the pairs lie outside the 4e-6 m where a bit may differ
    r = _mref(K, T, paths, discs, vel, 0.0)
    assert float(np.mean(np.abs(r["dist"] - discs[:, 2][None, None, :, None]) > EDGE)) >= 0.995
    assert 0.10 <= float(np.mean(r["flag"].any(1))) <= 0.90
    rest = _mref(K, T, paths, discs, None, 0.0)
    assert float(np.mean(r["hits"] != rest["hits"])) >= 0.10        # the motion matters on this problem
    eng = _engine(K, T)
    noise = _stage(eng, K, T, paths)
    eng.set_obstacles(discs, 1.0e10, velocities=vel)
    mask, d = eng.obstacle_hits(noise)
    eng.close()
    q = p["free"]["q"]
    want_d = np.stack([np.cos(q[..., 0]), np.sin(q[..., 0]), np.cos(q.sum(-1)), np.sin(q.sum(-1))], -1)
    assert float(np.max(np.abs(d - want_d))) < 1e-4
    _compare_masks(mask, d, discs, vel, f"K {K} T {T} n {n}")
    assert 0.10 <= float(np.mean((mask != 0).any(1))) <= 0.90
    assert float(np.mean((mask != 0) == r["flag"])) >= 0.99


# ---------------------------------------------------------------- 3: the time index

def _fast_disc(free, T):
    """One disc with |v| dt = 3 r > 2 r that comes in against the end effector's direction of travel and is r ahead
    of the median final end-effector position (so the samples past the median touch it, with link 2's tip) exactly at
    the time of the final state, T dt: a step earlier it is three radii further ahead, where no sample has got to,
    a step later three radii behind."""
    ee = free["ee"][:, -1]
    ee0 = np.array([np.cos(X0[0]) + np.cos(X0[0] + X0[1]), np.sin(X0[0]) + np.sin(X0[0] + X0[1])])
    along = (np.median(ee, 0) - ee0) / np.linalg.norm(np.median(ee, 0) - ee0)
    r = 4.0 * float(np.std((ee - np.median(ee, 0)) @ along))
    tip = np.median(ee, 0) + r * along
    v = -(3.0 * r / DT) * along
    return np.array([[tip[0] - v[0] * T * DT, tip[1] - v[1] * T * DT, r]]), v[None, :]


_fast = {}


def _sigma(T):
    """run.py's Sigma; at T = 128 a thousandth of it: the samples then spread over centimetres, not over the whole
    workspace, so the fast disc's radius (four spreads) and its 3 r T of travel stay where fp32 resolves 4e-6 m."""
    return RUNPY["sigma"] * (1.0e-3 if T > 64 else 1.0)


def _fast_problem(K, T, paths):
    """The problem of a horizon of its own (T = 1, 5, 7, 128): noise read back, the unobstructed yardstick run;
    computed once and shared."""
    if (K, T) not in _fast:
        eng = _engine(K, T, sigma=_sigma(T))
        eps = eng.philox_noise(42, 3).cpu().numpy().transpose(1, 0, 2).astype(np.float64)
        eng.close()
        free = O.rollout_costs(X0, _u(T), eps, paths["xydq_circle"], 0, DT, 100.0, 0.98, _sigma(T),
                               RUNPY["stage_cost_weight"], RUNPY["terminal_cost_weight"], details=True)
        _fast[(K, T)] = (eps, free)
    return _fast[(K, T)]


@pytest.mark.parametrize("K,T,lps", [(1000, 9, 1), (1000, 9, 4), (300, 1, 1), (300, 1, 8), (300, 5, 1), (300, 5, 2),
                                     (300, 7, 1), (300, 7, 16), (256, 128, 1), (256, 128, 4)])
def test_time_index(K, T, lps, paths):
    """A fast disc (|v| dt = 3 r): the device's masks are the yardstick's at c + v (t + 1) dt and not the ones a step
    off; the final state's extra count uses step T - 1's centre.  T = 1; T = 5 and 7 (the remainder steps of the
    4-unrolled loop, with both peelings: LPS = 1 peels the first step); T = 128 (the table's last row)."""
    eps, free = _fast_problem(K, T, paths)
    discs, vel = _fast_disc(free, T)
    assert float(np.linalg.norm(vel[0])) * DT > 2.0 * discs[0, 2]
    kw = dict(discs=discs, vel=vel, obstacle_cost=0.0)
    args = (X0, _u(T), eps, paths["xydq_circle"], 0, DT, 100.0, 0.98, _sigma(T), RUNPY["stage_cost_weight"],
            RUNPY["terminal_cost_weight"])
    r = O.rollout_costs(*args, details=True, **kw)
    share = float(np.mean(r["flag"].any(1)))
    assert 0.10 <= share <= 0.90
    # the CPU side: either off-by-one definition changes the masks of >= 10 % of the samples
    for shift in (-1, 1):
        off = O.rollout_costs(*args, shift=shift, details=True, **kw)
        assert float(np.mean((off["flag"] != r["flag"]).any(1))) >= 0.10, shift
    w = 7.0
    eng = _engine(K, T, lps=lps, sigma=_sigma(T))
    eng.set_step_inputs(X0, _window(paths), _u(T))
    noise = eng.philox_noise(42, 3)
    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S_dev)
    S_free = S_dev.cpu().numpy()
    eng.set_obstacles(discs, w, velocities=vel)
    mask, d = eng.obstacle_hits(noise)
    eng.rollout(noise, S_out=S_dev)
    S = S_dev.cpu().numpy()
    eng.close()
    want = _compare_masks(mask, d, discs, vel, f"K {K} T {T} lps {lps}")
    agree = float(np.mean(((mask != 0) == r["flag"]).all(1)))
    assert agree >= 0.99
    for shift in (-1, 1):
        off, _ = O.moving_masks(d, discs, vel, DT, shift=shift)
        assert float(np.mean((off != mask).any(1))) >= 0.10, shift
    assert np.array_equal(mask, want) or float(np.mean(mask != want)) <= EDGE_CAP
    # the rollout counted what the debug kernel saw: every step's flag and the last one once more (T dt = step T - 1)
    hits = _hits_from_masks(mask)
    assert hits.max() <= T + 1 and np.array_equal(S, S_free + w * hits.astype(np.float64))
    assert (mask[:, -1] != 0).any()                            # the extra count is exercised


# ---------------------------------------------------------------- 4: the decomposition; forms bit-identical

@pytest.mark.parametrize("lam", [100.0, 3.0e6])
@pytest.mark.parametrize("K,T", SHAPES)
def test_S_is_the_free_S_plus_w_hits_and_forms_agree(K, T, lam, paths, monkeypatch):
    """S = S_free + w * hits bit for bit with the device's own masks, at every LPS and in both hand-off forms; S and
    the hits are bit-identical across all of them, w_eps across the hand-off forms of one LPS (and across LPS where
    one sample carries all the weight, else to 1e-10: the property the kernels have without moving discs)."""
    p = _problem(K, T, paths)
    runs = {}
    for lps in LPS:
        for h in ("default", "counter"):
            if h == "counter":
                monkeypatch.setenv("MPPI_HANDOFF", "counter")
            else:
                monkeypatch.delenv("MPPI_HANDOFF", raising=False)
            eng = _engine(K, T, lps=lps, param_lambda=lam)
            assert eng.lanes_per_sample == lps and eng.handoff == ("counter" if h == "counter" else "poll")
            noise = _stage(eng, K, T, paths)
            S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
            eng.rollout(noise, S_out=S_dev)
            S_free, weps_free = S_dev.cpu().numpy(), eng.weighted_noise()
            out = {}
            for n, w in ((8, 1.0e10), (3, 3.0e6), (1, 7.0)):   # integer-valued: w * hits is exact
                discs, vel = _arrive(p, T, n)
                eng.set_obstacles(discs, w, velocities=vel)
                eng.rollout(noise, S_out=S_dev)
                S, weps = S_dev.cpu().numpy(), eng.weighted_noise()
                mask, _ = eng.obstacle_hits(noise)
                hits = _hits_from_masks(mask)
                assert hits.max() <= T + 1 and 0.10 <= float(np.mean(hits > 0)) <= 0.90
                assert np.array_equal(S, S_free + w * hits.astype(np.float64)), (lps, h, n)
                out[n] = (S, weps, hits)
            # n = 0 after moving discs: the kernels of a context that never had discs
            eng.set_obstacles(None, 1.0e10)
            assert eng.obstacle_velocities is None
            eng.rollout(noise, S_out=S_dev)
            assert np.array_equal(S_dev.cpu().numpy(), S_free) and np.array_equal(eng.weighted_noise(), weps_free)
            eng.close()
            runs[(lps, h)] = out
    first = runs[(LPS[0], "default")]
    for (lps, h), out in runs.items():
        for n in out:
            assert np.array_equal(out[n][0], first[n][0]) and np.array_equal(out[n][2], first[n][2]), (lps, h, n)
            assert np.array_equal(out[n][1], runs[(lps, "default")][n][1]), (lps, h, n)
            if np.count_nonzero(np.exp(-(out[n][0] - out[n][0].min()) / lam)) == 1:
                assert np.array_equal(out[n][1], first[n][1]), (lps, h, n)
            else:
                np.testing.assert_allclose(out[n][1], first[n][1], rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("lam,w", [(100.0, 1.0e10), (3.0e6, 3.0e6)])
@pytest.mark.parametrize("K,T", SHAPES)
def test_weighted_noise_and_nominal(K, T, lam, w, paths):
    p = _problem(K, T, paths)
    discs, vel = _arrive(p, T, 8)
    eng = _engine(K, T, param_lambda=lam)
    noise = _stage(eng, K, T, paths)
    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.set_obstacles(discs, w, velocities=vel)
    eng.rollout(noise, S_out=S_dev)
    S, weps = S_dev.cpu().numpy(), eng.weighted_noise()
    mask, _ = eng.obstacle_hits(noise)
    hits = _hits_from_masks(mask)
    r = _mref(K, T, paths, discs, vel, w, lam)
    assert float(np.mean(hits == r["hits"])) >= 0.99
    S_ref = r["S_track"] + w * hits
    up = O.update(S_ref, _u(T), p["eps"], lam, X0, DT)
    host = O.weighted_noise(O.compute_weights(S, lam), p["eps"])
    print(f"K {K} T {T} lam {lam}: S rel {float(np.max(np.abs(S - S_ref) / np.abs(S_ref))):.2e}, "
          f"w_eps vs host sum {float(np.max(np.abs(weps - host))):.2e}, vs yardstick {_urel(weps, up['w_eps_raw']):.2e}")
    assert float(np.max(np.abs(S - S_ref) / np.abs(S_ref))) < S_TOL
    np.testing.assert_allclose(weps, host, rtol=W_TOL, atol=W_TOL)
    assert _urel(weps, up["w_eps_raw"]) < U_TOL
    if lam == 100.0:
        j, j_ref = int(np.argmin(S)), int(np.argmin(S_ref))
        assert j == j_ref or abs(S_ref[j] - S_ref[j_ref]) <= 1e-6 * abs(S_ref[j_ref])
    eng.rollout(noise, fused_update=True)
    assert _urel(eng.nominal(), up["u_seq"]) < U_TOL
    eng.close()


# ---------------------------------------------------------------- 5: the fixtures through the drop-in

def _load(kind, name):
    return dict(np.load(os.path.join(GOLDEN, f"move_{kind}_{name}.npz")))


@pytest.mark.parametrize("how", ["general", "tick"])
@pytest.mark.parametrize("name", MOVE_STEPS)
def test_moving_step_matches_reference(name, how, paths):
    g = _load("step", name)
    eps = g["eps"].astype(np.float64)
    c = _ctrl(g, paths, obstacle_velocities=g["obstacle_velocities"],
              **(dict(noise="device", seed=3) if how == "tick" else {}))
    _feed(c, eps, how)
    c.keep_costs = True
    u_prev = c.u_prev
    u0, u_seq, opt, _ = c.calc_control_input(g["x0"])
    if how == "tick":
        assert c._bound is not None                          # the native tick really ran
    assert np.array_equal(c._engine.obstacle_velocities, g["obstacle_velocities"])
    _check_S(c.last_S, g["S"], g["clearance"], f"{name}/{how}")
    assert u_seq is u_prev and np.shares_memory(u0, u_prev)
    assert c.prev_waypoints_idx == int(g["prev_idx_after"])
    # the device's own hit counts (S_dev - S_track, exact multiples of w)
    w = float(g["obstacle_cost"])
    r = O.rollout_costs(g["x0"], g["u_prev"], eps, paths[str(g["path"])], int(g["prev_idx_after"]),
                        float(g["delta_t"]), float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"],
                        g["stage_cost_weight"], g["terminal_cost_weight"], float(g["param_exploration"]),
                        lo=g.get("u_min"), hi=g.get("u_max"), discs=g["obstacles"], vel=g["obstacle_velocities"],
                        obstacle_cost=w, details=True)
    hits = np.rint((c.last_S - r["S_track"]) / w)
    assert float(np.mean(hits == r["hits"])) >= 0.99
    assert float(np.mean(hits != g["hits_rest"])) >= 0.50     # not the static feature: the same discs at rest
    if bool(g["one_hot"]):
        assert int(np.argmin(c.last_S)) == int(np.argmin(g["S"]))
        assert _urel(u_seq, g["u_seq"]) < U_TOL and _urel(u0, g["u0"]) < U_TOL
        np.testing.assert_allclose(opt, g["optimal_traj"], rtol=1e-4, atol=1e-4)
    else:
        # dense weights: the yardstick takes the device's hit counts, so a boundary tie cannot move a weight
        up = O.update(r["S_track"] + w * hits, g["u_prev"], eps, float(g["param_lambda"]), g["x0"],
                      float(g["delta_t"]), g.get("u_min"), g.get("u_max"))
        assert _urel(u_seq, up["u_seq"]) < U_TOL
    c.close()


def test_moving_closed_loop_ticks(paths):
    """Each tick of run.py's loop from the reference's own state / u_prev / index, the test advancing the discs as
    the generator did (the fixture stores each tick's positions).  S with the device's own waypoint picks, as
    test_gpu_obstacles.test_obstructed_closed_loop_ticks (which says why)."""
    from mppi_robotarm_amd.controller import MPPIControllerForPathTracking
    g = _load("loop", "k64_t20")
    T, K = int(g["T"]), int(g["K"])
    w, vel = float(g["obstacle_cost"]), g["obstacle_velocities"]
    discs = g["obstacles"][0].copy()
    c = MPPIControllerForPathTracking(delta_t=DT, ref_path=paths["xydq_circle"], horizon_step_T=T,
                                      number_of_samples_K=K, verbose=False, obstacles=discs, obstacle_cost=w,
                                      obstacle_velocities=vel, **RUNPY)
    c.keep_costs = True
    u_prev, prev = np.array([[10.0, -2.0]] * T), 0
    compared = 0
    for i in range(int(g["ticks"])):
        np.testing.assert_allclose(discs, g["obstacles"][i], rtol=0, atol=1e-12)
        c.u_prev = u_prev.copy()
        c.prev_waypoints_idx = prev
        eps = g["eps"][i].astype(np.float64)
        c._calc_epsilon = lambda *a, e=eps, **k: e
        u, u_seq, _, _ = c.calc_control_input(g["states"][i])
        u, u_seq, S = np.array(u), np.array(u_seq), c.last_S.copy()
        assert c.prev_waypoints_idx == int(g["prev_idx"][i])
        clean = g["clearance"][i].min(1) >= 1e-4
        assert float(np.mean(clean)) >= 0.80, i
        window = paths["xydq_circle"][c.prev_waypoints_idx:c.prev_waypoints_idx + 30]
        c._engine.set_step_inputs(g["states"][i], window, u_prev)
        slots, _ = c._engine.nearest_slots(c._noise_dev)
        r = O.rollout_costs(g["states"][i], u_prev, eps, paths["xydq_circle"], c.prev_waypoints_idx, DT, 100.0, 0.98,
                            RUNPY["sigma"], RUNPY["stage_cost_weight"], RUNPY["terminal_cost_weight"],
                            discs=discs, vel=vel, obstacle_cost=w, details=True)
        delta, gap, differ = waypoint_pick_delta(r, slots, window, RUNPY["stage_cost_weight"],
                                                 RUNPY["terminal_cost_weight"])
        ref = g["S"][i] + delta
        rel = float(np.max(np.abs(S[clean] - ref[clean]) / np.abs(ref[clean])))
        print(f"tick {i}: {float(np.mean(g['flag'][i].any(1))):.0%} collide, {float(np.mean(clean)):.0%} clean, "
              f"S rel {rel:.2e} with the device's picks, {int(differ.sum())} picks differ")
        assert float(gap.max()) <= EDGE and float(np.mean(differ)) <= EDGE_CAP, i
        assert rel < S_TOL, i
        order = np.argsort(g["S"][i])
        if (g["S"][i][order[1]] - g["S"][i][order[0]]) >= 1e-3 * abs(g["S"][i][order[0]]) and clean[order[:2]].all():
            compared += 1
            assert int(np.argmin(S)) == int(order[0]), i
            assert _urel(u_seq, g["u_seq"][i]) < U_TOL and _urel(u, g["u"][i]) < U_TOL, i
        u_prev, prev = g["u_seq"][i].copy(), int(g["prev_idx"][i])
        discs[:, :2] += vel * 0.003              # the world moves on by one plant step, in place: seen by value
    assert compared >= 5
    c.close()


# ---------------------------------------------------------------- 6: state handling

def test_velocities_change_while_a_deferred_step_is_pending(paths):
    """The pending step finishes with the discs it was launched with; the new launch uses the new ones."""
    K, T = SHAPES[0]
    p = _problem(K, T, paths)
    discs, v1 = _arrive(p, T, 8)
    v2 = -v1
    lam, w = 3.0e6, 3.0e6
    a, b = (_engine(K, T, param_lambda=lam) for _ in range(2))
    noise = _stage(a, K, T, paths)
    _stage(b, K, T, paths)
    for e in (a, b):
        e.set_obstacles(discs, w, velocities=v1)
    a.rollout(noise, fused_update=True)                      # stays pending
    assert a.pending()
    b.rollout(noise, fused_update=True, merge="inline")
    first = (b.weighted_noise(), b.nominal())
    for e in (a, b):
        e.set_obstacles(discs, w, velocities=v2)             # no device call: the pending step is not touched
    assert a.pending()
    S_a, S_b = (torch.empty(K, dtype=torch.float64, device="cuda") for _ in range(2))
    a.rollout(noise, fused_update=True, S_out=S_a)
    b.rollout(noise, fused_update=True, merge="inline", S_out=S_b)
    assert np.array_equal(S_a.cpu().numpy(), S_b.cpu().numpy())
    assert np.array_equal(a.weighted_noise(), b.weighted_noise()) and np.array_equal(a.nominal(), b.nominal())
    # the first step ran with v1: a third engine that only ever had v1 leaves the same first step
    c = _engine(K, T, param_lambda=lam)
    _stage(c, K, T, paths)
    c.set_obstacles(discs, w, velocities=v1)
    c.rollout(noise, fused_update=True, merge="inline")
    assert np.array_equal(c.weighted_noise(), first[0]) and np.array_equal(c.nominal(), first[1])
    # ... and v2 is not v1
    c.set_step_inputs(X0, _window(paths), _u(T))
    c.set_obstacles(discs, w, velocities=v2)
    c.rollout(noise, fused_update=True, merge="inline")
    assert not np.array_equal(c.weighted_noise(), first[0])
    for e in (a, b, c):
        e.synchronize()
        e.close()


def test_a_graph_freezes_discs_and_velocities(paths):
    K, T = SHAPES[0]
    p = _problem(K, T, paths)
    discs, vel = _arrive(p, T, 8)
    lam, w = 3.0e6, 3.0e6
    eager, graphed = (_engine(K, T, param_lambda=lam) for _ in range(2))
    noises = [eager.philox_noise(19, s) for s in range(2)]
    for e in (eager, graphed):
        e.set_step_inputs(X0, _window(paths), _u(T))
        e.set_obstacles(discs, w, velocities=vel)
    for nz in noises:
        eager.rollout(nz, fused_update=True)
    ref = (eager.weighted_noise(), eager.nominal())
    graphed.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        for nz in noises:
            graphed.rollout(nz, fused_update=True)
    torch.cuda.current_stream().wait_stream(s)
    graphed.set_obstacles(discs, w, velocities=-vel)         # after the capture: the replay does not see it
    graphed.set_step_inputs(X0, _window(paths), _u(T))
    graphed.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(graphed.weighted_noise(), ref[0]) and np.array_equal(graphed.nominal(), ref[1])
    for e in (eager, graphed):
        e.synchronize()
        e.close()


@pytest.mark.parametrize("how", ["general", "tick"])
def test_a_change_of_velocities_between_calls_is_seen(how, paths):
    """A rebind, an in-place edit and None each reach the device on the next call: the bound tick's "nothing
    changed" comparison includes the velocities, by value."""
    g = _load("step", "a_k128_t20")
    eps = g["eps"].astype(np.float64)
    vel = g["obstacle_velocities"].copy()
    c = _ctrl(g, paths, obstacle_velocities=vel, **(dict(noise="device", seed=3) if how == "tick" else {}))
    c.keep_costs = True

    def call():
        c.u_prev[:] = g["u_prev"]
        c.prev_waypoints_idx = int(g["prev_idx"])
        _feed(c, eps, how)
        c.calc_control_input(g["x0"])
        return c.last_S.copy()

    S1 = call()
    assert np.array_equal(call(), S1)                        # nothing changed (the tick takes its fast path)
    if how == "tick":
        assert c._fast is not None
    vel[0] = 0.0                                             # in place
    S2 = call()
    assert not np.array_equal(S2, S1)
    c.obstacle_velocities = None                             # the static path: the obst_step fixture's costs
    S3 = call()
    s = dict(np.load(os.path.join(GOLDEN, "obst_step_a_k128_t20.npz")))
    assert np.array_equal(s["obstacles"], g["obstacles"])
    _check_S(S3, s["S"], s["clearance"], f"static/{how}")
    c.obstacle_velocities = np.zeros((4, 2))                 # at rest, given: the same bits
    assert np.array_equal(call(), S3)
    c.obstacle_velocities = g["obstacle_velocities"].tolist()
    assert np.array_equal(call(), S1)
    c.obstacle_velocities = [[0.0, float("nan")]] * 4
    with pytest.raises(ValueError):
        c.calc_control_input(g["x0"])
    c.close()


def test_set_moving_obstacles_rejects_bad_arguments(paths):
    from mppi_robotarm_amd import _native as N
    K, T = SHAPES[0]
    p = _problem(K, T, paths)
    discs, vel = _arrive(p, T, 2)
    eng = _engine(K, T)
    noise = _stage(eng, K, T, paths)
    eng.set_obstacles(discs, 1.0e10, velocities=vel)
    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S_dev)
    S = S_dev.cpu().numpy()
    nan, inf = float("nan"), float("inf")
    ok_d, ok_v = [[0.0, 0.0, 0.1]], [[0.1, 0.0]]
    for d, v, cost in ((ok_d, [[nan, 0.0]], 1.0), (ok_d, [[0.0, inf]], 1.0), (ok_d, [[-inf, 0.0]], 1.0),
                       (ok_d, [[1e300, 0.0]], 1.0),                       # not finite in fp32
                       ([[3.0e38, 0.0, 0.1]], [[1.0e39, 0.0]], 1.0),
                       ([[3.3e38, 0.0, 0.1]], [[3.0e38, 0.0]], 1.0),      # both finite, the centre at T dt is not
                       ([[0.0, 0.0, -0.1]], ok_v, 1.0), ([[nan, 0.0, 0.1]], ok_v, 1.0), (ok_d, ok_v, -1.0),
                       (ok_d, ok_v, nan)):
        assert _set_moving_raw(eng, d, v, cost) == N.MPPI_E_ARG, (d, v, cost)
        assert b"obstacles" in eng._lib.mppi_last_error()
    dp = C.POINTER(C.c_double)
    z = np.zeros(3)
    assert eng._lib.mppi_set_moving_obstacles(eng._ctx, 9, z.ctypes.data_as(dp), None, 1.0) == N.MPPI_E_ARG
    assert eng._lib.mppi_set_moving_obstacles(eng._ctx, 1, None, None, 1.0) == N.MPPI_E_ARG
    for bad in ([[0.1, 0.0]], [[0.1, nan], [0.0, 0.0]], np.zeros((2, 3))):
        with pytest.raises(ValueError):
            eng.set_obstacles(discs, 1.0, velocities=bad)
    with pytest.raises(ValueError):
        eng.set_obstacles(None, 1.0, velocities=ok_v)
    eng.rollout(noise, S_out=S_dev)                           # a rejected call keeps discs and velocities in effect
    assert np.array_equal(S_dev.cpu().numpy(), S)
    assert _set_moving_raw(eng, [[3.0e38, 0.0, 0.1]], [[1.0, 0.0]], 1.0) == N.MPPI_OK
    eng.close()
