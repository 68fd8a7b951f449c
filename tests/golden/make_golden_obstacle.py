"""Generate the obstacle fixtures (``obst_step_*.npz``, ``obst_loop_*.npz``) from the imported reference.

Run ONCE where the reference checkout exists, like ``make_golden.py`` (whose
import shim, instrumentation and run.py constants this reuses) and
``make_golden_clamp.py`` (whose ``_g`` override the case with torque limits
reuses).  The reference's cost is hard-wired to ``_c`` / ``_phi``
(control.py:174-198); here the controller is subclassed and ONLY those two are
overridden, to return ``super() + w * collides(x)``: the penalty is added after
the x 10000.  A state collides when either link, a zero-thickness segment in
the cost's kinematics (``self.l1``, ``self.l2``, base at the origin, as ``_c``
computes x and y), is closer than ``r`` to a disc's centre, the projection
clipped to the segment.  Nothing else changes.

Only outputs are stored, plus per (sample, step) the fp64 collision flag and
the clearance |d - r| of the nearest boundary; no reference text is copied.
Every case asserts that it exercises the feature (see ``check``) and fails
loudly otherwise.  The discs of a case are placed from that case's own
unobstructed run (``layout``): one of radius 6 mm centred 2 mm off the
unobstructed best sample's final end-effector position (so the obstacle changes
the decision), one that link 1's interior sweeps into, one ahead of the end
effector, and a far one that is never hit.

Usage:  python tests/golden/make_golden_obstacle.py
"""
from __future__ import annotations

import contextlib
import io
import math
import os

import numpy as np

import make_golden as MG
import make_golden_clamp as MC

HERE = os.path.dirname(os.path.abspath(__file__))
CLEAR = 1.0e-4      # the suite's trajectory tolerance: a device within it agrees on every flag of such a sample


def seg_dist(cx, cy, bx, by, ux, uy, L):
    """Distance from (cx, cy) to the segment from (bx, by) along the unit vector (ux, uy), length L; and whether
    the projection parameter was clipped."""
    px, py = cx - bx, cy - by
    s = px * ux + py * uy
    t = min(max(s, 0.0), L)
    return math.hypot(px - t * ux, py - t * uy), t != s


def link_dists(l1, l2, q1, q2, discs):
    """[(d link 1, clipped, d link 2, clipped)] per disc for the pose (q1, q2)."""
    c1, s1, c12, s12 = math.cos(q1), math.sin(q1), math.cos(q1 + q2), math.sin(q1 + q2)
    out = []
    for cx, cy, _ in discs:
        d1, k1 = seg_dist(cx, cy, 0.0, 0.0, c1, s1, l1)
        d2, k2 = seg_dist(cx, cy, l1 * c1, l1 * s1, c12, s12, l2)
        out.append((d1, k1, d2, k2))
    return out


def obstructed_class(base, discs, w, rec):
    """`base` with only _c and _phi overridden; every evaluation is recorded in rec["calls"] as
    (kind, flag, clearance, per-disc (d1, clipped1, d2, clipped2), end effector)."""
    discs = [tuple(map(float, d)) for d in np.asarray(discs, np.float64).reshape(-1, 3)]
    rec["calls"] = []

    class Obstructed(base):
        def _collides(self, x, kind):
            q1, q2 = float(x[0]), float(x[1])
            ds = link_dists(self.l1, self.l2, q1, q2, discs)
            flag = any(d1 < r or d2 < r for (d1, _, d2, _), (_, _, r) in zip(ds, discs))
            clear = min([abs(d - r) for (d1, _, d2, _), (_, _, r) in zip(ds, discs) for d in (d1, d2)], default=math.inf)
            ee = (self.l1 * math.cos(q1) + self.l2 * math.cos(q1 + q2), self.l1 * math.sin(q1) + self.l2 * math.sin(q1 + q2))
            rec["calls"].append((kind, flag, clear, ds, ee))
            return 1.0 if flag else 0.0

        def _c(self, x_t):
            return super()._c(x_t) + w * self._collides(x_t, 0)

        def _phi(self, x_T):
            return super()._phi(x_T) + w * self._collides(x_T, 1)

    return Obstructed


def unpack(rec, K, T, discs):
    """flag (K, T) bool, clear (K, T), hit (K, T, n, 2) bool, clipped (K, T, n, 2) bool, ee (K, T, 2) of the K * T
    stage evaluations (sample-major, as the reference's loops call _c), and the terminal flags (K,)."""
    calls = rec["calls"]
    stage = [c for c in calls if c[0] == 0][-K * T:]
    term = [c for c in calls if c[0] == 1][-K:]
    n = len(np.asarray(discs).reshape(-1, 3))
    r = np.asarray(discs, np.float64).reshape(-1, 3)[:, 2]
    flag = np.array([c[1] for c in stage], dtype=bool).reshape(K, T)
    clear = np.array([c[2] for c in stage], dtype=np.float64).reshape(K, T)
    d = np.array([[(x[0], x[2]) for x in c[3]] for c in stage], dtype=np.float64).reshape(K, T, n, 2)
    clipped = np.array([[(x[1], x[3]) for x in c[3]] for c in stage], dtype=bool).reshape(K, T, n, 2)
    ee = np.array([c[4] for c in stage], dtype=np.float64).reshape(K, T, 2)
    tflag = np.array([c[1] for c in term], dtype=bool)
    assert np.array_equal(tflag, flag[:, -1]), "the terminal state is the last stage state"
    return flag, clear, d < r[None, None, :, None], clipped, ee, tflag


def layout(ee_best_final, r_link1=0.02):
    """The discs of a case from its unobstructed run's best sample's final end-effector position; r_link1: the
    radius of the disc beside link 1 (a longer horizon sweeps further into it)."""
    return np.array([[ee_best_final[0] + 0.002, ee_best_final[1] + 0.002, 0.006],
                     [0.2900, 0.7466, r_link1],
                     [1.3538, 0.7419, 0.015],
                     [-1.5, -1.5, 0.1]])


def check(name, S, S0, flag, clear, hit, clipped, one_hot):
    """The conditions every fixture must meet to mean something."""
    share = float(np.mean(flag.any(1)))
    assert 0.10 <= share <= 0.90, f"{name}: {share:.1%} of the samples collide at least once (want 10-90 %)"
    assert hit[..., 0].any() and hit[..., 1].any(), f"{name}: both links must touch a disc somewhere"
    assert (hit & clipped).any() and (hit & ~clipped).any(), f"{name}: a clipped and an unclipped projection must hit"
    far = float(np.mean(clear.min(1) >= CLEAR))
    assert far >= 0.80, f"{name}: only {far:.1%} of the samples keep {CLEAR} m from every boundary on every step"
    order = np.argsort(S)
    gap = float((S[order[1]] - S[order[0]]) / abs(S[order[0]]))
    if one_hot:
        k0 = int(np.argmin(S0))
        assert flag[k0].any(), f"{name}: the unobstructed argmin {k0} does not collide: the discs change nothing"
        assert int(order[0]) != k0, f"{name}: the argmin did not move"
        assert clear[order[:2]].min() >= CLEAR, f"{name}: the two best samples come within {CLEAR} m of a boundary"
        assert gap >= 1e-3, f"{name}: the two smallest costs differ by {gap:.1e} relative (argmin not meaningful)"
    return share, far, gap


def run_once(cls, ref_path, K, T, seed, vis, kw, x0=None):
    mppi = cls(delta_t=0.006, ref_path=ref_path, horizon_step_T=T, number_of_samples_K=K,
               visualize_optimal_traj=vis, visualze_sampled_trajs=False, **kw)
    u_before = mppi.u_prev.copy()
    rec = {}
    MG._instrument(mppi, rec)
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        u0, u_seq, opt, _ = mppi.calc_control_input(observed_x=MG.X0.copy() if x0 is None else x0)
    return mppi, rec, u_before, np.array(u0), np.array(u_seq), np.array(opt)


def one_step(control, name, ref_path, K, T, seed, w, one_hot, lo=None, hi=None, r_link1=0.02, **over):
    kw = dict(MG.RUNPY)
    kw.update(over)
    base = control.MPPIControllerForPathTracking if lo is None else MC.clamped_class(control, lo, hi)
    # the unobstructed run places the discs: the same class with no discs records the end effector
    r0 = {}
    _, rec0, _, _, _, _ = run_once(obstructed_class(base, np.zeros((0, 3)), 0.0, r0), ref_path, K, T, seed, True, kw)
    _, _, _, _, ee0, _ = unpack(r0, K, T, np.zeros((0, 3)))
    S0 = rec0["S"]
    discs = layout(ee0[int(np.argmin(S0)), -1], r_link1)
    r1 = {}
    mppi, rec, u_before, u0, u_seq, opt = run_once(obstructed_class(base, discs, w, r1), ref_path, K, T, seed, True, kw)
    flag, clear, hit, clipped, ee, _ = unpack(r1, K, T, discs)
    assert np.array_equal(rec["eps"], rec0["eps"])
    share, far, gap = check(name, rec["S"], S0, flag, clear, hit, clipped, one_hot)
    out = dict(
        path=np.array("xydq_circle"), K=np.int64(K), T=np.int64(T), seed=np.int64(seed),
        delta_t=np.float64(0.006), x0=MG.X0.copy(), prev_idx=np.int64(0),
        u_prev=u_before, param_exploration=np.float64(kw["param_exploration"]),
        param_lambda=np.float64(kw["param_lambda"]), param_alpha=np.float64(kw["param_alpha"]),
        sigma=np.asarray(kw["sigma"], np.float64),
        stage_cost_weight=np.asarray(kw["stage_cost_weight"], np.float64),
        terminal_cost_weight=np.asarray(kw["terminal_cost_weight"], np.float64),
        sampled=np.bool_(False), visualize_optimal_traj=np.bool_(True),
        obstacles=discs, obstacle_cost=np.float64(w), one_hot=np.bool_(one_hot),
        eps=rec["eps"], S=rec["S"], S_free=S0, w=rec["w"], w_eps_raw=rec["w_eps_raw"],
        w_eps_filt=rec["w_eps_filt"], u_new=u_before + rec["w_eps_filt"],
        u0=u0, u_seq=u_seq, optimal_traj=opt, prev_idx_after=np.int64(mppi.prev_waypoints_idx),
        flag=flag, clearance=clear,
    )
    if lo is not None:
        out["u_min"] = np.broadcast_to(np.asarray(lo, np.float64), (2,)).copy()
        out["u_max"] = np.broadcast_to(np.asarray(hi, np.float64), (2,)).copy()
    np.savez_compressed(os.path.join(HERE, f"obst_step_{name}.npz"), **out)
    print(f"obst_step_{name}: K={K} T={T} argmin {int(np.argmin(S0))} -> {int(np.argmin(rec['S']))}, {share:.0%} collide, "
          f"max hits {int((flag.sum(1) + flag[:, -1]).max())}, {far:.0%} keep {CLEAR} m, S gap {gap:.1e}, "
          f"min clearance {clear.min():.1e}")


def closed_loop(control, utils, name, ref_path, K, T, seed, ticks, w):
    """run.py:48-71 for `ticks` ticks with a disc the unobstructed loop's planned arm passes through."""
    def loop(discs, w=w):
        r = {}
        mppi = obstructed_class(control.MPPIControllerForPathTracking, discs, w, r)(
            delta_t=MG.DT_PLANT * 2, ref_path=ref_path, horizon_step_T=T, number_of_samples_K=K,
            visualze_sampled_trajs=False, **MG.RUNPY)
        rec = {}
        MG._instrument(mppi, rec)
        q, dq = MG.X0[:2].copy(), MG.X0[2:].copy()
        state = [q[0], q[1], dq[0], dq[1]]
        np.random.seed(seed)
        res = dict(states=[], u=[], u_seq=[], prev_idx=[], eps=[], S=[], flag=[], clearance=[], pose=[])
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(ticks):
                res["states"].append(np.array(state, dtype=np.float64))
                u, u_seq, _, _ = mppi.calc_control_input(observed_x=state)
                flag, clear, _, _, ee, _ = unpack(r, K, T, discs)
                res.setdefault("ee_best", []).append(ee[int(np.argmin(rec["S"])), -1])
                res["eps"].append(rec["eps"])
                res["S"].append(rec["S"])
                res["flag"].append(flag)
                res["clearance"].append(clear)
                res["u"].append(np.array(u))
                res["u_seq"].append(np.array(u_seq))
                res["prev_idx"].append(mppi.prev_waypoints_idx)
                dq += MG.DT_PLANT * utils.Arm_Dynamic(q, dq, u)
                q += MG.DT_PLANT * dq
                state = np.concatenate((q, dq))
                res["pose"].append(q.copy())
        res["final_state"] = np.array(state)
        return res

    # From rest the plant moves a fraction of a millimetre in ten ticks, so the arm itself cannot reach anything
    # it does not already touch; what passes through the disc is the arm as the unobstructed loop plans it.  The
    # disc (radius 6 mm) sits 2 mm off the final end-effector position of the first tick's best sample, as in the
    # step fixtures, so the loop has to plan around it from its first tick on.
    free = loop(np.zeros((0, 3)), 0.0)
    e = free["ee_best"][0]
    # ... and a disc of radius 10 mm whose boundary lies 12 mm ahead of link 1's interior (0.8 along the link at
    # the start pose, on the side q1 moves to), which the samples' link 1 sweeps into late in the horizon
    th = MG.X0[0]
    c = 0.8 * np.array([math.cos(th), math.sin(th)]) + (0.012 + 0.01) * np.array([-math.sin(th), math.cos(th)])
    discs = np.array([[e[0] + 0.002, e[1] + 0.002, 0.006], [c[0], c[1], 0.01], [-1.5, -1.5, 0.1]])
    probe = loop(discs, 0.0)     # w = 0: the unobstructed loop again, with the flags of its own samples
    through = [bool(f[int(np.argmin(S))].any()) for f, S in zip(probe["flag"], probe["S"])]
    assert through[0], f"{name}: the unobstructed loop's first best sample misses the disc: {through}"
    got = loop(discs)
    flags = np.array(got["flag"])
    share = [float(f.any(1).mean()) for f in flags]
    assert 0.10 <= np.mean(flags.any(2)) <= 0.90, f"{name}: {np.mean(flags.any(2)):.1%} of the samples collide"
    assert not np.allclose(np.array(got["u"]), np.array(free["u"])), f"{name}: the discs change no control"
    far_t = np.mean(np.array(got["clearance"]).min(2) >= CLEAR, axis=1)
    far = float(np.mean(far_t))
    assert far_t.min() >= 0.80, f"{name}: a tick has only {far_t.min():.1%} of its samples {CLEAR} m from every boundary"
    # The loop closes around the discs: nearly every sample of the first tick runs into one, the update steers away,
    # and from the third tick on only the few samples that stray still touch.  Per tick, then: at least two ticks
    # in which 10-95 % collide, at least five in which something does, and at least eight whose two best samples
    # are 1e-3 apart and clear of every boundary (the ticks a test compares the argmin and the controls on).
    assert sum(0.10 <= s <= 0.95 for s in share) >= 2 and sum(s > 0 for s in share) >= 5, f"{name}: shares {share}"
    decided = 0
    for S, cl in zip(got["S"], got["clearance"]):
        o = np.argsort(S)
        decided += bool((S[o[1]] - S[o[0]]) >= 1e-3 * abs(S[o[0]]) and cl[o[:2]].min() >= CLEAR)
    assert decided >= 8, f"{name}: only {decided} ticks have a decided argmin"
    np.savez_compressed(
        os.path.join(HERE, f"obst_loop_{name}.npz"), K=np.int64(K), T=np.int64(T),
        seed=np.int64(seed), ticks=np.int64(ticks), states=np.array(got["states"]),
        u=np.array(got["u"]), u_seq=np.array(got["u_seq"]), prev_idx=np.array(got["prev_idx"], dtype=np.int64),
        eps=np.array(got["eps"]), S=np.array(got["S"]), final_state=got["final_state"], flag=flags,
        clearance=np.array(got["clearance"]), obstacles=discs, obstacle_cost=np.float64(w),
        u_free=np.array(free["u"]), visualize_optimal_traj=np.bool_(True))
    print(f"obst_loop_{name}: ticks={ticks} collide share per tick {['%.2f' % s for s in share]}, "
          f"{far:.0%} keep {CLEAR} m, final={got['final_state']}")


def main():
    control, utils = MG._import_reference()
    circle = np.loadtxt(os.path.join(MG.REF, "xydq_circle.txt"))[:, 0:4]
    # one-hot weights (run.py's lambda): the obstacle moves the argmin
    one_step(control, "a_k128_t20", circle, 128, 20, 21, 1.0e10, True)
    # dense weights with a live gamma term (clamp_step_c's lambda and alpha); w of the order of lambda, so a
    # collision moves a weight instead of zeroing it
    one_step(control, "b_dense_k256_t24", circle, 256, 24, 22, 5.0e6, False, r_link1=0.01, param_lambda=5.0e6, param_alpha=0.9)
    # exploration split (control.py:98-101)
    one_step(control, "c_expl_k128_t20", circle, 128, 20, 23, 1.0e10, True, param_exploration=0.25)
    # with torque limits as well (_g clipping in place, as the clamp fixtures)
    one_step(control, "d_clamp_k128_t20", circle, 128, 20, 21, 1.0e10, True, lo=(4.0, -6.0), hi=(14.0, 2.0))
    closed_loop(control, utils, "k64_t20", circle, 64, 20, 26, 10, 1.0e10)


if __name__ == "__main__":
    main()
