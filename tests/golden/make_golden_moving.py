"""Generate the moving-obstacle fixtures (``move_step_*.npz``, ``move_loop_*.npz``) from the imported reference.

Run ONCE where the reference checkout exists, like ``make_golden_obstacle.py``, whose import shim, disc layout,
recording format and ``check`` this reuses.  The controller is subclassed and ONLY ``_c`` and ``_phi`` are
overridden, to return ``super() + w * collides(x, discs at this evaluation's time)``.  A disc is (cx, cy, r) plus a
velocity (vx, vy) in m/s, constant over the horizon; its position is the one at the observed state.  The evaluation
time comes from a call counter: ``calc_control_input`` calls ``_c`` T times and then ``_phi`` once per sample, in
order, and the optimal and sampled re-rolls call only ``_F``; so the j-th ``_c`` of a sample sees its state at time
(j + 1) delta_t, j = 0 .. T - 1, and ``_phi`` the final state at T delta_t, the centres of step T - 1.

Only outputs are stored.  Every case asserts ``make_golden_obstacle.check``'s conditions and two that make the motion
matter: at least 50 % of the samples have a hit count different from the same discs at rest, and at least 10 % one
different from the off-by-one definition c + v t delta_t.

Usage:  python tests/golden/make_golden_moving.py
"""
from __future__ import annotations

import contextlib
import io
import math
import os

import numpy as np

import make_golden as MG
import make_golden_clamp as MC
import make_golden_obstacle as MO

HERE = os.path.dirname(os.path.abspath(__file__))
# m/s, one row per disc of make_golden_obstacle.layout: the disc by the best sample's final end effector, the one
# link 1 sweeps into, the one ahead of the end effector, and the far one (at rest)
VEL = np.array([[0.15, -0.10], [-0.05, 0.03], [0.20, 0.10], [0.0, 0.0]])


def moving_class(base, world, w, dt, T, rec, shift=0):
    """`base` with only _c and _phi overridden.  world: dict(discs (n, 3), vel (n, 2)), read at every evaluation
    (a closed loop advances world["discs"] between ticks).  Every evaluation is recorded in rec["calls"] in
    make_golden_obstacle's format.  shift: whole steps added to the evaluation time (-1: the off-by-one definition)."""
    rec["calls"] = []
    count = {"c": 0}

    class Moving(base):
        def _collides(self, x, kind, step):
            tau = (step + 1 + shift) * dt
            discs = [(float(cx + vx * tau), float(cy + vy * tau), float(r))
                     for (cx, cy, r), (vx, vy) in zip(world["discs"], world["vel"])]
            q1, q2 = float(x[0]), float(x[1])
            ds = MO.link_dists(self.l1, self.l2, q1, q2, discs)
            flag = any(d1 < r or d2 < r for (d1, _, d2, _), (_, _, r) in zip(ds, discs))
            clear = min([abs(d - r) for (d1, _, d2, _), (_, _, r) in zip(ds, discs) for d in (d1, d2)], default=math.inf)
            ee = (self.l1 * math.cos(q1) + self.l2 * math.cos(q1 + q2), self.l1 * math.sin(q1) + self.l2 * math.sin(q1 + q2))
            rec["calls"].append((kind, flag, clear, ds, ee))
            return 1.0 if flag else 0.0

        def _c(self, x_t):
            step = count["c"] % T            # the j-th _c of this sample
            count["c"] += 1
            return super()._c(x_t) + w * self._collides(x_t, 0, step)

        def _phi(self, x_T):
            assert count["c"] % T == 0, "_phi follows a sample's T calls of _c"
            return super()._phi(x_T) + w * self._collides(x_T, 1, T - 1)

    return Moving


def check(name, S, flag, clear, hit, clipped, one_hot):
    """make_golden_obstacle.check's conditions on the samples themselves (its two on the unobstructed argmin are
    printed, not asserted: a disc that moves need not be where that sample ends)."""
    share = float(np.mean(flag.any(1)))
    assert 0.10 <= share <= 0.90, f"{name}: {share:.1%} of the samples collide at least once (want 10-90 %)"
    assert hit[..., 0].any() and hit[..., 1].any(), f"{name}: both links must touch a disc somewhere"
    assert (hit & clipped).any() and (hit & ~clipped).any(), f"{name}: a clipped and an unclipped projection must hit"
    far = float(np.mean(clear.min(1) >= MO.CLEAR))
    assert far >= 0.80, f"{name}: only {far:.1%} of the samples keep {MO.CLEAR} m from every boundary on every step"
    order = np.argsort(S)
    gap = float((S[order[1]] - S[order[0]]) / abs(S[order[0]]))
    if one_hot:
        assert clear[order[:2]].min() >= MO.CLEAR, f"{name}: the two best samples come within {MO.CLEAR} m of a boundary"
        assert gap >= 1e-3, f"{name}: the two smallest costs differ by {gap:.1e} relative (argmin not meaningful)"
    return share, far, gap


def motion_matters(name, hits, hits_rest, hits_off):
    a, b = float(np.mean(hits != hits_rest)), float(np.mean(hits != hits_off))
    assert a >= 0.50, f"{name}: only {a:.1%} of the samples have a hit count different from the discs at rest"
    assert b >= 0.10, f"{name}: only {b:.1%} of the samples have a hit count different from the off-by-one definition"
    return a, b


def one_step(control, name, ref_path, K, T, seed, w, one_hot, lo=None, hi=None, r_link1=0.02, vel=VEL, **over):
    kw = dict(MG.RUNPY)
    kw.update(over)
    dt = 0.006
    base = control.MPPIControllerForPathTracking if lo is None else MC.clamped_class(control, lo, hi)
    r0 = {}
    _, rec0, _, _, _, _ = MO.run_once(MO.obstructed_class(base, np.zeros((0, 3)), 0.0, r0), ref_path, K, T, seed, True, kw)
    _, _, _, _, ee0, _ = MO.unpack(r0, K, T, np.zeros((0, 3)))
    S0 = rec0["S"]
    discs = MO.layout(ee0[int(np.argmin(S0)), -1], r_link1)

    def run(vel, shift=0):
        r = {}
        cls = moving_class(base, dict(discs=discs, vel=vel), w, dt, T, r, shift)
        mppi, rec, u_before, u0, u_seq, opt = MO.run_once(cls, ref_path, K, T, seed, True, kw)
        return (mppi, rec, u_before, u0, u_seq, opt) + MO.unpack(r, K, T, discs)

    mppi, rec, u_before, u0, u_seq, opt, flag, clear, hit, clipped, ee, _ = run(vel)
    assert np.array_equal(rec["eps"], rec0["eps"])
    share, far, gap = check(name, rec["S"], flag, clear, hit, clipped, one_hot)
    hits = flag.sum(1) + flag[:, -1]
    f_rest, f_off = run(np.zeros_like(vel))[6], run(vel, shift=-1)[6]
    a, b = motion_matters(name, hits, f_rest.sum(1) + f_rest[:, -1], f_off.sum(1) + f_off[:, -1])
    out = dict(
        path=np.array("xydq_circle"), K=np.int64(K), T=np.int64(T), seed=np.int64(seed),
        delta_t=np.float64(dt), x0=MG.X0.copy(), prev_idx=np.int64(0),
        u_prev=u_before, param_exploration=np.float64(kw["param_exploration"]),
        param_lambda=np.float64(kw["param_lambda"]), param_alpha=np.float64(kw["param_alpha"]),
        sigma=np.asarray(kw["sigma"], np.float64),
        stage_cost_weight=np.asarray(kw["stage_cost_weight"], np.float64),
        terminal_cost_weight=np.asarray(kw["terminal_cost_weight"], np.float64),
        sampled=np.bool_(False), visualize_optimal_traj=np.bool_(True),
        obstacles=discs, obstacle_velocities=np.array(vel), obstacle_cost=np.float64(w), one_hot=np.bool_(one_hot),
        eps=rec["eps"], S=rec["S"], S_free=S0, w=rec["w"], w_eps_raw=rec["w_eps_raw"],
        w_eps_filt=rec["w_eps_filt"], u_new=u_before + rec["w_eps_filt"],
        u0=u0, u_seq=u_seq, optimal_traj=opt, prev_idx_after=np.int64(mppi.prev_waypoints_idx),
        flag=flag, clearance=clear, hits_rest=f_rest.sum(1) + f_rest[:, -1], hits_off=f_off.sum(1) + f_off[:, -1],
    )
    if lo is not None:
        out["u_min"] = np.broadcast_to(np.asarray(lo, np.float64), (2,)).copy()
        out["u_max"] = np.broadcast_to(np.asarray(hi, np.float64), (2,)).copy()
    np.savez_compressed(os.path.join(HERE, f"move_step_{name}.npz"), **out)
    print(f"move_step_{name}: K={K} T={T} argmin {int(np.argmin(S0))} -> {int(np.argmin(rec['S']))}, {share:.0%} collide, "
          f"{far:.0%} keep {MO.CLEAR} m, S gap {gap:.1e}, min clearance {clear.min():.1e}, "
          f"hits differ from rest {a:.0%}, from off-by-one {b:.0%}")


def closed_loop(control, utils, name, ref_path, K, T, seed, ticks, w, vel=None):
    """run.py:48-71 for `ticks` ticks; between ticks the generator advances the discs by v * (the plant's step)."""
    dt = MG.DT_PLANT * 2

    def loop(discs0, vel, w=w, shift=0):
        r = {}
        world = dict(discs=np.array(discs0, dtype=np.float64), vel=np.array(vel, dtype=np.float64))
        mppi = moving_class(control.MPPIControllerForPathTracking, world, w, dt, T, r, shift)(
            delta_t=dt, ref_path=ref_path, horizon_step_T=T, number_of_samples_K=K,
            visualze_sampled_trajs=False, **MG.RUNPY)
        rec = {}
        MG._instrument(mppi, rec)
        q, dq = MG.X0[:2].copy(), MG.X0[2:].copy()
        state = [q[0], q[1], dq[0], dq[1]]
        np.random.seed(seed)
        res = dict(states=[], u=[], u_seq=[], prev_idx=[], eps=[], S=[], flag=[], clearance=[], discs=[], ee_best=[])
        with contextlib.redirect_stdout(io.StringIO()):
            for _ in range(ticks):
                res["states"].append(np.array(state, dtype=np.float64))
                res["discs"].append(world["discs"].copy())
                u, u_seq, _, _ = mppi.calc_control_input(observed_x=state)
                flag, clear, _, _, ee, _ = MO.unpack(r, K, T, world["discs"])
                res["ee_best"].append(ee[int(np.argmin(rec["S"])), -1])
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
                world["discs"][:, :2] += world["vel"] * MG.DT_PLANT     # the world moves on by one control period
        res["final_state"] = np.array(state)
        return res

    free = loop(np.zeros((0, 3)), np.zeros((0, 2)), 0.0)
    e = free["ee_best"][0]
    th = MG.X0[0]
    c = 0.8 * np.array([math.cos(th), math.sin(th)]) + (0.012 + 0.01) * np.array([-math.sin(th), math.cos(th)])
    vel = np.array(VEL[[0, 1, 3]] if vel is None else vel)
    # make_golden_obstacle's closed-loop discs, the first one set back so that it arrives 2 mm off the final
    # end-effector position of the first tick's unobstructed best sample when that sample does (at T dt)
    discs = np.array([[e[0] + 0.002, e[1] + 0.002, 0.006], [c[0], c[1], 0.01], [-1.5, -1.5, 0.1]])
    discs[0, :2] -= vel[0] * T * dt
    got = loop(discs, vel)
    flags = np.array(got["flag"])
    share = [float(f.any(1).mean()) for f in flags]
    assert 0.10 <= np.mean(flags.any(2)) <= 0.90, f"{name}: {np.mean(flags.any(2)):.1%} of the samples collide"
    assert not np.allclose(np.array(got["u"]), np.array(free["u"])), f"{name}: the discs change no control"
    far_t = np.mean(np.array(got["clearance"]).min(2) >= MO.CLEAR, axis=1)
    assert far_t.min() >= 0.80, f"{name}: a tick has only {far_t.min():.1%} of its samples {MO.CLEAR} m from every boundary"
    # the motion matters on the first tick's samples (later ticks run from other states in the other loops)
    hits = flags[0].sum(1) + flags[0][:, -1]
    rest, off = loop(discs, np.zeros_like(vel))["flag"][0], loop(discs, vel, shift=-1)["flag"][0]
    a, b = motion_matters(name, hits, rest.sum(1) + rest[:, -1], off.sum(1) + off[:, -1])
    np.savez_compressed(
        os.path.join(HERE, f"move_loop_{name}.npz"), K=np.int64(K), T=np.int64(T),
        seed=np.int64(seed), ticks=np.int64(ticks), states=np.array(got["states"]),
        u=np.array(got["u"]), u_seq=np.array(got["u_seq"]), prev_idx=np.array(got["prev_idx"], dtype=np.int64),
        eps=np.array(got["eps"]), S=np.array(got["S"]), final_state=got["final_state"], flag=flags,
        clearance=np.array(got["clearance"]), obstacles=np.array(got["discs"]), obstacle_velocities=vel,
        obstacle_cost=np.float64(w), u_free=np.array(free["u"]), visualize_optimal_traj=np.bool_(True))
    print(f"move_loop_{name}: ticks={ticks} collide share per tick {['%.2f' % s for s in share]}, "
          f"{float(np.mean(far_t)):.0%} keep {MO.CLEAR} m, hits differ from rest {a:.0%}, from off-by-one {b:.0%}")


def main():
    control, utils = MG._import_reference()
    circle = np.loadtxt(os.path.join(MG.REF, "xydq_circle.txt"))[:, 0:4]
    one_step(control, "a_k128_t20", circle, 128, 20, 21, 1.0e10, True)                      # one-hot weights
    one_step(control, "b_dense_k256_t24", circle, 256, 24, 22, 5.0e6, False, r_link1=0.01,   # obst_step_b's lambda, alpha
             param_lambda=5.0e6, param_alpha=0.9)
    # (the exploring quarter of the samples scatters wide of the discs: faster discs, so the step index still matters)
    one_step(control, "c_expl_k128_t20", circle, 128, 20, 23, 1.0e10, True, vel=1.25 * VEL, param_exploration=0.25)
    one_step(control, "d_clamp_k128_t20", circle, 128, 20, 21, 1.0e10, True, lo=(4.0, -6.0), hi=(14.0, 2.0))
    closed_loop(control, utils, "k64_t20", circle, 64, 20, 26, 10, 1.0e10)


if __name__ == "__main__":
    main()
