"""Generate the asymmetric-parameter fixtures (``asym_step_*.npz``, ``asym_loop_*.npz``) from the imported reference.

Run ONCE where the reference checkout exists, like ``make_golden.py`` (whose import shim and instrumentation this
reuses), ``make_golden_clamp.py`` (the ``_g`` override) and ``make_golden_obstacle.py`` (the ``_c`` / ``_phi``
override).  Every other fixture runs the reference at its one shipped parameter point, which is symmetric:
``m1 = m2``, ``l1 = l2``, ``lc1 = lc2``, ``self.l1 = self.l2``, cost weights with equal halves, one ``delta_t``.
Here the reference's dynamics constants, which it reads from module-level names (control.py:11-18, utils.py:4-11),
are assigned after the import, and the cost's kinematics lengths (control.py:55-56) on the instance; nothing else
changes.  Only outputs are stored, with the constants that produced them; no reference text is copied.

Two parameter sets (``SET_A``, ``SET_B``).  Each meets the conditioning rule the tests assert: over q2 the minimum of
det M / (M11 M22) is no smaller than the shipped arm's, so the fp32 tolerances of the suite apply unchanged.

Usage:  python tests/golden/make_golden_asym.py
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
ARM_FIELDS = ("m1", "m2", "l1", "l2", "lc1", "lc2", "g", "fk_l1", "fk_l2")

# every constant distinct from every other; fk_l1, fk_l2, l1, l2 all different
ARM_A = dict(m1=1.3, m2=0.7, l1=1.05, l2=0.8, lc1=0.6, lc2=0.35, g=9.81, fk_l1=1.1, fk_l2=0.9)
SET_A = dict(arm=ARM_A, delta_t=0.004, param_exploration=0.1, param_lambda=100.0, param_alpha=0.98,
             sigma=np.array([[20.0, 6.0], [6.0, 12.0]]), stage_cost_weight=np.array([0.4, 0.7, 3.0, 6.0]),
             terminal_cost_weight=np.array([4.0, 7.0, 30.0, 60.0]))
# the heavier link is the distal one, its centre of mass further out
ARM_B = dict(m1=0.8, m2=1.1, l1=1.2, l2=0.7, lc1=0.3, lc2=0.4, g=9.7, fk_l1=1.25, fk_l2=0.75)
SET_B = dict(arm=ARM_B, delta_t=0.008, param_exploration=0.25, param_lambda=3.0e6, param_alpha=0.9,
             sigma=np.array([[15.0, -4.0], [-4.0, 25.0]]), stage_cost_weight=np.array([0.6, 0.3, 7.0, 4.0]),
             terminal_cost_weight=np.array([6.0, 3.0, 70.0, 40.0]))


def override(control, utils, arm):
    """The reference's module-level dynamics constants (controller and plant) := arm's."""
    for mod in (control, utils):
        for f in ("m1", "m2", "l1", "l2", "lc1", "lc2", "g"):
            setattr(mod, f, arm[f])


def ik(x, y, a, b, elbow_up):
    """Joint angles that put the end of links (a, b) at (x, y); elbow_up: q2 > 0."""
    c2 = (x * x + y * y - a * a - b * b) / (2.0 * a * b)
    q2 = math.acos(c2) * (1.0 if elbow_up else -1.0)
    return np.array([math.atan2(y, x) - math.atan2(b * math.sin(q2), a + b * math.cos(q2)), q2])


def gravity_hold(q, arm):
    """The torques that hold the arm still at q: G of control.py:248-250."""
    c1, c12 = math.cos(q[0]), math.cos(q[0] + q[1])
    return np.array([arm["m1"] * arm["lc1"] * arm["g"] * c1 + arm["m2"] * arm["g"] * (arm["lc2"] * c12 + arm["l1"] * c1),
                     arm["m2"] * arm["lc2"] * arm["g"] * c12])


def start_pose(ref_path, idx, off, rate_off, arm, elbow_up):
    """The pose whose end effector (the cost's kinematics) is `off` metres from waypoint idx, at the path's joint
    rates there plus `rate_off`."""
    q = ik(ref_path[idx, 0] + off[0], ref_path[idx, 1] + off[1], arm["fk_l1"], arm["fk_l2"], elbow_up)
    return np.concatenate([q, ref_path[idx, 2:4] + np.asarray(rate_off)])


def make(control, base, P, ref_path, K, T, vis, sampled):
    mppi = base(delta_t=P["delta_t"], ref_path=ref_path, horizon_step_T=T, number_of_samples_K=K,
                visualize_optimal_traj=vis, visualze_sampled_trajs=sampled,
                **{k: P[k] for k in ("param_exploration", "param_lambda", "param_alpha", "sigma", "stage_cost_weight",
                                     "terminal_cost_weight")})
    mppi.l1, mppi.l2 = P["arm"]["fk_l1"], P["arm"]["fk_l2"]
    return mppi


def run_once(control, base, P, ref_path, K, T, seed, x0, prev_idx, u_prev, vis=True, sampled=False):
    mppi = make(control, base, P, ref_path, K, T, vis, sampled)
    mppi.prev_waypoints_idx = prev_idx
    mppi.u_prev = np.array(u_prev, dtype=np.float64).copy()
    rec = {}
    MG._instrument(mppi, rec)
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        u0, u_seq, opt, samp = mppi.calc_control_input(observed_x=np.array(x0, dtype=np.float64))
    return mppi, rec, np.array(u0), np.array(u_seq), np.array(opt), np.array(samp)


def separating_discs(states, arm):
    """Two discs that tell the two link lengths apart, from the unobstructed run's final states (K, 4): one beside
    link 1's last 5 cm (2.5 cm short of the elbow, on the side away from link 2), which the samples whose link 1
    turned furthest that way touch and a link 1 as short as link 2 cannot; one 3 cm past link 2's tip along it,
    which only a link 2 as long as link 1 would reach."""
    a, b = arm["fk_l1"], arm["fk_l2"]
    q1, q2 = states[:, 0], states[:, 1]
    side = 1.0 if np.median(q2) < 0 else -1.0
    th = float(np.quantile(q1, 0.6 if side > 0 else 0.4))
    d = a - 0.025
    r1 = max(4.0 * d * float(np.std(q1)), 1e-4)
    c1 = d * np.array([math.cos(th), math.sin(th)]) + side * r1 * np.array([-math.sin(th), math.cos(th)])
    m1, m12 = float(np.median(q1)), float(np.median(q1 + q2))
    tip = a * np.array([math.cos(m1), math.sin(m1)]) + (b + 0.03) * np.array([math.cos(m12), math.sin(m12)])
    return np.array([[c1[0], c1[1], r1], [tip[0], tip[1], 0.015]])


def one_step(control, utils, name, P, ref_path, K, T, seed, x0, prev_idx, lo=None, hi=None, discs_w=None,
             sampled=False, sampled_every=1):
    arm = P["arm"]
    override(control, utils, arm)
    u_prev = np.tile(np.round(gravity_hold(x0[:2], arm), 2), (T, 1))
    base = control.MPPIControllerForPathTracking if lo is None else MC.clamped_class(control, lo, hi)
    out = {}
    if discs_w is not None:
        # the unobstructed run places the discs: the same class with no discs records every state it costs
        states = []

        class Recording(base):
            def _c(self, x_t):
                states.append(np.array(x_t, dtype=np.float64))
                return super()._c(x_t)

        _, rec0, *_ = run_once(control, Recording, P, ref_path, K, T, seed, x0, prev_idx, u_prev)
        final = np.array(states[-K * T:]).reshape(K, T, 4)[:, -1]
        discs = separating_discs(final, arm)
        r1 = {}
        base = MO.obstructed_class(base, discs, discs_w, r1)
    mppi, rec, u0, u_seq, opt, samp = run_once(control, base, P, ref_path, K, T, seed, x0, prev_idx, u_prev,
                                               sampled=sampled)
    if discs_w is not None:
        flag, clear, hit, clipped, ee, _ = MO.unpack(r1, K, T, discs)
        assert np.array_equal(rec["eps"], rec0["eps"])
        share, far = float(np.mean(flag.any(1))), float(np.mean(clear.min(1) >= MO.CLEAR))
        assert 0.10 <= share <= 0.90, f"{name}: {share:.1%} of the samples collide"
        assert far >= 0.80, f"{name}: only {far:.1%} of the samples keep {MO.CLEAR} m from every boundary"
        assert hit[..., 0, 0].any() and not hit[..., 1, :].any(), f"{name}: link 1 touches disc 0, nothing disc 1"
        out.update(obstacles=discs, obstacle_cost=np.float64(discs_w), S_free=rec0["S"], flag=flag, clearance=clear,
                   one_hot=np.bool_(False))
        print(f"  {share:.0%} collide, {far:.0%} keep {MO.CLEAR} m")
    s = np.sort(rec["S"])
    gap = float((s[1] - s[0]) / abs(s[0]))
    if P["param_lambda"] < 1e4:
        assert gap >= 1e-3, f"{name}: the two smallest costs differ by {gap:.1e} relative (argmin not meaningful)"
    if lo is not None:
        eps = rec["eps"].astype(np.float64)
        exploit = (np.arange(K) < (1.0 - P["param_exploration"]) * K)[:, None, None]
        v_raw = np.where(exploit, u_prev[None] + eps, eps)
        frac = float(np.mean((v_raw < lo) | (v_raw > hi)))
        assert 0.35 <= frac <= 0.65, f"{name}: {frac:.1%} of the sampled controls are clamped (want about half)"
        out.update(u_min=np.asarray(lo, np.float64), u_max=np.asarray(hi, np.float64))
        print(f"  {frac:.0%} of the sampled controls clamped")
    out.update(
        path=np.array("xydq_circle"), K=np.int64(K), T=np.int64(T), seed=np.int64(seed),
        delta_t=np.float64(P["delta_t"]), x0=np.asarray(x0, np.float64), prev_idx=np.int64(prev_idx), u_prev=u_prev,
        param_exploration=np.float64(P["param_exploration"]), param_lambda=np.float64(P["param_lambda"]),
        param_alpha=np.float64(P["param_alpha"]), sigma=np.asarray(P["sigma"], np.float64),
        stage_cost_weight=np.asarray(P["stage_cost_weight"], np.float64),
        terminal_cost_weight=np.asarray(P["terminal_cost_weight"], np.float64),
        sampled=np.bool_(sampled), visualize_optimal_traj=np.bool_(True),
        eps=rec["eps"], S=rec["S"], w=rec["w"], w_eps_raw=rec["w_eps_raw"], w_eps_filt=rec["w_eps_filt"],
        u_new=u_prev + rec["w_eps_filt"], u0=u0, u_seq=u_seq, optimal_traj=opt,
        prev_idx_after=np.int64(mppi.prev_waypoints_idx), **{f: np.float64(arm[f]) for f in ARM_FIELDS})
    if sampled:   # every sampled_every-th sample's trajectory: the file stays the size of its kind
        out["sampled_idx"] = np.arange(0, K, sampled_every, dtype=np.int64)
        out["sampled_traj"] = samp[out["sampled_idx"]]
    np.savez_compressed(os.path.join(HERE, f"asym_step_{name}.npz"), **out)
    ee = (arm["fk_l1"] * math.cos(x0[0]) + arm["fk_l2"] * math.cos(x0[0] + x0[1]),
          arm["fk_l1"] * math.sin(x0[0]) + arm["fk_l2"] * math.sin(x0[0] + x0[1]))
    print(f"asym_step_{name}: K={K} T={T} argmin={int(np.argmin(rec['S']))} prev {prev_idx}->{mppi.prev_waypoints_idx} "
          f"q2 {x0[1]:+.3f} ee ({ee[0]:.4f}, {ee[1]:.4f}) S gap {gap:.1e}")


def closed_loop(control, utils, name, P, ref_path, K, T, seed, ticks, x0, prev_idx):
    """run.py:48-71 for `ticks` ticks at the set's constants, the plant stepping at delta_t / 2 (run.py:10, 25)."""
    arm = P["arm"]
    override(control, utils, arm)
    dt_plant = P["delta_t"] / 2
    mppi = make(control, control.MPPIControllerForPathTracking, P, ref_path, K, T, True, False)
    u_init = np.tile(np.round(gravity_hold(x0[:2], arm), 2), (T, 1))
    mppi.u_prev = u_init.copy()
    mppi.prev_waypoints_idx = prev_idx
    rec = {}
    MG._instrument(mppi, rec)
    q, dq = x0[:2].copy(), x0[2:].copy()
    state = [q[0], q[1], dq[0], dq[1]]
    np.random.seed(seed)
    states, us, useqs, prevs, eps, Ss = [], [], [], [], [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(ticks):
            states.append(np.array(state, dtype=np.float64))
            u, u_seq, _, _ = mppi.calc_control_input(observed_x=state)
            eps.append(rec["eps"])
            Ss.append(rec["S"])
            us.append(np.array(u))
            useqs.append(np.array(u_seq))
            prevs.append(mppi.prev_waypoints_idx)
            dq += dt_plant * utils.Arm_Dynamic(q, dq, u)
            q += dt_plant * dq
            state = np.concatenate((q, dq))
    assert len(set(prevs)) >= 3, f"{name}: the waypoint index barely moves: {prevs}"
    np.savez_compressed(
        os.path.join(HERE, f"asym_loop_{name}.npz"), K=np.int64(K), T=np.int64(T), seed=np.int64(seed),
        prev_idx0=np.int64(prev_idx),
        ticks=np.int64(ticks), delta_t=np.float64(P["delta_t"]), dt_plant=np.float64(dt_plant), u_init=u_init,
        param_exploration=np.float64(P["param_exploration"]), param_lambda=np.float64(P["param_lambda"]),
        param_alpha=np.float64(P["param_alpha"]), sigma=np.asarray(P["sigma"], np.float64),
        stage_cost_weight=np.asarray(P["stage_cost_weight"], np.float64),
        terminal_cost_weight=np.asarray(P["terminal_cost_weight"], np.float64),
        states=np.array(states), u=np.array(us), u_seq=np.array(useqs), prev_idx=np.array(prevs, dtype=np.int64),
        eps=np.array(eps), S=np.array(Ss), final_state=np.array(state), visualize_optimal_traj=np.bool_(True),
        **{f: np.float64(arm[f]) for f in ARM_FIELDS})
    print(f"asym_loop_{name}: ticks={ticks} prev {prevs} final={state}")


def main():
    control, utils = MG._import_reference()
    circle = np.loadtxt(os.path.join(MG.REF, "xydq_circle.txt"))[:, 0:4]
    # set a, elbow-down at the path start: the end effector 2 cm and -1 cm off waypoint 0
    xa = start_pose(circle, 0, (0.02, -0.01), (0.005, -0.004), ARM_A, False)
    one_step(control, utils, "a_k128_t20", SET_A, circle, 128, 20, 31, xa, 0)
    # set b, elbow-down a fifth of the way round: dense weights, exploration, sampled trajectories
    xb = start_pose(circle, 400, (-0.05, 0.10), (-0.015, 0.025), ARM_B, False)
    one_step(control, utils, "b_dense_k256_t24", SET_B, circle, 256, 24, 32, xb, 392, sampled=True, sampled_every=4)
    # set a, elbow-up on the far side of the circle
    xc = start_pose(circle, 900, (0.013, 0.019), (-0.02, 0.015), ARM_A, True)
    one_step(control, utils, "c_elbowup_k128_t20", SET_A, circle, 128, 20, 33, xc, 893)
    # set a with torque limits distinct per joint (about half the sampled controls clipped) and two discs that
    # tell the link lengths apart
    # (joint rates of a few tenths of a rad/s: link 1 then sweeps 1 mm a step, and few samples end a step within
    # the 1e-4 m of a boundary that the tests leave to either side)
    xd = start_pose(circle, 0, (0.018, -0.011), (0.3, -0.2), ARM_A, False)
    ug = np.round(gravity_hold(xd[:2], ARM_A), 2)
    lo, hi = ug + np.array([-3.0, -2.0]), ug + np.array([3.5, 2.5])
    one_step(control, utils, "d_clamp_k128_t20", SET_A, circle, 128, 20, 34, xd, 0, lo=lo, hi=hi, discs_w=1.0e10)
    # the loop starts a fifth of the way round, where the waypoints lie 1 mm apart and the index moves every tick
    xl = start_pose(circle, 400, (0.004, -0.003), (0.02, -0.01), ARM_A, False)
    closed_loop(control, utils, "k64_t20", SET_A, circle, 64, 20, 35, 6, xl, 395)


if __name__ == "__main__":
    main()
