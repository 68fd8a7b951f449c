"""Generate the torque-limit fixtures (``clamp_step_*.npz``, ``clamp_loop_*.npz``) from the imported reference.

Run ONCE where the reference checkout exists, like ``make_golden.py`` (whose
import shim, instrumentation and run.py constants this reuses).  The reference
ships its clamp hook ``_g`` (control.py:166-172) with the two ``np.clip`` lines
commented out; here the controller is subclassed and ONLY ``_g`` is overridden,
with an in-place ``np.clip(v, lo, hi, out=v)`` — what those lines do once
enabled, per-component limits instead of the hard-coded +-0.8.  ``v[k, t-1]``
and ``u[t-1]`` are views, so the clip writes through (control.py:104, 133, 143):
the dynamics and the control cost see the clipped sample, the weights still
multiply the unclamped noise, and the optimal-trajectory loop — which runs
with ``visualize_optimal_traj`` only — clips the updated nominal.

Only outputs are stored; no reference text is copied.  Every case asserts that
it exercises the clamp (see ``check``) and fails loudly otherwise.

Usage:  python tests/golden/make_golden_clamp.py
"""
from __future__ import annotations

import contextlib
import io
import os

import numpy as np

import make_golden as MG

HERE = os.path.dirname(os.path.abspath(__file__))


def clamped_class(control, lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)

    class Clamped(control.MPPIControllerForPathTracking):
        def _g(self, v):
            np.clip(v, lo, hi, out=v)
            return v

    return Clamped


def check(name, S, v_raw, u_new_raw, u_seq, lo, hi, vis, want_visible):
    """The conditions every fixture must meet to mean something."""
    frac = float(np.mean((v_raw < lo) | (v_raw > hi)))
    assert frac >= 0.10, f"{name}: only {frac:.1%} of the sampled controls are clamped"
    s = np.sort(S)
    gap = float((s[1] - s[0]) / abs(s[0]))
    assert gap >= 1e-3, f"{name}: the two smallest costs differ by {gap:.1e} relative (argmin not meaningful)"
    out = int(np.sum((u_new_raw < lo) | (u_new_raw > hi)))
    inside = bool(np.all((u_seq >= lo) & (u_seq <= hi)))
    if vis:
        assert inside, f"{name}: the returned nominal leaves the limits"
    if want_visible:
        assert out >= 1 or inside, f"{name}: no clamp visible in the returned nominal"
    return frac, gap, out, inside


def one_step(control, name, ref_path, K, T, seed, lo, hi, vis=True, sampled=False, visible=True, **over):
    kw = dict(MG.RUNPY)
    kw.update(over)
    mppi = clamped_class(control, lo, hi)(
        delta_t=0.006, ref_path=ref_path, horizon_step_T=T, number_of_samples_K=K,
        visualize_optimal_traj=vis, visualze_sampled_trajs=sampled, **kw)
    u_before = mppi.u_prev.copy()
    rec = {}
    MG._instrument(mppi, rec)
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        u0, u_seq, opt, samp = mppi.calc_control_input(observed_x=MG.X0.copy())
    lo2, hi2 = np.broadcast_to(np.asarray(lo, np.float64), (2,)), np.broadcast_to(np.asarray(hi, np.float64), (2,))
    eps = rec["eps"].astype(np.float64)
    exploit = (np.arange(K) < (1.0 - kw["param_exploration"]) * K)[:, None, None]
    v_raw = np.where(exploit, u_before[None] + eps, eps)
    u_new_raw = u_before + rec["w_eps_filt"]
    frac, gap, n_out, inside = check(name, rec["S"], v_raw, u_new_raw, np.array(u_seq), lo2, hi2, vis, visible)
    if not vis:
        assert not inside, f"{name}: without the optimal-trajectory loop the nominal should stay unclamped here"
    out = dict(
        path=np.array("xydq_circle"), K=np.int64(K), T=np.int64(T), seed=np.int64(seed),
        delta_t=np.float64(0.006), x0=MG.X0.copy(), prev_idx=np.int64(0),
        u_prev=u_before, param_exploration=np.float64(kw["param_exploration"]),
        param_lambda=np.float64(kw["param_lambda"]), param_alpha=np.float64(kw["param_alpha"]),
        sigma=np.asarray(kw["sigma"], np.float64),
        stage_cost_weight=np.asarray(kw["stage_cost_weight"], np.float64),
        terminal_cost_weight=np.asarray(kw["terminal_cost_weight"], np.float64),
        sampled=np.bool_(sampled), visualize_optimal_traj=np.bool_(vis), u_min=lo2.copy(), u_max=hi2.copy(),
        eps=rec["eps"], S=rec["S"], w=rec["w"], w_eps_raw=rec["w_eps_raw"],
        w_eps_filt=rec["w_eps_filt"], u_new=u_new_raw,
        u0=np.array(u0), u_seq=np.array(u_seq), optimal_traj=np.array(opt),
        prev_idx_after=np.int64(mppi.prev_waypoints_idx),
    )
    if sampled:
        out["sampled_traj"] = np.array(samp)
    np.savez_compressed(os.path.join(HERE, f"clamp_step_{name}.npz"), **out)
    print(f"clamp_step_{name}: K={K} T={T} argmin={int(np.argmin(rec['S']))} clamped {frac:.0%} of v, "
          f"{n_out}/{u_new_raw.size} u_new entries outside, returned nominal inside={inside}, S gap {gap:.1e}")


def closed_loop(control, utils, name, ref_path, K, T, seed, ticks, lo, hi):
    """run.py:48-71 for `ticks` ticks with the limits on (as make_golden.closed_loop)."""
    lo2, hi2 = np.broadcast_to(np.asarray(lo, np.float64), (2,)), np.broadcast_to(np.asarray(hi, np.float64), (2,))
    mppi = clamped_class(control, lo, hi)(
        delta_t=MG.DT_PLANT * 2, ref_path=ref_path, horizon_step_T=T, number_of_samples_K=K,
        visualze_sampled_trajs=False, **MG.RUNPY)
    rec = {}
    MG._instrument(mppi, rec)
    q = MG.X0[:2].copy()
    dq = MG.X0[2:].copy()
    state = [q[0], q[1], dq[0], dq[1]]
    np.random.seed(seed)
    states, us, useqs, prevs, eps, Ss = [], [], [], [], [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for i in range(ticks):
            states.append(np.array(state, dtype=np.float64))
            u_before = mppi.u_prev.copy()
            u, u_seq, _, _ = mppi.calc_control_input(observed_x=state)
            check(f"{name} tick {i}", rec["S"], u_before[None] + rec["eps"].astype(np.float64),
                  u_before + rec["w_eps_filt"], np.array(u_seq), lo2, hi2, True, True)
            eps.append(rec["eps"])
            Ss.append(rec["S"])
            us.append(np.array(u))
            useqs.append(np.array(u_seq))
            prevs.append(mppi.prev_waypoints_idx)
            dq += MG.DT_PLANT * utils.Arm_Dynamic(q, dq, u)
            q += MG.DT_PLANT * dq
            state = np.concatenate((q, dq))
    np.savez_compressed(
        os.path.join(HERE, f"clamp_loop_{name}.npz"), K=np.int64(K), T=np.int64(T),
        seed=np.int64(seed), ticks=np.int64(ticks), states=np.array(states),
        u=np.array(us), u_seq=np.array(useqs), prev_idx=np.array(prevs, dtype=np.int64),
        eps=np.array(eps), S=np.array(Ss), final_state=np.array(state), u_min=lo2.copy(), u_max=hi2.copy(),
        visualize_optimal_traj=np.bool_(True))
    print(f"clamp_loop_{name}: ticks={ticks} final={state}")


def main():
    control, utils = MG._import_reference()
    circle = np.loadtxt(os.path.join(MG.REF, "xydq_circle.txt"))[:, 0:4]
    lo, hi = (4.0, -6.0), (14.0, 2.0)
    one_step(control, "a_k128_t20", circle, 128, 20, 21, lo, hi)
    # the nominal is left unclamped without the optimal-trajectory loop (control.py:130)
    one_step(control, "b_novis_k128_t20", circle, 128, 20, 21, lo, hi, vis=False, visible=False)
    # dense weights with a live gamma term
    one_step(control, "c_dense_k256_t24", circle, 256, 24, 22, (6.0, -5.0), (12.0, 1.0),
             param_lambda=5.0e6, param_alpha=0.9)
    # exploration split (control.py:98-101): the exploration samples are clipped as eps alone
    one_step(control, "d_expl_k128_t20", circle, 128, 20, 23, lo, hi, param_exploration=0.25)
    # the reference's own commented-out values; the nominal starts outside them
    one_step(control, "e_runpy_k100_t30", circle, 100, 30, 24, -0.8, 0.8, sampled=True)
    closed_loop(control, utils, "k64_t20", circle, 64, 20, 25, 10, lo, hi)


if __name__ == "__main__":
    main()
