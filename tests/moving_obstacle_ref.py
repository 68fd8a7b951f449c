"""The fp64 yardstick of moving obstacles (mppi_set_moving_obstacles), built on the oracles as they are:
``O.horizon_loop(model, ..., penalty=)`` is the K x T loop and ``O.update_in_place`` the update tail, as in
chain_obstacle_ref.py.

A disc is (cx, cy, r) plus a velocity (vx, vy) in m/s, constant over the horizon of one call; the position given is
the position at the observed state x0.  Rollout step t (0-based) produces the state at time (t + 1) dt, and that
state is tested against the discs centred at c + v (t + 1) dt.  The final state's extra count (the ``_phi`` term) uses
the centres at T dt, the ones of step T - 1, so it repeats that step's flag: S = S_track + obstacle_cost * hits,
hits = flag.sum(1) + flag[:, -1].  Zero velocities are the static definition (O.rollout_costs(discs=),
chain_obstacle_costs), bit for bit.  ``shift`` moves the evaluation time by whole steps (shift = -1 is the off-by-one
definition c + v t dt that the tests tell the device apart from).
"""
import numpy as np

import chain_oracle as CO
import mppi_oracle as O
from chain_obstacle_ref import chain_collides


def discs_at(discs, vel, t, dt, shift=0):
    """The discs (n, 3) as rollout step t's new state meets them: centres c + v (t + 1 + shift) dt, radii kept."""
    d = np.array(np.zeros((0, 3)) if discs is None else discs, dtype=np.float64).reshape(-1, 3)
    if vel is not None and d.shape[0]:
        v = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
        assert v.shape[0] == d.shape[0]
        tau = (t + 1 + shift) * dt
        d[:, 0] = d[:, 0] + v[:, 0] * tau
        d[:, 1] = d[:, 1] + v[:, 1] * tau
    return d


def moving_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
                 p: O.ArmParams = O.ArmParams(), k_offset=0, K_total=None, gamma=None, *, lo=None, hi=None, discs=None,
                 vel=None, obstacle_cost=0.0, shift=0):
    """The arm's K x T loop with the collision cost on moving discs: the dict of O.rollout_costs(details=True)."""
    K, T, _ = eps.shape
    n = np.asarray(np.zeros((0, 3)) if discs is None else discs).reshape(-1, 3).shape[0]
    rec = dict(flag=np.zeros((K, T), dtype=bool), clear=np.zeros((K, T)), dist=np.zeros((K, T, n, 2)),
               clipped=np.zeros((K, T, n, 2), dtype=bool), ee=np.zeros((K, T, 2)), q=np.zeros((K, T, 2)),
               dq=np.zeros((K, T, 2)))

    def penalty(t, state):
        q1, q2, dq1, dq2 = state
        rec["flag"][:, t], rec["clear"][:, t], rec["dist"][:, t], rec["clipped"][:, t] = \
            O.collides(q1, q2, discs_at(discs, vel, t, dt, shift), p)
        rec["ee"][:, t, 0] = p.fk_l1 * np.cos(q1) + p.fk_l2 * np.cos(q1 + q2)
        rec["ee"][:, t, 1] = p.fk_l1 * np.sin(q1) + p.fk_l2 * np.sin(q1 + q2)
        rec["q"][:, t, 0], rec["q"][:, t, 1] = q1, q2
        rec["dq"][:, t, 0], rec["dq"][:, t, 1] = dq1, dq2
        return obstacle_cost * rec["flag"][:, t]

    S, S_track = O.horizon_loop(O.arm_model(p), x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w,
                                term_w, expl, k_offset, K_total, gamma, lo, hi, penalty)
    return dict(S=S, S_track=S_track, hits=rec["flag"].sum(1) + rec["flag"][:, -1], **rec)


def moving_step(x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
                p: O.ArmParams = O.ArmParams(), gamma=None, *, lo=None, hi=None, discs=None, vel=None,
                obstacle_cost=0.0, hits=None, visualize_optimal_traj=True):
    """One calc_control_input after its waypoint update with moving discs: moving_costs joined with
    O.update_in_place's dict.  ``hits`` (K,), when given, replaces the yardstick's own hit counts in S (the
    device's: a state within rounding of a boundary may fall on either side, and must not move a weight)."""
    u = np.array(u_prev, dtype=np.float64)
    r = moving_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl, p, gamma=gamma,
                     lo=lo, hi=hi, discs=discs, vel=vel, obstacle_cost=obstacle_cost)
    if hits is not None:
        r["S"] = r["S_track"] + obstacle_cost * np.asarray(hits, dtype=np.float64)
    return {**r, **O.update_in_place(O.arm_model(p), r["S"], u, eps, lam, x0, dt, lo, hi, expl,
                                     visualize_optimal_traj, False)}


def moving_masks(dirs, discs, vel, dt, fk1=1.0, fk2=1.0, shift=0):
    """The fp64 predicate on recorded direction values dirs (K, T, 4) = (c1, s1, c12, s12), step t against the
    discs at c + v (t + 1 + shift) dt: (mask (K, T) uint32 as mppi_debug_obstacle_hits lays it out, gap (K, T, n, 2)
    = |dist - r|)."""
    dirs = np.asarray(dirs, dtype=np.float64)
    K, T, _ = dirs.shape
    n = np.asarray(discs).reshape(-1, 3).shape[0]
    mask, gap = np.zeros((K, T), dtype=np.uint32), np.zeros((K, T, n, 2))
    for t in range(T):
        d = discs_at(discs, vel, t, dt, shift)
        dist, _ = O.segment_test(dirs[:, t, 0], dirs[:, t, 1], dirs[:, t, 2], dirs[:, t, 3], d, fk1, fk2)
        mask[:, t] = O.touch_mask(dist, d)
        gap[:, t] = np.abs(dist - d[:, 2][:, None])
    return mask, gap


def chain_moving_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
                       P=CO.ChainParams(), k_offset=0, K_total=None, gamma=None, *, lo=None, hi=None, discs=None,
                       vel=None, obstacle_cost=0.0, shift=0):
    """The chain's K x T loop with the collision cost on moving discs: S, S_track, flag, clear (K, T), hits (K,),
    q and dq (K, T, n), as chain_obstacle_ref.chain_obstacle_costs."""
    K, T, n = eps.shape
    rec = dict(flag=np.zeros((K, T), dtype=bool), clear=np.zeros((K, T)), q=np.zeros((K, T, n)),
               dq=np.zeros((K, T, n)))

    def penalty(t, state):
        q, dq = state
        rec["flag"][:, t], rec["clear"][:, t], _, _ = chain_collides(q, discs_at(discs, vel, t, dt, shift), P)
        rec["q"][:, t], rec["dq"][:, t] = q, dq
        return obstacle_cost * rec["flag"][:, t]

    S, S_track = O.horizon_loop(CO.chain_model(P), x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w,
                                term_w, expl, k_offset, K_total, gamma, lo, hi, penalty)
    return dict(S=S, S_track=S_track, hits=rec["flag"].sum(1) + rec["flag"][:, -1], **rec)


def chain_moving_step(x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
                      P=CO.ChainParams(), *, gamma=None, lo=None, hi=None, discs=None, vel=None, obstacle_cost=0.0,
                      hits=None, visualize_optimal_traj=True):
    """One calc_control_input of the chain after its waypoint update with moving discs: chain_moving_costs joined with
    O.update_in_place's dict; ``hits`` as in moving_step."""
    u = np.array(u_prev, dtype=np.float64)
    r = chain_moving_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl, P,
                           gamma=gamma, lo=lo, hi=hi, discs=discs, vel=vel, obstacle_cost=obstacle_cost)
    if hits is not None:
        r["S"] = r["S_track"] + obstacle_cost * np.asarray(hits, dtype=np.float64)
    return {**r, **O.update_in_place(CO.chain_model(P), r["S"], u, eps, lam, x0, dt, lo, hi, expl,
                                     visualize_optimal_traj, False)}


def chain_moving_masks(dirs, discs, vel, dt, fk, shift=0):
    """The fp64 predicate on recorded direction values dirs (K, T, 2 n) = (cos th_a at a, sin th_a at n + a), step t
    against the discs at c + v (t + 1 + shift) dt: (mask (K, T) uint64 as mppi_chain_debug_obstacle_hits lays it out,
    gap (K, T, nd, n) = |dist - r|)."""
    from chain_obstacle_ref import chain_segment_test, chain_touch_mask
    dirs = np.asarray(dirs, dtype=np.float64)
    K, T, n2 = dirs.shape
    n, nd = n2 // 2, np.asarray(discs).reshape(-1, 3).shape[0]
    mask, gap = np.zeros((K, T), dtype=np.uint64), np.zeros((K, T, nd, n))
    for t in range(T):
        d = discs_at(discs, vel, t, dt, shift)
        dist, _ = chain_segment_test(dirs[:, t, :n], dirs[:, t, n:], d, fk)
        mask[:, t] = chain_touch_mask(dist, d)
        gap[:, t] = np.abs(dist - d[:, 2][:, None])
    return mask, gap
