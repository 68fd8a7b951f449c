"""The fp64 yardstick of the chain's workspace obstacles (mppi_chain_set_obstacles), built on the oracles as they are:
``O.horizon_loop(chain_model(P), ..., penalty=)`` is the K x T loop and ``O.update_in_place`` the update tail.

Link a (0-based) is the zero-thickness segment from b_{a-1} to b_a, b_a = sum_{i <= a} fk_i (cos th_i, sin th_i) with
b_{-1} the origin, th the absolute angles and fk the cost's link lengths (chain_oracle.chain_fk's); it touches disc
(cx, cy, r) when the distance from the centre to the segment, the projection clipped to [0, fk_a], is < r.  A state
collides when any link touches any disc; every step whose new state collides adds the cost and the final state adds it
once more.  At n = 2 with ChainParams.from_arm2() this is mppi_oracle's definition (test_chain_obstacle_cpu.py).
"""
import numpy as np

import chain_oracle as CO
import mppi_oracle as O


def chain_segment_test(c, s, discs, fk):
    """Every link against every disc from the direction values c, s (..., n): (dist (..., nd, n) fp64, the distance
    from disc j's centre to link a with the projection clipped to the segment; clipped (..., nd, n) int8, -1 / +1
    where the projection was clipped to the link's base / tip, 0 where it is interior)."""
    d = np.asarray(discs, dtype=np.float64).reshape(-1, 3)
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    fk = np.asarray(fk, dtype=np.float64)
    n = c.shape[-1]
    bx = np.cumsum(fk * c, -1) - fk * c            # base of link a: b_{a-1}
    by = np.cumsum(fk * s, -1) - fk * s
    px = d[:, 0][:, None] - bx[..., None, :]       # (..., nd, n)
    py = d[:, 1][:, None] - by[..., None, :]
    ux, uy = c[..., None, :], s[..., None, :]
    pr = px * ux + py * uy
    t = np.clip(pr, 0.0, fk)
    dist = np.hypot(px - t * ux, py - t * uy)
    clipped = np.where(pr < 0.0, -1, np.where(pr > fk, 1, 0)).astype(np.int8)
    assert dist.shape[-1] == n
    return dist, clipped


def chain_touch_mask(dist, discs):
    """The masks of mppi_chain_debug_obstacle_hits from chain_segment_test's distances: bit 8 j + a is link a
    touching disc j (uint64, dist's shape without its last two axes)."""
    r = np.asarray(discs, dtype=np.float64).reshape(-1, 3)[:, 2]
    hit = dist < r[:, None]
    nd, n = hit.shape[-2:]
    bits = np.uint64(1) << (np.uint64(8) * np.arange(nd, dtype=np.uint64)[:, None] + np.arange(n, dtype=np.uint64))
    return np.bitwise_or.reduce(np.where(hit, bits, np.uint64(0)).reshape(hit.shape[:-2] + (-1,)), axis=-1) \
        if nd else np.zeros(hit.shape[:-2], dtype=np.uint64)


def chain_collides(q, discs, P):
    """(flag, clearance, dist, clipped) of the states q (..., n) against the discs: flag where any link touches any
    disc, clearance |dist - r| of the nearest boundary (inf without discs)."""
    th = np.cumsum(np.asarray(q, dtype=np.float64), -1)
    dist, clipped = chain_segment_test(np.cos(th), np.sin(th), discs, P.fk)
    r = np.asarray(discs, dtype=np.float64).reshape(-1, 3)[:, 2]
    flag = np.any(dist < r[:, None], axis=(-1, -2))
    gap = np.abs(dist - r[:, None]).reshape(dist.shape[:-2] + (-1,))
    clear = gap.min(-1) if gap.shape[-1] else np.full(gap.shape[:-1], np.inf)
    return flag, clear, dist, clipped


def chain_obstacle_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
                         P=CO.ChainParams(), k_offset=0, K_total=None, gamma=None, *, lo=None, hi=None, discs=None,
                         obstacle_cost=0.0):
    """The chain's K x T loop with the collision cost: the dict of the arm's rollout_costs(details=True) — S,
    S_track (the same loop without the penalty), flag (K, T), clear (K, T), hits (K,) = flag.sum(1) + flag[:, -1],
    dist and clipped (K, T, nd, n), ee (K, T, 2), q and dq (K, T, n)."""
    K, T, n = eps.shape
    discs = np.asarray(np.zeros((0, 3)) if discs is None else discs, dtype=np.float64).reshape(-1, 3)
    nd = discs.shape[0]
    rec = dict(flag=np.zeros((K, T), dtype=bool), clear=np.zeros((K, T)), dist=np.zeros((K, T, nd, n)),
               clipped=np.zeros((K, T, nd, n), dtype=np.int8), ee=np.zeros((K, T, 2)), q=np.zeros((K, T, n)),
               dq=np.zeros((K, T, n)))

    def penalty(t, state):
        q, dq = state
        rec["flag"][:, t], rec["clear"][:, t], rec["dist"][:, t], rec["clipped"][:, t] = chain_collides(q, discs, P)
        rec["ee"][:, t, 0], rec["ee"][:, t, 1] = CO.chain_fk(q, P)
        rec["q"][:, t], rec["dq"][:, t] = q, dq
        return obstacle_cost * rec["flag"][:, t]

    S, S_track = O.horizon_loop(CO.chain_model(P), x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w,
                                term_w, expl, k_offset, K_total, gamma, lo, hi, penalty)
    return dict(S=S, S_track=S_track, hits=rec["flag"].sum(1) + rec["flag"][:, -1], **rec)


def chain_obstacle_step(x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
                        P=CO.ChainParams(), *, gamma=None, lo=None, hi=None, discs=None, obstacle_cost=0.0, hits=None,
                        visualize_optimal_traj=True):
    """One calc_control_input after its waypoint update with the discs: chain_obstacle_costs joined with
    O.update_in_place's dict.  ``hits`` (K,), when given, replaces the yardstick's own hit counts in S (the device's:
    a state within rounding of a boundary may fall on either side, and must not move a weight)."""
    u = np.array(u_prev, dtype=np.float64)
    r = chain_obstacle_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl, P,
                             gamma=gamma, lo=lo, hi=hi, discs=discs, obstacle_cost=obstacle_cost)
    if hits is not None:
        r["S"] = r["S_track"] + obstacle_cost * np.asarray(hits, dtype=np.float64)
    return {**r, **O.update_in_place(CO.chain_model(P), r["S"], u, eps, lam, x0, dt, lo, hi, expl,
                                     visualize_optimal_traj, False)}
