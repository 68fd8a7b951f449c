"""The fp64 yardstick of the chain's self-collision cost (mppi_chain_set_self_collision), for the tests.

The oracle's horizon loop takes a ``penalty(t, state)`` hook (O.horizon_loop) and returns S_track beside S, so the
yardstick of a new state cost lives here, beside the tests, on oracle/chain_oracle.py's model and its disc test.

Definition.  Joint j of the chain is b_{j-1} = sum_{i < j} fk_i (cos th_i, sin th_i) (joint 0 the origin, joint n the
tip), link a the zero-thickness segment from joint a to joint a + 1.  For every pair of links a < b with b >= a + 2:

  * e(a, b): the smallest of the four endpoint-to-segment distances (the ends of b against a, the ends of a against b),
    each with the projection on the link's direction clipped to [0, fk] as chain_segment_test clips it;
  * x(a, b): the segments cross properly, the two ends of each strictly on opposite sides of the other's line;
  * the pair self-collides when x(a, b) or e(a, b) < d, d >= 0 the clearance (d = 0: crossings only).

A state self-collides when any pair does.  Every step of the horizon whose new state self-collides adds the cost to its
sample's S, the final state once more: S = S_track + obstacle_cost hits_disc + self_collision_cost hits_self, each count
in [0, T + 1].  The pairs are enumerated a ascending, then b ascending; bit i of a mask (uint32) is pair i.
"""
import numpy as np

import chain_oracle as CO
import mppi_oracle as O


def pairs(n):
    """The non-adjacent link pairs in mask order: (0, 2), (0, 3), ..., (1, 3), ...: (n - 1)(n - 2) / 2 of them."""
    return [(a, b) for a in range(n) for b in range(a + 2, n)]


def joints(c, s, fk):
    """(jx, jy), each (..., n + 1): joint j = b_{j-1} from the direction values c, s (..., n)."""
    c, s, fk = (np.asarray(v, dtype=np.float64) for v in (c, s, fk))
    z = np.zeros(c.shape[:-1] + (1,))
    return (np.concatenate([z, np.cumsum(fk * c, -1)], -1), np.concatenate([z, np.cumsum(fk * s, -1)], -1))


def _point_link(jx, jy, c, s, fk, j, L):
    """(distance, signed perpendicular offset) of joint j from link L, the projection clipped to [0, fk_L]."""
    px, py = jx[..., j] - jx[..., L], jy[..., j] - jy[..., L]
    ux, uy = c[..., L], s[..., L]
    pr = px * ux + py * uy
    t = np.clip(pr, 0.0, fk[L])
    return np.hypot(px - t * ux, py - t * uy), ux * py - uy * px


def self_test(c, s, fk, d=0.0):
    """The predicate on direction values c, s (..., n): (e (..., P) fp64, x (..., P) bool, mask (...) uint32) over the
    P = len(pairs(n)) pairs; bit i of mask is pair i in self-collision: x or e < d.  n = 2: no pairs, mask 0."""
    c, s, fk = (np.asarray(v, dtype=np.float64) for v in (c, s, fk))
    n = c.shape[-1]
    jx, jy = joints(c, s, fk)
    e = np.zeros(c.shape[:-1] + (len(pairs(n)),))
    x = np.zeros(e.shape, dtype=bool)
    mask = np.zeros(c.shape[:-1], dtype=np.uint32)
    for i, (a, b) in enumerate(pairs(n)):
        d0, s0 = _point_link(jx, jy, c, s, fk, b, a)          # the ends of link b against link a
        d1, s1 = _point_link(jx, jy, c, s, fk, b + 1, a)
        d2, s2 = _point_link(jx, jy, c, s, fk, a, b)          # the ends of link a against link b
        d3, s3 = _point_link(jx, jy, c, s, fk, a + 1, b)
        e[..., i] = np.minimum(np.minimum(d0, d1), np.minimum(d2, d3))
        x[..., i] = (s0 * s1 < 0.0) & (s2 * s3 < 0.0)
        mask |= np.where(x[..., i] | (e[..., i] < d), np.uint32(1 << i), np.uint32(0))
    return e, x, mask


def self_collides(q, fk, d):
    """(flag (...), e, x, mask) of the states q (..., n)."""
    th = np.cumsum(np.asarray(q, dtype=np.float64), -1)
    e, x, mask = self_test(np.cos(th), np.sin(th), fk, d)
    return mask != 0, e, x, mask


def brute_distance(p0, p1, q0, q1, m=2001):
    """The distance of two segments by sampling each at m points (an upper bound, within the sampling step)."""
    t = np.linspace(0.0, 1.0, m)[:, None]
    A = (1.0 - t) * np.asarray(p0, dtype=np.float64) + t * np.asarray(p1, dtype=np.float64)
    B = (1.0 - t) * np.asarray(q0, dtype=np.float64) + t * np.asarray(q1, dtype=np.float64)
    return float(np.sqrt(np.min((A[:, None, 0] - B[None, :, 0]) ** 2 + (A[:, None, 1] - B[None, :, 1]) ** 2)))


def rollout_costs(P, x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0, *, lo=None,
                  hi=None, discs=None, vel=None, obstacle_cost=0.0, clearance=None, self_cost=0.0, hits=None):
    """The K x T loop with both state costs composed in one penalty: S, S_track (K,), hits_disc, hits_self (K,) and per
    step flag_disc, flag_self (K, T), e, x (K, T, P), mask (K, T), q, dq (K, T, n).  ``clearance=None``: no self cost.
    ``hits=(hits_disc, hits_self)`` replaces the yardstick's own counts in S (the device's: a state within rounding of
    a boundary may fall on either side and must not move a weight), either entry None for the yardstick's own."""
    model = CO.chain_model(P)
    steps = []

    def penalty(t, state):
        fd = CO.chain_collides(state[0], O.discs_at(discs, vel, t, dt), P)[0]
        if clearance is None:
            fs, e, x, m = (np.zeros(fd.shape, dtype=bool), np.zeros(fd.shape + (len(pairs(P.n)),)),
                           np.zeros(fd.shape + (len(pairs(P.n)),), dtype=bool), np.zeros(fd.shape, dtype=np.uint32))
        else:
            fs, e, x, m = self_collides(state[0], P.fk, clearance)
        steps.append((fd, fs, e, x, m, state[0], state[1]))
        return obstacle_cost * fd + self_cost * fs

    S, S_track = O.horizon_loop(model, x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl,
                                lo=lo, hi=hi, penalty=penalty)
    rec = {k: np.stack(a, 1) for k, a in zip(("flag_disc", "flag_self", "e", "x", "mask", "q", "dq"), zip(*steps))}
    hd = rec["flag_disc"].sum(1) + rec["flag_disc"][:, -1]
    hs = rec["flag_self"].sum(1) + rec["flag_self"][:, -1]
    out = dict(S=S, S_track=S_track, hits_disc=hd, hits_self=hs, **rec)
    if hits is not None:
        gd = hd if hits[0] is None else np.asarray(hits[0])
        gs = hs if hits[1] is None else np.asarray(hits[1])
        out["S"] = (S_track + obstacle_cost * gd.astype(np.float64)) + self_cost * gs.astype(np.float64)
    return out


def step(P, x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0, *, lo=None, hi=None,
         visualize_optimal_traj=True, **kw):
    """One control step: rollout_costs joined with the oracle's update tail (O.update_in_place on a copy of u_prev)."""
    u = np.array(u_prev, dtype=np.float64)
    out = rollout_costs(P, x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl, lo=lo, hi=hi,
                        **kw)
    out.update(O.update_in_place(CO.chain_model(P), out["S"], u, eps, lam, x0, dt, lo, hi, expl,
                                 visualize_optimal_traj))
    return out
