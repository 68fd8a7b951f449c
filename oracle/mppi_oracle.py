"""CPU ORACLE — test infrastructure only, never shipped, never on the product path.

A vectorised fp64 NumPy restatement of the reference MPPI step
(junofficial/mppi_RobotArm ``control.py:67-152``), used ONLY by ``tests/``,
``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg as the
checker.  The HIP product path (``mppi_robotarm_amd``) never imports this file.

Parity is PINNED: ``tests/test_oracle_golden.py`` checks this restatement
against the golden fixtures captured from the imported reference
(``tests/golden/make_golden.py``) — S to ~1e-15 relative, u bit-for-bit in the
one-hot regime, closed loops tick by tick.  The same loop and update tail, with
torque limits (``lo`` / ``hi``: the reference's clamp hook ``_g`` switched on)
and with workspace obstacles (``discs``: a collision cost inside ``_c`` and
``_phi``), are pinned by ``tests/test_clamp_cpu.py`` and
``tests/test_obstacle_cpu.py`` to fixtures captured from the reference with
only those hooks overridden; discs that move (``vel``) by
``tests/test_moving_obstacle_cpu.py``.  There is ONE horizon loop
(``horizon_loop``), ONE collision-cost loop around it (``collision_costs``: the
discs and, for the chain, self-collision, in one penalty) and
ONE update tail (``update_in_place``); the chain (``chain_oracle.py``) runs the
same three with its own model.

Every function cites the reference line it restates.  Quirks kept on purpose
(SURVEY §3.3): the returned ``u0`` is the post-shift row, ``u_seq`` aliases
``u_prev``, the median filter is scipy's upper median with ``reflect``
boundaries, the optimal / sampled trajectories use the off-by-one control
``u[t-1]`` (``t = 0`` reads ``u[-1]``), the weighted noise uses ``eps`` (not
``v``), the nearest-waypoint window is shared by every sample and step of one
control step, and ``_F`` (link lengths from ``sys_params``) and the
kinematics in the cost (``self.l1 = self.l2 = 1``) keep separate lengths.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass

import numpy as np

SEARCH_IDX_LEN = 30  # control.py:203


@dataclass(frozen=True)
class ArmParams:
    """sys_params.py:1-13 (constants used by ``_F``, control.py:11-18)."""
    m1: float = 1.0
    m2: float = 1.0
    l1: float = 1.0
    l2: float = 1.0
    lc1: float = 0.5
    lc2: float = 0.5
    g: float = 9.81
    # forward kinematics inside the cost / waypoint search: control.py:55-56
    fk_l1: float = 1.0
    fk_l2: float = 1.0


def forward_dynamics(q1, q2, dq1, dq2, u1, u2, dt, p: ArmParams):
    """``_F`` (control.py:234-263), vectorised over samples.

    Mass matrix exactly as written (control.py:241-245: link lengths stand in
    for the link inertias); ``np.linalg.inv`` of the stacked 2x2 matrices as at
    control.py:252; semi-implicit Euler (control.py:256, 259).
    """
    c2 = np.cos(q2)
    M11 = p.m1 * p.lc1 ** 2 + p.l1 + p.m2 * (p.l1 ** 2 + p.lc2 ** 2 + 2 * p.l1 * p.lc2 * c2) + p.l2
    M22 = p.m2 * p.lc2 ** 2 + p.l2
    M12 = p.m2 * p.l1 * p.lc2 * c2 + p.m2 * p.lc2 ** 2 + p.l2
    M21 = M12
    h = p.m2 * p.l1 * p.lc2 * np.sin(q2)
    g1 = p.m1 * p.lc1 * p.g * np.cos(q1) + p.m2 * p.g * (p.lc2 * np.cos(q1 + q2) + p.l1 * np.cos(q1))
    g2 = p.m2 * p.lc2 * p.g * np.cos(q1 + q2)
    # C.dot(dq) with C = [[-h dq2, -h dq1 - h dq2], [h dq1, 0]]   (control.py:251)
    cdq1 = (-h * dq2) * dq1 + (-h * dq1 - h * dq2) * dq2
    cdq2 = (h * dq1) * dq1 + 0.0 * dq2
    r1 = (u1 - cdq1) - g1
    r2 = (u2 - cdq2) - g2
    n = np.broadcast(q1, q2).shape
    M = np.empty(n + (2, 2))
    M[..., 0, 0] = M11
    M[..., 0, 1] = M12
    M[..., 1, 0] = M21
    M[..., 1, 1] = M22
    Mi = np.linalg.inv(M)
    ddq1 = Mi[..., 0, 0] * r1 + Mi[..., 0, 1] * r2
    ddq2 = Mi[..., 1, 0] * r1 + Mi[..., 1, 1] * r2
    dq1n = dq1 + ddq1 * dt
    dq2n = dq2 + ddq2 * dt
    q1n = q1 + dq1n * dt
    q2n = q2 + dq2n * dt
    return q1n, q2n, dq1n, dq2n


def arm_dynamic(q, dq, u, p: ArmParams = ArmParams()):
    """Plant ``Arm_Dynamic`` (utils.py:14-29): returns ddq for the host loop."""
    c2 = np.cos(q[1])
    M11 = p.m1 * p.lc1 ** 2 + p.l1 + p.m2 * (p.l1 ** 2 + p.lc2 ** 2 + 2 * p.l1 * p.lc2 * c2) + p.l2
    M22 = p.m2 * p.lc2 ** 2 + p.l2
    M12 = p.m2 * p.l1 * p.lc2 * c2 + p.m2 * p.lc2 ** 2 + p.l2
    M = np.array([[M11, M12], [M12, M22]])
    h = p.m2 * p.l1 * p.lc2 * np.sin(q[1])
    g1 = p.m1 * p.lc1 * p.g * np.cos(q[0]) + p.m2 * p.g * (p.lc2 * np.cos(q[0] + q[1]) + p.l1 * np.cos(q[0]))
    g2 = p.m2 * p.lc2 * p.g * np.cos(q[0] + q[1])
    C = np.array([[-h * dq[1], -h * dq[0] - h * dq[1]], [h * dq[0], 0]])
    return np.linalg.inv(M).dot(u - C.dot(dq) - np.array([g1, g2]))


def forward_kinematics(q, p: ArmParams = ArmParams()):
    """``Forward_Kinemetic`` (utils.py:32-38)."""
    x1 = p.l1 * np.cos(q[0])
    y1 = p.l1 * np.sin(q[0])
    x2 = p.l1 * np.cos(q[0]) + p.l2 * np.cos(q[0] + q[1])
    y2 = p.l1 * np.sin(q[0]) + p.l2 * np.sin(q[0] + q[1])
    return x1, y1, x2, y2


def first_min_index(d):
    """``d.index(min(d))`` (control.py:213-215) along the last axis.  Python's
    min() keeps d[0] and replaces it only on a strict '<': a NaN at j > 0 is
    never chosen, a NaN at j = 0 always is (np.argmin returns the first NaN)."""
    j = np.argmin(d, axis=-1)
    nan = np.isnan(np.take_along_axis(d, np.asarray(j)[..., None], axis=-1)[..., 0])
    if np.any(nan):
        alt = np.argmin(np.where(np.isnan(d), np.inf, d), axis=-1)   # the first minimum of the numbers
        alt = np.where(np.isnan(d[..., 0]), 0, alt)
        j = np.where(nan, alt, j)
    return j


def nearest_waypoint(q1, q2, ref_path, prev_idx, p: ArmParams):
    """``_get_nearest_waypoint`` (control.py:200-232) vectorised over samples.

    Window ``ref_path[prev:prev+30]`` (slice-truncated at the path end),
    ``d.index(min(d))`` of ``((x-rx)^2 + (y-ry)^2) * 100`` (control.py:212-215).
    Returns (nearest_idx, ref_x, ref_y, ref_dq1, ref_dq2).
    """
    x = p.fk_l1 * np.cos(q1) + p.fk_l2 * np.cos(q1 + q2)
    y = p.fk_l1 * np.sin(q1) + p.fk_l2 * np.sin(q1 + q2)
    win = ref_path[prev_idx:prev_idx + SEARCH_IDX_LEN]
    dx = np.asarray(x)[..., None] - win[:, 0]
    dy = np.asarray(y)[..., None] - win[:, 1]
    d = (dx ** 2 + dy ** 2) * 100
    j = first_min_index(d)
    idx = j + prev_idx
    return idx, ref_path[idx, 0], ref_path[idx, 1], ref_path[idx, 2], ref_path[idx, 3]


def state_cost(q1, q2, dq1, dq2, ref_path, prev_idx, weight, p: ArmParams):
    """``_c`` / ``_phi`` (control.py:174-198): weighted squared error x 10000."""
    x = p.fk_l1 * np.cos(q1) + p.fk_l2 * np.cos(q1 + q2)
    y = p.fk_l1 * np.sin(q1) + p.fk_l2 * np.sin(q1 + q2)
    _, rx, ry, rdq1, rdq2 = nearest_waypoint(q1, q2, ref_path, prev_idx, p)
    c = weight[0] * (x - rx) ** 2 + weight[1] * (y - ry) ** 2 + \
        weight[2] * (dq1 - rdq1) ** 2 + weight[3] * (dq2 - rdq2) ** 2
    return c * 10000


def _limits(lo, hi, n):
    """(lo, hi) per joint from scalars or n values, a missing side +-inf; None when there are no limits."""
    if lo is None and hi is None:
        return None
    return (np.broadcast_to(np.asarray(-np.inf if lo is None else lo, dtype=np.float64), (n,)),
            np.broadcast_to(np.asarray(np.inf if hi is None else hi, dtype=np.float64), (n,)))


def sampled_controls(u, eps, lo=None, hi=None, expl=0.0, k_offset=0, K_total=None):
    """v: u + eps for the exploitation samples, eps for the rest (control.py:98-104), for any n; eps (K, T, n)
    with u (T, n), or one step's eps (K, n) with its row of u.  With limits, the reference's clamp hook ``_g``
    (control.py:166-172) switched on.  ``_g`` ships with its two ``np.clip`` lines commented out; enabled, it
    clips its argument IN PLACE, and every argument it is given is a view (``v[k, t-1]``, ``u[t-1]``), so:

      1. rollout (control.py:97-106): ``v = clip(u[t-1] + eps)`` (``clip(eps)`` for an exploration sample);
         ``_F`` and the control cost ``gamma u^T Sigma^-1 v`` take the clipped ``v``;
      2. weights and weighted noise (control.py:112-118): unchanged, the UNCLAMPED eps;
      3. update (control.py:126-134): ``u += w_eps`` is not clipped by itself; the optimal-trajectory loop calls
         ``_g(u[t-1])`` for every row, which clips the whole updated ``u`` in place, only when
         ``visualize_optimal_traj``;
      4. sampled trajectories (control.py:139-145): re-rolled from the clipped ``v``.

    ``k_offset`` / ``K_total`` restate the exploration split ``k < (1 - expl) * K`` (control.py:98) for a shard
    of a larger sample set."""
    exploit = _exploit(eps.shape[0], expl, k_offset, K_total)
    return _controls(u, eps, exploit.reshape((-1,) + (1,) * (eps.ndim - 1)), _limits(lo, hi, eps.shape[-1]))


def _exploit(K, expl, k_offset, K_total):
    return (np.arange(K) + k_offset) < (1.0 - expl) * (K if K_total is None else K_total)   # control.py:98


def _controls(u, eps, exploit, lim):
    e = eps.astype(np.float64)
    v = np.where(exploit, u + e, e)
    return v if lim is None else np.clip(v, *lim)


# What the one horizon loop and the one update tail need of a model (the chain's is chain_oracle.chain_model):
# start(x0, K) -> state, step(state, v, dt) -> state, cost(state, ref_path, prev_idx, weight) -> (K,),
# dot(a, v) -> (K,) the control cost a . v in the model's own expression (its bits are pinned),
# trajectory(x0, controls, dt) -> states, and for the collision cost (collision_costs):
# collides(state, discs) -> (flag, clear, dist, clipped), the model's collision test,
# record(state) -> (ee (K, 2), q (K, n), dq (K, n)), what a state records per step, and
# self_collides(state, d) -> (flag, e, x, mask), its self-collision test at the clearance d (None: it has none).
Model = namedtuple("Model", "start step cost dot trajectory collides record self_collides")


def arm_model(p: ArmParams = ArmParams()):
    def record(s):
        q1, q2, dq1, dq2 = s
        return (np.stack([p.fk_l1 * np.cos(q1) + p.fk_l2 * np.cos(q1 + q2),
                          p.fk_l1 * np.sin(q1) + p.fk_l2 * np.sin(q1 + q2)], -1),
                np.stack([q1, q2], -1), np.stack([dq1, dq2], -1))

    return Model(start=lambda x0, K: tuple(np.full(K, float(x0[i])) for i in range(4)),
                 step=lambda s, v, dt: forward_dynamics(*s, v[:, 0], v[:, 1], dt, p),
                 cost=lambda s, ref_path, prev_idx, weight: state_cost(*s, ref_path, prev_idx, weight, p),
                 dot=lambda a, v: a[0] * v[:, 0] + a[1] * v[:, 1],
                 trajectory=lambda x0, controls, dt: rollout_trajectory(x0, controls, dt, p),
                 collides=lambda s, discs: collides(s[0], s[1], discs, p), record=record,
                 self_collides=None)                       # two links have no non-adjacent pair


def horizon_loop(model, x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
                 k_offset=0, K_total=None, gamma=None, lo=None, hi=None, penalty=None):
    """The K x T hot loop, control.py:81-109, for either model.  Returns (S (K,) fp64, S_track).

    ``penalty(t, state)``, when given, is added to the state cost of step t inside ``_c`` and, its last value,
    to ``_phi``; S_track is then the same loop without it (None otherwise, and no work is done for it).
    ``gamma``: the controller's ``param_gamma`` (fixed at construction, control.py:45, read at :106); default
    lam (1 - alpha)."""
    K, T, n = eps.shape
    if gamma is None:
        gamma = lam * (1.0 - alpha)                   # control.py:45
    sig_inv = np.linalg.inv(sigma)                    # control.py:106 (raises on singular)
    exploit, lim = _exploit(K, expl, k_offset, K_total)[:, None], _limits(lo, hi, n)
    S, S_track, pen = np.zeros(K), None if penalty is None else np.zeros(K), 0.0
    state = model.start(x0, K)
    for t in range(T):
        v = _controls(u[t], eps[:, t], exploit, lim)      # control.py:99-104, one step of sampled_controls
        state = model.step(state, v, dt)
        c = model.cost(state, ref_path, prev_idx, stage_w)
        ctrl = model.dot((gamma * u[t].T) @ sig_inv, v)   # ((γ uᵀ) Σ⁻¹) v, left-to-right
        if penalty is not None:
            pen = penalty(t, state)
            S_track = S_track + (c + ctrl)
            c = c + pen
        S = S + (c + ctrl)
    phi = model.cost(state, ref_path, prev_idx, term_w)   # control.py:109
    if penalty is not None:
        S_track = S_track + phi
        phi = phi + pen
    return S + phi, S_track


def discs_at(discs, vel, t, dt, shift=0):
    """The discs (n, 3) as rollout step t's new state meets them.  A disc is (cx, cy, r) plus, in ``vel``, a
    velocity (vx, vy) in m/s, constant over the horizon of one call; the position given is the one at the observed
    state x0.  Step t (0-based) produces the state at time (t + 1) dt, so it meets the centres
    c + v (t + 1 + shift) dt, radii kept; ``vel=None`` is the discs at rest.  ``shift`` moves the evaluation time by
    whole steps (shift = -1 is the off-by-one definition c + v t dt that the tests tell the device apart from)."""
    d = np.array(np.zeros((0, 3)) if discs is None else discs, dtype=np.float64).reshape(-1, 3)
    if vel is not None and d.shape[0]:
        v = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
        assert v.shape[0] == d.shape[0]
        tau = (t + 1 + shift) * dt
        d[:, 0] = d[:, 0] + v[:, 0] * tau
        d[:, 1] = d[:, 1] + v[:, 1] * tau
    return d


def collision_costs(model, x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
                    k_offset=0, K_total=None, gamma=None, lo=None, hi=None, *, discs=None, vel=None,
                    obstacle_cost=0.0, shift=0, clearance=None, self_cost=0.0, details=False):
    """S (K,) fp64 of either model's K x T loop (horizon_loop) with the collision cost on ``discs``, which move
    with ``vel`` (discs_at), and, with a ``clearance``, the model's self-collision cost in the same penalty.

    The collision cost is the reference with ONLY ``_c`` and ``_phi`` (control.py:174-198) overridden to return
    ``... + obstacle_cost * collides(x)``, the penalty added after the x 10000: every step of the horizon whose
    new state collides adds it to its sample's cost and the final state adds it once more (against the centres of
    the last step, so it repeats that step's flag): ``S = S_track + obstacle_cost * hits``, ``hits`` in
    ``[0, T + 1]``.  With ``clearance`` (not None) the penalty of a state is
    ``obstacle_cost * flag + self_cost * flag_self``, flag_self from ``model.self_collides(state, clearance)``:
    ``S = S_track + obstacle_cost * hits + self_cost * hits_self``; a model without one raises ValueError.

    ``details=True`` returns a dict instead: S, S_track (K,) (the same loop without the penalty), flag (K, T)
    bool per step's new state, clear (K, T) clearance, hits (K,) = flag.sum(1) + flag[:, -1], dist and clipped
    (K, T) + whatever model.collides returns per state, ee (K, T, 2) end effector, q and dq (K, T, n) joint angles
    and rates; for a model with a self-collision test also flag_self (K, T) bool, e and x (K, T, P) and mask (K, T)
    of model.self_collides and hits_self (K,), zeros while ``clearance`` is None.  Without discs, clearance and
    details the loop does no collision or bookkeeping work."""
    if clearance is not None and model.self_collides is None:
        raise ValueError("the model has no self-collision test")
    steps, penalty = [], None
    if discs is not None or clearance is not None or details:
        def penalty(t, state):
            hit = model.collides(state, discs_at(discs, vel, t, dt, shift))
            own = () if clearance is None else model.self_collides(state, clearance)
            steps.append(hit + model.record(state) + own)
            if clearance is None:
                return obstacle_cost * hit[0]
            return obstacle_cost * hit[0] + self_cost * own[0]

    S, S_track = horizon_loop(model, x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl,
                              k_offset, K_total, gamma, lo, hi, penalty)
    if not details:
        return S
    rec = {k: np.stack(a, 1) for k, a in zip(("flag", "clear", "dist", "clipped", "ee", "q", "dq",
                                              "flag_self", "e", "x", "mask"), zip(*steps))}
    if clearance is None and model.self_collides is not None:        # the same keys, whatever the keywords
        off = zip(("flag_self", "e", "x", "mask"), model.self_collides(model.start(x0, eps.shape[0]), 0.0))
        rec.update({k: np.zeros(a.shape[:1] + eps.shape[1:2] + a.shape[1:], a.dtype) for k, a in off})
    hits = {h: rec[f].sum(1) + rec[f][:, -1] for h, f in (("hits", "flag"), ("hits_self", "flag_self")) if f in rec}
    return dict(S=S, S_track=S_track, **hits, **rec)


def rollout_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w,
                  expl=0.0, p: ArmParams = ArmParams(), k_offset=0, K_total=None, gamma=None, *,
                  lo=None, hi=None, discs=None, vel=None, obstacle_cost=0.0, shift=0, details=False):
    """collision_costs for the arm: S (K,) fp64 of its K x T loop, optionally with torque limits ``lo`` / ``hi`` (a
    scalar or per joint; sampled_controls has the clamp's rules) and the collision cost on ``discs`` moving with
    ``vel``; ``details=True`` returns collision_costs' dict, dist and clipped (K, T, n, 2) of segment_test."""
    return collision_costs(arm_model(p), x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl,
                           k_offset, K_total, gamma, lo, hi, discs=discs, vel=vel, obstacle_cost=obstacle_cost,
                           shift=shift, details=details)


def segment_test(c1, s1, c12, s12, discs, fk1=1.0, fk2=1.0):
    """Both links against every disc ``(cx, cy, r)`` from the direction values (any common shape).  A link is a
    zero-thickness segment in the cost's kinematics (``fk_l1``, ``fk_l2``, base at the origin, as ``_c``
    computes x and y): link 1 from (0, 0) to e = fk_l1 (cos q1, sin q1), link 2 from e to
    e + fk_l2 (cos(q1 + q2), sin(q1 + q2)).  Returns (dist (..., n, 2) fp64, the distance from disc j's centre
    to link 1 / link 2, the projection parameter clipped to the segment, and clipped (..., n, 2), whether it was
    clipped to an end of the segment)."""
    d = np.asarray(discs, dtype=np.float64).reshape(-1, 3)
    c1, s1, c12, s12 = (np.asarray(a, dtype=np.float64)[..., None] for a in (c1, s1, c12, s12))
    cx, cy = d[:, 0], d[:, 1]

    def seg(px, py, ux, uy, L):
        s = px * ux + py * uy
        t = np.clip(s, 0.0, L)
        return np.hypot(px - t * ux, py - t * uy), t != s

    d1, k1 = seg(cx, cy, c1, s1, fk1)
    d2, k2 = seg(cx - fk1 * c1, cy - fk1 * s1, c12, s12, fk2)
    return np.stack([d1, d2], -1), np.stack([k1, k2], -1)


def touch_mask(dist, discs):
    """The masks of mppi_debug_obstacle_hits from segment_test's distances: bit 2j link 1 touches disc j,
    bit 2j + 1 link 2 does (uint32, dist's shape without its last two axes)."""
    r = np.asarray(discs, dtype=np.float64).reshape(-1, 3)[:, 2]
    hit = dist < r[:, None]
    n = hit.shape[-2]
    bits = (np.uint32(1) << np.arange(2 * n, dtype=np.uint32)).reshape(n, 2)
    return np.sum(np.where(hit, bits, np.uint32(0)), axis=(-1, -2), dtype=np.uint32)


def clearance(dist, discs):
    """|d - r| of the nearest boundary over discs and links (inf without discs)."""
    r = np.asarray(discs, dtype=np.float64).reshape(-1, 3)[:, 2]
    gap = np.abs(dist - r[:, None])
    return gap.reshape(gap.shape[:-2] + (-1,)).min(-1) if gap.shape[-2] else np.full(gap.shape[:-2], np.inf)


def collides(q1, q2, discs, p: ArmParams = ArmParams()):
    """(flag, clearance, dist, clipped) of the states (q1, q2) against the discs: a state collides when either
    link touches a disc, its distance to the centre (segment_test) ``< r``."""
    dist, clipped = segment_test(np.cos(q1), np.sin(q1), np.cos(q1 + q2), np.sin(q1 + q2), discs, p.fk_l1, p.fk_l2)
    r = np.asarray(discs, dtype=np.float64).reshape(-1, 3)[:, 2]
    flag = np.any(dist < r[:, None], axis=(-1, -2))
    return flag, clearance(dist, discs), dist, clipped


def masks_over_horizon(segments, touch, dirs, discs, vel, dt, shift=0):
    """The fp64 predicate on recorded direction values dirs (K, T, ...), step t against discs_at(t): (mask (K, T)
    of ``touch(dist, discs)``, gap (K, T) + dist's = |dist - r|), dist from ``segments(dirs[:, t], discs)``."""
    dirs = np.asarray(dirs, dtype=np.float64)
    mask, gap = [], []
    for t in range(dirs.shape[1]):
        d = discs_at(discs, vel, t, dt, shift)
        dist = segments(dirs[:, t], d)
        mask.append(touch(dist, d))
        gap.append(np.abs(dist - d[:, 2][:, None]))
    return np.stack(mask, 1), np.stack(gap, 1)


def moving_masks(dirs, discs, vel, dt, fk1=1.0, fk2=1.0, shift=0):
    """masks_over_horizon for the arm, dirs (K, T, 4) = (c1, s1, c12, s12): mask uint32 as
    mppi_debug_obstacle_hits lays it out, gap (K, T, n, 2)."""
    return masks_over_horizon(lambda a, d: segment_test(a[:, 0], a[:, 1], a[:, 2], a[:, 3], d, fk1, fk2)[0],
                              touch_mask, dirs, discs, vel, dt, shift)


def compute_weights(S, lam):
    """``_compute_weights`` (control.py:297-314), sequential sums as in the loops."""
    rho = S.min()
    e = np.exp((-1.0 / lam) * (S - rho))
    eta = np.cumsum(e)[-1] if e.size else 0.0
    return (1.0 / eta) * e


def weighted_noise(w, eps):
    """control.py:115-118: w_eps[t] = sum_k w[k] eps[k,t], k in order."""
    return np.cumsum(w[:, None, None] * eps.astype(np.float64), axis=0)[-1]


def median_filter_reflect(x, size=10):
    """``scipy.ndimage.median_filter(x, size, mode='reflect')`` (control.py:325).

    Window [i - size//2, i + size - size//2 - 1], half-sample-symmetric
    ('reflect': d c b a | a b c d | d c b a) boundaries, rank size//2 of the
    sorted window (the UPPER median for even sizes).
    """
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if n < 5 and size == 10:
        # SciPy 1.15.3's 1-D rank filter does not follow its own 'reflect'
        # definition when the input is shorter than half the window (n <= 3
        # returns zeros, n = 4 differs); the reference inherits that, so the
        # pinned dependency itself is the oracle for horizons T < 5.
        from scipy.ndimage import median_filter
        return median_filter(x, size=size, mode="reflect")
    lo = size // 2
    out = np.empty(n)
    for i in range(n):
        idx = np.arange(i - lo, i - lo + size)
        # reflect with period 2n: index -1 -> 0, -2 -> 1, n -> n-1, ...
        m = np.mod(idx, 2 * n)
        m = np.where(m >= n, 2 * n - 1 - m, m)
        out[i] = np.sort(x[m])[size // 2]
    return out


def moving_median_filter(xx, window_size=10):
    """``_moving_median_filter`` (control.py:319-327): per column."""
    out = np.zeros(xx.shape)
    for d in range(xx.shape[1]):
        out[:, d] = median_filter_reflect(xx[:, d], window_size)
    return out


def rollout_trajectory(x0, controls, dt, p: ArmParams = ArmParams()):
    """control.py:129-145: states after each of T steps driven by ``controls`` (..., T, 2)."""
    controls = np.asarray(controls, dtype=np.float64)
    lead = controls.shape[:-2]
    T = controls.shape[-2]
    q1 = np.full(lead, float(x0[0]))
    q2 = np.full(lead, float(x0[1]))
    dq1 = np.full(lead, float(x0[2]))
    dq2 = np.full(lead, float(x0[3]))
    out = np.zeros(lead + (T, 4))
    for t in range(T):
        q1, q2, dq1, dq2 = forward_dynamics(q1, q2, dq1, dq2, controls[..., t, 0], controls[..., t, 1], dt, p)
        out[..., t, 0] = q1
        out[..., t, 1] = q2
        out[..., t, 2] = dq1
        out[..., t, 3] = dq2
    return out


def update_in_place(model, S, u, eps, lam, x0, dt, lo=None, hi=None, expl=0.0, visualize_optimal_traj=True,
                    sampled=False):
    """The update tail, control.py:112-152, from the costs S: weights, weighted noise, median filter,
    ``u += w_eps``, the trajectories, the shift.  ``u`` (T, n) is updated IN PLACE, as the reference updates its
    ``u_prev``.  With limits the updated nominal is clipped only when ``visualize_optimal_traj`` (``_g`` in
    place, rule 3 of sampled_controls).  Returns w, w_eps_raw, w_eps_filt, u_new (the update before any clip),
    u_seq (``u`` itself, shifted: what the reference returns and keeps), u0 (its first row, the post-shift one),
    optimal_traj and sampled_traj (zeros when off)."""
    K, T, n = eps.shape
    w = compute_weights(S, lam)
    w_eps_raw = weighted_noise(w, eps)
    w_eps_filt = moving_median_filter(w_eps_raw, 10)
    v = sampled_controls(u, eps, lo, hi, expl) if sampled else None   # control.py:139-145: from the pre-update u
    u += w_eps_filt                                                  # control.py:126
    u_new = u.copy()
    optimal_traj = np.zeros((T, 2 * n))
    if visualize_optimal_traj:                                       # control.py:129-134
        if _limits(lo, hi, n) is not None:
            np.clip(u, *_limits(lo, hi, n), out=u)                   # _g(u[t-1]) over every row, in place
        optimal_traj = model.trajectory(x0, np.roll(u, 1, axis=0), dt)
    sampled_traj = np.zeros((K, T, 2 * n))
    if sampled:
        sampled_traj = model.trajectory(x0, np.roll(v, 1, axis=1), dt)
    u[:-1] = u[1:]                                                   # control.py:148-149 (the last row stays)
    return dict(w=w, w_eps_raw=w_eps_raw, w_eps_filt=w_eps_filt, u_new=u_new, u_seq=u, u0=u[0],
                optimal_traj=optimal_traj, sampled_traj=sampled_traj)


def update(S, u_prev, eps, lam, x0, dt, lo=None, hi=None, visualize_optimal_traj=True, p: ArmParams = ArmParams()):
    """update_in_place for the arm on a copy of ``u_prev``: the tail from costs S that a test composed itself."""
    return update_in_place(arm_model(p), S, np.array(u_prev, dtype=np.float64), eps, lam, x0, dt, lo, hi, 0.0,
                           visualize_optimal_traj)


def model_step(model, x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
               gamma=None, *, lo=None, hi=None, discs=None, vel=None, obstacle_cost=0.0, hits=None, clearance=None,
               self_cost=0.0, self_hits=None, visualize_optimal_traj=True, sampled=False):
    """One calc_control_input of either model after its waypoint update (control.py:81-152), with limits,
    (moving) discs and the self-collision cost when given; ``prev_idx`` is the updated index.
    collision_costs(details=True)'s dict joined with update_in_place's.  ``hits`` / ``self_hits`` (K,), when either
    is given, replace the yardstick's own hit counts in S (the device's: a state within rounding of a boundary may
    fall on either side, and must not move a weight), a None entry the yardstick's own:
    S = (S_track + obstacle_cost hits) + self_cost hits_self, the second addend only with a ``clearance``."""
    u = np.array(u_prev, dtype=np.float64)
    out = collision_costs(model, x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl,
                          gamma=gamma, lo=lo, hi=hi, discs=discs, vel=vel, obstacle_cost=obstacle_cost,
                          clearance=clearance, self_cost=self_cost, details=True)
    if hits is not None or self_hits is not None:
        count = lambda given, own: np.asarray(out[own] if given is None else given, dtype=np.float64)  # noqa: E731
        out["S"] = out["S_track"] + obstacle_cost * count(hits, "hits")
        if clearance is not None:
            out["S"] = out["S"] + self_cost * count(self_hits, "hits_self")
    out.update(update_in_place(model, out["S"], u, eps, lam, x0, dt, lo, hi, expl, visualize_optimal_traj, sampled))
    return out


def step(x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
         p: ArmParams = ArmParams(), gamma=None, **kw):
    """model_step for the arm, with its keywords: lo, hi, discs, vel, obstacle_cost, hits, visualize_optimal_traj,
    sampled."""
    return model_step(arm_model(p), x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl,
                      gamma, **kw)


class OracleController:
    """Stateful restatement of ``MPPIControllerForPathTracking`` (control.py:20-152)."""

    def __init__(self, delta_t=0.01, ref_path=0, horizon_step_T=20, number_of_samples_K=500,
                 param_exploration=0.0, param_lambda=50.0, param_alpha=1.0,
                 sigma=np.array([[10.0, 10.0], [100.0, 100.0]]),
                 stage_cost_weight=np.array([10.0, 10.0, 10.0, 10.0]),
                 terminal_cost_weight=np.array([10.0, 10.0, 10.0, 10.0]),
                 visualize_optimal_traj=True, visualze_sampled_trajs=False,
                 arm: ArmParams = ArmParams(), *, u_min=None, u_max=None, obstacles=None, obstacle_cost=1.0e10):
        self.dim_x, self.dim_u = 4, 2
        self.T, self.K = horizon_step_T, number_of_samples_K
        self.param_exploration = param_exploration
        self.param_lambda = param_lambda
        self.param_alpha = param_alpha
        self.param_gamma = param_lambda * (1.0 - param_alpha)
        self.Sigma = sigma
        self.stage_cost_weight = stage_cost_weight
        self.terminal_cost_weight = terminal_cost_weight
        self.visualize_optimal_traj = visualize_optimal_traj
        self.visualze_sampled_trajs = visualze_sampled_trajs
        self.delta_t = delta_t
        self.ref_path = ref_path
        self.arm = arm
        self.u_min, self.u_max, self.obstacles, self.obstacle_cost = u_min, u_max, obstacles, obstacle_cost
        self.u_prev = np.array([[10.0, -2.0] for _ in range(self.T)])
        self.prev_waypoints_idx = 0
        self.last = {}

    def _calc_epsilon(self, sigma, size_sample, size_time_step, size_dim_u):
        """control.py:154-164."""
        if sigma.shape[0] != sigma.shape[1] or sigma.shape[0] != size_dim_u or size_dim_u < 1:
            raise ValueError
        return np.random.multivariate_normal(np.zeros(size_dim_u), sigma, (size_sample, size_time_step))

    def calc_control_input(self, observed_x, epsilon=None):
        u = self.u_prev
        x0 = np.asarray(observed_x, dtype=np.float64)
        idx, *_ = nearest_waypoint(x0[0], x0[1], self.ref_path, self.prev_waypoints_idx, self.arm)
        self.prev_waypoints_idx = int(idx)                              # control.py:75,230
        if self.prev_waypoints_idx >= self.ref_path.shape[0] - 1:      # control.py:76-78
            raise IndexError
        eps = self._calc_epsilon(self.Sigma, self.K, self.T, self.dim_u) if epsilon is None else \
            np.asarray(epsilon, dtype=np.float64)
        S = rollout_costs(x0, u, eps, self.ref_path, self.prev_waypoints_idx, self.delta_t,
                          self.param_lambda, self.param_alpha, self.Sigma,
                          self.stage_cost_weight, self.terminal_cost_weight,
                          self.param_exploration, self.arm, gamma=self.param_gamma, lo=self.u_min, hi=self.u_max,
                          discs=self.obstacles, obstacle_cost=self.obstacle_cost)
        r = update_in_place(arm_model(self.arm), S, u, eps, self.param_lambda, x0, self.delta_t, self.u_min,
                            self.u_max, self.param_exploration, self.visualize_optimal_traj,
                            self.visualze_sampled_trajs)
        self.last = dict(S=S, eps=eps, **r)
        return r["u0"], u, r["optimal_traj"], r["sampled_traj"]
