"""CPU ORACLE — test infrastructure only, never shipped, never on the product path.

fp64 NumPy restatement of the n-link planar-chain MPPI step that this build
defines for SURVEY §8 f4 / BASELINE config 5 ("7-DoF arm dynamics (extended
sys_params.py), K=131072 T=128, xydq_circle.txt reference").  The reference has
no 7-DoF model, so the model is BUILD-DEFINED and parity at n = 7 is UNPINNED by
the reference.  What IS pinned: at n = 2 with the reference's constants and its
mass-matrix convention (link inertia I_i := l_i, control.py:241-245) the chain
dynamics reduce term by term to the reference ``_F`` (control.py:234-263);
``tests/test_chain_oracle.py`` checks that against ``mppi_oracle`` (itself pinned
to the reference fixtures) and checks the whole n = 2 chain step against the
reference's golden steps.

Model (planar chain, joint angles q, absolute angles theta = S q, S = lower-
triangular ones, so theta_a = q_1 + ... + q_a):

  kinetic energy  T = 1/2 theta_dot^T D(theta) theta_dot,
                  D_ab = mu_ab cos(theta_a - theta_b) + delta_ab I_a
  mu_ab (a < b)   = l_a (m_b lc_b + l_b sum_{k>b} m_k)          (constant)
  mu_aa           = m_a lc_a^2 + l_a^2 sum_{k>a} m_k
  bias            c_a = sum_b mu_ab sin(theta_a - theta_b) theta_dot_b^2
  gravity         g_a = g nu_a cos theta_a,  nu_a = m_a lc_a + l_a sum_{k>a} m_k
  joint drives    armature (rotor inertia) J_a and viscous damping b_a per joint: the
                  joint-space mass matrix S^T D S + diag(J) is, in theta-space,
                  D' = D + S^-T diag(J) S^-1  (diagonal + J_a + J_{a+1}, first
                  off-diagonal - J_{a+1}); the joint torques are u - b dq
  joint torques   u' = u - b dq map to theta-space as tau_a = u'_a - u'_{a+1}  (u'_{n+1} = 0)
  D' theta_ddot = tau - c - g;  q_ddot_1 = theta_ddot_1, q_ddot_a = theta_ddot_a - theta_ddot_{a-1}
  semi-implicit Euler as control.py:256-259: dq += q_ddot dt; q += dq dt

(At n = 2 with J = b = 0: M = S^T D S gives M11 = m1 lc1^2 + m2 l1^2 + I1 + 2 m2 l1 lc2 c2 + m2 lc2^2 + I2,
M12 = m2 l1 lc2 c2 + m2 lc2^2 + I2, M22 = m2 lc2^2 + I2 — control.py:241-245 with I = l.)

Cost: end-effector (x, y) from forward kinematics with the fk
lengths, the windowed nearest waypoint of control.py:200-232, and the
reference's 4-term weighted squared error x 10000 on (x, y, dq_1, dq_2) against
xydq_circle.txt's (x, y, dq1, dq2) columns; control cost (gamma u_t^T Sigma^-1) v
(control.py:106) with the n x n Sigma; weights / weighted noise / median filter /
update / shift exactly as the 2-DoF step (control.py:112-152).

Workspace obstacles (discs, at rest or moving): the arm's collision cost
(O.collision_costs) with every link of the chain tested (chain_collides); a
state collides when any link touches any disc.  At n = 2 with
ChainParams.from_arm2() it is the arm's definition (test_chain_obstacle_cpu.py,
test_chain_moving_obstacle_cpu.py).

Self-collision (mppi_chain_set_self_collision).  Joint j of the chain is
b_{j-1} = sum_{i < j} fk_i (cos th_i, sin th_i) (joint 0 the origin, joint n the
tip), link a the zero-thickness segment from joint a to joint a + 1.  For every
pair of links a < b with b >= a + 2:

  * e(a, b): the smallest of the four endpoint-to-segment distances (the ends of
    b against a, the ends of a against b), each with the projection on the link's
    direction clipped to [0, fk] as chain_segment_test clips it;
  * x(a, b): the segments cross properly, the two ends of each strictly on
    opposite sides of the other's line;
  * the pair self-collides when x(a, b) or e(a, b) < d, d >= 0 the clearance
    (d = 0: crossings only).

A state self-collides when any pair does.  Every step of the horizon whose new
state self-collides adds the cost to its sample's S, the final state once more,
in the discs' one penalty (O.collision_costs' ``clearance`` and ``self_cost``):
S = S_track + obstacle_cost hits + self_cost hits_self, each count in
[0, T + 1].  The pairs are enumerated a ascending, then b ascending
(chain_self_pairs); bit i of a mask (uint32) is pair i.  Pinned by
test_chain_self_collision_cpu.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import mppi_oracle as O

MAX_DOF = 8


def _default(v):
    return field(default_factory=lambda: tuple(v))


@dataclass(frozen=True)
class ChainParams:
    """Link constants of an n-link planar chain (build-defined 'extended sys_params')."""
    m: tuple = _default([1.0] * 7)
    l: tuple = _default([2.0 / 7.0] * 7)
    lc: tuple = _default([1.0 / 7.0] * 7)
    I: tuple = _default([(2.0 / 7.0) ** 2 / 12.0] * 7)   # slender rods, m l^2 / 12
    fk: tuple = _default([2.0 / 7.0] * 7)                # lengths used by the cost's kinematics
    J: tuple = _default([0.1] * 7)                       # joint armature (rotor inertia), kg m^2
    b: tuple = _default([1.0] * 7)                       # joint viscous damping, N m s / rad
    g: float = 9.81

    @property
    def n(self) -> int:
        return len(self.m)

    @staticmethod
    def from_arm2(a: O.ArmParams = O.ArmParams()) -> "ChainParams":
        """The reference 2-link model (control.py:11-18, 241-245): inertia := link length."""
        return ChainParams(m=(a.m1, a.m2), l=(a.l1, a.l2), lc=(a.lc1, a.lc2), I=(a.l1, a.l2),
                           fk=(a.fk_l1, a.fk_l2), J=(0.0, 0.0), b=(0.0, 0.0), g=a.g)


def coefficients(P: ChainParams):
    """(mu n x n, nu n, D' diagonal n): the constant parts of D' and gravity."""
    n = P.n
    m, l, lc = map(np.asarray, (P.m, P.l, P.lc))
    tail = np.array([m[k + 1:].sum() for k in range(n)])        # sum_{k>a} m_k
    mu = np.zeros((n, n))
    for a in range(n):
        mu[a, a] = m[a] * lc[a] ** 2 + l[a] ** 2 * tail[a]
        for b in range(a + 1, n):
            mu[a, b] = mu[b, a] = l[a] * (m[b] * lc[b] + l[b] * tail[b])
    nu = m * lc + l * tail
    J = np.asarray(P.J, dtype=np.float64)
    return mu, nu, np.diag(mu) + np.asarray(P.I) + J + np.append(J[1:], 0.0)


def chain_forward_dynamics(q, dq, v, dt, P: ChainParams):
    """One semi-implicit Euler step of the chain, vectorised over leading dims (..., n)."""
    mu, nu, Dd = coefficients(P)
    th = np.cumsum(q, axis=-1)
    thd = np.cumsum(dq, axis=-1)
    dth = th[..., :, None] - th[..., None, :]                   # theta_a - theta_b
    D = mu * np.cos(dth)
    idx = np.arange(P.n)
    D[..., idx, idx] = Dd
    J = np.asarray(P.J, dtype=np.float64)
    D[..., idx[:-1], idx[1:]] -= J[1:]
    D[..., idx[1:], idx[:-1]] -= J[1:]
    c = np.einsum("ab,...ab,...b->...a", mu, np.sin(dth), thd ** 2)
    gt = P.g * nu * np.cos(th)
    ve = v - np.asarray(P.b) * dq
    tau = ve - np.concatenate([ve[..., 1:], np.zeros(ve.shape[:-1] + (1,))], axis=-1)
    thdd = np.linalg.solve(D, (tau - c - gt)[..., None])[..., 0]
    qdd = np.diff(thdd, axis=-1, prepend=0.0)
    dq_n = dq + qdd * dt
    q_n = q + dq_n * dt
    return q_n, dq_n


def chain_fk(q, P: ChainParams):
    """End effector (x, y) with the cost's link lengths."""
    th = np.cumsum(q, axis=-1)
    fk = np.asarray(P.fk)
    return (fk * np.cos(th)).sum(-1), (fk * np.sin(th)).sum(-1)


def nearest_waypoint_xy(x, y, ref_path, prev_idx):
    """control.py:200-232 on an end-effector position (d.index(min(d)), O.first_min_index)."""
    win = ref_path[prev_idx:prev_idx + O.SEARCH_IDX_LEN]
    d = ((np.asarray(x)[..., None] - win[:, 0]) ** 2 + (np.asarray(y)[..., None] - win[:, 1]) ** 2) * 100
    idx = O.first_min_index(d) + prev_idx
    return idx, ref_path[idx, 0], ref_path[idx, 1], ref_path[idx, 2], ref_path[idx, 3]


def chain_state_cost(q, dq, ref_path, prev_idx, weight, P: ChainParams):
    """control.py:174-198 on (x, y, dq_1, dq_2) of the chain."""
    x, y = chain_fk(q, P)
    _, rx, ry, r1, r2 = nearest_waypoint_xy(x, y, ref_path, prev_idx)
    c = weight[0] * (x - rx) ** 2 + weight[1] * (y - ry) ** 2 + \
        weight[2] * (dq[..., 0] - r1) ** 2 + weight[3] * (dq[..., 1] - r2) ** 2
    return c * 10000


def chain_segment_test(c, s, discs, fk):
    """Every link against every disc from the direction values c, s (..., n): (dist (..., nd, n) fp64, the distance
    from disc j's centre to link a with the projection clipped to the segment; clipped (..., nd, n) int8, -1 / +1
    where the projection was clipped to the link's base / tip, 0 where it is interior).

    Link a (0-based) is the zero-thickness segment from b_{a-1} to b_a, b_a = sum_{i <= a} fk_i (cos th_i, sin th_i)
    with b_{-1} the origin, th the absolute angles and fk the cost's link lengths (chain_fk's).  At n = 2 with
    ChainParams.from_arm2() this is O.segment_test (test_chain_obstacle_cpu.py)."""
    d = np.asarray(discs, dtype=np.float64).reshape(-1, 3)
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    fk = np.asarray(fk, dtype=np.float64)
    bx = np.cumsum(fk * c, -1) - fk * c            # base of link a: b_{a-1}
    by = np.cumsum(fk * s, -1) - fk * s
    px = d[:, 0][:, None] - bx[..., None, :]       # (..., nd, n)
    py = d[:, 1][:, None] - by[..., None, :]
    ux, uy = c[..., None, :], s[..., None, :]
    pr = px * ux + py * uy
    t = np.clip(pr, 0.0, fk)
    dist = np.hypot(px - t * ux, py - t * uy)
    clipped = np.where(pr < 0.0, -1, np.where(pr > fk, 1, 0)).astype(np.int8)
    return dist, clipped


def chain_self_pairs(n):
    """The non-adjacent link pairs in mask order: (0, 2), (0, 3), ..., (1, 3), ...: (n - 1)(n - 2) / 2 of them."""
    return [(a, b) for a in range(n) for b in range(a + 2, n)]


def chain_joints(c, s, fk):
    """(jx, jy), each (..., n + 1): joint j = b_{j-1} from the direction values c, s (..., n)."""
    c, s, fk = (np.asarray(v, dtype=np.float64) for v in (c, s, fk))
    z = np.zeros(c.shape[:-1] + (1,))
    return (np.concatenate([z, np.cumsum(fk * c, -1)], -1), np.concatenate([z, np.cumsum(fk * s, -1)], -1))


def chain_self_test(c, s, fk, d=0.0):
    """Every non-adjacent link pair from the direction values c, s (..., n): (e (..., P) fp64, x (..., P) bool,
    mask (...) uint32) over the P = len(chain_self_pairs(n)) pairs; bit i of mask is pair i in self-collision: x or
    e < d.  n = 2: no pairs, mask 0."""
    c, s, fk = (np.asarray(v, dtype=np.float64) for v in (c, s, fk))
    pairs = chain_self_pairs(c.shape[-1])
    jx, jy = chain_joints(c, s, fk)

    def point_link(j, L):
        """(distance, signed perpendicular offset) of joint j from link L, the projection clipped to [0, fk_L]."""
        px, py = jx[..., j] - jx[..., L], jy[..., j] - jy[..., L]
        ux, uy = c[..., L], s[..., L]
        pr = px * ux + py * uy
        t = np.clip(pr, 0.0, fk[L])
        return np.hypot(px - t * ux, py - t * uy), ux * py - uy * px

    e = np.zeros(c.shape[:-1] + (len(pairs),))
    x = np.zeros(e.shape, dtype=bool)
    mask = np.zeros(c.shape[:-1], dtype=np.uint32)
    for i, (a, b) in enumerate(pairs):
        d0, s0 = point_link(b, a)                             # the ends of link b against link a
        d1, s1 = point_link(b + 1, a)
        d2, s2 = point_link(a, b)                             # the ends of link a against link b
        d3, s3 = point_link(a + 1, b)
        e[..., i] = np.minimum(np.minimum(d0, d1), np.minimum(d2, d3))
        x[..., i] = (s0 * s1 < 0.0) & (s2 * s3 < 0.0)
        mask |= np.where(x[..., i] | (e[..., i] < d), np.uint32(1 << i), np.uint32(0))
    return e, x, mask


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
    disc (its distance to the centre ``< r``), clearance |dist - r| of the nearest boundary (inf without discs)."""
    th = np.cumsum(np.asarray(q, dtype=np.float64), -1)
    dist, clipped = chain_segment_test(np.cos(th), np.sin(th), discs, P.fk)
    r = np.asarray(discs, dtype=np.float64).reshape(-1, 3)[:, 2]
    flag = np.any(dist < r[:, None], axis=(-1, -2))
    return flag, O.clearance(dist, discs), dist, clipped


def chain_self_collides(q, fk, d):
    """(flag (...), e, x, mask) of the states q (..., n): flag where any non-adjacent pair self-collides
    (chain_self_test at the clearance d)."""
    th = np.cumsum(np.asarray(q, dtype=np.float64), -1)
    e, x, mask = chain_self_test(np.cos(th), np.sin(th), fk, d)
    return mask != 0, e, x, mask


def chain_moving_masks(dirs, discs, vel, dt, fk, shift=0):
    """O.masks_over_horizon for the chain, dirs (K, T, 2 n) = (cos th_a at a, sin th_a at n + a): mask uint64 as
    mppi_chain_debug_obstacle_hits lays it out, gap (K, T, nd, n)."""
    n = np.shape(dirs)[-1] // 2
    return O.masks_over_horizon(lambda a, d: chain_segment_test(a[:, :n], a[:, n:], d, fk)[0], chain_touch_mask,
                                dirs, discs, vel, dt, shift)


def chain_model(P: ChainParams = ChainParams()):
    """The chain for mppi_oracle's horizon loop, collision cost and update tail (O.Model); the state is (q, dq),
    each (K, n)."""
    n = P.n
    return O.Model(start=lambda x0, K: (np.tile(np.asarray(x0[:n], dtype=np.float64), (K, 1)),
                                        np.tile(np.asarray(x0[n:], dtype=np.float64), (K, 1))),
                   step=lambda s, v, dt: chain_forward_dynamics(*s, v, dt, P),
                   cost=lambda s, ref_path, prev_idx, weight: chain_state_cost(*s, ref_path, prev_idx, weight, P),
                   dot=lambda a, v: v @ a,
                   trajectory=lambda x0, controls, dt: chain_rollout_trajectory(x0, controls, dt, P),
                   collides=lambda s, discs: chain_collides(s[0], discs, P),
                   record=lambda s: (np.stack(chain_fk(s[0], P), -1), s[0], s[1]),
                   self_collides=lambda s, d: chain_self_collides(s[0], P.fk, d))


def chain_rollout_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w,
                        expl=0.0, P: ChainParams = ChainParams(), k_offset=0, K_total=None, *, gamma=None,
                        lo=None, hi=None, **kw):
    """O.collision_costs for the chain: the K x T loop (control.py:81-109 with the chain model).  eps (K, T, n);
    returns S (K,), or with ``details=True`` the dict, dist and clipped (K, T, nd, n) of chain_segment_test.
    ``lo`` / ``hi``: torque limits, a scalar or per joint (the four rules of O.sampled_controls, per joint);
    ``discs``, ``vel``, ``obstacle_cost``, ``shift``: the collision cost, as O.rollout_costs'; ``clearance``,
    ``self_cost``: the self-collision cost in the same penalty (None: off).  The dict always has flag_self (K, T),
    e and x (K, T, P) of chain_self_test, mask (K, T) and hits_self (K,), zeros while the self-collision cost is off."""
    return O.collision_costs(chain_model(P), x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w,
                             expl, k_offset, K_total, gamma, lo, hi, **kw)


def step(x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, expl=0.0,
         P: ChainParams = ChainParams(), **kw):
    """O.model_step for the chain, with its keywords: gamma, lo, hi, discs, vel, obstacle_cost, hits, clearance,
    self_cost, self_hits, visualize_optimal_traj, sampled."""
    return O.model_step(chain_model(P), x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w,
                        expl, **kw)


def chain_rollout_trajectory(x0, controls, dt, P: ChainParams = ChainParams()):
    """States (..., T, 2n) driven by ``controls`` (..., T, n) (control.py:129-145 analogue)."""
    controls = np.asarray(controls, dtype=np.float64)
    n = P.n
    lead, T = controls.shape[:-2], controls.shape[-2]
    q = np.broadcast_to(np.asarray(x0[:n], dtype=np.float64), lead + (n,)).copy()
    dq = np.broadcast_to(np.asarray(x0[n:], dtype=np.float64), lead + (n,)).copy()
    out = np.zeros(lead + (T, 2 * n))
    for t in range(T):
        q, dq = chain_forward_dynamics(q, dq, controls[..., t, :], dt, P)
        out[..., t, :n] = q
        out[..., t, n:] = dq
    return out


def gravity_torque(q, P: ChainParams = ChainParams()):
    """Joint torques holding the chain still at q (tau = S^T g_theta): a natural u_prev init."""
    _, nu, _ = coefficients(P)
    g_th = P.g * nu * np.cos(np.cumsum(q))
    return np.cumsum(g_th[::-1])[::-1]


class ChainOracleController:
    """Stateful fp64 restatement of the chain controller (control.py:20-152 with the chain model)."""

    def __init__(self, delta_t, ref_path, horizon_step_T, number_of_samples_K, param_exploration, param_lambda,
                 param_alpha, sigma, stage_cost_weight, terminal_cost_weight, chain: ChainParams = ChainParams(),
                 u_init=None, visualize_optimal_traj=True, visualze_sampled_trajs=False, *, u_min=None, u_max=None):
        self.chain = chain
        self.u_min, self.u_max = u_min, u_max
        self.dim_u, self.dim_x = chain.n, 2 * chain.n
        self.T, self.K = horizon_step_T, number_of_samples_K
        self.param_exploration, self.param_lambda, self.param_alpha = param_exploration, param_lambda, param_alpha
        self.Sigma = np.asarray(sigma, dtype=np.float64)
        self.stage_cost_weight, self.terminal_cost_weight = stage_cost_weight, terminal_cost_weight
        self.delta_t, self.ref_path = delta_t, ref_path
        self.visualize_optimal_traj, self.visualze_sampled_trajs = visualize_optimal_traj, visualze_sampled_trajs
        u0 = np.zeros(self.dim_u) if u_init is None else np.asarray(u_init, dtype=np.float64)
        self.u_prev = np.tile(u0, (self.T, 1)) if u0.ndim == 1 else u0.copy()
        self.prev_waypoints_idx = 0
        self.last = {}

    def calc_control_input(self, observed_x, epsilon):
        n = self.dim_u
        u = self.u_prev
        x0 = np.asarray(observed_x, dtype=np.float64)
        ex, ey = chain_fk(x0[:n], self.chain)
        idx, *_ = nearest_waypoint_xy(ex, ey, self.ref_path, self.prev_waypoints_idx)
        self.prev_waypoints_idx = int(idx)
        if self.prev_waypoints_idx >= self.ref_path.shape[0] - 1:
            raise IndexError
        eps = np.asarray(epsilon, dtype=np.float64)
        S = chain_rollout_costs(x0, u, eps, self.ref_path, self.prev_waypoints_idx, self.delta_t,
                                self.param_lambda, self.param_alpha, self.Sigma, self.stage_cost_weight,
                                self.terminal_cost_weight, self.param_exploration, self.chain,
                                lo=self.u_min, hi=self.u_max)
        r = O.update_in_place(chain_model(self.chain), S, u, eps, self.param_lambda, x0, self.delta_t, self.u_min,
                              self.u_max, self.param_exploration, self.visualize_optimal_traj,
                              self.visualze_sampled_trajs)
        self.last = dict(S=S, eps=eps, **r)
        return r["u0"], u, r["optimal_traj"], r["sampled_traj"]
