"""Test yardstick: the reference MPPI step with a collision cost on both links, in vectorised fp64 NumPy.

The reference with ONLY ``_c`` and ``_phi`` (control.py:174-198) overridden to return
``... + w * collides(x)``, the penalty added after the x 10000: every step of the horizon
whose new state collides adds ``w`` to its sample's cost and the final state adds it once
more, so ``S = S_track + w * hits`` with ``hits`` in ``[0, T + 1]``.  A state collides when
either link touches a disc ``(cx, cy, r)``.  A link is a zero-thickness segment in the
cost's kinematics (``fk_l1``, ``fk_l2``, base at the origin, as ``_c`` computes x and y):
link 1 from (0, 0) to e = fk_l1 (cos q1, sin q1), link 2 from e to
e + fk_l2 (cos(q1 + q2), sin(q1 + q2)); "touches": the distance from the centre to the
segment, the projection parameter clipped to the segment, is ``< r``.

The dynamics, the tracking cost, the weights, the median filter and the clamp are
``oracle/mppi_oracle.py``'s and ``tests/clamp_ref.py``'s, unchanged.
``tests/test_obstacle_cpu.py`` pins this restatement to the fixtures captured from the
reference itself (``tests/golden/make_golden_obstacle.py``); the GPU tests then use it at
shapes the fixtures do not cover, and ``segment_test`` on the device's own recorded
directions.
"""
from __future__ import annotations

import glob
import os

import numpy as np

import clamp_ref as CR
import mppi_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OBST_STEPS = sorted(os.path.basename(f)[len("obst_step_"):-4] for f in glob.glob(os.path.join(GOLDEN, "obst_step_*.npz")))
INF2 = (-np.inf, -np.inf), (np.inf, np.inf)


def load_obst_step(name):
    return dict(np.load(os.path.join(GOLDEN, f"obst_step_{name}.npz")))


def load_obst_loop(name):
    return dict(np.load(os.path.join(GOLDEN, f"obst_loop_{name}.npz")))


def segment_test(c1, s1, c12, s12, discs, fk1=1.0, fk2=1.0):
    """Both links against every disc from the direction values (any common shape): returns
    (dist (..., n, 2) fp64, the distance from disc j's centre to link 1 / link 2, and clipped (..., n, 2),
    whether the projection parameter was clipped to an end of the segment)."""
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


def collides(q1, q2, discs, p: O.ArmParams = O.ArmParams()):
    """(flag, clearance, dist, clipped) of the states (q1, q2) against the discs."""
    dist, clipped = segment_test(np.cos(q1), np.sin(q1), np.cos(q1 + q2), np.sin(q1 + q2), discs, p.fk_l1, p.fk_l2)
    r = np.asarray(discs, dtype=np.float64).reshape(-1, 3)[:, 2]
    flag = np.any(dist < r[:, None], axis=(-1, -2))
    return flag, clearance(dist, discs), dist, clipped


def rollout(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, discs, w, lo=None, hi=None,
            expl=0.0, p: O.ArmParams = O.ArmParams(), k_offset=0, K_total=None, gamma=None):
    """control.py:81-109 with the collision cost (and, with lo / hi, the clamp).  Returns a dict: S (K,), S_track
    (K,) (the same loop without the penalty), flag (K, T) bool per step's new state, clear (K, T) clearance,
    hits (K,) = flag.sum(1) + flag[:, -1], dist (K, T, n, 2), clipped (K, T, n, 2), ee (K, T, 2) end effector, q (K, T, 2) joint angles, dq (K, T, 2) joint rates."""
    K, T, _ = eps.shape
    if gamma is None:
        gamma = lam * (1.0 - alpha)
    lo, hi = (INF2[0] if lo is None else lo), (INF2[1] if hi is None else hi)
    sig_inv = np.linalg.inv(sigma)
    v = CR.sampled_controls(u, eps, lo, hi, expl, k_offset, K_total)
    n = np.asarray(discs, dtype=np.float64).reshape(-1, 3).shape[0]
    S, St = np.zeros(K), np.zeros(K)
    flag, clear = np.zeros((K, T), dtype=bool), np.zeros((K, T))
    dist, clipped = np.zeros((K, T, n, 2)), np.zeros((K, T, n, 2), dtype=bool)
    ee, q, dqs = np.zeros((K, T, 2)), np.zeros((K, T, 2)), np.zeros((K, T, 2))
    q1, q2, dq1, dq2 = (np.full(K, float(x0[i])) for i in range(4))
    for t in range(1, T + 1):
        v1, v2 = v[:, t - 1, 0], v[:, t - 1, 1]
        q1, q2, dq1, dq2 = O.forward_dynamics(q1, q2, dq1, dq2, v1, v2, dt, p)
        c = O.state_cost(q1, q2, dq1, dq2, ref_path, prev_idx, stage_w, p)
        flag[:, t - 1], clear[:, t - 1], dist[:, t - 1], clipped[:, t - 1] = collides(q1, q2, discs, p)
        ee[:, t - 1, 0] = p.fk_l1 * np.cos(q1) + p.fk_l2 * np.cos(q1 + q2)
        ee[:, t - 1, 1] = p.fk_l1 * np.sin(q1) + p.fk_l2 * np.sin(q1 + q2)
        q[:, t - 1, 0], q[:, t - 1, 1] = q1, q2
        dqs[:, t - 1, 0], dqs[:, t - 1, 1] = dq1, dq2
        a = (gamma * u[t - 1].T) @ sig_inv
        ctrl = a[0] * v1 + a[1] * v2
        S = S + ((c + w * flag[:, t - 1]) + ctrl)
        St = St + (c + ctrl)
    phi = O.state_cost(q1, q2, dq1, dq2, ref_path, prev_idx, term_w, p)
    S = S + (phi + w * flag[:, -1])
    St = St + phi
    return dict(S=S, S_track=St, flag=flag, clear=clear, hits=flag.sum(1) + flag[:, -1], dist=dist, clipped=clipped,
                ee=ee, q=q, dq=dqs)


def waypoint_pick_delta(r, slots, window, stage_w, term_w):
    """The other discontinuity of the cost: the nearest-waypoint argmin inside _c (control.py:205-215).  Where the
    fp64 end effector lies within fp32 resolution of the bisector between two window slots, the device may pick the
    neighbour; the states do not depend on the pick, so S then differs by exactly those steps' cost difference
    between the two slots.  From rollout()'s dict `r` and the device's own picks `slots` (K, T) (mppi_debug_nearest):
    (delta (K,) to add to the fp64 S, gap (K, T) the distance to the picked slot minus the distance to the fp64
    nearest, 0 where the picks agree, differ (K, T) bool)."""
    win = np.asarray(window, dtype=np.float64)
    x, y, dq = r["ee"][..., 0], r["ee"][..., 1], r["dq"]
    d = (x[..., None] - win[:, 0]) ** 2 + (y[..., None] - win[:, 1]) ** 2
    j1 = O.first_min_index(d * 100)
    jd = np.asarray(slots, dtype=np.int64)
    T = x.shape[1]
    w = np.tile(np.asarray(stage_w, dtype=np.float64), (T, 1))
    w[-1] += np.asarray(term_w, dtype=np.float64)          # the terminal cost takes the same slot

    def cost(j):
        ref = win[j]
        return 10000 * (w[:, 0] * (x - ref[..., 0]) ** 2 + w[:, 1] * (y - ref[..., 1]) ** 2 +
                        w[:, 2] * (dq[..., 0] - ref[..., 2]) ** 2 + w[:, 3] * (dq[..., 1] - ref[..., 3]) ** 2)

    differ = jd != j1
    delta = np.where(differ, cost(jd) - cost(j1), 0.0).sum(1)
    take = lambda j: np.sqrt(np.take_along_axis(d, j[..., None], -1)[..., 0])
    return delta, np.where(differ, take(jd) - take(j1), 0.0), differ


def update(S, u_prev, eps, lam, x0, dt, lo=None, hi=None, visualize_optimal_traj=True,
           p: O.ArmParams = O.ArmParams()):
    """control.py:112-152 from the costs S: w, w_eps_raw, w_eps_filt, u_new, u_seq, u0, optimal_traj (with
    limits and visualize_optimal_traj the updated nominal is clipped, as clamp_ref.step)."""
    u = np.array(u_prev, dtype=np.float64)
    T = u.shape[0]
    w = O.compute_weights(S, lam)
    w_raw = O.weighted_noise(w, eps)
    w_filt = O.moving_median_filter(w_raw, 10)
    u_new = u + w_filt
    un = u_new.copy()
    opt = np.zeros((T, 4))
    if visualize_optimal_traj:
        if lo is not None or hi is not None:
            un = np.clip(un, CR._lim(INF2[0] if lo is None else lo), CR._lim(INF2[1] if hi is None else hi))
        opt = O.rollout_trajectory(x0, np.roll(un, 1, axis=0), dt, p)
    u_seq = np.concatenate([un[1:], un[-1:]], 0)
    return dict(w=w, w_eps_raw=w_raw, w_eps_filt=w_filt, u_new=u_new, u_seq=u_seq, u0=u_seq[0].copy(),
                optimal_traj=opt)


def step(x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, discs, w, lo=None, hi=None,
         expl=0.0, visualize_optimal_traj=True, p: O.ArmParams = O.ArmParams(), gamma=None):
    """One calc_control_input after its waypoint update (control.py:81-152) with the collision cost;
    `prev_idx` is the updated index.  rollout()'s dict joined with update()'s."""
    u = np.array(u_prev, dtype=np.float64)
    out = rollout(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, discs, w, lo, hi, expl,
                  p, gamma=gamma)
    out.update(update(out["S"], u, eps, lam, x0, dt, lo, hi, visualize_optimal_traj, p))
    return out
