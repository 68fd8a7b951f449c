"""Test yardstick: the reference MPPI step with its clamp hook ``_g`` switched on, in vectorised fp64 NumPy.

``_g`` (control.py:166-172) ships with its two ``np.clip`` lines commented out.
Enabled, it clips its argument IN PLACE, and every argument it is given is a
view (``v[k, t-1]``, ``u[t-1]``), so:

  1. rollout (control.py:97-106): ``v = clip(u[t-1] + eps)`` (``clip(eps)`` for an
     exploration sample); ``_F`` and the control cost ``gamma u^T Sigma^-1 v`` take
     the clipped ``v``;
  2. weights and weighted noise (control.py:112-118): unchanged, the UNCLAMPED eps;
  3. update (control.py:126-134): ``u += w_eps`` is not clipped by itself; the
     optimal-trajectory loop calls ``_g(u[t-1])`` for every row, which clips the
     whole updated ``u`` in place — only when ``visualize_optimal_traj``;
  4. sampled trajectories (control.py:139-145): re-rolled from the clipped ``v``.

The dynamics, cost, weights and median filter are ``oracle/mppi_oracle.py``'s,
unchanged.  ``tests/test_clamp_cpu.py`` pins this restatement to the fixtures
captured from the reference itself (``tests/golden/make_golden_clamp.py``); the GPU
tests then use it at shapes the fixtures do not cover.
"""
from __future__ import annotations

import glob
import os

import numpy as np

import mppi_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the fixtures' names (tests/conftest.py globs step_* / loop_* into the unclamped tests: these keep clear of both)
CLAMP_STEPS = sorted(os.path.basename(f)[len("clamp_step_"):-4] for f in glob.glob(os.path.join(GOLDEN, "clamp_step_*.npz")))


def load_clamp_step(name):
    return dict(np.load(os.path.join(GOLDEN, f"clamp_step_{name}.npz")))


def load_clamp_loop(name):
    return dict(np.load(os.path.join(GOLDEN, f"clamp_loop_{name}.npz")))


def _lim(x):
    return np.broadcast_to(np.asarray(x, dtype=np.float64), (2,))


def sampled_controls(u, eps, lo, hi, expl=0.0, k_offset=0, K_total=None):
    """v (K, T, 2): clip(u + eps) for the exploitation samples, clip(eps) for the rest (control.py:98-104)."""
    K = eps.shape[0]
    K_total = K if K_total is None else K_total
    exploit = ((np.arange(K) + k_offset) < (1.0 - expl) * K_total)[:, None, None]
    e = eps.astype(np.float64)
    return np.clip(np.where(exploit, u[None] + e, e), _lim(lo), _lim(hi))


def rollout_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, lo, hi,
                  expl=0.0, p: O.ArmParams = O.ArmParams(), k_offset=0, K_total=None, gamma=None):
    """S (K,) of control.py:81-109 with the clamp: O.rollout_costs with v clipped before _F and the control cost."""
    K, T, _ = eps.shape
    if gamma is None:
        gamma = lam * (1.0 - alpha)
    sig_inv = np.linalg.inv(sigma)
    v = sampled_controls(u, eps, lo, hi, expl, k_offset, K_total)
    S = np.zeros(K)
    q1, q2, dq1, dq2 = (np.full(K, float(x0[i])) for i in range(4))
    for t in range(1, T + 1):
        v1, v2 = v[:, t - 1, 0], v[:, t - 1, 1]
        q1, q2, dq1, dq2 = O.forward_dynamics(q1, q2, dq1, dq2, v1, v2, dt, p)
        c = O.state_cost(q1, q2, dq1, dq2, ref_path, prev_idx, stage_w, p)
        a = (gamma * u[t - 1].T) @ sig_inv
        S = S + (c + (a[0] * v1 + a[1] * v2))
    return S + O.state_cost(q1, q2, dq1, dq2, ref_path, prev_idx, term_w, p)


def step(x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, lo, hi, expl=0.0,
         visualize_optimal_traj=True, sampled=False, p: O.ArmParams = O.ArmParams(), gamma=None):
    """One calc_control_input after its waypoint update (control.py:81-152) with the clamp; `prev_idx` is the
    updated index.  Returns S, w, w_eps_raw, w_eps_filt, u_new (the update before any clip), u_seq (what the
    reference returns and keeps: clipped when visualize_optimal_traj, then shifted), u0, optimal_traj and
    sampled_traj (zeros when off)."""
    u = np.array(u_prev, dtype=np.float64)
    K, T, _ = eps.shape
    S = rollout_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, lo, hi, expl, p,
                      gamma=gamma)
    w = O.compute_weights(S, lam)
    w_raw = O.weighted_noise(w, eps)
    w_filt = O.moving_median_filter(w_raw, 10)
    u_new = u + w_filt
    un = u_new.copy()
    opt = np.zeros((T, 4))
    if visualize_optimal_traj:
        un = np.clip(un, _lim(lo), _lim(hi))                     # _g(u[t-1]) over every row, in place
        opt = O.rollout_trajectory(x0, np.roll(un, 1, axis=0), dt, p)
    samp = np.zeros((K, T, 4))
    if sampled:
        v = sampled_controls(u, eps, lo, hi, expl)
        samp = O.rollout_trajectory(x0, np.roll(v, 1, axis=1), dt, p)
    u_seq = np.concatenate([un[1:], un[-1:]], 0)
    return dict(S=S, w=w, w_eps_raw=w_raw, w_eps_filt=w_filt, u_new=u_new, u_seq=u_seq, u0=u_seq[0].copy(),
                optimal_traj=opt, sampled_traj=samp)
