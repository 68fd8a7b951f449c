"""Test yardstick: the n-link chain MPPI step with the clamp hook ``_g`` switched on, in vectorised fp64 NumPy.

``tests/clamp_ref.py`` for the chain: the same four rules (control.py:97-145 with ``_g`` clipping in place), per
joint, on ``oracle/chain_oracle.py``'s dynamics, cost, weights and median filter, which are unchanged:

  1. rollout: ``v = clip(u_t + eps)`` (``clip(eps)`` for an exploration sample); the dynamics and the control
     cost ``a_t . v`` take the clipped ``v``;
  2. weights and weighted noise: the UNCLAMPED eps;
  3. update: ``u += w_eps`` is clipped only by the optimal-trajectory loop (``visualize_optimal_traj``);
  4. sampled trajectories: re-rolled from the clipped ``v``.

``tests/test_chain_clamp_cpu.py`` pins it, at n = 2 with the reference arm's constants, to the ``clamp_step_*``
fixtures captured from the reference itself; the GPU tests use it at n = 3 and 7.
"""
from __future__ import annotations

import numpy as np

import chain_oracle as CO
import mppi_oracle as O


def _lim(x, n):
    return np.broadcast_to(np.asarray(x, dtype=np.float64), (n,))


def sampled_controls(u, eps, lo, hi, expl=0.0, k_offset=0, K_total=None):
    """v (K, T, n): clip(u + eps) for the exploitation samples, clip(eps) for the rest (control.py:98-104)."""
    K, _, n = eps.shape
    K_total = K if K_total is None else K_total
    exploit = ((np.arange(K) + k_offset) < (1.0 - expl) * K_total)[:, None, None]
    e = eps.astype(np.float64)
    return np.clip(np.where(exploit, u[None] + e, e), _lim(lo, n), _lim(hi, n))


def chain_rollout_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, lo, hi, expl=0.0,
                        P: CO.ChainParams = CO.ChainParams(), k_offset=0, K_total=None, gamma=None):
    """S (K,): CO.chain_rollout_costs with v clipped before the dynamics and the control cost.  eps (K, T, n)."""
    K, T, n = eps.shape
    if gamma is None:
        gamma = lam * (1.0 - alpha)
    sig_inv = np.linalg.inv(sigma)
    v = sampled_controls(u, eps, lo, hi, expl, k_offset, K_total)
    q = np.tile(np.asarray(x0[:n], dtype=np.float64), (K, 1))
    dq = np.tile(np.asarray(x0[n:], dtype=np.float64), (K, 1))
    S = np.zeros(K)
    for t in range(T):
        q, dq = CO.chain_forward_dynamics(q, dq, v[:, t, :], dt, P)
        a = (gamma * u[t]) @ sig_inv
        S = S + (CO.chain_state_cost(q, dq, ref_path, prev_idx, stage_w, P) + v[:, t, :] @ a)
    return S + CO.chain_state_cost(q, dq, ref_path, prev_idx, term_w, P)


def step(x0, u_prev, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, lo, hi, expl=0.0,
         visualize_optimal_traj=True, sampled=False, P: CO.ChainParams = CO.ChainParams(), gamma=None):
    """One calc_control_input after its waypoint update with the clamp; `prev_idx` is the updated index.  Returns
    S, w, w_eps (raw), w_eps_filt, u_new (the update before any clip), u_seq (clipped when
    visualize_optimal_traj, then shifted), optimal_traj and sampled_traj (zeros when off)."""
    u = np.array(u_prev, dtype=np.float64)
    K, T, n = eps.shape
    S = chain_rollout_costs(x0, u, eps, ref_path, prev_idx, dt, lam, alpha, sigma, stage_w, term_w, lo, hi, expl, P,
                            gamma=gamma)
    w = O.compute_weights(S, lam)
    w_raw = O.weighted_noise(w, eps.astype(np.float64))
    w_filt = O.moving_median_filter(w_raw, 10) if T >= 1 else w_raw
    u_new = u + w_filt
    un = u_new.copy()
    opt = np.zeros((T, 2 * n))
    if visualize_optimal_traj:
        un = np.clip(un, _lim(lo, n), _lim(hi, n))                # _g(u[t-1]) over every row, in place
        opt = CO.chain_rollout_trajectory(x0, np.roll(un, 1, axis=0), dt, P)
    samp = np.zeros((K, T, 2 * n))
    if sampled:
        v = sampled_controls(u, eps, lo, hi, expl)
        samp = CO.chain_rollout_trajectory(x0, np.roll(v, 1, axis=1), dt, P)
    u_seq = np.concatenate([un[1:], un[-1:]], 0)
    return dict(S=S, w=w, w_eps=w_raw, w_eps_filt=w_filt, u_new=u_new, u_seq=u_seq, optimal_traj=opt,
                sampled_traj=samp)
