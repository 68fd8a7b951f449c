"""CPU: what tests/test_gpu_chain_update.py relies on, shown without a device.

  * its check of the next launch's constants means something: at helpers.UPDATE_LAMBDA a zeroed a_t column of any one
    joint moves the fp64 oracle's S of those very inputs by a median >= 100 x the bound the device test holds;
  * its torque limits clip some entries of the updated nominal and leave others, in the fp64 oracle's own run;
  * the restatement of chain_update_block's four-window median (test_host_logic._sliding_median10) equals SciPy at
    that module's horizons with n columns laid out as the kernel's LDS rows are, stride n, for every link count;
  * the structured noise of the device test gives the windows it claims.
"""
import numpy as np
import pytest

import chain_oracle as CO
from helpers import (UPDATE_ALPHA, UPDATE_CLAMP_LAMBDA, UPDATE_LAMBDA, UPDATE_NS, UPDATE_S_RTOL, UPDATE_TS, asym_chain_inputs,
                     clipped_share, median10, reflected_windows, sorted_median10, update_limits, update_reference)
from test_host_logic import _sliding_median10


@pytest.mark.parametrize("T", [6, 128])
@pytest.mark.parametrize("n", UPDATE_NS)
def test_a_zeroed_a_t_column_of_any_joint_moves_S_past_the_device_bound(n, T, paths):
    """The control cost is additive, sum_t sum_d a_t[d] v[k, t, d] with a_t = (gamma u_t)^T Sigma^-1
    (control.py:106): a launch whose a_t column d were zero would miss joint d's share of it.  K = 64."""
    _, S, u, eps = update_reference(n, T, paths, K=64)
    sig = asym_chain_inputs(n, T, CO)[2]
    a = (UPDATE_LAMBDA[n] * (1.0 - UPDATE_ALPHA) * u) @ np.linalg.inv(sig)
    share = np.einsum("td,ktd->kd", a, u[None] + eps)                    # (K, n): joint d's part of S
    # the parts add up to the control cost: S without them is the state cost, the same at gamma = 0
    S0 = CO.chain_rollout_costs(*_oracle_args(n, T, paths, eps), gamma=0.0)
    np.testing.assert_allclose(S - share.sum(1), S0, rtol=1e-9)
    moved = np.median(np.abs(share) / np.abs(S)[:, None], axis=0)
    print(f"n={n} T={T} lambda={UPDATE_LAMBDA[n]:g}: median |dS| / S per zeroed joint {np.array2string(moved, precision=2)}")
    assert np.all(moved >= 100.0 * max(UPDATE_S_RTOL.values()))


def _oracle_args(n, T, paths, eps):
    from helpers import UPDATE_DT, UPDATE_TW, UPDATE_W, UPDATE_WIN
    Po, x0, sig, u = asym_chain_inputs(n, T, CO)
    return (x0, u, eps, paths["xydq_circle"], UPDATE_WIN.start, UPDATE_DT, UPDATE_LAMBDA[n], UPDATE_ALPHA, sig,
            UPDATE_W, UPDATE_TW, 0.0, Po)


@pytest.mark.parametrize("K", [300, 100])
@pytest.mark.parametrize("T", [9, 127])
@pytest.mark.parametrize("n", [2, 5, 6, 7])
def test_update_limits_clip_some_entries_and_leave_others(n, T, K, paths):
    """The oracle's run with the limits in force (mode 2 clips the sampled controls too, so its weights are not the
    unlimited run's), at the sample counts of the device forms: of the entries of u + filt, the clipped and the
    unclipped share both lie in (0.1, 0.9)."""
    lo, hi = update_limits(n, T, paths)
    assert np.all(lo < hi) and len(set(np.round(hi - lo, 9))) == n       # distinct per joint
    un = update_reference(n, T, paths, K=K, lo=lo, hi=hi, lam=UPDATE_CLAMP_LAMBDA)[0]
    share = clipped_share(un, lo, hi)
    print(f"n={n} T={T} K={K}: {share:.2f} of the updated nominal clipped")
    assert 0.1 < share < 0.9


@pytest.mark.parametrize("n", UPDATE_NS)
@pytest.mark.parametrize("T", UPDATE_TS)
def test_chain_sliding_median_equals_scipy_at_every_width(T, n):
    """test_chain_sliding_median_equals_scipy's restatement with the kernel's row layout: column d of a flat
    buffer of stride n (thread (q, d) reads weps[m * n + d]), n = 2 .. 7, ties included."""
    rng = np.random.default_rng(100 * T + n)
    for x in (rng.standard_normal((T, n)), rng.integers(-3, 4, (T, n)).astype(float)):
        flat = np.ascontiguousarray(x).ravel()
        got = np.stack([_sliding_median10(flat[d::n]) for d in range(n)], axis=1)
        assert np.array_equal(got, median10(x))
        assert np.array_equal(got, sorted_median10(x))


@pytest.mark.parametrize("T", [7, 13])
def test_sparse_noise_windows_have_a_zero_median(T):
    """Noise at helpers.sparse_steps(T) alone: no two steps adjacent, at most four, and no reflected window holds
    more than four of them (a reflection repeats a step), so rank 5 of every window is one of its zeroes whatever
    the signs; six consecutive steps put a non-zero median into some window."""
    from helpers import dense_steps, sparse_steps
    steps = sparse_steps(T)
    assert 1 <= len(steps) <= 4 and np.all(np.diff(steps) > 1) and steps[-1] < T
    win = reflected_windows(T)
    assert np.isin(win, steps).sum(1).max() <= 4
    rng = np.random.default_rng(T)
    w = np.zeros((T, 3))
    w[steps] = rng.normal(0, 1, (len(steps), 3))
    assert not np.any(median10(w)) and not np.any(np.signbit(median10(w)))
    run = dense_steps(T)
    assert len(run) == 6 and np.all(np.diff(run) == 1) and run[-1] < T
    w = np.zeros((T, 3))
    w[run] = np.abs(rng.normal(0, 1, (6, 3))) + 0.1
    assert np.any(median10(w)) and np.array_equal(median10(w), sorted_median10(w))
