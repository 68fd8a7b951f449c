"""GPU: the update tail of a fused chain step, chain_update_block<N, CLAMP> (mppi_chain.hip), bit for bit at every
link count and at the horizons where it takes another path.

The block filters the weighted noise with the median of 10 (four consecutive windows per thread from one sorted
7-value core plus three sorted extras, reads reflected at both ends, windows past T read through a clamped index and
not written), adds it to the nominal (one fp64 add), clips under mode-2 torque limits, shifts, and writes the next
launch's u, ua and a_t = (gamma u)^T Sigma^-1 rows plus u_first.  Thread (q, d) = (tid / N, tid % N) reads LDS at
stride N; the second pass takes t = tid % MPPI_MAX_T and splits a row across two waves, joints 0 - 3 and 4 .. N - 1.

Inputs: helpers.asym_chain_inputs (a non-uniform chain, a dense SPD Sigma, joint rates around 1 rad/s), the window
xydq_circle[40:70], Philox noise; the three horizon forms of the chain tests (helpers.UPDATE_FORMS: two workgroups,
the second ragged); n = 2 .. 7; T in helpers.UPDATE_TS.  Every expectation is built from the launch's OWN weighted
noise (the chain always writes w_eps_out, the row the filter read), so nothing here depends on the rollout's
precision: the filter selects an element and the update is one fp64 add, and equal bits are asserted.

  1. median, add and shift against SciPy over three chained steps (the device-written block feeds the next step);
  2. structured noise that needs no SciPy: every window's median +0, and six consecutive non-zero steps against
     np.sort on the reflected index list; u_first through the host trajectory;
  3. mode-2 torque limits distinct per joint (the late-prefetch variant at one lane per sample), and mode 1;
  4. the next launch's constants: a launch on the device-written block against one on the staged nominal, at a
     lambda where a wrong a_t row of any joint would show (test_chain_update_cpu.py);
  5. chain_merge_kernel's fused update;
  6. the host outputs: wait_outputs' nominal and trajectory (u_first, the stride-MPPI_CHAIN_MAX_DOF read-back).

Bit equality held in every case of 1, 2, 3, 5 and 6 on MI355X; 4 holds the bounds of
test_gpu_chain.test_chain_fused_update_matches_host_update (the device may contract the a_t sum to fma).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chain_oracle as CO  # noqa: E402
import mppi_oracle as O  # noqa: E402
from helpers import (UPDATE_ALPHA, UPDATE_CLAMP_LAMBDA, UPDATE_DT, UPDATE_FORM_IDS, UPDATE_FORMS,  # noqa: E402, F401
                     UPDATE_LAMBDA, UPDATE_NS, UPDATE_S_RTOL, UPDATE_TS, UPDATE_TW, UPDATE_W, UPDATE_WIN, _gpu,
                     asym_chain_inputs, clipped_share, dense_steps, expected_nominal, median10, shift_nominal,
                     sparse_steps, step_noise, update_limits, update_seed)

forms = pytest.mark.parametrize("precision,lps,K", UPDATE_FORMS, ids=UPDATE_FORM_IDS)


def _case(n, T, precision, lps, K, paths, lam=None, **kw):
    """The engine of one (n, T, form) at UPDATE_LAMBDA[n] (or lam) with asym_chain_inputs staged: (eng, x0, win, u)."""
    import mppi_robotarm_amd.chain as chain_mod
    P, x0, sig, u = asym_chain_inputs(n, T, chain_mod)
    eng = chain_mod.ChainEngine(K, T, UPDATE_DT, UPDATE_LAMBDA[n] if lam is None else lam, UPDATE_ALPHA, sig, UPDATE_W,
                                UPDATE_TW, 0.0, P, device=0, precision=precision, lanes_per_sample=lps, **kw)
    assert eng.lanes_per_sample == lps and eng.n == n
    win = paths["xydq_circle"][UPDATE_WIN]
    eng.set_step_inputs(x0, win, u)
    return eng, x0, win, u


def _bad(got, expect):
    """The entries whose bits differ, for the failure message: (t, d, got, expected) of the first few."""
    t, d = np.nonzero(~((got == expect) | (np.isnan(got) & np.isnan(expect))))
    return [(int(a), int(b), float(got[a, b]), float(expect[a, b])) for a, b in zip(t[:6], d[:6])]


# ---------------------------------------------------------------- 1: median, add and shift against SciPy

@pytest.mark.parametrize("n", UPDATE_NS)
@forms
def test_fused_update_equals_scipy_median_add_and_shift_bit_for_bit(precision, lps, K, n, paths):
    """Every T of UPDATE_TS, three chained fused steps each: nominal() == shift(u + median_filter(w, 10, reflect))
    with w the launch's own weighted noise; the nominal read back is fed forward as u without restaging it, so steps
    2 and 3 prefetch their u from the block the device wrote."""
    for T in UPDATE_TS:
        eng, _, _, u = _case(n, T, precision, lps, K, paths)
        for step in range(3):
            eng.rollout(eng.philox_noise(update_seed(n), step), fused_update=True)
            w = eng.weighted_noise()
            got = eng.nominal()
            expect = expected_nominal(u, w)
            assert np.all(np.isfinite(w)) and np.any(median10(w))
            assert np.array_equal(got, expect), (n, T, step, _bad(got, expect))
            u = got
        eng.close()


# ---------------------------------------------------------------- 2: structured noise, no SciPy

@pytest.mark.parametrize("T", [7, 13])
@pytest.mark.parametrize("n", [5, 6])
@forms
def test_sparse_noise_leaves_the_plain_shift_and_dense_noise_the_sorted_median(precision, lps, K, n, T, paths):
    """Host noise that is +0 except at sparse_steps(T): w_eps is exactly +0 elsewhere, no window holds more than four
    non-zero values (test_chain_update_cpu.py), every median is +0, and the nominal is the plain shift of u with
    u_first = u[0] (read through wait_outputs' trajectory, which starts from it).  Then six consecutive non-zero
    steps: the median of np.sort over the reflected index list."""
    eng, x0, win, u = _case(n, T, precision, lps, K, paths)
    sig = asym_chain_inputs(n, T, CO)[2]
    steps = sparse_steps(T)
    eng.rollout(eng.upload_noise(step_noise(K, T, n, steps, sig, 10 * n + T)), fused_update=True, host_out=True)
    u_out, traj = eng.wait_outputs(x0)
    w = eng.weighted_noise()
    rest = np.setdiff1d(np.arange(T), steps)
    assert np.all(w[steps] != 0.0) and not np.any(w[rest]) and not np.any(np.signbit(w[rest]))
    got = eng.nominal()
    assert np.array_equal(got, shift_nominal(u)), (n, T, _bad(got, shift_nominal(u)))
    assert np.array_equal(u_out, got)
    assert np.array_equal(traj, eng.optimal_traj_host(x0, u))           # u_first == u[0]
    # six consecutive steps, on the staged nominal again
    eng.set_step_inputs(x0, win, u)
    eng.rollout(eng.upload_noise(step_noise(K, T, n, dense_steps(T), sig, 10 * n + T + 1)), fused_update=True)
    w = eng.weighted_noise()
    filt = O.moving_median_filter(w)                                    # np.sort over the reflected index list
    assert np.any(filt) and not np.all(filt)
    got = eng.nominal()
    assert np.array_equal(got, shift_nominal(u + filt)), (n, T, _bad(got, shift_nominal(u + filt)))
    eng.close()


# ---------------------------------------------------------------- 3: torque limits, distinct per joint

@pytest.mark.parametrize("T", [9, 127])
@pytest.mark.parametrize("n", [2, 5, 6, 7])
@forms
def test_mode_2_clips_the_updated_nominal_per_joint_bit_for_bit(precision, lps, K, n, T, paths):
    """Limits inside the spread of u + filt (helpers.update_limits): mode 2 gives shift(clip(u + filt, lo, hi)),
    mode 1 (clamp_nominal=False) the unclipped update, each from its own launch's weighted noise; of the mode-2
    update's entries the clipped and the unclipped share both lie in (0.1, 0.9)."""
    lo, hi = update_limits(n, T, paths)
    for mode2 in (True, False):
        eng, _, _, u = _case(n, T, precision, lps, K, paths, lam=UPDATE_CLAMP_LAMBDA, u_min=lo, u_max=hi,
                             clamp_nominal=mode2)
        u1 = u
        for step in range(2):   # the second step takes its nominal from the clipped block
            eng.rollout(eng.philox_noise(update_seed(n), step), fused_update=True)
            w = eng.weighted_noise()
            got = eng.nominal()
            expect = expected_nominal(u1, w, lo, hi) if mode2 else expected_nominal(u1, w)
            assert np.array_equal(got, expect), (n, T, mode2, step, _bad(got, expect))
            if step == 0:
                share = clipped_share(u1 + median10(w), lo, hi)
                print(f"n={n} T={T} {precision} lps={lps} mode {2 if mode2 else 1}: {share:.2f} of the update clipped")
                assert 0.1 < share < 0.9
                assert mode2 == bool(np.all((got >= lo) & (got <= hi)))
            u1 = got
        eng.close()


# ---------------------------------------------------------------- 4: the next launch's constants

@pytest.mark.parametrize("T", [6, 128])
@pytest.mark.parametrize("n", UPDATE_NS)
@forms
def test_launch_on_the_device_written_block_equals_one_on_the_staged_nominal(precision, lps, K, n, T, paths):
    """After a fused step the block holds u, the fp32 ua rows and a_t as the device computed them; S of a launch on
    it against S of a launch on the same nominal staged by the host (set_step_inputs computes a_t itself), at
    test_chain_fused_update_matches_host_update's bounds.  At UPDATE_LAMBDA[n] a zeroed a_t column of any one joint
    moves S by a median >= 100 x these bounds (test_chain_update_cpu.py)."""
    eng, x0, win, _ = _case(n, T, precision, lps, K, paths)
    noise = eng.philox_noise(update_seed(n), 0)
    eng.rollout(noise, fused_update=True)
    noise1 = eng.philox_noise(update_seed(n), 1)
    S1 = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.rollout(noise1, S_out=S1)
    S1 = S1.cpu().numpy()
    eng.set_step_inputs(x0, win, eng.nominal())
    S2 = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.rollout(noise1, S_out=S2)
    S2 = S2.cpu().numpy()
    eng.close()
    rel = np.abs(S1 - S2) / np.abs(S2)
    print(f"n={n} T={T} {precision} lps={lps}: S on the device-written block vs the staged nominal, max rel {rel.max():.2e}")
    assert np.all(np.isfinite(S1))
    np.testing.assert_allclose(S1, S2, rtol=UPDATE_S_RTOL[precision])


# ---------------------------------------------------------------- 5: chain_merge_kernel with the fused update

@pytest.mark.parametrize("limits", [False, True], ids=["free", "mode2"])
@pytest.mark.parametrize("T", [7, 126])
@pytest.mark.parametrize("n", [3, 5, 6])
@forms
def test_merge_kernel_fused_update_bit_for_bit(precision, lps, K, n, T, limits, paths):
    """Two shards of K / 2 (Philox slices of the unsharded draw) merged on shard 0 with the fused update: its
    nominal is shift(clip(u + median_filter(w))) of the merge's own weighted noise."""
    kw = {}
    if limits:
        lo, hi = update_limits(n, T, paths)
        kw = dict(u_min=lo, u_max=hi, lam=UPDATE_CLAMP_LAMBDA)
    full, _, _, u = _case(n, T, precision, lps, K, paths, **kw)
    draw = full.philox_noise(update_seed(n), 0)
    full.close()
    parts = torch.empty(2 * full.partial_len, dtype=torch.float64, device="cuda")
    shards = []
    for s in range(2):
        e = _case(n, T, precision, lps, K // 2, paths, K_total=K, k_offset=s * (K // 2), **kw)[0]
        nz = e.philox_noise(update_seed(n), 0)
        assert torch.equal(nz, draw[:, s * (K // 2):(s + 1) * (K // 2), :])
        e.rollout(nz, partial_out=parts[s * e.partial_len:(s + 1) * e.partial_len])
        shards.append(e)
    shards[0].merge(parts, 2, fused_update=True)
    w = shards[0].weighted_noise()
    got = shards[0].nominal()
    expect = expected_nominal(u, w, lo, hi) if limits else expected_nominal(u, w)
    assert np.all(np.isfinite(w)) and np.any(median10(w))
    assert np.array_equal(got, expect), (n, T, limits, _bad(got, expect))
    if limits:
        assert 0.0 < clipped_share(u + median10(w), lo, hi) < 1.0
    for e in shards:
        e.close()


# ---------------------------------------------------------------- 6: the host outputs

@pytest.mark.parametrize("T", [5, 128])
@pytest.mark.parametrize("n", UPDATE_NS)
@forms
def test_host_outputs_equal_the_nominal_and_the_host_trajectory(precision, lps, K, n, T, paths):
    """rollout(host_out=True) + wait_outputs(x0): u_out is nominal() and traj is optimal_traj_host(x0, u + filt),
    the update before its shift, whose first row only u_first holds (rows of MPPI_CHAIN_MAX_DOF doubles read back at
    every n)."""
    eng, x0, _, u = _case(n, T, precision, lps, K, paths)
    eng.rollout(eng.philox_noise(update_seed(n), 0), fused_update=True, host_out=True)
    u_out, traj = eng.wait_outputs(x0)
    w = eng.weighted_noise()
    un = u + median10(w)
    assert np.array_equal(u_out, eng.nominal())
    assert np.array_equal(u_out, shift_nominal(un)), (n, T, _bad(u_out, shift_nominal(un)))
    want = eng.optimal_traj_host(x0, un)
    assert np.all(np.isfinite(traj)) and np.array_equal(traj, want), (n, T, _bad(traj, want))
    # the first row of the update shows in the trajectory: one built from the shifted rows alone differs
    assert not np.array_equal(want, eng.optimal_traj_host(x0, np.vstack([un[1:2], un[1:]])))
    eng.close()
