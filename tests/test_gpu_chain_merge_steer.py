"""GPU: the chain's hand-off merges steered with crafted noise (tests/merge_steer.py), as test_gpu_merge_steer.py
does for the arm.

The chain's partial rows take four column chunks (kCMaxCh): its direct merge has one column group and a limit of 16
weighted rows, its row merges go in rounds of 16 rows and batches of four in either hand-off form, and it has no
deferred form.  Shapes: n = 3, T = 5 (16 columns) and n = 7, T = 37 (260 columns: the second chunk holds four); the
fp32 rollout with 1 and with 4 lanes per sample and the fp64 rollout; 20 and 70 workgroups, the last one partial.
Scenarios: 1, 16 and 17 weighted rows (the direct merge, and past its limit), 33 with the minimum in the last
group behind mid-tier rows, every row; and 1, 9, 16, 17 and every sample of a workgroup kept, in one launch.  Both
hand-off forms run every case and must leave the same bits.

Each case: the model's prediction from the device's S is the scenario's intent (guard band included), w_eps and
partial_out's eta and N against the plain fp64 sum at rtol = atol = 1e-10, rho bit for bit.
"""
import numpy as np
import pytest
import torch

import merge_steer as M
from conftest import record
from helpers import _chains, _gpu, _sigma  # noqa: F401

pytestmark = pytest.mark.gpu

LAM = 100.0
POOL_N = 8192
W, TW = [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0]
_POOLS = {}


def _engine(n, K, T, precision, lps):
    """The uniform chain of helpers._chains (config 5's arm at n = 7)."""
    from mppi_robotarm_amd.chain import ChainEngine
    eng = ChainEngine(K, T, 0.006, LAM, 0.98, _sigma(n), W, TW, 0.0, _chains(n)[0], device=0, precision=precision,
                      lanes_per_sample=lps)
    assert eng.lanes_per_sample == lps and eng.threads == 256
    return eng


def _inputs(eng, paths):
    from mppi_robotarm_amd.chain import gravity_torque
    n = eng.n
    q = np.array([1.4] + [-2.2 / (n - 1)] * (n - 1))
    eng.set_step_inputs(np.concatenate([q, np.zeros(n)]), paths["xydq_circle"][40:70],
                        np.tile(gravity_torque(q, _chains(n)[0]), (eng.T, 1)))


def _rollout(eng, cols, paths, partial=False):
    _inputs(eng, paths)
    noise = eng.upload_noise(cols)
    S = torch.empty(eng.K_local, dtype=torch.float64, device=eng.device)
    part = eng.new_partial() if partial else None
    eng.rollout(noise, S_out=S, partial_out=part)
    w = eng.weighted_noise()
    return S.cpu().numpy(), (part.cpu().numpy() if partial else None), w


def _pool(n, T, precision, lps, paths):
    """The pool pass of one kernel form, once per module."""
    key = (n, T, precision, lps)
    if key not in _POOLS:
        eng = _engine(n, POOL_N, T, precision, lps)
        c1 = M.gaussian_columns(POOL_N, T, _sigma(n), 3000 + n)
        S1 = _rollout(eng, c1, paths)[0]
        best = int(np.argmin(S1))
        c2 = M.perturbed_columns(c1[best], POOL_N, _sigma(n), 4000 + n)
        S2 = _rollout(eng, c2, paths)[0]
        eng.close()
        pool = M.make_pool(np.concatenate([c1, c2]), np.concatenate([S1, S2]), LAM, best)
        print(f"pool {key}: near {len(pool.near)} mid {len(pool.mid)} heavy {len(pool.heavy)}")
        # the sample scenario at one lane per sample draws 469 near columns, the row scenarios at most 3 mid ones
        assert len(pool.near) >= 480 and len(pool.mid) >= 3 and len(pool.heavy) >= 256
        _POOLS[key] = pool
    return _POOLS[key]


CASES = [(n, T, prec, lps, blocks, s)
         for n, T in M.CHAIN_SHAPES for prec, lps in M.CHAIN_FORMS for blocks in M.CHAIN_BLOCKS
         for s in M.chain_scenarios(M.chain_grid(n, T, lps, blocks))]


@pytest.mark.parametrize("n,T,prec,lps,blocks,scn", CASES,
                         ids=[f"n{n}-T{T}-{p}-lps{l}-b{b}-{s.name}" for n, T, p, l, b, s in CASES])
def test_chain_merge_steered(n, T, prec, lps, blocks, scn, paths, monkeypatch):
    g = M.chain_grid(n, T, lps, blocks)
    pool = _pool(n, T, prec, lps, paths)
    idx, light = M.build_index(scn, pool, g)
    eps = pool.cols[idx]
    out, errs = {}, []
    for form in ("poll", "counter"):
        monkeypatch.delenv("MPPI_HANDOFF", raising=False)
        if form == "counter":
            monkeypatch.setenv("MPPI_HANDOFF", "counter")
        eng = _engine(n, g.K, T, prec, lps)
        monkeypatch.delenv("MPPI_HANDOFF", raising=False)
        assert (eng.blocks, eng.handoff) == (g.rows, form)
        S, part, w = _rollout(eng, eps, paths, partial=True)
        eng.close()
        assert len(np.unique(S[light])) == int(light.sum())           # distinct weights: a swapped row would show
        M.check_intent(scn, M.predict(S, g, LAM, form), g, form)
        rho, eta, N = M.plain_sum(S, eps, LAM)
        ref = N / eta
        errs.append(float(np.max(np.abs(w - ref))))
        print(f"    {form}: max |w_eps - plain sum| = {errs[-1]:.3e} (max |ref| {np.max(np.abs(ref)):.3e})")
        np.testing.assert_allclose(w, ref, rtol=M.W_TOL, atol=M.W_TOL)
        assert part[0] == rho                                         # bit for bit
        np.testing.assert_allclose(part[1], eta, rtol=M.W_TOL, atol=M.W_TOL)
        np.testing.assert_allclose(part[2:].reshape(N.shape), N, rtol=M.W_TOL, atol=M.W_TOL)
        out[form] = (w, part)
    for a, b in zip(out["poll"], out["counter"]):                     # granule against counter: the same bits
        assert np.array_equal(a, b)
    record("merge_steer", model=f"chain n={n} T={T} {prec} lps={lps}", grid=f"b{blocks}", scenario=scn.name,
           path=scn.path, rescale=scn.rescale, weighted_rows=len(scn.light_rows()), max_abs_err=max(errs))
