"""GPU: the row merge over more than one round, with the online rescale (merge_rows_block, mppi_merge.h).

No rollout at a test's size reaches these paths: a merge of more than 32 rows (the eager form, one column chunk)
or more than 16 (the sparse form, several chunks) in which a later round lowers the running minimum.
mppi_merge_partials / mppi_chain_merge_partials take caller-made rows, so the rows are made here:

  arm    T = 5, 70 rows: the eager form's rounds of 32, 32 and 6 rows;
  chain  n = 3 links, T = 5, 40 rows: four column chunks, rounds of 16, 16 and 8 rows in batches of four.

Rows: rho_i = 1000 + lambda U(0, 3); rho[n/2] -= 5 lambda and rho[n-2] -= 9 lambda, so the second and the third
round each lower the minimum (two rescales); rho[3] += 60 lambda and rho[n-1] += 60 lambda, two rows below the
merge floor 2^-64 = e^-44.4; eta_i = U(1, 256); N_i = eta_i U(-1, 1).

Expected: plain fp64 NumPy, w = sum s_i N_i / sum s_i eta_i with s_i = exp((min rho - rho_i) / lambda), no floor
and no rounds.  Tolerance: rtol 1e-10, atol 1e-12, test_shard_invariance_and_merge's for a device merge; a CPU
simulation of the round structure with the floor (68 of 70 and 38 of 40 rows kept, two rescales) differs from the
plain sum by at most 5e-16 relative on these rows, which leaves five orders for the device's exp.
"""
import numpy as np
import pytest
import torch

from helpers import _engine, _gpu  # noqa: F401

pytestmark = pytest.mark.gpu

LAMBDAS = [1.0, 100.0, 1.0e6]


def _rows(n, nval, lam):
    rng = np.random.default_rng(20261020)
    rho = 1000.0 + lam * rng.uniform(0.0, 3.0, n)
    rho[n // 2] -= 5.0 * lam
    rho[n - 2] -= 9.0 * lam
    rho[3] += 60.0 * lam
    rho[n - 1] += 60.0 * lam
    eta = rng.uniform(1.0, 256.0, n)
    N = eta[:, None] * rng.uniform(-1.0, 1.0, (n, nval))
    return rho, eta, N


def _expected(rho, eta, N, lam):
    s = np.exp((rho.min() - rho) / lam)
    return (s[:, None] * N).sum(0) / (s * eta).sum()


def _check(eng, n, lam):
    nval = eng.T * eng.dim_u
    assert eng.partial_len == 2 + nval
    rho, eta, N = _rows(n, nval, lam)
    parts = torch.from_numpy(np.concatenate([rho[:, None], eta[:, None], N], axis=1)).to(eng.device).contiguous()
    eng.merge(parts, n)
    w = eng.weighted_noise()
    eng.merge(parts, n)
    w2 = eng.weighted_noise()
    ref = _expected(rho, eta, N, lam).reshape(eng.T, eng.dim_u)
    err = float(np.max(np.abs(w - ref) / np.maximum(np.abs(ref), 1e-300)))
    print(f"merge rounds dim_u={eng.dim_u} n={n} lambda={lam:g}: max rel err {err:.2e}")
    np.testing.assert_allclose(w, ref, rtol=1e-10, atol=1e-12)
    assert np.array_equal(w, w2)
    eng.close()


@pytest.mark.parametrize("lam", LAMBDAS)
def test_arm_merge_three_eager_rounds(lam):
    _check(_engine(256, 5, param_lambda=lam), 70, lam)


@pytest.mark.parametrize("lam", LAMBDAS)
def test_chain_merge_three_sparse_rounds(lam):
    from mppi_robotarm_amd.chain import ChainEngine, ChainParams
    n, L = 3, 2.0 / 3
    P = ChainParams(m=(1.0,) * n, l=(L,) * n, lc=(L / 2,) * n, I=(L * L / 12.0,) * n, fk=(L,) * n, J=(0.1,) * n,
                    b=(1.0,) * n)
    eng = ChainEngine(256, 5, 0.006, lam, 0.98, np.eye(n) * 4.0, [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0], 0.0, P,
                      device=0)
    _check(eng, 40, lam)
