"""GPU: the n-link chain kernels at non-uniform links.

Every other chain test gives all links the same m, l, lc, I, fk, J and b, so an off-by-one in any per-link table the
host packs (the J table's interleaved slots, the pad link of an odd chain, the quad form's split) cannot show.  Here
every entry of every vector differs (helpers.asym_chain_kwargs, seeded per n); tests/test_asym_cpu.py shows that
rolling any one vector by one position moves the fp64 cost of these very inputs by a median >= 2e-3, checks the chain
oracle at such links against a Lagrangian written from first principles, and the C chain oracle against it.

Tolerances are test_gpu_chain.py's: fp32 S at the 99th percentile within 2e-4 with the argmin rule and every sample
beyond 1e-3 a nearest-waypoint tie, w_eps 1e-4; fp64 S 1e-11 and w_eps 1e-10; trajectories 1e-4.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import chain_oracle as CO  # noqa: E402
import coracle  # noqa: E402
import mppi_oracle as O  # noqa: E402
from conftest import record  # noqa: E402
from helpers import ASYM_LINK_CASES, _gpu, _urel, asym_chain_inputs  # noqa: E402, F401
from tieflip import tie_flip_residual  # noqa: E402

U_TOL = 1e-4
TIE_GAP_M = 1e-5   # test_gpu_chain.py's
W, TW = [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0]
WIN = slice(40, 70)


def _limits(u, sig):
    """Torque limits around the nominal's first row, a different margin on each side of each joint."""
    n = u.shape[1]
    sd = np.sqrt(np.diag(sig))
    return u[0] - sd * np.linspace(0.3, 0.7, n), u[0] + sd * np.linspace(0.9, 0.5, n)


def _case(n, K, T, lam, paths, precision="f32", lps=1, limits=False):
    """One non-uniform chain through the engine and the fp64 chain oracle (the C one; the NumPy one with torque
    limits, which the C one does not have): (S, S_ref, w_eps, w_eps_ref, tie inputs)."""
    import mppi_robotarm_amd.chain as chain_mod
    P, x0, sig, u = asym_chain_inputs(n, T, chain_mod)
    Po = asym_chain_inputs(n, T, CO)[0]
    lo, hi = _limits(u, sig) if limits else (None, None)
    eng = chain_mod.ChainEngine(K, T, 0.006, lam, 0.98, sig, W, TW, 0.0, P, device=0, precision=precision,
                                lanes_per_sample=lps, u_min=lo, u_max=hi)
    assert eng.lanes_per_sample == lps
    win = paths["xydq_circle"][WIN]
    eng.set_step_inputs(x0, win, u)
    noise = eng.philox_noise(3 + n, 1)
    S_dev = torch.empty(K, dtype=torch.float64, device="cuda")
    eng.rollout(noise, S_out=S_dev)
    w, S = eng.weighted_noise(), S_dev.cpu().numpy()
    nz = noise.cpu().numpy().transpose(0, 2, 1)   # device [T][K][n] -> (T, n, K)
    eng.close()
    if limits:
        eps = nz.transpose(2, 0, 1).astype(np.float64)
        clipped = O.sampled_controls(u, eps, lo, hi) != (u[None] + eps)
        assert np.all((clipped.mean(axis=(0, 1)) > 0.2) & (clipped.mean(axis=(0, 1)) < 0.8))
        Sr = CO.chain_rollout_costs(x0, u, eps, paths["xydq_circle"], WIN.start, 0.006, lam, 0.98, sig, W, TW, 0.0, Po,
                                    lo=lo, hi=hi)
    else:
        Sr = coracle.chain_rollout_costs(x0, u, nz, win, 0.006, lam, 0.98, sig, W, TW, Po, layout="TNK")
    _, wr = coracle.chain_weighted_noise(Sr, nz, lam, layout="TNK")
    return S, Sr, w, wr, (x0, u, nz, win, Po)


def _check_f32(S, Sr, w, wr, tie, what, ties=True):
    rel = np.abs(S - Sr) / np.abs(Sr)
    print(f"{what}: S rel-err p99 {np.percentile(rel, 99):.2e} max {rel.max():.2e}, w_eps {_urel(w, wr):.2e}")
    assert np.all(np.isfinite(S))
    j, jr = int(np.argmin(S)), int(np.argmin(Sr))
    assert j == jr or abs(Sr[j] - Sr[jr]) <= 1e-5 * abs(Sr[jr])
    assert float(np.percentile(rel, 99)) < 2e-4
    out = np.flatnonzero(rel > 1e-3)   # nearest-waypoint ties only (tests/tieflip.py)
    if ties and len(out):
        x0, u, nz, win, Po = tie
        res, gap = tie_flip_residual(S, Sr, out, x0, u, nz, win, 0.006, W, TW, Po)
        assert res.max() < 2e-4 and gap.max() < TIE_GAP_M
    else:
        assert float(np.mean(rel > 1e-3)) <= 2e-3
    assert _urel(w, wr) < U_TOL
    return rel


@pytest.mark.parametrize("lps", [1, 4])
@pytest.mark.parametrize("n,K,T,lam", ASYM_LINK_CASES)
def test_chain_every_link_count_against_c_oracle(n, K, T, lam, lps, paths):
    S, Sr, w, wr, tie = _case(n, K, T, lam, paths, lps=lps)
    rel = _check_f32(S, Sr, w, wr, tie, f"non-uniform chain n={n} K={K} T={T} lps={lps}")
    record("asym_chain_f32", n=n, K=K, T=T, lps=lps, S_p99=float(np.percentile(rel, 99)), S_max=float(rel.max()),
           w_eps_rel_err=_urel(w, wr))


@pytest.mark.parametrize("n,K,T,lam", ASYM_LINK_CASES)
def test_chain_f64_every_link_count_against_c_oracle(n, K, T, lam, paths):
    """The sharp one: the fp64 rollout equals the oracle to rounding, so a wrong index into m, l, lc, I, J or b
    (1e-3 or more, test_asym_cpu.py) cannot hide in a tolerance."""
    S, Sr, w, wr, _ = _case(n, K, T, lam, paths, precision="f64", lps=1)
    rel = np.abs(S - Sr) / np.abs(Sr)
    print(f"non-uniform chain f64 n={n} K={K} T={T}: S rel-err max {rel.max():.2e}, w_eps {_urel(w, wr):.2e}")
    record("asym_chain_f64", n=n, K=K, T=T, S_max=float(rel.max()), w_eps_rel_err=_urel(w, wr))
    assert int(np.argmin(S)) == int(np.argmin(Sr))
    assert float(rel.max()) < 1e-11
    assert _urel(w, wr) < 1e-10


@pytest.mark.parametrize("precision,lps", [("f32", 4), ("f64", 1)], ids=["f32-lps4", "f64"])
@pytest.mark.parametrize("n,K,T,lam", [c for c in ASYM_LINK_CASES if c[0] in (3, 7)])
def test_chain_with_torque_limits_distinct_per_joint(n, K, T, lam, precision, lps, paths):
    """Odd chains (a pad link in the quad form) with limits that differ per joint and per side, against the NumPy
    chain oracle with limits."""
    S, Sr, w, wr, tie = _case(n, K, T, lam, paths, precision=precision, lps=lps, limits=True)
    if precision == "f64":
        rel = np.abs(S - Sr) / np.abs(Sr)
        print(f"non-uniform chain f64 n={n} clamped: S rel-err max {rel.max():.2e}, w_eps {_urel(w, wr):.2e}")
        assert int(np.argmin(S)) == int(np.argmin(Sr))
        assert float(rel.max()) < 1e-11 and _urel(w, wr) < 1e-10
    else:
        rel = _check_f32(S, Sr, w, wr, tie, f"non-uniform chain n={n} lps={lps} clamped", ties=False)
    record("asym_chain_clamped", n=n, precision=precision, S_max=float(rel.max()), w_eps_rel_err=_urel(w, wr))


@pytest.mark.parametrize("n", [3, 7])
def test_chain_trajectories_match_oracle(n, paths):
    """chain_traj_kernel (the sampled re-roll) and mppi_chain_optimal_traj_host against the fp64 chain dynamics."""
    import mppi_robotarm_amd.chain as chain_mod
    K, T = 64, 20
    P, x0, sig, u = asym_chain_inputs(n, T, chain_mod)
    Po = asym_chain_inputs(n, T, CO)[0]
    eng = chain_mod.ChainEngine(K, T, 0.006, 100.0, 0.98, sig, W, TW, 0.0, P, device=0)
    eng.set_step_inputs(x0, paths["xydq_circle"][WIN], u)
    noise = eng.philox_noise(2, 0)
    tr = eng.trajectories(base_u=u, noise=noise).double().cpu().numpy()
    eps = noise.cpu().numpy().astype(np.float64).transpose(1, 0, 2)            # (K, T, n)
    want = CO.chain_rollout_trajectory(x0, np.roll(u[None] + eps, 1, axis=1), 0.006, Po)
    np.testing.assert_allclose(tr, want, rtol=1e-4, atol=1e-4)
    un = u + np.random.default_rng(9).normal(0, 0.5, u.shape)
    got = eng.optimal_traj_host(x0, un)
    want0 = CO.chain_rollout_trajectory(x0, np.roll(un, 1, axis=0), 0.006, Po)
    np.testing.assert_allclose(got, want0, rtol=1e-4, atol=1e-4)
    print(f"n={n}: sampled re-roll max abs err {float(np.max(np.abs(tr - want))):.2e}, host trajectory "
          f"{float(np.max(np.abs(got - want0))):.2e}")
    record("asym_chain_traj", n=n, sampled=float(np.max(np.abs(tr - want))), host=float(np.max(np.abs(got - want0))))
    eng.close()
