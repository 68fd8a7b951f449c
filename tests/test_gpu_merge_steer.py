"""GPU: the arm's hand-off merges (mppi_merge.h) steered into every branch with crafted noise (tests/merge_steer.py).

Philox noise reaches the two ends of the merge's range: one weighted row at lambda = 100, every row at 1e6.  Here the
noise buffer is built column by column from a pool whose costs the device itself has measured, so that a chosen
number of samples of chosen workgroups, and a chosen number of workgroup rows, carry weight above 2^-64:

  rows      1, 2, 16, 17, 64, 65 and all 70 weighted rows on the grouped direct merge's grid (T = 8: 15 column groups,
            limit 64), rows 15 | 16 (a group edge), 63 | 64 (the lane-slot edge of rho_l[j]) and the partial last row
            among them, the minimum in the last group behind mid-tier rows; 1, 16, 17, 32, 33 on the single-group
            grid (T = 64, limit 16; 32 | 33 is the batch edge of the deferred walk); 16 and 17 at 512 threads
            (T = 128); one group of 8 and of 16 rows; 257 and 530 rows (past kDirectRows; 34 group rows merge in
            rounds of 32 and 2, and the minimum in the second round rescales the running sums); ties;
  samples   1, 2, 3, 5, 9, 16, 17 and 32 kept samples in a workgroup (the gather's buckets and the dense gather), at
            the first and the last slot and on either side of every wave edge, alone and mixed in one launch; with
            one lane per sample 17 and 256 in a row;
  finishes  every row scenario of at most 256 rows as a plain rollout, a fused in-launch step and a fused deferred
            step (finished by a read, and by the next launch), in the granule and the counter hand-off.

Every case is two or three tiny launches per engine.  From the S of the steered launch the NumPy model predicts the
kept samples and gather of every light workgroup, the weighted rows, the path, the level-2 rounds and the rescale;
the test asserts that this is the scenario's intent, with every deciding exponent outside (30, 50) (the floor is at
44.36).  Then w_eps, and eta and N of partial_out, against the plain fp64 sum over the device's own S and the
widened fp32 noise at rtol = atol = 1e-10 (merge_steer.W_TOL: the structure itself costs below 1e-13,
test_merge_steer_cpu.py), rho bit for bit, and np.array_equal across the forms documented as bit-identical.
"""
import numpy as np
import pytest
import torch

import merge_steer as M
from conftest import record
from helpers import RUNPY, X0, _engine, _gpu, _window  # noqa: F401

pytestmark = pytest.mark.gpu

LAM = 100.0
POOL_N = 8192      # candidates per half of a pool
CUS = 256          # an MI355X's compute units: a larger grid takes the counter hand-off
# (near, mid) columns the scenarios of a horizon draw at most; heavy ones are reused
NEED = {5: (530, 4), 7: (274, 0), 8: (100, 8), 64: (33, 2), 128: (17, 1)}
_POOLS = {}


def _inputs(eng, paths):
    eng.set_step_inputs(X0, _window(paths, 3), np.array([[10.0, -2.0]] * eng.T))


def _costs(eng, cols):
    noise = eng.upload_noise(cols)
    S = torch.empty(eng.K_local, dtype=torch.float64, device=eng.device)
    eng.rollout(noise, S_out=S)
    eng.synchronize()
    return S.cpu().numpy()


def _pool(T, paths):
    """The pool pass of horizon T, once per module: the Gaussian half, then the half around its best column."""
    if T not in _POOLS:
        eng = _engine(POOL_N, T, param_lambda=LAM)
        _inputs(eng, paths)
        c1 = M.gaussian_columns(POOL_N, T, RUNPY["sigma"], 1000 + T)
        S1 = _costs(eng, c1)
        best = int(np.argmin(S1))
        c2 = M.perturbed_columns(c1[best], POOL_N, RUNPY["sigma"], 2000 + T)
        S2 = _costs(eng, c2)
        eng.close()
        pool = M.make_pool(np.concatenate([c1, c2]), np.concatenate([S1, S2]), LAM, best)
        print(f"pool T={T}: near {len(pool.near)} mid {len(pool.mid)} heavy {len(pool.heavy)}")
        assert len(pool.near) >= NEED[T][0] and len(pool.mid) >= NEED[T][1] and len(pool.heavy) >= 256
        assert np.mean((S1 - S1[best]) / LAM >= M.HEAVY_MIN) >= 0.9       # plain Gaussian columns are heavy
        _POOLS[T] = pool
    return _POOLS[T]


def _make(g, form, monkeypatch):
    """An engine on grid g in hand-off form `form`.  A grid larger than the device takes the counter form by
    itself, and is left to: the assertion below is then the context's own choice."""
    monkeypatch.delenv("MPPI_HANDOFF", raising=False)
    if form == "counter" and g.rows <= CUS:
        monkeypatch.setenv("MPPI_HANDOFF", "counter")
    eng = _engine(g.K, g.T, lps=g.lps, param_lambda=LAM)
    monkeypatch.delenv("MPPI_HANDOFF", raising=False)
    assert (eng.blocks, eng.threads, eng.lanes_per_sample, eng.handoff) == (g.rows, g.threads, g.lps, form)
    return eng


def _forms(g):
    return ("counter",) if g.rows > CUS else ("poll", "counter")


def _plain(eng, noise, paths):
    """A plain rollout: (S, partial_out row, w_eps)."""
    _inputs(eng, paths)
    S = torch.empty(eng.K_local, dtype=torch.float64, device=eng.device)
    part = eng.new_partial()
    eng.rollout(noise, S_out=S, partial_out=part)
    w = eng.weighted_noise()
    return S.cpu().numpy(), part.cpu().numpy(), w


def _close_to_plain_sum(S, eps, w, part=None):
    """w_eps (and the partial row) against the plain fp64 sum; returns the largest |w - ref|."""
    rho, eta, N = M.plain_sum(S, eps, LAM)
    ref = N / eta
    err = float(np.max(np.abs(w - ref)))
    print(f"    max |w_eps - plain sum| = {err:.3e} (max |ref| {np.max(np.abs(ref)):.3e}, eta {eta:.6g})")
    np.testing.assert_allclose(w, ref, rtol=M.W_TOL, atol=M.W_TOL)
    if part is not None:
        assert part[0] == rho                                                    # bit for bit
        np.testing.assert_allclose(part[1], eta, rtol=M.W_TOL, atol=M.W_TOL)
        np.testing.assert_allclose(part[2:].reshape(N.shape), N, rtol=M.W_TOL, atol=M.W_TOL)
    return err


def _result(eng):
    """What a fused step leaves: w_eps, the shifted nominal, the trajectory of the unshifted update."""
    return eng.weighted_noise(), eng.nominal(), eng.optimal_traj().cpu().numpy()


def _same(ra, rb):
    for x, y in zip(ra, rb):
        assert np.all(np.isfinite(x))
        assert np.array_equal(x, y)


def _steer(name, scn, paths, monkeypatch, finishes):
    """The scenario on ARM_GRIDS[name] in every hand-off form the grid can take; with `finishes` also the fused
    steps.  Returns nothing: every claim is asserted."""
    g = M.ARM_GRIDS[name]
    pool = _pool(g.T, paths)
    idx, light = M.build_index(scn, pool, g)
    eps = pool.cols[idx]
    tied = any(k == "tie" for _, _, k in scn.places)
    runs, errs, S0 = {}, [], None
    for form in _forms(g):
        eng = _make(g, form, monkeypatch)
        noise = eng.upload_noise(eps)
        S, part, w = _plain(eng, noise, paths)
        if S0 is None:
            S0 = S
            if not tied:
                assert len(np.unique(S[light])) == int(light.sum())   # distinct weights: a swapped row would show
        p = M.predict(S, g, LAM, form)
        M.check_intent(scn, p, g, form)
        errs.append(_close_to_plain_sum(S, eps, w, part))
        runs[form] = [w]
        if finishes:
            _inputs(eng, paths)
            eng.rollout(noise, fused_update=True, merge="inline")
            assert not eng.pending()
            r1 = _result(eng)
            errs.append(_close_to_plain_sum(S, eps, r1[0]))
            eng.rollout(noise, fused_update=True, merge="inline")     # a second step, from the updated nominal
            runs[form] += [r1, _result(eng)]
        eng.synchronize()
        eng.close()
    forms = list(runs)
    if len(forms) == 2:                                               # granule against counter
        assert np.array_equal(runs["poll"][0], runs["counter"][0])
        for ra, rb in zip(runs["poll"][1:], runs["counter"][1:]):
            _same(ra, rb)
    if finishes and g.rows <= M.K_DIRECT_ROWS:
        # the deferred form (counter-form rows, whatever the in-launch hand-off), finished by a read ...
        p = M.predict(S0, g, LAM, "counter")
        if scn.path == "two-level":
            assert sorted(p["walk"]) == scn.light_rows()              # the walk's row list, in batches of 32
            assert p["walk_batches"] == -(-len(scn.light_rows()) // 32)
        eng = _make(g, forms[0], monkeypatch)
        noise = eng.upload_noise(eps)
        _inputs(eng, paths)
        eng.rollout(noise, fused_update=True)
        assert eng.pending()
        rd = _result(eng)
        assert not eng.pending()
        _same(rd, runs[forms[0]][1])
        # ... and by the next launch's prologue
        _inputs(eng, paths)
        eng.rollout(noise, fused_update=True)
        eng.rollout(noise, fused_update=True)
        assert eng.pending()
        _same(_result(eng), runs[forms[0]][2])
        eng.synchronize()
        eng.close()
    record("merge_steer", model="arm", grid=name, scenario=scn.name, path=scn.path, rescale=scn.rescale,
           weighted_rows=len(scn.light_rows()), max_abs_err=max(errs))


ROW_CASES = [(name, s) for name in ("t8", "t64", "t128", "g8", "g16", "r257", "r530") for s in M.arm_row_scenarios(name)]


@pytest.mark.parametrize("name,scn", ROW_CASES, ids=[f"{n}-{s.name}" for n, s in ROW_CASES])
def test_weighted_rows(name, scn, paths, monkeypatch):
    """One light sample per light row; every finish in both hand-off forms (the grids past kDirectRows have no
    deferred form and, being larger than the device, no granule form)."""
    _steer(name, scn, paths, monkeypatch, finishes=True)


SAMPLE_CASES = M.arm_sample_scenarios()


@pytest.mark.parametrize("scn", SAMPLE_CASES, ids=[s.name for s in SAMPLE_CASES])
def test_kept_samples_per_workgroup(scn, paths, monkeypatch):
    """The epilogue's gather: every bucket and the dense form, the slots at the wave edges."""
    _steer("t8", scn, paths, monkeypatch, finishes=False)


def test_one_lane_per_sample(paths, monkeypatch):
    """256 samples per workgroup: the dense gather's four passes per lane, 17 and 256 kept samples in a row."""
    (scn,) = M.arm_lps1_scenarios()
    _steer("lps1", scn, paths, monkeypatch, finishes=False)
