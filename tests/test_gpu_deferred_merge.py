"""GPU: the deferred finish of a fused step (the next launch's prologue merges the previous launch's rows and
updates the nominal, in every workgroup) leaves the same bits as the finish inside the launch.

Every case drives two engines of equal configuration over the same noise buffers, one with merge="auto" (which
takes the deferred form wherever it applies) and one with merge="inline" (MPPI_FLAG_INLINE_MERGE), and compares the
weighted noise, the nominal and the optimal trajectory of the unshifted update with np.array_equal.  The unshifted
update `upd` itself has no getter: it is compared through that trajectory, the fp32 re-roll that mppi_optimal_traj
makes from it with the same kernel in both engines (and not at all in the graph test, which says why).

Shapes: the smallest that reach each branch of the merge (kGroup = 16 workgroups per group, kDirectMax = 16 weighted
rows for the direct merge, kSparseMax = 16 weighted samples for the sparse epilogue):
  one group                 K =  256, LPS 8:  8 workgroups, T = 5 (the median filter's minimum);
  two groups, ragged last   K = 4500, LPS 1: 18 workgroups, the last one partial, T = 7 (T mod 4 != 0);
  many groups               K = 2048, LPS 8: 64 workgroups, T = 32;
  512-thread workgroups     K = 16384, LPS 8: 256 workgroups of 512 threads, T = 5.  The direct merge groups the
                            weighted rows by block size (46 column groups here), so the finish that runs on its own
                            (a read in between) must run at the rollout's block size to leave the same bits.
Regimes: lambda = 1 (one-hot: one row carries weight, the direct merge), 100, 1e6 (every row and every sample
weighted: the two-level merge and the dense epilogue).
"""
import numpy as np
import pytest
import torch

from helpers import X0, _engine, _gpu, _window  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(256, 8, 5), (4500, 1, 7), (2048, 8, 32), (16384, 8, 5)]   # K, LPS, T
BLOCKS = {256: 8, 4500: 18, 2048: 64, 16384: 256}
THREADS = {16384: 512}
LAMBDAS = [1.0, 100.0, 1.0e6]
STEPS = 5


def _pair(K, lps, T, lam, **kw):
    a, b = (_engine(K, T, lps=lps, param_lambda=lam, **kw) for _ in range(2))
    assert a.blocks == b.blocks == BLOCKS.get(K, a.blocks)
    assert a.threads == b.threads == THREADS.get(K, 256)
    return a, b


def _start(eng, paths, T):
    eng.set_step_inputs(X0, _window(paths, 3), np.array([[10.0, -2.0]] * T))


def _result(eng):
    """What a fused step leaves: w_eps, the shifted nominal, the trajectory of the unshifted update (upd)."""
    return eng.weighted_noise(), eng.nominal(), eng.optimal_traj().cpu().numpy()


def _same(ra, rb):
    for x, y in zip(ra, rb):
        assert np.all(np.isfinite(x))
        assert np.array_equal(x, y)


def _close(*engines):
    for e in engines:
        e.synchronize()
        e.close()


@pytest.mark.parametrize("read_between", [False, True])
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("K,lps,T", SHAPES)
def test_chained_launches(K, lps, T, lam, read_between, paths):
    """Five chained launches: without a read in between the step stays pending four times over; with the
    nominal and the weighted noise read after each launch the step is finished on its own and the loop goes on."""
    auto, inline = _pair(K, lps, T, lam)
    noises = [auto.philox_noise(7, s) for s in range(STEPS)]
    for e in (auto, inline):
        _start(e, paths, T)
    for nz in noises:
        auto.rollout(nz, fused_update=True)
        inline.rollout(nz, fused_update=True, merge="inline")
        assert auto.pending() and not inline.pending()
        if read_between:
            assert np.array_equal(auto.nominal(), inline.nominal())
            assert not auto.pending()
            assert np.array_equal(auto.weighted_noise(), inline.weighted_noise())
    _same(_result(auto), _result(inline))
    assert not auto.pending()
    _close(auto, inline)


@pytest.mark.parametrize("lam", [3.0, 10.0, 30.0, 300.0])
def test_finish_on_its_own_at_512_threads(lam, paths):
    """256 workgroups of 512 threads, lambda swept between the one-hot and the dense regime so that some case has
    more than kDirectMax and at most 64 weighted rows: there the direct merge's verdict and its grouped sums depend
    on the block size.  Launches one and three are finished by the next launch's prologue, the others by the
    finish that runs on its own."""
    K, lps, T = 16384, 8, 5
    auto, inline = _pair(K, lps, T, lam)
    noises = [auto.philox_noise(23, s) for s in range(4)]
    for e in (auto, inline):
        _start(e, paths, T)
    for i, nz in enumerate(noises):
        auto.rollout(nz, fused_update=True)
        inline.rollout(nz, fused_update=True, merge="inline")
        if i % 2:
            _same(_result(auto), _result(inline))
    _close(auto, inline)


@pytest.mark.parametrize("new_u", [False, True])
def test_set_step_inputs_while_pending(new_u, paths):
    """New inputs while a step is pending: a state and window alone reach the next launch and leave the step
    pending; a new nominal replaces the step's result, which still lands first (w_eps stays readable)."""
    K, lps, T = 4500, 1, 7
    auto, inline = _pair(K, lps, T, 100.0)
    noises = [auto.philox_noise(11, s) for s in range(4)]
    x1 = X0 + np.array([0.01, -0.02, 0.1, -0.1])
    u1 = np.array([[9.0, -1.0]] * T) + np.arange(T)[:, None] * 0.1
    for e in (auto, inline):
        _start(e, paths, T)
    for i, nz in enumerate(noises):
        auto.rollout(nz, fused_update=True)
        inline.rollout(nz, fused_update=True, merge="inline")
        if i == 1:
            for e in (auto, inline):
                e.set_step_inputs(x1, _window(paths, 5), u1 if new_u else None)
            assert auto.pending() == (not new_u)
            if new_u:
                assert np.array_equal(auto.weighted_noise(), inline.weighted_noise())
    _same(_result(auto), _result(inline))
    _close(auto, inline)


@pytest.mark.parametrize("modes", [("auto", "inline", "auto", "auto", "inline"),
                                   ("inline", "auto", "inline", "auto", "auto")])
def test_forms_alternate(modes, paths):
    """A deferred launch followed by a forced in-launch one, and the reverse, on one context."""
    K, lps, T = 2048, 8, 32
    mixed, inline = _pair(K, lps, T, 100.0)
    noises = [mixed.philox_noise(13, s) for s in range(len(modes))]
    for e in (mixed, inline):
        _start(e, paths, T)
    for nz, m in zip(noises, modes):
        mixed.rollout(nz, fused_update=True, merge=m)
        inline.rollout(nz, fused_update=True, merge="inline")
        assert mixed.pending() == (m == "auto")
    _same(_result(mixed), _result(inline))
    _close(mixed, inline)


@pytest.mark.parametrize("variant", ["clamp2", "obstacle"])
@pytest.mark.parametrize("K,lps,T", SHAPES)
def test_clamp_and_obstacle_kernels(K, lps, T, variant, paths):
    """The CLAMP and CLAMP + OBST instantiations: clamp_mode 2 with finite limits that bind (the updated nominal
    is clipped in the deferred update too), and one disc at the end effector."""
    kw = dict(u_min=[-5.0, -2.5], u_max=[10.5, 0.0]) if variant == "clamp2" else {}
    auto, inline = _pair(K, lps, T, 100.0, **kw)
    if variant == "obstacle":
        for e in (auto, inline):
            e.set_obstacles(np.array([[1.393, 0.7811, 0.006]]), 50.0)
    noises = [auto.philox_noise(17, s) for s in range(STEPS)]
    for e in (auto, inline):
        _start(e, paths, T)
    for nz in noises:
        auto.rollout(nz, fused_update=True)
        inline.rollout(nz, fused_update=True, merge="inline")
    assert auto.pending()
    ra, rb = _result(auto), _result(inline)
    _same(ra, rb)
    if variant == "clamp2":
        assert ra[1][:, 0].max() <= 10.5 and ra[1][:, 1].min() >= -2.5
    _close(auto, inline)


def test_graph_capture_takes_the_in_launch_form(paths):
    """Two fused steps captured into a graph: a replay cannot track the pending state, so the capture takes the
    in-launch form, and the replay leaves what two eager (deferred) steps leave."""
    K, lps, T = 2048, 8, 32
    eager, graphed = _pair(K, lps, T, 100.0)
    noises = [eager.philox_noise(19, s) for s in range(2)]
    _start(eager, paths, T)
    for nz in noises:
        eager.rollout(nz, fused_update=True)
    assert eager.pending()
    ref = _result(eager)
    _start(graphed, paths, T)
    graphed.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        for nz in noises:
            graphed.rollout(nz, fused_update=True)
        assert not graphed.pending()
    torch.cuda.current_stream().wait_stream(s)
    _start(graphed, paths, T)
    graphed.synchronize()
    g.replay()
    torch.cuda.synchronize()
    # (no optimal trajectory here: the context cannot know that a replay ran a fused update after the new nominal)
    _same((graphed.weighted_noise(), graphed.nominal()), ref[:2])
    _close(eager, graphed)
