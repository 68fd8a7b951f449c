"""GPU: sampled_traj_list's host read-back (include/mppi_rocm.h mppi_readback_*, control.py:135-145).

The device re-roll writes fp32 states; the read-back DMAs them in chunks and widens them to fp64 on host
threads.  fp32 -> fp64 is exact, so the result must equal torch's own widening bit for bit, whatever the
chunking, the ring size, the worker count and the destination's alignment.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers import _gpu  # noqa: E402, F401


def _values(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3.0
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1e-45, -1e-45, 1.17e-38,
                            3.4e38, -3.4e38], dtype=torch.float32)
    m = min(n, special.numel())
    x[:m] = special[:m]
    x[n - m:] = special[:m]
    return x.to(torch.float32)


def _bits_equal(a: np.ndarray, b: np.ndarray) -> bool:
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n,chunk,slots,workers,streams", [
    (1, 128, 2, 1, 0), (17, 128, 2, 3, 1), (1000, 128, 2, 4, 2), (100003, 4096, 3, 7, 3), (1 << 20, 1 << 16, 4, 16, 2),
    (3 * (1 << 20) + 5, 1 << 18, 8, 16, 2), (5_000_001, 1 << 20, 8, 16, 4), (5_000_001, 1 << 21, 2, 5, 0)])
def test_readback_equals_torch_widening(n, chunk, slots, workers, streams):
    from mppi_robotarm_amd.engine import HostReadback
    rb = HostReadback(torch.device("cuda", 0), workers=workers, chunk=chunk, slots=slots, streams=streams)
    try:
        src = _values(n, n).cuda()
        want = src.double().cpu().numpy()
        for off in (0, 1, 3):                      # destinations off the 32 B store alignment
            buf = np.full(n + off, 7.0)
            dst = buf[off:]
            rb.run(src, dst)
            assert _bits_equal(dst, want)
            assert np.all(buf[:off] == 7.0)
        # ordered after work queued on the stream: a kernel writing src right before the read-back
        src2 = src * 2.0
        dst = np.empty(n)
        rb.run(src2, dst)
        assert _bits_equal(dst, src2.double().cpu().numpy())
    finally:
        rb.close()


def test_readback_of_trajectory_shaped_tensor_and_reuse():
    """(K, T, 4) like the c3 re-roll, read back repeatedly into the same array (the pool's reuse)."""
    from mppi_robotarm_amd.engine import HostReadback
    rb = HostReadback(torch.device("cuda", 0))
    try:
        K, T = 8192, 64
        out = np.empty((K, T, 4))
        for i in range(3):
            tr = torch.randn((K, T, 4), device="cuda", dtype=torch.float32) + i
            rb.run(tr, out)
            assert _bits_equal(out, tr.double().cpu().numpy())
        with pytest.raises(ValueError):
            rb.run(tr, np.empty((K, T, 3)))
        with pytest.raises(ValueError):
            rb.run(tr.double(), out)
    finally:
        rb.close()
