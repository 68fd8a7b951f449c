"""GPU: the four native contexts give back what they allocate (csrc/mppi_host.h's owners behind every
mppi_*_destroy).  One cycle creates, uses once and closes an arm engine, an fp32 and an fp64 3-link chain engine
(each with its exchange inbox allocated and attached, world 1), a NumPy-stream draw that grows its buffers once
and a host read-back; the device's free memory after 32 such cycles is compared with its drop F while the first
cycle's contexts are alive.  A drop below F over the 32 cycles excludes a leak of F / 32 or more per cycle and
tolerates the allocator's granularity.  No kernel is under test: the shapes are the smallest the contexts take."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K, T = 1024, 20
WARMUP, CYCLES = 4, 32
W, TW = [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0]


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _cycle(win, probe=None):
    from mppi_robotarm_amd import hostrng
    from mppi_robotarm_amd.chain import ChainEngine, ChainParams, gravity_torque
    from mppi_robotarm_amd.engine import HostReadback, NpDeviceStream, RolloutEngine
    from mppi_robotarm_amd.params import X0_RUNPY
    dev = torch.device("cuda", 0)
    ln = 2.0 / 3.0   # three uniform slender links, total reach 2 m, drives as the 7-link default's
    P3 = ChainParams(m=(1.0,) * 3, l=(ln,) * 3, lc=(ln / 2,) * 3, I=(ln * ln / 12.0,) * 3, fk=(ln,) * 3,
                     J=(0.1,) * 3, b=(1.0,) * 3)
    x3 = np.array([1.2, -0.4, -0.4, 0.0, 0.0, 0.0])
    engines = [(RolloutEngine(K, T, 0.01, 50.0, 0.98, np.eye(2) * 20.0, W, TW, device=0), X0_RUNPY,
                np.array([[10.0, -2.0]] * T))]
    for prec in ("f32", "f64"):
        engines.append((ChainEngine(K, T, 0.006, 100.0, 0.98, np.diag([8.0, 4.0, 2.0]), W, TW, chain=P3, device=0,
                                    precision=prec), x3, np.tile(gravity_torque(x3[:3], P3), (T, 1))))
    for eng, x0, u in engines:
        eng.exchange_attach(0, 1, [eng.exchange_handle(1)])   # the inbox exists; the step below is this rank's own
        eng.set_step_inputs(x0, win, u)
        eng.rollout(eng.philox_noise(3, 0), fused_update=True)
        eng.synchronize()
    nd = NpDeviceStream(dev)
    plan = hostrng.device_plan(np.zeros(2), np.eye(2) * 20.0)
    np.random.seed(11)
    for k in (hostrng._MIN_NORMALS // (2 * 16), hostrng._MIN_NORMALS // 16):   # the second draw grows d_words, d_look
        out = torch.empty((16, k, 2), dtype=torch.float32, device=dev)
        nd.draw(np.random.get_state(), (k, 16, 2), plan, out, torch.cuda.current_stream().cuda_stream, 0, k,
                (k * 2, 2, 1))
        assert nd.result() is not None
    rb = HostReadback(dev, chunk=4096, slots=2)
    src = torch.arange(8192, dtype=torch.float32, device=dev)
    dst = rb.run(src, np.empty(8192))
    assert dst[-1] == 8191.0
    if probe is not None:
        probe()
    for eng, _, _ in engines:
        eng.close()
    nd.close()
    rb.close()


def test_contexts_return_their_memory(paths):
    torch.cuda.set_device(0)
    win = paths["xydq_circle"][:30]
    alive = []
    before = _free()
    _cycle(win, probe=lambda: alive.append(_free()))
    F = before - alive[0]
    for _ in range(WARMUP - 1):
        _cycle(win)
    start = _free()
    for _ in range(CYCLES):
        _cycle(win)
    drop = start - _free()
    print(f"lifetime: F = {F} B with one cycle's contexts alive, drop over {CYCLES} cycles = {drop} B")
    assert F > 0
    assert drop < F
