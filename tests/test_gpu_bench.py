"""GPU: bench.py's plain run at a small size: --steps is the number of timed steps, the legs beside the headline
figure stay behind --full, and --dump-outputs writes the last timed step's outputs, equal from run to run.
"""
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers import _gpu  # noqa: E402, F401


def _run(monkeypatch, capsys, *argv):
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1   # one JSON line
    return json.loads(lines[0])


@pytest.mark.parametrize("workload,launch,K,T,du", [("c3", "eager", 640, 12, 2), ("c3", "graph", 640, 12, 2),
                                                    ("c5", "eager", 512, 8, 7)])
def test_plain_run_and_dumped_outputs(monkeypatch, capsys, tmp_path, workload, launch, K, T, du):
    """Two plain runs with different settle times (a different number of untimed steps before the warmup): 13 timed
    steps each (no multiple of the 10 noise buffers a captured graph holds), no latency or CPU legs in the line,
    and u_nominal / w_eps of the last timed step as fp64 (T, du) arrays, bit-equal between the runs."""
    outs = []
    for tag, settle in (("a", "0"), ("b", "30")):
        d = tmp_path / tag
        r = _run(monkeypatch, capsys, "--gpus", "1", "--steps", "13", "--warmup", "3", "--settle-ms", settle,
                 "--workload", workload, "--launch", launch, "--K", str(K), "--T", str(T), "--dump-outputs", str(d))
        assert r["steps"] == 13 and r["warmup"] == 3
        assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(K * T / (r["ms_per_step"] * 1e-3))
        assert r["unit"] == "state-steps/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
        assert r["control_step_latency_ms"] is None and "cpu_baseline" not in r
        assert not [k for k in r if k.startswith("control_step_latency_") and k != "control_step_latency_ms"]
        assert sorted(p.name for p in d.iterdir()) == ["u_nominal.npy", "w_eps.npy"]
        arrs = {n: np.load(d / f"{n}.npy") for n in ("u_nominal", "w_eps")}
        for a in arrs.values():
            assert a.dtype == np.float64 and a.shape == (T, du) and np.all(np.isfinite(a))
        assert np.any(arrs["w_eps"] != 0.0)
        outs.append(arrs)
    for n in ("u_nominal", "w_eps"):
        assert np.array_equal(outs[0][n], outs[1][n]), n
