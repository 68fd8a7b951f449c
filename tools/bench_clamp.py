#!/usr/bin/env python
"""Cost of the torque limits on the device loop: clamped against unclamped, same process.

The timed region is bench.py's: back-to-back fused rollout + update launches (the
device-resident closed loop, no host synchronisation) over rotated Philox noise
buffers whose total exceeds the caches, one event pair around the whole region,
after a settle phase and the same number of converging steps.  Two engines of the
same size are built, one without limits and one with u_min = (4, -6),
u_max = (14, 2) (about a third of the sampled controls clipped at run.py's
settings); they share the noise buffers and are timed alternately, `--rounds`
times each, so clock drift lands on both.  Sizes: c3 (K = 65536, T = 64) and c2
(K = 4096, T = 32), bench.py's.

One JSON line per size: ms per step of each round, the medians and their ratio.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mppi_robotarm_amd.engine import RolloutEngine  # noqa: E402
from mppi_robotarm_amd.params import ArmParams  # noqa: E402

X0 = np.array([1.152198236517471885e00, -1.266101672070702344e00, 0.0, 0.0])
SIZES = {"c3": (65536, 64), "c2": (4096, 32)}
LO, HI = (4.0, -6.0), (14.0, 2.0)
CONVERGE_STEPS = 4000


def engine(K, T, lps, limits):
    kw = dict(u_min=LO, u_max=HI) if limits else {}
    return RolloutEngine(K, T, 0.006, 100.0, 0.98, np.eye(2) * 20.0, [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0],
                         0.0, ArmParams(), device=0, lanes_per_sample=lps, **kw)


def timed(eng, noise, steps, start):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream()
    a.record(stream)
    for i in range(start, start + steps):
        eng.rollout(noise[i % len(noise)], fused_update=True)
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--sizes", default="c3,c2")
    p.add_argument("--steps", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--nbuf", type=int, default=10)
    p.add_argument("--settle-ms", type=float, default=200.0)
    p.add_argument("--lps", type=int, default=0)
    args = p.parse_args()
    torch.cuda.set_device(0)
    window = np.load(os.path.join(ROOT, "tests", "golden", "paths.npz"))["xydq_circle"][0:30, :4]
    for size in args.sizes.split(","):
        K, T = SIZES[size]
        u = np.array([[10.0, -2.0]] * T)
        engs = {"unclamped": engine(K, T, args.lps, False), "clamped": engine(K, T, args.lps, True)}
        noise = [engs["unclamped"].philox_noise(1234, i) for i in range(args.nbuf)]
        for eng in engs.values():
            eng.set_step_inputs(X0, window, u)
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
                for i in range(16):
                    eng.rollout(noise[i % args.nbuf], fused_update=True)
                torch.cuda.synchronize()
            eng.set_step_inputs(X0, window, u)
            for i in range(CONVERGE_STEPS):
                eng.rollout(noise[i % args.nbuf], fused_update=True)
            torch.cuda.synchronize()
        ms = {name: [] for name in engs}
        for r in range(args.rounds):
            for name, eng in engs.items():
                timed(eng, noise, args.warmup, 0)
                ms[name].append(timed(eng, noise, args.steps, args.warmup))
        inside = engs["clamped"].nominal()
        assert np.all((inside >= LO) & (inside <= HI))
        med = {name: statistics.median(v) for name, v in ms.items()}
        e = engs["clamped"]
        print(json.dumps({"size": size, "K": K, "T": T, "lanes_per_sample": e.lanes_per_sample, "threads": e.threads,
                          "handoff": e.handoff, "u_min": LO, "u_max": HI, "steps": args.steps,
                          "ms_per_step": {k: [round(x, 6) for x in v] for k, v in ms.items()},
                          "median_ms": {k: round(v, 6) for k, v in med.items()},
                          "clamped_over_unclamped": round(med["clamped"] / med["unclamped"], 4)}), flush=True)
        for eng in engs.values():
            eng.synchronize()
            eng.close()


if __name__ == "__main__":
    main()
