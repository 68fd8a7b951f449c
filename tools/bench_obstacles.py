#!/usr/bin/env python
"""Cost of the workspace obstacles on the device loop: 0, 1, 4 and 8 discs, same process.

The timed region is bench.py's: back-to-back fused rollout + update launches (the
device-resident closed loop, no host synchronisation) over rotated Philox noise
buffers whose total exceeds the caches, one event pair around the whole region,
after a settle phase and the same number of converging steps.  Engines of the
same size are built with n = 0, 1, 4 and 8 discs (n = 0: a context that never had
any, which launches the kernels without the feature) and, with `--parent-lib`, one
more on another build of the library (the parent commit's, built from its
sources) through the same Python; they share the noise buffers and are timed
alternately, `--rounds` times each, so clock drift lands on all.  The discs: one
the end effector runs into, one beside link 1, one ahead of the end effector, the
rest out of reach (a disc costs the same whether it is touched or not).  Sizes: c3
(K = 65536, T = 64) and c2 (K = 4096, T = 32), bench.py's.

One JSON line per size: ms per step of each round, the medians, and each
median's ratio to n = 0.
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

from mppi_robotarm_amd import _native as N  # noqa: E402
from mppi_robotarm_amd.engine import RolloutEngine  # noqa: E402
from mppi_robotarm_amd.params import ArmParams  # noqa: E402

X0 = np.array([1.152198236517471885e00, -1.266101672070702344e00, 0.0, 0.0])
SIZES = {"c3": (65536, 64), "c2": (4096, 32)}
DISCS = np.array([[1.393, 0.7811, 0.006], [0.2900, 0.7466, 0.02], [1.3538, 0.7419, 0.015], [-1.5, -1.5, 0.1],
                  [2.5, 0.0, 0.2], [0.0, 2.5, 0.2], [-2.5, 0.0, 0.2], [0.0, -2.5, 0.2]])
COST = 1.0e10
CONVERGE_STEPS = 4000


def engine(K, T, lps, n, lib=None):
    orig = N.load
    if lib is not None:
        L = N.open_library(lib)
        N.load = lambda: L
    try:
        eng = RolloutEngine(K, T, 0.006, 100.0, 0.98, np.eye(2) * 20.0, [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0],
                            0.0, ArmParams(), device=0, lanes_per_sample=lps)
    finally:
        N.load = orig
    if n:
        eng.set_obstacles(DISCS[:n], COST)
    return eng


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
    p.add_argument("--counts", default="0,1,4,8")
    p.add_argument("--parent-lib", default=None, help="another build of libmppi_rocm.so to time beside n = 0")
    args = p.parse_args()
    torch.cuda.set_device(0)
    window = np.load(os.path.join(ROOT, "tests", "golden", "paths.npz"))["xydq_circle"][0:30, :4]
    for size in args.sizes.split(","):
        K, T = SIZES[size]
        u = np.array([[10.0, -2.0]] * T)
        engs = {}
        if args.parent_lib:
            engs["parent"] = engine(K, T, args.lps, 0, args.parent_lib)
        for n in (int(x) for x in args.counts.split(",")):
            engs[f"n{n}"] = engine(K, T, args.lps, n)
        first = next(iter(engs.values()))
        noise = [first.philox_noise(1234, i) for i in range(args.nbuf)]
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
        if "parent" in engs and "n0" in engs:   # the same launch sequence on the same noise: the same nominal
            assert np.array_equal(engs["parent"].nominal(), engs["n0"].nominal())
        med = {name: statistics.median(v) for name, v in ms.items()}
        base = med.get("n0", next(iter(med.values())))
        e = first
        print(json.dumps({"size": size, "K": K, "T": T, "lanes_per_sample": e.lanes_per_sample, "threads": e.threads,
                          "handoff": e.handoff, "cost": COST, "steps": args.steps,
                          "ms_per_step": {k: [round(x, 6) for x in v] for k, v in ms.items()},
                          "median_ms": {k: round(v, 6) for k, v in med.items()},
                          "over_n0": {k: round(v / base, 4) for k, v in med.items()}}), flush=True)
        for eng in engs.values():
            eng.synchronize()
            eng.close()


if __name__ == "__main__":
    main()
