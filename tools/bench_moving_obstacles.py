#!/usr/bin/env python
"""Cost of moving obstacles on the device loop, arm and chain: discs at rest before and after, and discs that move.

The timed region is bench.py's: back-to-back fused rollout + update launches over rotated Philox noise buffers, one
event pair around the whole region (tools/bench_obstacles.py for the arm's sizes, whose discs, settle phase and
converging steps this reuses; tools/bench_chain_obstacles.py for the chain's, with its discs and its reset of the
step inputs every 32 steps).  For each size and disc count (1, 4, 8) three engines share the noise buffers and are
timed alternately, `--rounds` times each, so clock drift lands on all:

  parent   `--parent-lib`, the parent commit's library (built from its sources), discs at rest;
  rest     this library, the same discs at rest (mppi_[chain_]set_obstacles: the kernels the parent launches);
  moving   this library, the same discs with velocities (mppi_[chain_]set_moving_obstacles: the MOVE kernels).

Sizes: c3 (K = 65536, T = 64) and c2 (K = 4096, T = 32), the arm's; c5 (the 7-link chain, K = 131072, T = 128, one
lane per sample) and c5s (its 8-way shard, K = 16384, a quad per sample).  One JSON line per size and count: ms per
step of each round, the medians, moving over rest, and `rest_in_parent_range`: whether the median of `rest` lies within
the parent's own round-to-round range in this run (the acceptance for discs at rest).  On the arm `parent` and `rest`
run the same launch sequence on the same noise and must leave the same nominal.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_chain_obstacles as BC  # noqa: E402
import bench_obstacles as BA  # noqa: E402
from mppi_robotarm_amd import _native  # noqa: E402
from mppi_robotarm_amd.engine import RolloutEngine  # noqa: E402
from mppi_robotarm_amd.params import ArmParams  # noqa: E402

# m/s: every disc moves, the touched ones slowly enough to stay in reach over the timed steps' horizons
VEL = np.array([[0.15, -0.10], [-0.05, 0.03], [0.20, 0.10], [0.1, 0.1], [0.1, 0.0], [0.0, 0.1], [-0.1, 0.0], [0.0, -0.1]])


def make(size, lps, lib=None):
    """The engine of a size on this library or, with `lib`, on another build of it (which the engine keeps)."""
    product = _native.load()
    if lib is not None:
        _native._lib = _native.open_library(lib)   # (it has no set_moving_obstacles: the engine resolves that leniently)
    try:
        if size in BA.SIZES:
            K, T = BA.SIZES[size]
            return RolloutEngine(K, T, 0.006, 100.0, 0.98, np.eye(2) * 20.0, [0.5, 0.5, 5.0, 5.0],
                                 [5.0, 5.0, 50.0, 50.0], 0.0, ArmParams(), device=0, lanes_per_sample=lps)
        K, T = BC.SIZES[size]
        return BC.ChainEngine(K, T, 0.006, 100.0, 0.98, BC.CHAIN7_SIGMA, [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0],
                              0.0, BC.ChainParams(), device=0, precision="f32", lanes_per_sample=lps)
    finally:
        _native._lib = product


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--sizes", default="c3,c2,c5,c5s")
    p.add_argument("--steps", type=int, default=None, help="timed steps per round (arm: 2000, chain: 320)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--settle-ms", type=float, default=200.0)
    p.add_argument("--lps", type=int, default=0)
    p.add_argument("--counts", default="1,4,8")
    p.add_argument("--parent-lib", default=None, help="the parent commit's libmppi_rocm.so")
    args = p.parse_args()
    torch.cuda.set_device(0)
    window = np.load(os.path.join(ROOT, "tests", "golden", "paths.npz"))["xydq_circle"][0:30, :4]
    for size in args.sizes.split(","):
        arm = size in BA.SIZES
        K, T = (BA.SIZES if arm else BC.SIZES)[size]
        steps = args.steps or (2000 if arm else 320)
        warmup, nbuf = steps // 10, (10 if arm else 4)
        discs = BA.DISCS if arm else BC.discs()
        inputs = (BA.X0, window, np.array([[10.0, -2.0]] * T)) if arm else \
            (BC.CHAIN7_X0.copy(), window, np.tile(BC.UG, (T, 1)))

        def run(eng, noise, n, start):     # (the chain's plant-less loop drifts: bench.py resets its inputs)
            for i in range(start, start + n):
                if not arm and i % BC.RESET == 0:
                    eng.set_step_inputs(*inputs)
                eng.rollout(noise[i % nbuf], fused_update=True)

        def timed(eng, noise, n, start):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream = torch.cuda.current_stream()
            a.record(stream)
            run(eng, noise, n, start)
            b.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(b) / n

        for n in (int(x) for x in args.counts.split(",")):
            engs = {}
            if args.parent_lib:
                engs["parent"] = make(size, args.lps, args.parent_lib)
                engs["parent"].set_obstacles(discs[:n], BA.COST)
            engs["rest"] = make(size, args.lps)
            engs["rest"].set_obstacles(discs[:n], BA.COST)
            engs["moving"] = make(size, args.lps)
            engs["moving"].set_obstacles(discs[:n], BA.COST, velocities=VEL[:n])
            first = engs["rest"]
            noise = [first.philox_noise(1234, i) for i in range(nbuf)]
            for eng in engs.values():
                eng.set_step_inputs(*inputs)
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
                    run(eng, noise, 16, 0)
                    torch.cuda.synchronize()
                eng.set_step_inputs(*inputs)
                run(eng, noise, BA.CONVERGE_STEPS if arm else 0, 0)
                torch.cuda.synchronize()
            ms = {name: [] for name in engs}
            for r in range(args.rounds):
                for name, eng in engs.items():
                    timed(eng, noise, warmup, 0)
                    ms[name].append(timed(eng, noise, steps, warmup))
            if "parent" in engs and arm:
                assert np.array_equal(engs["parent"].nominal(), engs["rest"].nominal())
            med = {name: statistics.median(v) for name, v in ms.items()}
            out = {"size": size, "K": K, "T": T, "discs": n, "lanes_per_sample": first.lanes_per_sample,
                   "handoff": first.handoff, "steps": steps,
                   "ms_per_step": {k: [round(x, 6) for x in v] for k, v in ms.items()},
                   "median_ms": {k: round(v, 6) for k, v in med.items()},
                   "moving_over_rest": round(med["moving"] / med["rest"], 4)}
            if "parent" in engs:
                out["rest_over_parent"] = round(med["rest"] / med["parent"], 4)
                out["rest_in_parent_range"] = bool(min(ms["parent"]) <= med["rest"] <= max(ms["parent"]))
            print(json.dumps(out), flush=True)
            for eng in engs.values():
                eng.synchronize()
                eng.close()
            del noise, engs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
