#!/usr/bin/env python
"""Cost of the self-collision cost on the chain's device loop: off, on, on beside one disc, same process.

tools/bench_chain_obstacles.py for mppi_chain_set_self_collision.  The timed region is bench.py's at
--workload c5: back-to-back fused rollout + update launches over rotated Philox noise buffers, the
start nominal staged again every 32 steps (the plant-less chain loop drifts), one event pair around
the whole region, after a settle phase.  Three legs are timed alternately, `--rounds` times each, so
clock drift lands on all of them:

  other_lib   an engine on another build of the library (`--other-lib PATH`: the parent commit's,
              which has no such entry point), feature off by construction;
  off         this library, self-collision disabled: the kernels a context launched before;
  self, self_disc1
              this library, self-collision enabled (clearance 3 cm, cost 1e10: the SELF kernels)
              without discs and beside bench_chain_obstacles.py's first disc.

Config 5's start pose is an open arc, its closest non-adjacent links a link length (29 cm) apart: no rollout pays, and
the SELF kernels test every pair at every step all the same.
Sizes: c5 (K = 131072, T = 128, one lane per sample) and its 8-way shard c5s (K = 16384, a quad per sample).

One JSON line per size: us per step of each round, the medians, the ranges, the ratios to `off`.
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

from mppi_robotarm_amd import _native  # noqa: E402
from mppi_robotarm_amd.chain import CHAIN7_SIGMA, CHAIN7_X0, ChainEngine, ChainParams, gravity_torque  # noqa: E402

SIZES = {"c5": (131072, 128), "c5s": (16384, 128)}
RESET = 32   # bench.py's C5_RESET
UG = gravity_torque(CHAIN7_X0[:7])
CLEARANCE, COST = 0.03, 1.0e10


def disc():
    """bench_chain_obstacles.py's first disc: beside the tip of the start pose, 1.5 mm clear of it."""
    P = ChainParams()
    th = np.cumsum(CHAIN7_X0[:7])
    tip = np.array([(np.asarray(P.fk) * np.cos(th)).sum(), (np.asarray(P.fk) * np.sin(th)).sum()])
    side = np.array([-np.sin(th[-1]), np.cos(th[-1])])
    return np.array([[tip[0] + 0.0115 * side[0], tip[1] + 0.0115 * side[1], 0.01]])


def engine(K, T, lps, precision, lib=None):
    product = _native.load()
    if lib is not None:
        _native._lib = _native.open_library(lib)   # the engine keeps the library it was built on
    try:
        return ChainEngine(K, T, 0.006, 100.0, 0.98, CHAIN7_SIGMA, [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0], 0.0,
                           ChainParams(), device=0, precision=precision, lanes_per_sample=lps)
    finally:
        _native._lib = product


def run(eng, noise, steps, start, inputs):
    for i in range(start, start + steps):
        if i % RESET == 0:
            eng.set_step_inputs(*inputs)
        eng.rollout(noise[i % len(noise)], fused_update=True)


def timed(eng, noise, steps, start, inputs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream()
    a.record(stream)
    run(eng, noise, steps, start, inputs)
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e3   # us per step


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--sizes", default="c5,c5s")
    p.add_argument("--steps", type=int, default=320)
    p.add_argument("--warmup", type=int, default=32)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--nbuf", type=int, default=4)
    p.add_argument("--settle-ms", type=float, default=200.0)
    p.add_argument("--lps", type=int, default=0)
    p.add_argument("--precision", choices=("f32", "f64"), default="f32")
    p.add_argument("--other-lib", default=None, help="another build of libmppi_rocm.so: an engine without the feature")
    args = p.parse_args()
    torch.cuda.set_device(0)
    window = np.load(os.path.join(ROOT, "tests", "golden", "paths.npz"))["xydq_circle"][0:30, :4]
    D = disc()

    def setup(e, mode):
        if mode == "other":
            return
        e.set_obstacles(D if mode == "self_disc1" else None, 1.0e10)
        e.set_self_collision(None if mode == "off" else CLEARANCE, COST)

    for size in args.sizes.split(","):
        K, T = SIZES[size]
        inputs = (CHAIN7_X0.copy(), window, np.tile(UG, (T, 1)))
        eng = engine(K, T, args.lps, args.precision)
        other = engine(K, T, args.lps, args.precision, lib=args.other_lib) if args.other_lib else None
        noise = [eng.philox_noise(1234, i) for i in range(args.nbuf)]
        variants = ([("other_lib", other, "other")] if other else []) + \
            [("off", eng, "off"), ("self", eng, "self"), ("self_disc1", eng, "self_disc1")]
        for name, e, mode in variants:
            setup(e, mode)
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.settle_ms / 2:
                run(e, noise, 16, 0, inputs)
                torch.cuda.synchronize()
        us = {name: [] for name, _, _ in variants}
        for r in range(args.rounds):
            for name, e, mode in variants:
                setup(e, mode)
                timed(e, noise, args.warmup, 0, inputs)
                us[name].append(timed(e, noise, args.steps, args.warmup, inputs))
        # the feature is seen: a clearance wider than the reach makes every rollout pay at every step
        S = torch.empty(K, dtype=torch.float64, device="cuda")
        eng.set_step_inputs(*inputs)
        eng.set_obstacles(None)
        eng.set_self_collision(CLEARANCE, COST)
        eng.rollout(noise[0], S_out=S)
        paying = float((S >= COST).double().mean().item())
        eng.set_self_collision(10.0, COST)
        eng.rollout(noise[0], S_out=S)
        paying_wide = float((S >= (T + 1) * COST).double().mean().item())
        med = {name: statistics.median(v) for name, v in us.items()}
        out = {"size": size, "K": K, "T": T, "precision": args.precision, "lanes_per_sample": eng.lanes_per_sample,
               "handoff": eng.handoff, "steps": args.steps, "clearance": CLEARANCE,
               "share_paying_first_step": round(paying, 4), "share_paying_every_step_at_10m": round(paying_wide, 4),
               "us_per_step": {k: [round(x, 3) for x in v] for k, v in us.items()},
               "median_us": {k: round(v, 3) for k, v in med.items()},
               "range_us": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
               "over_off": {k: round(v / med["off"], 4) for k, v in med.items()},
               "added_us": {k: round(v - med["off"], 3) for k, v in med.items()}}
        print(json.dumps(out), flush=True)
        for e in (eng, other):
            if e is not None:
                e.synchronize()
                e.close()
        del noise
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
