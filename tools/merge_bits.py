"""The hand-off merges' result bits of two builds of the C ABI, in ONE process on the same Philox buffers
(diagnostic tool, not product).  The tests compare the merge forms of one build with each other; this compares
every form with another build's, which is what a change to the shared merge code has to keep.

    python tools/merge_bits.py PARENT.so NEW.so [OUTDIR]

Per build and case: sha1 (12 hex digits) of w_eps and of the nominal after four fused launches.  Arm cases run with
the rows polled and behind counters (MPPI_HANDOFF=counter), each deferred (merge="auto") and in the launch
(merge="inline"); chain cases polled and behind counters; the multi-round row merges of
tests/test_gpu_merge_rounds.py go through mppi_merge_partials / mppi_chain_merge_partials.  With OUTDIR, each
build's lines go to OUTDIR/merge_bits_<library name>.txt.  Exit status 1 when the builds differ.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mppi_robotarm_amd import _native as N  # noqa: E402
from mppi_robotarm_amd import chain as CH  # noqa: E402
from mppi_robotarm_amd.engine import RolloutEngine  # noqa: E402
from mppi_robotarm_amd.params import X0_RUNPY, ArmParams  # noqa: E402

PATH = np.load(os.path.join(ROOT, "tests", "golden", "paths.npz"))["xydq_circle"][:, :4]
W, TW = [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0]
ARM = [(256, 8, 5), (4500, 1, 7), (4352, 1, 8), (16640, 1, 8), (2048, 8, 32), (16384, 8, 5)]   # K, LPS, T
ARM_LAMBDAS = {16384: (1.0, 3.0, 10.0, 30.0, 100.0, 300.0, 1.0e9)}
CHAIN3 = [(4352, 1), (1024, 1), (1088, 4)]               # n = 3, T = 5: K, lanes per sample
CHAIN7 = [(100.0, 1), (1.0e9, 1), (100.0, 4)]            # test_chain_handoff_forms_are_bit_identical: lambda, lanes
LAUNCHES = 4


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def handoff(form):
    if form == "counter":
        os.environ["MPPI_HANDOFF"] = "counter"
    else:
        os.environ.pop("MPPI_HANDOFF", None)


def fused(eng, x0, win, u, merge="auto"):
    noises = [eng.philox_noise(29, s) for s in range(LAUNCHES)]
    eng.set_step_inputs(x0, win, u)
    for nz in noises:
        eng.rollout(nz, fused_update=True, merge=merge)
    out = f"w_eps {sha(eng.weighted_noise())} nominal {sha(eng.nominal())}"
    eng.synchronize()
    eng.close()
    return out


def merge_rows(n, nval, lam):
    """The rows of tests/test_gpu_merge_rounds.py."""
    rng = np.random.default_rng(20261020)
    rho = 1000.0 + lam * rng.uniform(0.0, 3.0, n)
    rho[n // 2] -= 5.0 * lam
    rho[n - 2] -= 9.0 * lam
    rho[3] += 60.0 * lam
    rho[n - 1] += 60.0 * lam
    eta = rng.uniform(1.0, 256.0, n)
    return np.concatenate([rho[:, None], eta[:, None], eta[:, None] * rng.uniform(-1.0, 1.0, (n, nval))], axis=1)


def merged(eng, n):
    parts = torch.from_numpy(merge_rows(n, eng.T * eng.dim_u, eng.lam)).to(eng.device).contiguous()
    eng.merge(parts, n)
    out = f"w_eps {sha(eng.weighted_noise())}"
    eng.close()
    return out


def arm_engine(K, lps, T, lam):
    eng = RolloutEngine(K, T, 0.006, lam, 0.98, np.eye(2) * 20.0, np.array(W), np.array(TW), 0.0, ArmParams(),
                        device=0, lanes_per_sample=lps)
    eng.lam = lam
    return eng


def chain3():
    n, L = 3, 2.0 / 3
    P = CH.ChainParams(m=(1.0,) * n, l=(L,) * n, lc=(L / 2,) * n, I=(L * L / 12.0,) * n, fk=(L,) * n, J=(0.1,) * n,
                       b=(1.0,) * n)
    q = np.array([1.4, -1.1, -1.1])
    return P, np.concatenate([q, [0.1, -0.2, 0.05]]), np.eye(n) * 4.0, CH.gravity_torque(q, P)


def chain_engine(K, T, lam, lps, P, sig):
    eng = CH.ChainEngine(K, T, 0.006, lam, 0.98, sig, W, TW, 0.0, P, device=0, lanes_per_sample=lps)
    eng.lam = lam
    return eng


def cases():
    """(label, thunk) in a fixed order; a thunk returns the case's line."""
    x0 = np.asarray(X0_RUNPY, dtype=np.float64)
    for K, lps, T in ARM:
        for lam in ARM_LAMBDAS.get(K, (1.0, 100.0, 1.0e9)):
            for form in ("poll", "counter"):
                for merge in ("auto", "inline"):
                    def run(K=K, lps=lps, T=T, lam=lam, form=form, merge=merge):
                        handoff(form)
                        eng = arm_engine(K, lps, T, lam)
                        assert eng.handoff == form
                        return fused(eng, x0, PATH[3:33], np.array([[10.0, -2.0]] * T), merge)
                    yield f"arm K={K} lps={lps} T={T} lambda={lam:g} {form} {merge}", run
    P3, x3, sig3, ug3 = chain3()
    for K, lps in CHAIN3:
        for lam in (100.0, 1.0e9):
            for form in ("poll", "counter"):
                def run(K=K, lps=lps, lam=lam, form=form):
                    handoff(form)
                    eng = chain_engine(K, 5, lam, lps, P3, sig3)
                    assert eng.handoff == form
                    return fused(eng, x3, PATH[40:70], np.tile(ug3, (5, 1)))
                yield f"chain n=3 K={K} lps={lps} T=5 lambda={lam:g} {form}", run
    ug7 = CH.gravity_torque(CH.CHAIN7_X0[:7])
    for lam, lps in CHAIN7:
        for form in ("poll", "counter"):
            def run(lam=lam, lps=lps, form=form):
                handoff(form)
                eng = chain_engine(32768 // lps, 48, lam, lps, CH.ChainParams(), CH.CHAIN7_SIGMA)
                assert eng.handoff == form
                return fused(eng, CH.CHAIN7_X0, PATH[2:32], np.tile(ug7, (48, 1)))
            yield f"chain n=7 K={32768 // lps} lps={lps} T=48 lambda={lam:g} {form}", run
    handoff("poll")
    for lam in (1.0, 100.0, 1.0e6):
        yield f"arm merge_partials 70 rows T=5 lambda={lam:g}", lambda lam=lam: merged(arm_engine(256, 1, 5, lam), 70)
        yield (f"chain merge_partials 40 rows n=3 T=5 lambda={lam:g}",
               lambda lam=lam: merged(chain_engine(256, 5, lam, 1, P3, sig3), 40))


def main():
    libs = [os.path.abspath(a) for a in sys.argv[1:] if a.endswith(".so")]
    outdir = next((a for a in sys.argv[1:] if not a.endswith(".so")), None)
    assert len(libs) == 2, __doc__
    torch.cuda.set_device(0)
    lines = {}
    orig = N.load
    for p in libs:
        L = N.open_library(p)
        N.load = lambda L=L: L   # the engines of this pass bind this build
        try:
            lines[p] = [f"{label}: {run()}" for label, run in cases()]
        finally:
            N.load = orig
        print(f"== {p}\n" + "\n".join(lines[p]), flush=True)
        if outdir:
            os.makedirs(outdir, exist_ok=True)
            with open(os.path.join(outdir, f"merge_bits_{os.path.splitext(os.path.basename(p))[0]}.txt"), "w") as f:
                f.write("\n".join(lines[p]) + "\n")
    a, b = (lines[p] for p in libs)
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in diff:
        print(f"DIFFERENT\n  {x}\n  {y}")
    print(f"{len(a)} cases, {len(diff)} differ")
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
