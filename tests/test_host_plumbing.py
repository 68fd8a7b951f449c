"""CPU: the host plumbing both native contexts share (csrc/mppi_host.h) in a stand-alone host build under
AddressSanitizer and UBSan (tests/host_plumbing_main.hip: its own main, run directly, no device touched),
against the same arithmetic in NumPy in the same operation order.  A sanitizer build of host code: not a GPU test."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mppi_robotarm_amd import _native as N
from mppi_robotarm_amd.build import hipcc

K_SLOTS, PAD_KEY = 32, np.float32(1.0e30)   # mppi_device.h: kSlots, kPadKey
K_GROUP = 16                                # kGroup
TMO_LOCAL, TMO_EXCHANGE, TMO_SPLIT = 1, 2, 4


def circle_window(W, cx, cy, radius, dphi):
    phi = 0.3 + dphi * np.arange(W)
    return np.stack([cx + radius * np.cos(phi), cy + radius * np.sin(phi), -np.sin(phi), np.cos(phi)], axis=1)


def line_window(W):
    """Far from the origin, 1e-3 apart: the keys' c' = rx'^2 + ry'^2 is ~1e-6 centred and ~2e6 uncentred, below
    fp32's resolution of the distances it is added to."""
    j = np.arange(W, dtype=np.float64)
    return np.stack([1.0e3 + 1.0e-3 * j, 1.0e3 - 1.0e-3 * j, 0.1 * j, -0.2 * j], axis=1)


WINDOWS = {
    "w1": circle_window(1, 0.0, 0.0, 1.5, 0.01),
    "w7": circle_window(7, 0.0, 0.0, 1.5, 0.01),
    "w30": circle_window(N.MPPI_SEARCH_LEN, 0.0, 0.0, 1.5, 0.01),
    "far1": line_window(1),
    "far7": line_window(7),
    "far30": line_window(N.MPPI_SEARCH_LEN),
}
EXPLOIT = [(p, K) for K in (7, 1000, 65536) for p in (0.0, 1.0, 0.1, float(np.nextafter(1.0, 2.0)), 1.5)]
GAMMA = [(0.25, 50.0, 0.98), (0.0, 50.0, 0.98), (float("nan"), 50.0, 0.98), (float("nan"), 0.3, 0.1)]
GEOMETRY = [(16, 16, 0, True), (8, 16, 8, True), (0, 16, 0, False), (16, 8, 0, False), (8, 16, -1, False),
            (8, 16, 9, False), (2 ** 31 - 1, 2 ** 31 - 1, 1, False)]
TIMEOUT = [(0, 0), (TMO_LOCAL, 0), (0, TMO_EXCHANGE), (0, TMO_SPLIT), (TMO_LOCAL, TMO_SPLIT),
           (0, TMO_EXCHANGE | TMO_SPLIT)]
# nblocks, ncu, per_cu, stride, extra words: one workgroup per CU (poll), occupancy unknown, shared CUs
# (counter form with acquire), and the chain's ticket words behind the counters
HANDOFF = [(256, 256, 1, 130, 0), (256, 256, 0, 130, 0), (257, 256, 2, 130, 0), (1, 256, 1, 4, 0),
           (1024, 256, 2, 114, 2048), (100, 256, 1, 114, 2048)]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cc = hipcc()
    if shutil.which(cc) is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("host_plumbing") / "host_plumbing"
    subprocess.run([cc, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "mppi_robotarm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_plumbing_main.hip"), "-o", str(exe)], check=True)
    lines = [f"window {len(w)} " + " ".join(float(v).hex() for v in w.ravel()) for w in WINDOWS.values()]
    lines += [f"exploit {float(p).hex()} {K}" for p, K in EXPLOIT]
    lines += ["gamma " + " ".join("nan" if math.isnan(v) else float(v).hex() for v in g) for g in GAMMA]
    lines += [f"geometry {kl} {kt} {ko}" for kl, kt, ko, _ in GEOMETRY]
    lines += [f"timeout {a} {b}" for a, b in TIMEOUT]
    lines += ["handoff " + " ".join(str(v) for v in h) for h in HANDOFF]
    lines += ["owners"]
    env = {k: v for k, v in os.environ.items() if k != "MPPI_HANDOFF"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # owners: no device, wherever this runs
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out.setdefault(key, []).append(rest)
    return out


def stage_window_ref(window):
    """stage_window's arithmetic: fp64, x then y summed over j in order, rounded to fp32 last."""
    W = len(window)
    cx = cy = 0.0
    for j in range(W):
        cx += float(window[j, 0])
        cy += float(window[j, 1])
    cx /= W
    cy /= W
    win = np.zeros((K_SLOTS, 4), dtype=np.float32)
    key = np.zeros((K_SLOTS, 4), dtype=np.float32)
    key[:, 2] = PAD_KEY
    for j in range(W):
        rx, ry = float(window[j, 0]) - cx, float(window[j, 1]) - cy
        win[j] = window[j].astype(np.float32)
        key[j] = np.array([-2.0 * rx, -2.0 * ry, rx * rx + ry * ry, 0.0]).astype(np.float32)
    ctr = np.array([cx, cy, float(W), 0.0]).astype(np.float32)
    return win, key, ctr


def words(text):
    return np.array([int(t, 16) for t in text.split()], dtype=np.uint32)


@pytest.mark.parametrize("i,name", list(enumerate(WINDOWS)))
def test_stage_window_bits(results, i, name):
    window = WINDOWS[name]
    W = len(window)
    win, key, ctr = stage_window_ref(window)
    got_win, got_key = words(results["win"][i]).reshape(K_SLOTS, 4), words(results["key"][i]).reshape(K_SLOTS, 4)
    assert np.array_equal(got_win, win.view(np.uint32))
    assert np.array_equal(got_key, key.view(np.uint32))
    assert np.array_equal(words(results["ctr"][i]), ctr.view(np.uint32))
    pad = np.array([0.0, 0.0, PAD_KEY, 0.0], dtype=np.float32).view(np.uint32)
    assert (got_win[W:] == 0).all() and (got_key[W:] == pad).all()
    if name.startswith("far"):   # centring matters here: the uncentred c' would be ~2e6
        assert (got_key[:W, 2].view(np.float32) < 1.0e-3).all()


def test_exploit_count(results):
    got = [int(t) for t in results["exploit"]]
    for (p, K), g in zip(EXPLOIT, got):
        thr = (1.0 - p) * float(K)   # control.py:98
        assert g == (0 if thr <= 0.0 else min(math.ceil(thr), K)), (p, K)
    by_case = dict(zip(EXPLOIT, got))
    for K in (7, 1000, 65536):
        assert by_case[(0.0, K)] == K and by_case[(1.0, K)] == 0 and by_case[(EXPLOIT[3][0], K)] == 0
        assert by_case[(0.1, K)] == math.ceil((1.0 - 0.1) * K)


def test_gamma_resolution(results):
    for (g, lam, alpha), text in zip(GAMMA, results["gamma"]):
        want = lam * (1.0 - alpha) if math.isnan(g) else g   # control.py:45
        assert float.fromhex(text) == want and not math.isnan(want)


def test_sample_geometry(results):
    for (kl, kt, ko, ok), text in zip(GEOMETRY, results["geometry"]):
        assert int(text) == (N.MPPI_OK if ok else N.MPPI_E_ARG), (kl, kt, ko)


def test_timeout_verdicts(results):
    for (w0, w1), text in zip(TIMEOUT, results["timeout"]):
        rc, v, after0, after1, *msg = text.split(" ", 4)
        bits = w0 | w1
        assert int(v) == bits and (int(after0), int(after1)) == (0, 0)
        msg = msg[0] if msg else ""
        if bits == 0:
            assert int(rc) == N.MPPI_OK and msg == ""
        elif bits == TMO_EXCHANGE:
            assert int(rc) == N.MPPI_E_EXCHANGE and "no rank applied the update" in msg
        elif bits & TMO_SPLIT:
            assert int(rc) == N.MPPI_E_HIP and "cannot be re-run" in msg
        else:
            assert int(rc) == N.MPPI_E_HIP and "in-launch hand-off timed out" in msg


def test_handoff_sizes(results):
    for (nblocks, ncu, per_cu, stride, extra), text in zip(HANDOFF, results["handoff"]):
        poll, acquire, ngroups, slab, gslab, extra_off, ctr_bytes = (int(t) for t in text.split())
        assert poll == int(per_cu >= 1 and nblocks <= ncu)
        assert acquire == int(not poll and nblocks > ncu)
        assert ngroups == -(-nblocks // K_GROUP)
        val = 16 if poll else 8   # a tagged granule, or a plain fp64
        assert (slab, gslab) == (nblocks * stride * val, ngroups * stride * val)
        # the arrival counters and the epoch word fit below the extra words, which start 256-B aligned
        assert extra_off * 4 % 256 == 0 and 0 <= extra_off * 4 - (ngroups + 2) * 4 < 256
        assert ctr_bytes == (extra_off + extra) * 4


OWNERS = {"DevBuf.alloc": "hipMalloc", "DevBuf.alloc_zeroed": "hipMalloc", "DevBuf.reserve": "hipMalloc",
          "PinnedBuf.alloc": "hipHostMalloc", "MappedBuf.alloc": "hipHostMalloc",
          "Event.create": "hipEventCreateWithFlags", "Stream.create": "hipStreamCreateWithFlags",
          "Handoff.setup": "hipMalloc", "Exchange.handle": "hipSetDevice"}


def test_owners_without_device(results):
    """No device is visible: every member that allocates or creates fails with MPPI_E_HIP, its message names the
    HIP call (<failing HIP call>: <hipGetErrorString>), and the owner stays empty; reserve(0) has nothing to do.
    The double reset() and the destructors are the sanitizers' to judge (the fixture's exit status)."""
    got = {}
    for text in results["owners"]:
        name, rc, empty, *msg = text.split(" ", 3)
        got[name] = (int(rc), int(empty), msg[0] if msg else "")
    assert got.pop("DevBuf.reserve0") == (N.MPPI_OK, 1, "")
    assert set(got) == set(OWNERS)
    for name, call in OWNERS.items():
        rc, empty, msg = got[name]
        assert rc == N.MPPI_E_HIP and empty == 1, name
        expr, _, err = msg.rpartition(": ")
        assert expr.startswith(call + "(") and err, (name, msg)
