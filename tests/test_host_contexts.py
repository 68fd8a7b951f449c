"""CPU: the four native contexts' constructors in a stand-alone host build under AddressSanitizer and UBSan
(tests/host_contexts_main.hip: its own main, run directly; the library's four units compiled whole, since a
host-only compile of them does not link).  No device is visible to the program, so every constructor fails in
its first HIP call and hands the half-built context to its members' destructors (csrc/mppi_host.h's owners): the
error code, the cleared *out, the message and a clean sanitizer exit, leak check included.  A sanitizer build of
host code: not a GPU test."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from mppi_robotarm_amd import _native as N
from mppi_robotarm_amd.build import SRCS, hipcc

SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}   # the same run on a machine that has one


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cc = hipcc()
    if shutil.which(cc) is None:
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("host_contexts")
    flags = ["--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "include"),
             "-Xarch_host", "-ffp-contract=off"] + SAN
    objs, procs = [], []
    for src in SRCS + [os.path.join(ROOT, "tests", "host_contexts_main.hip")]:
        objs.append(str(tmp / (os.path.splitext(os.path.basename(src))[0] + ".o")))
        procs.append(subprocess.Popen([cc] + flags + ["-c", "-o", objs[-1], src]))
    assert all(p.wait() == 0 for p in procs)
    exe = str(tmp / "host_contexts")
    subprocess.run([cc, "--offload-arch=gfx950"] + SAN + ["-o", exe] + objs, check=True)   # host link only
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "LSAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(env, **NO_DEVICE), timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return dict(line.split(" ", 1) for line in r.stdout.splitlines())


@pytest.mark.parametrize("name", ["arm", "chain", "np", "readback"])
def test_create_without_device(lines, name):
    rc, out_null, msg = lines[name].split(" ", 2)
    assert int(rc) == N.MPPI_E_HIP == -2
    assert int(out_null) == 1
    call, _, text = msg.partition(": ")   # <failing HIP call>: <hipGetErrorString>
    assert call.startswith("hip") and text
