"""CPU: the C-ABI library loads and exports every entry point include/mppi_rocm.h
declares, and the ctypes mirror of the config structs matches the C layout
(checked against a gcc-compiled probe of the header).  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mppi_rocm.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mppi_[a-z_]+)\s*\(", text)))


def test_header_declares_the_python_export_list():
    from mppi_robotarm_amd import _native
    assert declared_functions() == sorted(_native.EXPORTS)


def test_library_loads_and_exports_every_symbol():
    from mppi_robotarm_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        from mppi_robotarm_amd.build import build_native
        build_native()
    lib = _native.load()
    for name in declared_functions():
        assert hasattr(lib, name), name
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (mppi_\w+)", nm))
    assert set(declared_functions()) <= exported


def test_engine_base_dispatch_names_exist_under_both_prefixes():
    """Every call engine._Engine resolves from prefix + name is exported, with a signature, by the 2-link
    ABI (mppi_<name>) and by the chain's (mppi_chain_<name>): a typo in the table fails here, without a GPU."""
    from mppi_robotarm_amd import _native
    from mppi_robotarm_amd.engine import _Engine
    if not os.path.exists(_native.LIB_PATH):
        from mppi_robotarm_amd.build import build_native
        build_native()
    lib = _native.open_library(_native.LIB_PATH)
    assert len(_Engine.CALLS) == len(set(_Engine.CALLS)) >= 15
    for name in _Engine.CALLS:
        for prefix in ("mppi_", "mppi_chain_"):
            assert prefix + name in _native.EXPORTS, prefix + name
            assert getattr(lib, prefix + name).argtypes is not None, prefix + name


def test_struct_layout_matches_header(tmp_path):
    from mppi_robotarm_amd import _native as N
    probe = tmp_path / "probe.c"
    probe.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "mppi_rocm.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mppi_config), sizeof(mppi_arm_params),
         offsetof(mppi_config, delta_t), offsetof(mppi_config, sigma), offsetof(mppi_config, stage_cost_weight),
         offsetof(mppi_config, terminal_cost_weight), offsetof(mppi_config, arm),
         offsetof(mppi_config, lanes_per_sample), offsetof(mppi_config, param_gamma));
  return 0;
}
''')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(probe), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Cc = N.ConfigC
    assert vals == [C.sizeof(Cc), C.sizeof(N.ArmParamsC), Cc.delta_t.offset, Cc.sigma.offset,
                    Cc.stage_cost_weight.offset, Cc.terminal_cost_weight.offset, Cc.arm.offset,
                    Cc.lanes_per_sample.offset, Cc.param_gamma.offset]


def test_chain_struct_layout_matches_header(tmp_path):
    from mppi_robotarm_amd import _native as N
    probe = tmp_path / "probe.c"
    probe.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "mppi_rocm.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(mppi_chain_config), sizeof(mppi_chain_params),
         offsetof(mppi_chain_config, delta_t), offsetof(mppi_chain_config, sigma),
         offsetof(mppi_chain_config, stage_cost_weight), offsetof(mppi_chain_config, terminal_cost_weight),
         offsetof(mppi_chain_config, chain), offsetof(mppi_chain_params, m), offsetof(mppi_chain_params, fk),
         offsetof(mppi_chain_params, g), offsetof(mppi_chain_config, precision), MPPI_CHAIN_MAX_DOF);
  return 0;
}
''')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(probe), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Cc, Pc = N.ChainConfigC, N.ChainParamsC
    assert vals == [C.sizeof(Cc), C.sizeof(Pc), Cc.delta_t.offset, Cc.sigma.offset, Cc.stage_cost_weight.offset,
                    Cc.terminal_cost_weight.offset, Cc.chain.offset, Pc.m.offset, Pc.fk.offset, Pc.g.offset,
                    Cc.precision.offset, N.CHAIN_MAX_DOF]


@pytest.mark.parametrize("cname,pyname", [("mppi_dropin_binding", "DropinBindingC"), ("mppi_np_state", "NpStateC"),
                                          ("mppi_np_target", "NpTargetC")])
def test_struct_layout_matches_header(tmp_path, cname, pyname):
    from mppi_robotarm_amd import _native as N
    probe = tmp_path / f"probe_{cname}.c"
    B = getattr(N, pyname)
    fields = [f for f, _ in B._fields_]
    probe.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"mppi_rocm.h\"\nint main(void) {\n"
                     + "".join(f'  printf("%zu ", offsetof({cname}, {f}));\n' for f in fields)
                     + f'  printf("%zu\\n", sizeof({cname}));\n  return 0;\n}}\n')
    exe = tmp_path / f"probe_{cname}"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(probe), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == [getattr(B, f).offset for f in fields] + [C.sizeof(B)]


def test_constants_match_header():
    from mppi_robotarm_amd import _native as N
    text = open(HEADER).read()
    for name in ("MPPI_MAX_T", "MPPI_SEARCH_LEN", "MPPI_OK", "MPPI_E_ARG", "MPPI_E_HIP", "MPPI_E_SINGULAR",
                 "MPPI_E_PATH_END"):
        m = re.search(rf"#define {name}\s+(-?\d+)", text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert re.search(r"#define MPPI_FLAG_FUSED_UPDATE\s+1u", text) and N.MPPI_FLAG_FUSED_UPDATE == 1


def test_config_init_defaults():
    """mppi_config_init / mppi_chain_config_init (host-only calls): a C caller that starts from them gets
    gamma = lambda (1 - alpha) (the NaN sentinel, control.py:45) and sys_params.py's arm, not the gamma = 0 of
    a memset / `= {0}` config."""
    import math
    from mppi_robotarm_amd import _native as N
    from mppi_robotarm_amd.params import ArmParams
    lib = N.load()
    cfg = N.ConfigC(param_gamma=1.0)
    cfg.K_local, cfg.delta_t, cfg.sigma[3] = 7, 0.5, 2.0
    lib.mppi_config_init(C.byref(cfg))
    assert math.isnan(cfg.param_gamma)
    assert [getattr(cfg.arm, f) for f, _ in N.ArmParamsC._fields_] == [
        getattr(ArmParams(), f) for f, _ in N.ArmParamsC._fields_]
    assert (cfg.K_local, cfg.T, cfg.delta_t, cfg.lanes_per_sample, list(cfg.sigma)) == (0, 0, 0.0, 0, [0.0] * 4)
    ch = N.ChainConfigC(param_gamma=1.0)
    ch.precision, ch.chain.n = 1, 7
    lib.mppi_chain_config_init(C.byref(ch))
    assert math.isnan(ch.param_gamma) and ch.chain.g == 9.81
    assert (ch.precision, ch.chain.n, ch.lanes_per_sample, ch.chain.m[0]) == (0, 0, 0, 0.0)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No silent fallback: a missing .so raises at load time."""
    from mppi_robotarm_amd import _native as N
    monkeypatch.setattr(N, "_lib", None)
    monkeypatch.setattr(N, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(OSError):
        N.load()
