"""Host side of the Picard standard errors of u and z (scasml_picard_tree_stderr_uz): the header and the binding declare the entry, the ABI
version stays 7, both new translation units (csrc/picard_tree_stderr_uz.hip, csrc/picard_tree_stderr_uz_deep.hip) are built, and their
kernels -- picard_se_uz_kernel<VAR, MODE, N, EQ>, the walker of picard_tree_kernel under its SEZ flag -- are exactly the expected set and
stay inside the scratch and loop figures of the plain instances, as tests/test_picard_stderr_host.py asks of the u-only kernels.  VGPR counts
are printed, not bounded (profiles/picard_stderr_uz_regs.txt records them).  Needs hipcc ($HIPCC or /opt/rocm)."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE_MLP, MODE_ACCUMULATE = 0, 2
UNITS = ("picard_tree_stderr_uz.hip", "picard_tree_stderr_uz_deep.hip")


def _plain_scratch(var, mode, n, eq):
    """Scratch bytes of picard_tree_kernel<var, mode, n, eq> without a flag, n <= 4 (profiles/picard_stderr_regs.txt)."""
    return 36 if (var == 0 and mode == MODE_MLP and n == 4) else 0


def test_header_declares_the_entry_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", text)
    m = re.search(r"int scasml_picard_tree_stderr_uz\(([^;]*)\);", text)
    assert m, "include/scasml_hip.h does not declare scasml_picard_tree_stderr_uz"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["prob_h", "plan_h", "mode", "x_t", "B", "site_stride", "rng", "points", "gp_vals", "out_uz", "out_uhat", "out_se_uz", "stream"]
    assert "float *out_se_uz" in args
    # the argument list of scasml_picard_tree_stderr with its last output replaced
    u_only = re.search(r"int scasml_picard_tree_stderr\(([^;]*)\);", text)
    assert [a.strip() for a in " ".join(u_only.group(1).split()).split(",")] == [a.replace("out_se_uz", "out_se") for a in args]


def test_binding_declares_the_entry_as_the_plain_one_plus_an_output():
    import ctypes as C
    from scasml_gp_amd import _lib
    assert _lib.ABI_VERSION == 7
    res, args = _lib.SIGNATURES["scasml_picard_tree_stderr_uz"]
    plain_res, plain_args = _lib.SIGNATURES["scasml_picard_tree"]
    assert res is plain_res and args == plain_args[:-1] + [C.c_void_p] + plain_args[-1:]
    assert (res, args) == _lib.SIGNATURES["scasml_picard_tree_stderr"]


def test_sources_of_the_build_hold_the_new_translation_units():
    from scasml_gp_amd import _build
    for name in UNITS:
        assert name in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, name))


def test_uz_mode_is_refused_without_a_gpu_where_the_u_only_mode_is():
    """stderr_supported is the one rule of both modes: a plan it refuses raises before anything touches the device or a counter."""
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    solver = MLP(Grad_Dependent_Nonlinear(21))
    assert solver._engine.stderr_supported(2, 2)[0] is False and solver._engine.stderr_supported(3, 3)[0] is True


def _kernel_regs(source, tmp):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), source], capture_output=True, text=True, check=True,
                          env=dict(os.environ, KERNEL_REGS_OUT=os.path.join(tmp, source.replace(".hip", ".s")))).stdout


def test_uz_instances_are_the_expected_set_inside_the_plain_scratch_and_loop_figures():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=2) as ex:
        out = "".join(ex.map(lambda src: _kernel_regs(src, tmp), UNITS))
    seen = {}
    for line in out.splitlines():
        m = re.search(r"picard_se_uz_kernel<(\d+), (\d+), (\d+), (\d+)>.*scratch\s+(\d+)\s+vgpr\s+(\d+)", line)
        if not m:
            assert "_kernel" not in line, "a kernel of another template in a translation unit of the (u, z) standard errors: " + line
            continue
        var, mode, n, eq, scratch, vgpr = (int(g) for g in m.groups())
        seen[(var, mode, n, eq)] = (scratch, vgpr, "!!" in line)
        if n <= 4:
            assert scratch <= _plain_scratch(var, mode, n, eq), line
            assert "!!" not in line, "scratch traffic inside a loop where the plain instance has none: " + line
        assert vgpr <= 512, line
    # VAR 0/1 x {MLP, ACCUMULATE} x N = 1..5 x equations 0 and 1, and equation 2 (f of |z|^2) in MLP only
    want = [(var, mode, n, eq) for var in (0, 1) for mode in (MODE_MLP, MODE_ACCUMULATE) for n in range(1, 6) for eq in (0, 1)]
    want += [(var, MODE_MLP, n, 2) for var in (0, 1) for n in range(1, 6)]
    assert sorted(seen) == sorted(want)
    # the full-history instances of n = 5 do not spill without the flag (0 bytes) and must not with it
    assert all(seen[key][0] == 0 and not seen[key][2] for key in want if key[0] == 1 and key[2] == 5)
    for key in sorted(seen):
        print("picard_se_uz_kernel<%d, %d, %d, %d> scratch %d vgpr %d%s" % (key + seen[key][:2] + (" (scratch inside loops)" if seen[key][2] else "",)))
