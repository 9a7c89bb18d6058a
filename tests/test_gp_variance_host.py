"""CPU-side checks of the GP posterior-variance entry point scasml_gp_variance: declared in the header within ABI 7, bound, its argument errors come
back as codes before anything is launched, and its kernel needs no scratch memory."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from scasml_gp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from scasml_gp_amd import _build
    _build.build_library()
    return _lib.load()


def test_entry_point_is_declared_bound_and_exported_within_abi_7(lib):
    header = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"\bint scasml_gp_variance\(const double \*L, int64_t Mp, double \*rows, int64_t ld, int64_t n, double prior,\s*double \*var_out, void \*stream\);", header)
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", header) and lib.scasml_abi_version() == 7
    res, args = _lib.SIGNATURES["scasml_gp_variance"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_void_p]
    assert hasattr(lib, "scasml_gp_variance")
    assert "gp_variance.hip" in __import__("scasml_gp_amd._build", fromlist=["SOURCES"]).SOURCES


def test_argument_errors_come_back_as_codes_without_a_gpu(lib):
    p8 = C.c_void_p(8)
    f = lib.scasml_gp_variance
    assert f(None, 64, p8, 64, 4, 1.0, p8, None) == -1 and b"gp_variance" in lib.scasml_last_error()      # null factor
    assert f(p8, 64, None, 64, 4, 1.0, p8, None) == -1                                                     # null rows
    assert f(p8, 64, p8, 64, 4, 1.0, None, None) == -1                                                     # null output
    assert f(p8, 0, p8, 64, 4, 1.0, p8, None) == -1                                                        # no columns
    assert f(p8, 64, p8, 63, 4, 1.0, p8, None) == -1                                                       # ld < Mp
    assert f(p8, 64, p8, 64, -1, 1.0, p8, None) == -1                                                      # negative n
    assert f(p8, 48, p8, 64, 4, 1.0, p8, None) == -2 and b"multiple of 32" in lib.scasml_last_error()      # Mp % 32 != 0
    assert f(p8, 64, p8, 64, 0, 1.0, p8, None) == 0                                                        # no points: nothing to do


def test_variance_kernel_uses_no_scratch():
    """One 256-thread workgroup is one wave per SIMD: up to 512 registers per lane; the point row of the triangular solve, the accumulators and the
    staged operands must all stay in them (tools/kernel_regs.py reads the code object's metadata)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "gp_variance.hip"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.splitlines() if "gp_variance_kernel" in l]
    assert len(lines) == 1, out
    m = re.search(r"scratch\s+(\d+)\s+vgpr\s+(\d+)", lines[0])
    assert m and int(m.group(1)) == 0 and int(m.group(2)) <= 512 and "!!" not in lines[0], lines[0]
