"""CPU-side checks of the joint-posterior sampling entry point scasml_gp_sample: declared in the header within ABI 7, bound with the declared argument
types, built from its own translation unit, its argument errors come back as codes (with a text) before anything is launched, and its kernel needs
no scratch memory."""
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
    assert re.search(r"\bint scasml_gp_sample\(const double \*Lc, int64_t np, int64_t n, const double \*mean, uint64_t seed, int64_t sample0, int64_t S,\s*"
                     r"double \*out,\s*int64_t ld_out, void \*stream\);", header)
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", header) and lib.scasml_abi_version() == 7 and _lib.ABI_VERSION == 7
    res, args = _lib.SIGNATURES["scasml_gp_sample"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    assert hasattr(lib, "scasml_gp_sample")
    from scasml_gp_amd import _build
    assert "gp_sample.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "gp_sample.hip"))


def test_the_reserved_stream_id_is_stated_once_and_bound():
    header = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    m = re.search(r"#define SCASML_STREAM_GP_SAMPLE (0x[0-9A-Fa-f]+)u\b", header)
    assert m and int(m.group(1), 16) == _lib.STREAM_GP_SAMPLE
    assert _lib.STREAM_GP_SAMPLE >= 1 << 30               # the solvers count their streams from 0, one per call
    assert "SCASML_STREAM_GP_SAMPLE" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_argument_errors_come_back_as_codes_without_a_gpu(lib):
    p8 = C.c_void_p(8)
    f = lib.scasml_gp_sample

    def refused(code, *args):
        lib.scasml_gp_variance(None, 64, p8, 64, 4, 1.0, p8, None)     # leaves another entry point's text behind
        assert b"gp_sample" not in lib.scasml_last_error()
        return f(*args) == code and b"gp_sample" in lib.scasml_last_error()

    #               Lc   np  n  mean seed sample0 S  out ld  stream
    assert refused(-1, None, 64, 4, p8, 1, 0, 2, p8, 4, None)          # null factor
    assert refused(-1, p8, 64, 4, None, 1, 0, 2, p8, 4, None)          # null mean
    assert refused(-1, p8, 64, 4, p8, 1, 0, 2, None, 4, None)          # null output
    assert refused(-1, p8, 64, 0, p8, 1, 0, 2, p8, 4, None)            # n < 1
    assert refused(-1, p8, 64, 65, p8, 1, 0, 2, p8, 65, None)          # n > np
    assert refused(-1, p8, 64, 4, p8, 1, 0, 2, p8, 3, None)            # ld_out < n
    assert refused(-1, p8, 64, 4, p8, 1, 0, -1, p8, 4, None)           # S < 0
    assert refused(-2, p8, 48, 4, p8, 1, 0, 2, p8, 4, None) and b"multiple of 32" in lib.scasml_last_error()
    assert refused(-2, p8, 64, 4, p8, 1, (1 << 32) - 1, 2, p8, 4, None) and b"2^32" in lib.scasml_last_error()   # the second draw's index is 2^32
    assert refused(-2, p8, 64, 4, p8, 1, 1 << 32, 1, p8, 4, None)
    assert refused(-2, p8, 64, 4, p8, 1, 0, (1 << 32) + 1, p8, 4, None)
    assert f(p8, 64, 4, p8, 1, 0, 0, p8, 4, None) == 0                 # no samples: nothing to do, nothing launched
    assert f(p8, 64, 4, p8, 1, (1 << 32) - 1, 0, p8, 4, None) == 0


def test_sampling_kernel_uses_no_scratch_and_two_workgroups_fit_a_cu():
    """256 threads = one wave per SIMD; two workgroups per CU (the LDS is sized for it) need <= 256 registers per lane."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "gp_sample.hip"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.splitlines() if "gp_sample_kernel" in l]
    assert len(lines) == 1, out
    m = re.search(r"scratch\s+(\d+)\s+vgpr\s+(\d+)", lines[0])
    assert m and int(m.group(1)) == 0 and int(m.group(2)) <= 256 and "!!" not in lines[0], lines[0]


def test_the_gp_class_has_the_joint_posterior_surface():
    from scasml_gp_amd.models.GP import GP
    for name in ("predict_covariance", "sample_posterior"):
        assert callable(getattr(GP, name))
