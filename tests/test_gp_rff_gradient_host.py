"""CPU-side checks of the per-component gradients of the pathwise GP posterior draws.  The first three pin the NumPy statement the GPU tests compare
the device with (tests/_gp_rff_grad_ref.py): the prior gradient against central differences of _gp_rff_ref.functionals' u, its spatial sum and time
component against that statement's div and dt, and the alpha form of the data term against central differences of the oracle's cross rows.  The
rest: scasml_gp_rff_gradient (csrc/gp_rff_grad.hip) is declared within ABI 7, bound, refuses bad arguments with codes before anything is launched,
and its kernels use no scratch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _gp_rff_grad_ref as gref
import _gp_rff_ref as ref
from scasml_gp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# VGPRs of gp_rff_grad_kernel<NCT>, NCT = 1 .. 4 component tiles, as the build gives them (profiles/gp_rff_gradient_regs.txt)
VGPRS = {1: 252, 2: 272, 3: 304, 4: 342}


@pytest.fixture(scope="module")
def lib():
    from scasml_gp_amd import _build
    _build.build_library()
    return _lib.load()


@pytest.mark.parametrize("d", [1, 3])
def test_prior_gradient_is_the_derivative_of_u(d):
    """Central differences of _gp_rff_ref.functionals' u in np.longdouble at points that are float64 values: step h = 2^-20, truncation error
    h^2 / 6 |u'''| ~ 1e-13 of the derivative's scale, rounding error 2^-64 / h ~ 6e-14 of |u|; asserted at 1e-6 of the component's scale
    sum_f |omega_fk| (|wc_f| + |ws_f|) F^-1/2, as test_gp_rff_host.py does for dt and div."""
    a, F, seed, draw = 0.7, 40, 11, 3
    feats = ref.features(d, a, F, seed, draw)
    X = np.random.default_rng(d).uniform(-1, 1, (7, d + 1)).astype(np.float32).astype(np.float64)
    h = 2.0 ** -20                                                          # X +- h e_k are float64 values exactly
    u = lambda Y: ref.functionals(d, a, F, seed, draw, Y, feats)[:, 0]
    e = np.eye(d + 1)
    want = np.stack([(u(X + h * e[k]) - u(X - h * e[k])) / (2 * np.longdouble(h)) for k in range(d + 1)], axis=1)
    got = gref.prior_gradient(d, a, F, seed, draw, X, feats)
    scale = (np.abs(feats[0]) * (np.abs(feats[1]) + np.abs(feats[2]))[:, None]).sum(0) / np.sqrt(F)
    err = np.abs(got - want).max(0) / scale
    print("d=%d central differences, error / scale per component: %s" % (d, err.astype(np.float64)))
    assert got.shape == (7, d + 1) and (err <= 1e-6).all()


@pytest.mark.parametrize("d", [1, 3, 6])
def test_spatial_sum_is_div_and_last_component_is_dt(d):
    """To rounding: both statements sum in np.longdouble, in different orders -- within 4 F of their common unit, sum_f over |terms| times 2^-64."""
    a, F, seed, draw = 0.7, 40, 5, 2
    feats = ref.features(d, a, F, seed, draw)
    X = np.random.default_rng(10 + d).uniform(-1, 1, (9, d + 1)).astype(np.float32)
    grad = gref.prior_gradient(d, a, F, seed, draw, X, feats)
    fun = ref.functionals(d, a, F, seed, draw, X, feats)
    amp = (np.abs(feats[1]) + np.abs(feats[2]))[:, None] * np.abs(feats[0])                       # (F, d+1)
    tol = 4 * F * 2.0 ** -64 / np.sqrt(F)
    assert (np.abs(grad[:, d] - fun[:, 2]) <= tol * amp[:, d].sum()).all()
    assert (np.abs(grad[:, :d].sum(1) - fun[:, 3]) <= tol * amp[:, :d].sum()).all()


@pytest.mark.parametrize("d,nd,nb", [(3, 5, 4), (6, 4, 0)])
def test_alpha_form_is_the_derivative_of_the_cross_rows(d, nd, nb):
    """Central differences of the oracle's op-0 cross rows in float64, h = 2^-17: truncation h^2 / 6 |K0'''| ~ 1e-11 |K0'''|, rounding
    2^-53 |K0| / h ~ 1.5e-11 |K0|; with the third derivatives a few hundred times the entries, asserted at 1e-7 of the largest entry of the
    gradient rows."""
    from _gp_evidence_ref import oracle, points
    dom, bdy = points(d, nd, nb)
    og = oracle(d)
    og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64))
    X = np.random.default_rng(20 + d).uniform(0, 1, (6, d + 1)).astype(np.float32).astype(np.float64)
    h = 2.0 ** -17
    e = np.eye(d + 1)
    want = np.stack([(ref.cross_rows(og, X + h * e[k])[0] - ref.cross_rows(og, X - h * e[k])[0]) / (2 * h) for k in range(d + 1)], axis=1)
    got = gref.gradient_rows(og, X)
    assert got.shape == (6, d + 1, 4 * nd + nb)
    err = float(np.abs(got - want).max() / np.abs(got).max())
    print("(%d, %d, %d): alpha form against central differences %.2e of the largest entry %.3g" % (d, nd, nb, err, np.abs(got).max()))
    assert err <= 1e-7
    v = np.random.default_rng(3).standard_normal(4 * nd + nb)
    assert np.array_equal(gref.data_gradient(og, X, v), got @ v)


def test_entry_point_is_declared_bound_and_exported_within_abi_7(lib):
    header = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"\bint scasml_gp_rff_gradient\(int32_t d, double a, const float \*x, int64_t n, int64_t ld_x, int32_t F, uint64_t seed, "
                     r"int64_t sample0, int64_t S,\s*double \*out, int64_t ld_out, void \*stream\);", header)
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", header) and lib.scasml_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert _lib.SIGNATURES["scasml_gp_rff_gradient"] == (C.c_int, [C.c_int32, C.c_double, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_uint64,
                                                                   C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p])
    assert hasattr(lib, "scasml_gp_rff_gradient")
    assert "gp_rff_grad.hip" in __import__("scasml_gp_amd._build", fromlist=["SOURCES"]).SOURCES


def test_refusals_come_back_as_codes_without_a_gpu(lib):
    p8 = C.c_void_p(8)
    ok = dict(d=3, a=0.5, x=p8, n=10, ld_x=4, F=64, seed=1, sample0=0, S=2, out=p8, ld_out=4)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.scasml_gp_rff_gradient(v["d"], v["a"], v["x"], v["n"], v["ld_x"], v["F"], v["seed"], v["sample0"], v["S"], v["out"], v["ld_out"], None)

    for name in ("x", "out"):
        assert call(**{name: None}) == -1 and b"gp_rff_gradient" in lib.scasml_last_error(), name
    assert call(d=0) == -1 and call(d=_lib.MAX_DIM + 1, ld_x=_lib.MAX_DIM + 2, ld_out=_lib.MAX_DIM + 2) == -1
    assert call(a=0.0) == -1 and call(a=float("nan")) == -1
    assert call(F=0) == -1 and b"F=0" in lib.scasml_last_error()
    assert call(ld_x=3) == -1
    assert call(ld_out=3) == -1 and b"ld_out=3" in lib.scasml_last_error()
    assert call(n=-1) == -1 and call(S=-1) == -1 and call(sample0=-1) == -1
    assert call(sample0=2 ** 32 - 1, S=2) == -2 and b"2^32" in lib.scasml_last_error()
    assert call(sample0=2 ** 32, S=1) == -2
    # the order of scasml_gp_rff_functionals: null, d, a, F, the leading dimensions, the draws -- each refusal names what it met first
    assert call(x=None, d=0) == -1 and b"null" in lib.scasml_last_error()
    assert call(d=0, a=0.0) == -1 and b"d=0" in lib.scasml_last_error()
    assert call(a=0.0, F=0) == -1 and b"a=0" in lib.scasml_last_error()
    assert call(F=0, ld_out=3) == -1 and b"F=0" in lib.scasml_last_error()
    assert call(ld_out=3, sample0=2 ** 32, S=1) == -1 and b"ld_out=3" in lib.scasml_last_error()
    assert call(n=0, sample0=2 ** 32, S=1) == -2                                # a refusal comes before the empty call
    assert call(n=0) == 0 and call(S=0) == 0                                   # nothing asked: nothing launched


def test_gradient_kernels_use_no_scratch(tmp_path):
    """Every instantiation holds 16 theta accumulators, 16 per component tile of G and the two operand stages in registers through an epilogue of 16
    double sincos: all of it must stay in registers, and the counts are pinned at what the build gives."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "gp_rff_grad.hip"], capture_output=True, text=True, check=True,
                         env=dict(os.environ, KERNEL_REGS_OUT=str(tmp_path / "gp_rff_grad.s"))).stdout
    for nct, vgprs in VGPRS.items():
        lines = [l for l in out.splitlines() if "gp_rff_grad_kernel<%d>" % nct in l]
        assert len(lines) == 1, out
        m = re.search(r"scratch\s+(\d+)\s+vgpr\s+(\d+)\s+lds\s+\d+\s+spill\s+(\d+)", lines[0])
        assert m and int(m.group(1)) == 0 and int(m.group(3)) == 0 and "!!" not in lines[0], lines[0]
        assert int(m.group(2)) == vgprs, lines[0]
    asm = open(str(tmp_path / "gp_rff_grad.s")).read()
    assert "v_mfma_f64_16x16x4" in asm and "atomic" not in asm
