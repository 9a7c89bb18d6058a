"""CPU-side checks of GP leave-one-out cross-validation: the NumPy statement the GPU tests compare the device with (tests/_gp_loo_ref.py) against
brute-force leave-one-out and against central differences, and the entry points scasml_gp_gram_da_rows, scasml_gp_loo_da_doubles and scasml_gp_loo_da
(csrc/gp_loo.hip): declared in the header within ABI 7, bound, exported, their refusals come back as codes before anything is launched, their kernels
need no scratch memory."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _gp_loo_ref as ref
from scasml_gp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in ref.SHAPES if 4 * s[1] + s[2] <= 323]


@pytest.fixture(scope="module")
def lib():
    from scasml_gp_amd import _build
    _build.build_library()
    return _lib.load()


def _problem(d, nd, nb):
    dom, bdy = ref.points(d, nd, nb)
    og = ref.oracle(d)
    M = 4 * nd + nb
    Kp = og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64)) + ref.NUGGET * np.eye(M)
    return dom, bdy, float(np.sqrt(og.s2)), Kp, ref.z_of(d, M)


# LOO, dLOO/dlog sigma, dLOO/dlog eta at the oracle's default scale and eta = 1e-2, computed when the formulas were derived: they anchor the helper
ANCHORS = {(1, 1, 0): (-9.543502313152546, 3.7423115773, -0.0098724192), (3, 50, 20): (-7125.36725859203, -10805.106498, 6220.590821),
           (5, 70, 0): (-4509.89554202182, -2821.452782, 3787.809846), (31, 64, 1): (-2258.666148799772, -2982.180733, 670.5553916),
           (33, 65, 63): (-2423.1203085855377, -2979.211330, 694.8555137), (100, 130, 40): (-7053.078406908693, -7592.882027, 3125.920155)}


def test_shapes_with_at_most_323_features_are_the_five_expected():
    assert SMALL == [(1, 1, 0), (3, 50, 20), (5, 70, 0), (31, 64, 1), (33, 65, 63)]


@pytest.mark.parametrize("d,nd,nb", SMALL)
def test_closed_forms_match_brute_force_leave_one_out(d, nd, nb):
    """Row and column i of K_p deleted, the rest solved, z_i predicted -- for every i.  Both sides solve with matrices of condition <= cond(K_p), so
    they may differ by a few cond(K_p) 2^-53 of the largest value: asserted at cap = 256 cond 2^-53 (5.5e-13 of max |mean| and 1.3e-13 of max var
    were the largest found when the formulas were derived; the cap is about 1e-8)."""
    _, _, _, Kp, z = _problem(d, nd, nb)
    A, alpha = ref.inverse(Kp, z)
    vals, _ = ref.loo_values(A, alpha, z)
    mean, var = ref.brute_force(Kp, z)
    em = float(np.abs(vals["mean"] - mean).max() / np.abs(mean).max())
    ev = float(np.abs(vals["variance"] - var).max() / var.max())
    cap = ref.cap(float(np.linalg.cond(Kp)))
    print("(%d, %d, %d): closed forms against brute force, mean off by %.2e of max |mean|, variance by %.2e of max var; cap %.2e" % (d, nd, nb, em, ev, cap))
    assert em <= cap and ev <= cap
    assert np.all(var > 0.0)
    resid = (z - mean) / np.sqrt(var)
    assert np.abs(vals["residual"] - resid).max() <= cap * np.abs(resid).max()
    logp = -0.5 * np.log(2.0 * np.pi * var) - 0.5 * resid ** 2
    assert np.abs(vals["log_predictive"] - logp).max() <= cap * np.abs(logp).max()


@pytest.mark.parametrize("d,nd,nb", ref.SHAPES)
def test_gradient_formula_matches_central_differences_and_the_anchors(d, nd, nb):
    """dLOO/dlog sigma and dLOO/dlog eta against (LOO(x + h) - LOO(x - h)) / 2h at h = 1e-5: the quotient's truncation error is ~h^2 of the third
    derivative and its cancellation error ~cond 2^-53 |LOO| / h, together below 1e-6 of sum_i |t1_i| + |t2_i| here (1e-8 was the largest found)."""
    dom, bdy, sigma, _, z = _problem(d, nd, nb)
    value, _, grads, _ = ref.loo_and_grad(d, dom, bdy, sigma, ref.NUGGET, z)
    h = 1e-5
    fd = {"log_sigma": (ref.loo_value(d, dom, bdy, sigma * np.exp(h), ref.NUGGET, z) - ref.loo_value(d, dom, bdy, sigma * np.exp(-h), ref.NUGGET, z)) / (2 * h),
          "log_nugget": (ref.loo_value(d, dom, bdy, sigma, ref.NUGGET * np.exp(h), z) - ref.loo_value(d, dom, bdy, sigma, ref.NUGGET * np.exp(-h), z)) / (2 * h)}
    got = {k: float((t1 + t2).sum()) for k, (t1, t2) in grads.items()}
    for k in got:
        scale = float(np.abs(grads[k][0]).sum() + np.abs(grads[k][1]).sum())
        print("(%d, %d, %d): dLOO/d%s = %.10g, central difference %.10g, apart by %.2e of sum |terms|" % (d, nd, nb, k, got[k], fd[k], abs(got[k] - fd[k]) / scale))
        assert abs(got[k] - fd[k]) <= 1e-6 * scale
    v0, gs0, ge0 = ANCHORS[(d, nd, nb)]
    assert abs(value - v0) <= 1e-9 * abs(v0)
    assert abs(got["log_sigma"] - gs0) <= 1e-8 * abs(gs0) and abs(got["log_nugget"] - ge0) <= 1e-8 * abs(ge0)


def test_entry_points_are_declared_bound_and_exported_within_abi_7(lib):
    header = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"\bint scasml_gp_gram_da_rows\(int32_t d, double a, const float \*x_dom, int32_t n_dom, const float \*x_bdy, int32_t n_bdy,\s*"
                     r"int64_t row0,\s*int32_t nrows,\s*int64_t ncols, double \*out, int64_t ld, void \*stream\);", header)
    assert re.search(r"\bint64_t scasml_gp_loo_da_doubles\(int32_t n_dom, int32_t n_bdy, int32_t panel_rows\);", header)
    assert re.search(r"\bint scasml_gp_loo_da\(int32_t d, double a, const float \*x_dom, int32_t n_dom, const float \*x_bdy, int32_t n_bdy, "
                     r"const double \*A,\s*int64_t lda,\s*const double \*alpha, int32_t panel_rows, double \*q_out, double \*v_out, double \*work, "
                     r"void \*stream\);", header)
    assert len(re.findall(r"LOO: added within ABI 7 \(additive\)", header)) == 2
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", header) and lib.scasml_abi_version() == 7 and _lib.ABI_VERSION == 7
    rows_args = [C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    assert _lib.SIGNATURES["scasml_gp_gram_da_rows"] == (C.c_int, rows_args) == _lib.SIGNATURES["scasml_gp_gram_rows"]      # the twin
    assert _lib.SIGNATURES["scasml_gp_loo_da_doubles"] == (C.c_int64, [C.c_int32, C.c_int32, C.c_int32])
    assert _lib.SIGNATURES["scasml_gp_loo_da"] == (C.c_int, [C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    for name in ("scasml_gp_gram_da_rows", "scasml_gp_loo_da_doubles", "scasml_gp_loo_da"):
        assert hasattr(lib, name), name
    assert "gp_loo.hip" in __import__("scasml_gp_amd._build", fromlist=["SOURCES"]).SOURCES


def test_refusals_come_back_as_codes_without_a_gpu(lib):
    p8 = C.c_void_p(8)
    g = lib.scasml_gp_loo_da
    ok = dict(d=3, a=1.0, x_dom=p8, n_dom=50, x_bdy=p8, n_bdy=20, A=p8, lda=220, alpha=p8, panel_rows=64, q=p8, v=p8, work=p8)

    def call(**kw):
        v = dict(ok, **kw)
        return g(v["d"], v["a"], v["x_dom"], v["n_dom"], v["x_bdy"], v["n_bdy"], v["A"], v["lda"], v["alpha"], v["panel_rows"], v["q"], v["v"], v["work"], None)

    for name in ("x_dom", "x_bdy", "A", "alpha", "q", "v", "work"):
        assert call(**{name: None}) == -1 and b"gp_loo_da" in lib.scasml_last_error(), name                # null pointers
    assert call(d=0) == -1
    assert call(n_dom=0) == -1
    assert call(n_bdy=-1) == -1
    assert call(lda=219) == -1                                                                              # lda < M = 4 * 50 + 20
    assert call(panel_rows=-64) == -1 and call(panel_rows=96) == -1 and b"panel_rows" in lib.scasml_last_error()
    big = 65535 * 64 + 1                                                                                    # scasml_gp_gram's 65535 rule
    assert call(n_dom=big, n_bdy=0, lda=4 * big) == -2 and b"too many" in lib.scasml_last_error()
    # the workspace: (panel rows in use + column tiles) * M doubles; the panel is never taller than M rounded up to 64; 0 for what the entry refuses
    doubles = lib.scasml_gp_loo_da_doubles
    assert doubles(50, 20, 64) == (64 + 4) * 220 and doubles(50, 20, 128) == (128 + 4) * 220
    assert doubles(50, 20, 0) == doubles(50, 20, 256) == doubles(50, 20, 4096) == (256 + 4) * 220
    assert doubles(1000, 200, 0) == (512 + 66) * 4200
    assert doubles(0, 5, 64) == 0 and doubles(5, -1, 64) == 0 and doubles(50, 20, 65) == 0 and doubles(50, 20, -64) == 0
    r = lib.scasml_gp_gram_da_rows
    rows_ok = dict(d=20, a=0.8, x_dom=p8, n_dom=10, x_bdy=p8, n_bdy=2, row0=0, nrows=8, ncols=42, out=p8, ld=42)

    def rows(**kw):
        v = dict(rows_ok, **kw)
        return r(v["d"], v["a"], v["x_dom"], v["n_dom"], v["x_bdy"], v["n_bdy"], v["row0"], v["nrows"], v["ncols"], v["out"], v["ld"], None)

    for name in ("x_dom", "x_bdy", "out"):
        assert rows(**{name: None}) == -1 and b"gp_gram_da_rows" in lib.scasml_last_error(), name
    assert rows(d=0) == -1 and rows(n_dom=0) == -1 and rows(n_bdy=-1) == -1 and rows(row0=-1) == -1 and rows(nrows=-1) == -1
    assert rows(row0=40, nrows=8) == -1                                                                     # rows beyond M = 42
    assert rows(ncols=43, ld=43) == -1 and rows(ld=41) == -1
    assert rows(n_dom=big, n_bdy=0) == -2 and b"too many" in lib.scasml_last_error()
    assert rows(nrows=0) == 0 and rows(ncols=0, ld=0) == 0                                                  # nothing asked: nothing launched


def test_loo_kernels_use_no_scratch(tmp_path):
    """The K_a rows kernel holds a pair's 16 polynomials and 16 derivatives beside the accumulators (one instance per operator row, so that the
    table is never indexed at run time), the tile kernel 16 accumulators and 16 weights: all of it must stay in registers."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "gp_loo.hip"], capture_output=True, text=True, check=True,
                         env=dict(os.environ, KERNEL_REGS_OUT=str(tmp_path / "gp_loo.s"))).stdout
    for kernel, count in (("gp_gram_rows_kernel", 4), ("gp_loo_panel_gemv_kernel", 1), ("gp_loo_tile_kernel", 1), ("gp_loo_sum_kernel", 1)):
        lines = [l for l in out.splitlines() if kernel in l]
        assert len(lines) == count, out
        for line in lines:
            m = re.search(r"scratch\s+(\d+)\s+vgpr\s+(\d+)", line)
            assert m and int(m.group(1)) == 0 and int(m.group(2)) <= 512 and "!!" not in line, line
