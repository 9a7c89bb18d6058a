"""CPU-side checks of the GP evidence entry points scasml_chol_logdet and scasml_gp_gram_da_contract (csrc/gp_evidence.hip): declared in the header
within ABI 7, bound, their refusals come back as codes before anything is launched, their kernels need no scratch memory.  Also pins the NumPy
K_a = dK/da the GPU tests compare the device with (tests/_gp_evidence_ref.py) against central differences of the oracle's Gram, and the host
optimiser of GP.optimize_hyperparameters on the NumPy statement of the likelihood."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _gp_evidence_ref as ref
from scasml_gp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from scasml_gp_amd import _build
    _build.build_library()
    return _lib.load()


def test_entry_points_are_declared_bound_and_exported_within_abi_7(lib):
    header = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"\bint scasml_chol_logdet\(const double \*L, int64_t Mp, double \*out_dev, void \*stream\);", header)
    assert re.search(r"\bint scasml_gp_gram_da_contract\(int32_t d, double a, const float \*x_dom, int32_t n_dom, const float \*x_bdy, int32_t n_bdy, "
                     r"const double \*A,\s*int64_t lda,\s*const double \*alpha, double \*out_dev, void \*stream\);", header)
    assert re.search(r"\bint64_t scasml_gp_gram_da_contract_doubles\(int32_t n_dom, int32_t n_bdy\);", header)
    assert len(re.findall(r"Added within ABI 7 \(additive\)\.  The (?:device pieces|two contractions)", header)) == 2
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", header) and lib.scasml_abi_version() == 7
    res, args = _lib.SIGNATURES["scasml_chol_logdet"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    res, args = _lib.SIGNATURES["scasml_gp_gram_da_contract"]
    assert res is C.c_int and args == [C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
    assert hasattr(lib, "scasml_chol_logdet") and hasattr(lib, "scasml_gp_gram_da_contract")
    assert "gp_evidence.hip" in __import__("scasml_gp_amd._build", fromlist=["SOURCES"]).SOURCES


def test_refusals_come_back_as_codes_without_a_gpu(lib):
    p8 = C.c_void_p(8)
    f = lib.scasml_chol_logdet
    assert f(None, 32, p8, None) == -1 and b"chol_logdet" in lib.scasml_last_error()                       # null factor
    assert f(p8, 32, None, None) == -1                                                                      # null output
    assert f(p8, 0, p8, None) == -1                                                                         # no rows
    g = lib.scasml_gp_gram_da_contract
    ok = dict(d=3, a=1.0, x_dom=p8, n_dom=50, x_bdy=p8, n_bdy=20, A=p8, lda=220, alpha=p8, out=p8)

    def call(**kw):
        v = dict(ok, **kw)
        return g(v["d"], v["a"], v["x_dom"], v["n_dom"], v["x_bdy"], v["n_bdy"], v["A"], v["lda"], v["alpha"], v["out"], None)

    for name in ("x_dom", "x_bdy", "A", "alpha", "out"):
        assert call(**{name: None}) == -1 and b"gp_gram_da_contract" in lib.scasml_last_error(), name     # null pointers
    assert call(d=0) == -1
    assert call(n_dom=0) == -1
    assert call(n_bdy=-1) == -1
    assert call(lda=219) == -1                                                                              # lda < M = 4 * 50 + 20
    # more pair tiles per side than one launch takes (scasml_gp_gram's 65535 rule)
    assert call(n_dom=65535 * 64 + 1, n_bdy=0, lda=4 * (65535 * 64 + 1)) == -2 and b"too many" in lib.scasml_last_error()
    assert lib.scasml_gp_gram_da_contract_doubles(50, 20) == 2 + 2 * 3 and lib.scasml_gp_gram_da_contract_doubles(64, 0) == 4
    assert lib.scasml_gp_gram_da_contract_doubles(0, 5) == 0


def test_evidence_kernels_use_no_scratch(tmp_path):
    """The epilogue holds the 16 polynomials and their 16 derivatives of a pair beside the accumulators: all of it must stay in registers."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "gp_evidence.hip"], capture_output=True, text=True, check=True,
                         env=dict(os.environ, KERNEL_REGS_OUT=str(tmp_path / "gp_evidence.s"))).stdout
    for kernel in ("chol_logdet_kernel", "gp_gram_da_contract_kernel", "gp_evidence_sum_kernel"):
        lines = [l for l in out.splitlines() if kernel in l]
        assert len(lines) == 1, out
        m = re.search(r"scratch\s+(\d+)\s+vgpr\s+(\d+)", lines[0])
        assert m and int(m.group(1)) == 0 and int(m.group(2)) <= 512 and "!!" not in lines[0], lines[0]


@pytest.mark.parametrize("d,nd,nb", [(3, 50, 20), (5, 70, 0), (31, 64, 1), (33, 65, 63)])
def test_numpy_gram_derivative_matches_central_differences(d, nd, nb):
    """The K_a table against (K(a + h) - K(a - h)) / 2h of OracleGP.kernel_phi_phi at h = 1e-5 a: within 1e-9 of the largest entry (1.6e-11 was
    measured; the difference quotient's own truncation and cancellation errors are ~1e-11 there)."""
    dom, bdy = ref.points(d, nd, nb)
    og = ref.oracle(d)
    a = og.a
    Ka = ref.gram_da(og, dom, bdy)
    assert Ka.shape == (4 * nd + nb, 4 * nd + nb) and np.array_equal(Ka, Ka.T)
    h = 1e-5 * a
    hi, lo = ref.oracle(d), ref.oracle(d)
    hi.a, lo.a = a + h, a - h
    fd = (hi.kernel_phi_phi(dom, bdy) - lo.kernel_phi_phi(dom, bdy)) / (2 * h)
    gap = float(np.abs(Ka - fd).max() / np.abs(Ka).max())
    print("d=%d nd=%d nb=%d: K_a against central differences, largest gap / largest entry = %.3e" % (d, nd, nb, gap))
    assert gap <= 1e-9


def test_bounded_bfgs_finds_the_numpy_likelihoods_maximum():
    """GP.optimize_hyperparameters' host iteration on the NumPy statement, the GPU test's problem: (3, 50, 20), z drawn from the prior at the
    library defaults, start at (2 sigma*, 10 eta*).  It must converge inside the default bounds within the default 50 iterations."""
    from scasml_gp_amd.models.GP import _maximize_bounded
    d, nd, nb = 3, 50, 20
    dom, bdy = ref.points(d, nd, nb)
    og = ref.oracle(d)
    s_true, e_true, M = float(np.sqrt(og.s2)), 1e-2, 4 * nd + nb
    K = og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64))
    z = np.linalg.cholesky(K + e_true * np.eye(M)) @ np.random.default_rng(7).standard_normal(M)

    def fun(x):
        value, _, grads, _ = ref.lml_and_grad(d, dom, bdy, float(np.exp(x[0])), float(np.exp(x[1])), z)
        return value, np.array([sum(grads["log_sigma"]), sum(grads["log_nugget"])])

    x0 = np.log([2 * s_true, 10 * e_true])
    lo, hi = np.log([2 * s_true / 8, 1e-6]), np.log([2 * s_true * 8, 1.0])
    x, value, grad, evals, iters, converged = _maximize_bounded(fun, x0, lo, hi, 1e-4 * M, 50)
    print("maximum at sigma = %.4f sigma*, nugget = %.4f eta*: LML %.3f (truth %.3f, start %.3f), |grad| %.2e, %d evaluations, %d iterations" % (
        np.exp(x[0]) / s_true, np.exp(x[1]) / e_true, value, fun(np.log([s_true, e_true]))[0], fun(x0)[0], np.abs(grad).max(), evals, iters))
    assert converged and iters <= 50 and np.abs(grad).max() <= 1e-4 * M
    assert np.all(x > lo) and np.all(x < hi)
    assert value >= fun(np.log([s_true, e_true]))[0] and value >= fun(x0)[0]
    # the held variable stays put, a bound that cuts the maximum off ends the search ON it
    x1, _, _, _, _, conv1 = _maximize_bounded(lambda v: (fun(np.array([v[0], x0[1]]))[0], fun(np.array([v[0], x0[1]]))[1][:1]), x0[:1], lo[:1], hi[:1], 1e-4 * M, 50)
    assert conv1 and lo[0] < x1[0] < hi[0]
    xb, _, gb, _, _, convb = _maximize_bounded(fun, x0, np.log([1.5 * s_true, 1e-6]), hi, 1e-4 * M, 50)
    assert convb and xb[0] == np.log(1.5 * s_true) and gb[0] < 0.0
