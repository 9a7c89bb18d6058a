"""CPU-side checks of scasml_gp_functional_covariance (csrc/gp_functional_cov.hip): declared in the header within ABI 7, bound, listed in the build,
its argument errors come back as codes before anything is launched, its kernel is one kernel without scratch, and the prior block the class hands it
is the oracle's Gram table at x = y."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _gp_functional_cov_ref as ref
from scasml_gp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from scasml_gp_amd import _build
    _build.build_library()
    return _lib.load()


def test_entry_point_is_declared_bound_and_exported_within_abi_7(lib):
    header = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"\bint scasml_gp_functional_covariance\(const double \*L, int64_t Mp, double \*rows, int64_t ld, int64_t n_points,\s*"
                     r"const double \*prior_h,\s*double \*cov_out,\s*void \*stream\);", header)
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", header) and lib.scasml_abi_version() == 7
    res, args = _lib.SIGNATURES["scasml_gp_functional_covariance"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    assert hasattr(lib, "scasml_gp_functional_covariance")
    sources = __import__("scasml_gp_amd._build", fromlist=["SOURCES"]).SOURCES
    assert sources[-1] == "gp_functional_cov.hip" and "gp_variance.hip" in sources
    assert os.path.exists(os.path.join(ROOT, "scasml_gp_amd", "csrc", "gp_variance_tile.hpp"))


def test_argument_errors_come_back_as_codes_without_a_gpu(lib):
    p8 = C.c_void_p(8)
    f = lib.scasml_gp_functional_covariance
    assert f(None, 64, p8, 64, 4, p8, p8, None) == -1 and b"gp_functional_covariance" in lib.scasml_last_error()   # null factor
    assert f(p8, 64, None, 64, 4, p8, p8, None) == -1                                                               # null rows
    assert f(p8, 64, p8, 64, 4, None, p8, None) == -1                                                               # null prior
    assert f(p8, 64, p8, 64, 4, p8, None, None) == -1                                                               # null output
    assert f(p8, 0, p8, 64, 4, p8, p8, None) == -1                                                                  # no columns
    assert f(p8, 64, p8, 63, 4, p8, p8, None) == -1                                                                 # ld < Mp
    assert f(p8, 64, p8, 64, -1, p8, p8, None) == -1                                                                # negative n_points
    assert f(p8, 48, p8, 64, 4, p8, p8, None) == -2 and b"multiple of 32" in lib.scasml_last_error()               # Mp % 32 != 0
    assert f(p8, 64, p8, 64, 16 * 2 ** 31, p8, p8, None) == -2 and b"too many" in lib.scasml_last_error()          # 2^31 tiles
    assert f(p8, 48, p8, 47, 4, p8, p8, None) == -1                                                                 # the order: arguments first
    assert f(p8, 64, p8, 64, 0, p8, p8, None) == 0                                                                  # no points: nothing to do


def test_functional_covariance_kernel_is_one_kernel_without_scratch():
    """The OPS = 4 instantiation of the variance tile carries three more sums per lane than the variance kernel: still in registers."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "gp_functional_cov.hip"], capture_output=True, text=True,
                         check=True).stdout
    kernels = [l for l in out.splitlines() if l.strip()]
    assert len(kernels) == 1 and "gp_functional_covariance_kernel" in kernels[0], out
    m = re.search(r"scratch\s+(\d+)\s+vgpr\s+(\d+)", kernels[0])
    assert m and int(m.group(1)) == 0 and int(m.group(2)) <= 512 and "!!" not in kernels[0], kernels[0]


@pytest.mark.parametrize("d", [1, 6, 100])
def test_prior_block_is_the_oracles_table_at_x_equal_y(d):
    from oracle.equation import GradDependentNonlinear
    from oracle.gp import OracleGP
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    og = OracleGP(GradDependentNonlinear(d + 1))
    x = np.zeros((1, d + 1))                           # the table depends on x - y alone; at the origin the oracle's norm expansion is exact
    x[0, -1] = 0.25
    want = np.array([[og.block(ox, oy, x, x.copy())[0, 0] for oy in ref.OPS] for ox in ref.OPS])
    P = ref.prior_block(d, og.a)
    np.testing.assert_allclose(P, want, rtol=1e-14, atol=0.0)
    assert np.array_equal(P, P.T) and np.all(np.diag(P) > 0.0)
    gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)
    np.testing.assert_allclose(gp._functional_prior(), want, rtol=1e-14, atol=0.0)


def test_the_reference_draws_alone_stay_inside_the_moment_cap():
    """The seed of the GPU moment test is chosen so that the NumPy statement alone -- reference draws against route A and the reference linearisation
    -- lies inside the cap of six standard errors that test uses (1.67 and 1.29 at this seed)."""
    from oracle.equation import GradDependentNonlinear
    mc = ref.moment_case()
    og, Kp, X = mc["og"], mc["Kp"], mc["X"]
    k = ref.rows(og, X)
    cov = ref.route_a(Kp, k, ref.prior_block(mc["d"], og.a))
    m, c, _, var = ref.residual_parts(GradDependentNonlinear(mc["d"] + 1), k, mc["alpha"], cov)
    fun = ref.posterior_functional_draws(og, Kp, mc["z"], ref.NUGGET, ref.MOMENT_FEATURES, ref.MOMENT_SEED, np.arange(ref.MOMENT_DRAWS), X)
    r_cov, r_var = ref.moment_ratios(fun, m, cov, c, var)
    print("reference alone: functional covariance within %.2f, residual variance within %.2f standard errors" % (r_cov, r_var))
    assert r_cov <= 6.0 and r_var <= 6.0
