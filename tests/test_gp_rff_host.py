"""CPU-side checks of the pathwise GP posterior draws.  The first three pin the NumPy statement the GPU tests compare the device with
(tests/_gp_rff_ref.py): its vectorised feature draw against oracle.philox.normals, its Lap / dt / div against central differences of its own u, and
the second moments of all 25 operator blocks against the oracle's closed-form Gram -- the check that pins every sign and multiplier (the
interpolation identity of the GPU tests cannot: the prior draw cancels in it).  The rest: scasml_gp_rff_functionals and scasml_gp_rff_noise
(csrc/gp_rff.hip) are declared within ABI 7, bound, refuse bad arguments with codes before anything is launched, and their kernels use no scratch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _gp_rff_ref as ref
from oracle import philox
from scasml_gp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENT_SEED = 7            # the largest of the 25 blocks is 2.58 standard errors at this seed (seeds 0 .. 7 give 2.2 .. 3.4)


@pytest.fixture(scope="module")
def lib():
    from scasml_gp_amd import _build
    _build.build_library()
    return _lib.load()


def test_feature_draw_is_the_oracles_normals():
    for d, draw, seed in ((1, 0, 3), (3, 5, 0x1234567890ABCDEF), (6, 2 ** 32 - 1, 9)):
        got = ref.feature_normals(d, seed, [draw, draw + 1 if draw < 2 ** 32 - 1 else 0], 5)
        for r, dr in enumerate((draw, draw + 1 if draw < 2 ** 32 - 1 else 0)):
            for f in range(5):
                want = philox.normals(seed, ref.STREAM_GP_RFF, np.array([dr], dtype=np.uint64), f, d + 3)[0]
                assert np.array_equal(got[r, f].view(np.uint32), want.view(np.uint32))
    assert ref.STREAM_GP_RFF == _lib.STREAM_GP_RFF and ref.STREAM_GP_RFF_NOISE == _lib.STREAM_GP_RFF_NOISE


@pytest.mark.parametrize("d", [1, 3])
def test_functionals_are_the_derivatives_of_u(d):
    """Central differences of the statement's own u in np.longdouble: step h = 2^-20, so the truncation error h^2 / 6 |u'''| (first derivatives) and
    h^2 / 12 |u''''| (second) is ~1e-13 of the derivative's scale and the rounding error 2^-64 / h^2 ~ 6e-8 of |u| at worst; asserted at 1e-6 of the
    functional's scale sum_f |mult_f| (|wc_f| + |ws_f|) F^-1/2."""
    L = np.longdouble
    a, F, seed, draw = 0.7, 40, 11, 3
    feats = ref.features(d, a, F, seed, draw)
    X = np.random.default_rng(d).uniform(-1, 1, (7, d + 1)).astype(np.float32).astype(L)
    h = L(2.0) ** -20

    def u(Y):
        omega, wc, ws = (v.astype(L) for v in feats)
        th = Y @ omega.T
        return ((wc * np.cos(th) + ws * np.sin(th)).sum(1)) / np.sqrt(L(F))

    got = ref.functionals(d, a, F, seed, draw, X.astype(np.float64), feats)
    scale = (np.abs(ref.multipliers(feats[0], d)) * (np.abs(feats[1]) + np.abs(feats[2]))[:, None]).sum(0) / np.sqrt(F)
    e = np.eye(d + 1, dtype=L)
    first = [(u(X + h * e[k]) - u(X - h * e[k])) / (2 * h) for k in range(d + 1)]
    second = [(u(X + h * e[k]) - 2 * u(X) + u(X - h * e[k])) / (h * h) for k in range(d)]
    want = np.stack([u(X), sum(second), first[d], sum(first[:d])], axis=1)
    err = np.abs(got - want).max(0) / scale
    print("d=%d central differences, error / scale of u, Lap, dt, div: %s" % (d, err.astype(np.float64)))
    assert (err <= 1e-6).all()


def second_moment_ratios(seed):
    """The feature average of phi phi^T of ONE draw with F = 2^17 features at (d, N_dom, N_bdy) = (3, 4, 2) against the oracle's Gram: the largest
    |average - K| / (empirical standard error) of every one of the 25 blocks."""
    from _gp_evidence_ref import oracle, points
    d, nd, nb, F = 3, 4, 2, 1 << 17
    dom, bdy = points(d, nd, nb)
    og = oracle(d)
    K = og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64))
    feats = ref.features(d, og.a, F, seed, 0)
    fd, fb = ref.per_feature(d, feats, dom, np.float64), ref.per_feature(d, feats, bdy, np.float64)      # (n, F, 4)
    phi = np.concatenate([fd[:, :, 0], fb[:, :, 0], fd[:, :, 1], fd[:, :, 2], fd[:, :, 3]])               # (M, F)
    mean, square = phi @ phi.T / F, (phi * phi) @ (phi * phi).T / F                                         # of the products phi_i phi_j over the features
    ratio = np.abs(mean - K) / np.sqrt((square - mean * mean) / (F - 1))
    edges = [0, nd, nd + nb, 2 * nd + nb, 3 * nd + nb, 4 * nd + nb]
    return np.array([[ratio[edges[i]:edges[i + 1], edges[j]:edges[j + 1]].max() for j in range(5)] for i in range(5)])


def test_second_moments_match_the_oracle_gram():
    """E[L_x f . L_y f] = L_x L_y kappa for every operator pair: within 6 empirical standard errors in every block; the seed is one at which the
    statement stays within 4.5 (324 entries: the largest of that many standard normals is ~3)."""
    blocks = second_moment_ratios(MOMENT_SEED)
    print("largest |feature average - K| / standard error per block:\n%s" % np.array2string(blocks, precision=2))
    assert blocks.shape == (5, 5) and (blocks <= 6.0).all()
    assert blocks.max() <= 4.5


def test_entry_points_are_declared_bound_and_exported_within_abi_7(lib):
    header = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"\bint scasml_gp_rff_functionals\(int32_t d, double a, const float \*x, int64_t n, int64_t ld_x, int32_t F, uint64_t seed, "
                     r"int64_t sample0, int64_t S,\s*double \*out, void \*stream\);", header)
    assert re.search(r"\bint scasml_gp_rff_noise\(int64_t M, uint64_t seed, int64_t sample0, int64_t S, double \*out, int64_t ld, void \*stream\);", header)
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", header) and lib.scasml_abi_version() == 7
    for name, value in (("SCASML_STREAM_GP_RFF", _lib.STREAM_GP_RFF), ("SCASML_STREAM_GP_RFF_NOISE", _lib.STREAM_GP_RFF_NOISE)):
        m = re.search(r"#define %s (0x[0-9A-Fa-f]+)u\b" % name, header)
        assert m and int(m.group(1), 16) == value and value >= 1 << 30           # the solvers count their streams from 0, one per call
    assert len({_lib.STREAM_GP_SAMPLE, _lib.STREAM_GP_RFF, _lib.STREAM_GP_RFF_NOISE}) == 3
    assert _lib.SIGNATURES["scasml_gp_rff_functionals"] == (C.c_int, [C.c_int32, C.c_double, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_uint64,
                                                                      C.c_int64, C.c_int64, C.c_void_p, C.c_void_p])
    assert _lib.SIGNATURES["scasml_gp_rff_noise"] == (C.c_int, [C.c_int64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p])
    assert hasattr(lib, "scasml_gp_rff_functionals") and hasattr(lib, "scasml_gp_rff_noise")
    assert "gp_rff.hip" in __import__("scasml_gp_amd._build", fromlist=["SOURCES"]).SOURCES


def test_refusals_come_back_as_codes_without_a_gpu(lib):
    p8 = C.c_void_p(8)
    ok = dict(d=3, a=0.5, x=p8, n=10, ld_x=4, F=64, seed=1, sample0=0, S=2, out=p8)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.scasml_gp_rff_functionals(v["d"], v["a"], v["x"], v["n"], v["ld_x"], v["F"], v["seed"], v["sample0"], v["S"], v["out"], None)

    for name in ("x", "out"):
        assert call(**{name: None}) == -1 and b"gp_rff_functionals" in lib.scasml_last_error(), name
    assert call(d=0) == -1 and call(d=_lib.MAX_DIM + 1, ld_x=_lib.MAX_DIM + 2) == -1
    assert call(a=0.0) == -1 and call(a=float("nan")) == -1
    assert call(F=0) == -1 and b"F=0" in lib.scasml_last_error()
    assert call(ld_x=3) == -1
    assert call(n=-1) == -1 and call(S=-1) == -1 and call(sample0=-1) == -1
    assert call(sample0=2 ** 32 - 1, S=2) == -2 and b"2^32" in lib.scasml_last_error()
    assert call(sample0=2 ** 32, S=1) == -2
    assert call(n=0) == 0 and call(S=0) == 0                                   # nothing asked: nothing launched
    noise = lib.scasml_gp_rff_noise
    assert noise(5, 1, 0, 2, None, 5, None) == -1 and b"gp_rff_noise" in lib.scasml_last_error()
    assert noise(-1, 1, 0, 2, p8, 5, None) == -1 and noise(5, 1, 0, 2, p8, 4, None) == -1
    assert noise(5, 1, -1, 2, p8, 5, None) == -1 and noise(5, 1, 0, -2, p8, 5, None) == -1
    assert noise(5, 1, 2 ** 32 - 1, 2, p8, 5, None) == -2
    assert noise(0, 1, 0, 2, p8, 5, None) == 0 and noise(5, 1, 0, 0, p8, 5, None) == 0


def test_rff_kernels_use_no_scratch(tmp_path):
    """The feature kernel holds 16 accumulators, 32 running sums and the two operand stages in registers through an epilogue of 16 double sincos:
    all of it must stay in registers."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "gp_rff.hip"], capture_output=True, text=True, check=True,
                         env=dict(os.environ, KERNEL_REGS_OUT=str(tmp_path / "gp_rff.s"))).stdout
    for kernel in ("gp_rff_kernel", "gp_rff_noise_kernel"):
        lines = [l for l in out.splitlines() if kernel in l]
        assert len(lines) == 1, out
        m = re.search(r"scratch\s+(\d+)\s+vgpr\s+(\d+)", lines[0])
        assert m and int(m.group(1)) == 0 and int(m.group(2)) <= 512 and "!!" not in lines[0], lines[0]
