"""The float64 training layer (csrc/gp_train.hip, csrc/dist_linalg.hip) against float64 references on the CPU, on every dispatch path of its
host code: the Cholesky factorisation, the triangular solves and the inverse at the sizes where the 64 x 64 (WS = 2), the 128 x 128 (WS = 4)
register-staged and the LDS-DMA update tiles take over, with and without the look-ahead and under forced outer panels; the 1-based `info`
of a non-positive pivot; the six block-row building blocks of the distributed fit; scasml_gemv and the four Newton kernels with lda > M.

Bounds are the standard backward-error ones, gamma_n = n eps / (1 - n eps) with a safety factor of 2 (the CPU reference rounds too), checked
on sampled rows or columns: the first and last, every 32- ... 512-boundary pair near both edges, and 64 random ones.  Where a case has an
exact property (untouched padding, a bit-identical alternative tile, a region that must never be read) it is asserted bitwise.

Run as a script (`python tests/test_gpu_f64_linalg.py outer <rows>`) the file is the child process of the forced-outer-panel cases:
SCASML_CHOL_OUTER is read once per process."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SAFETY = 2.0
REG_KNOB = "SCASML_F64_TILE_REGISTER_STAGED"


def gamma(n):
    return n * EPS / (1 - n * EPS)


def sample(n, seed, extra=64):
    """Indices < n: 0 and n - 1, the pairs around every 32/64/128/256/512 boundary near both ends, the ragged last tile, `extra` random."""
    idx = {0, 1, n - 2, n - 1}
    for b in (32, 64, 128, 256, 512):
        for m in (b, 2 * b, (n - 1) // b * b, (n - 1) // b * b - b):
            idx |= {m - 1, m}
    idx |= set(range((n - 1) // 64 * 64, n, 7))            # the ragged last 64-tile
    idx |= set(np.random.default_rng(seed).choice(n, min(n, extra), replace=False).tolist())
    return np.array(sorted(i for i in idx if 0 <= i < n))


def _lib_and_stream():
    from scasml_gp_amd import _lib
    return _lib, _lib.load(), _lib.stream_ptr()


def _gen(seed):
    import torch
    return torch.Generator(device="cuda").manual_seed(seed)


def _factor(M, seed):
    """L0 = D + N (D in [1, 2], N strictly lower with ||N||_F < 1) and A = L0 L0^T made exactly symmetric; kappa(A) <= ((2 + |N|)/(1 - |N|))^2."""
    import torch
    g = _gen(seed)
    N = torch.randn((M, M), dtype=torch.float64, device="cuda", generator=g).tril_(-1) * (0.6 / M)
    nF = float(torch.linalg.norm(N))
    assert nF < 0.9
    L0 = N + torch.diag(1.0 + torch.rand(M, dtype=torch.float64, device="cuda", generator=g))
    del N
    A = L0 @ L0.T
    A = A.tril() + A.tril(-1).T
    return L0, A, ((2 + nF) / (1 - nF)) ** 2


def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


def _cholesky(A, expect_info=0):
    import torch
    _lib, lib, s = _lib_and_stream()
    L = A.clone()
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    assert lib.scasml_cholesky(_lib.ptr(L), L.shape[0], 0.0, _lib.ptr(info), s) == 0, lib.scasml_last_error()
    torch.cuda.synchronize()
    assert int(info.item()) == expect_info
    return L


def _check_factor(L, A, seed):
    """|L L^T - A| <= gamma_{M+1} |L||L|^T on sampled rows, a strict upper triangle of exact zeros, a positive diagonal."""
    import torch
    M = L.shape[0]
    assert int(torch.triu(L, 1).count_nonzero()) == 0
    dg = torch.diagonal(L)
    assert bool(torch.all(dg > 0)) and bool(torch.all(torch.isfinite(L)))
    S = sample(M, seed)
    Lc = L.cpu().numpy()
    Ls = Lc[S]
    res = np.abs(Ls @ Lc.T - A[torch.from_numpy(S).cuda()].cpu().numpy())
    bound = SAFETY * gamma(M + 1) * (np.abs(Ls) @ np.abs(Lc).T)
    bad = res > bound
    assert not bad.any(), "M=%d: %d entries over the bound, worst ratio %g at row %d" % (
        M, bad.sum(), (res / np.maximum(bound, 1e-300)).max(), S[np.argwhere(bad)[0][0]])
    return Lc


def _inverse(L):
    import torch
    _lib, lib, s = _lib_and_stream()
    X = torch.full_like(L, float("nan"))
    assert lib.scasml_cholesky_inverse(_lib.ptr(L), L.shape[0], _lib.ptr(X), s) == 0, lib.scasml_last_error()
    torch.cuda.synchronize()
    return X


def _check_inverse(X, A, kappa, seed):
    """Exactly symmetric; |A X - I| <= gamma_M kappa |A||X| on sampled columns."""
    import torch
    M = X.shape[0]
    assert torch.equal(X, X.T)
    S = sample(M, seed)
    Ac = A.cpu().numpy()
    Xs = X[:, torch.from_numpy(S).cuda()].cpu().numpy()
    R = Ac @ Xs
    R[S, np.arange(len(S))] -= 1.0
    bound = SAFETY * gamma(M) * kappa * (np.abs(Ac) @ np.abs(Xs))
    assert np.all(np.abs(R) <= bound), "M=%d: worst ratio %g" % (M, (np.abs(R) / bound).max())
    return Ac


# ------------------------------------------------------------------------------------------------------------------ A. scasml_cholesky
# 32: the diagonal block alone; 96, 288: WS = 2 panel updates (288: a 32-row trailing update after one full outer panel); 4224: the reference's
# fit size; 4384: the first trailing update on the WS = 4 DMA tile (32-row edge tiles); 8160: the largest without look-ahead; 8192, 8288: look-ahead
# with 512-column outer panels, the last one 96 wide
@pytest.mark.parametrize("M", [32, 96, 288, 4224, 4384, 8160, 8192, 8192 + 96])
def test_cholesky_backward_error(M):
    import scipy.linalg
    L0, A, kappa = _factor(M, seed=M)
    L = _cholesky(A)
    Lc = _check_factor(L, A, seed=M)
    if M <= 4384:
        want = scipy.linalg.cholesky(A.cpu().numpy(), lower=True)
        assert np.abs(Lc - want).max() <= SAFETY * gamma(M) * kappa * np.abs(want).max()


def test_cholesky_register_staged_tile_equals_dma_tile(monkeypatch):
    """M = 4384: the first trailing update runs on the WS = 4 tile; the register-staged one sums in the DMA tile's order, bit for bit."""
    import torch
    _, A, _ = _factor(4384, seed=4384)
    L_dma = _cholesky(A)
    monkeypatch.setenv(REG_KNOB, "1")
    L_reg = _cholesky(A)
    monkeypatch.delenv(REG_KNOB)
    _check_factor(L_reg, A, seed=1)
    assert torch.equal(_bits(L_dma), _bits(L_reg))


@pytest.mark.parametrize("M,pivots", [(288, [0, 1, 31, 32, 33, 255, 256]), (4384, [0, 1, 31, 32, 33, 255, 256, 300]),
                                      (8192 + 96, [8191, 8250, 3 * 512 + 256 + 5])])
def test_cholesky_info_reports_the_first_bad_pivot(M, pivots):
    """A = L0 L0^T with A[p, p] lowered by L0[p, p]^2 + 1: the Schur pivot at p is -1, every earlier one untouched, so info = p + 1 and the
    call still succeeds.  p = 1, 33, 255, 8191: later in a diagonal block; 32, 256, 300: later panels; M = 8288: the look-ahead side stream,
    1797: the second sub-panel of an outer panel."""
    L0, A, _ = _factor(M, seed=M + 1)
    for p in pivots:
        Ab = A.clone()
        Ab[p, p] -= L0[p, p] ** 2 + 1.0
        _cholesky(Ab, expect_info=p + 1)


def _forced_outer(outer):
    """Child process: M = 8288 under SCASML_CHOL_OUTER=outer; checks the factor and the inverse, prints the digests."""
    M = 8192 + 96
    L0, A, kappa = _factor(M, seed=M)
    L = _cholesky(A)
    _check_factor(L, A, seed=outer)
    X = _inverse(L0)
    _check_inverse(X, A, kappa, seed=outer)
    print(json.dumps({"A": _digest(A), "L": _digest(L), "X": _digest(X)}))


def test_forced_outer_panels_in_a_fresh_process():
    """SCASML_CHOL_OUTER is read once per process: 768 (sub-panels of 256, ragged 608-row groups 256 + 256 + 96 in the inverse) and 1024 (the
    huge-panel schedule at a small M) run in child processes, one at a time.  Both pass their own checks and, from the same A, give a factor
    and an inverse that differ from the default schedule's (the knob took effect)."""
    M = 8192 + 96
    L0, A, _ = _factor(M, seed=M)
    ref = {"A": _digest(A), "L": _digest(_cholesky(A)), "X": _digest(_inverse(L0))}
    del L0, A
    env = dict(os.environ)
    env.pop(REG_KNOB, None)
    for outer in (768, 1024):
        env["SCASML_CHOL_OUTER"] = str(outer)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "outer", str(outer)], env=env, timeout=600, capture_output=True, text=True)
        assert r.returncode == 0, "outer=%d exit %d\n%s\n%s" % (outer, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        got = json.loads(r.stdout.strip().splitlines()[-1])
        assert got["A"] == ref["A"] and got["L"] != ref["L"] and got["X"] != ref["X"], outer


# ------------------------------------------------------------------------------------------------------------------ B. scasml_trsm_lower
def _check_solve(Lc, trans, Xs, Bs, what):
    Lm = Lc.T if trans else Lc
    res = np.abs(Lm @ Xs - Bs)
    bound = SAFETY * gamma(Lc.shape[0]) * (np.abs(Lm) @ np.abs(Xs))
    assert np.all(res <= bound), "%s: worst ratio %g" % (what, (res / bound).max())


def _trsm(L, B, trans):
    import torch
    _lib, lib, s = _lib_and_stream()
    assert lib.scasml_trsm_lower(_lib.ptr(L), L.shape[0], _lib.ptr(B), B.shape[1], trans, s) == 0, lib.scasml_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,nrhs", [(M, n) for M in (32, 288) for n in (1, 2, 31, 65, 129)] + [(4384, 1), (4384, 4097), (4384, 4098)])
def test_trsm_lower_residual(M, nrhs):
    """4097: the WS = 4 register-staged update (odd nrhs); 4098: the WS = 4 DMA update."""
    import torch
    L0, _, _ = _factor(M, seed=M + 2)
    Lc = L0.cpu().numpy()
    B0 = torch.randn((M, nrhs), dtype=torch.float64, device="cuda", generator=_gen(nrhs))
    S = torch.from_numpy(sample(nrhs, nrhs)).cuda()
    for trans in (0, 1):
        B = B0.clone()
        _trsm(L0, B, trans)
        _check_solve(Lc, trans, B[:, S].cpu().numpy(), B0[:, S].cpu().numpy(), "M=%d nrhs=%d trans=%d" % (M, nrhs, trans))


def test_trsm_lower_register_staged_tile_equals_dma_tile(monkeypatch):
    import torch
    L0, _, _ = _factor(4384, seed=4386)
    B0 = torch.randn((4384, 4098), dtype=torch.float64, device="cuda", generator=_gen(3))
    for trans in (0, 1):
        out = []
        for knob in (False, True):
            if knob:
                monkeypatch.setenv(REG_KNOB, "1")
            B = B0.clone()
            _trsm(L0, B, trans)
            monkeypatch.delenv(REG_KNOB, raising=False)
            out.append(B)
        assert torch.equal(_bits(out[0]), _bits(out[1])), trans


def test_trsm_lower_no_right_hand_sides_and_the_largest_count():
    """nrhs = 0 succeeds and touches nothing.  nrhs = 2^21 - 1 (1.6 GB), the largest count the entry accepts, is right on sampled columns,
    the last ragged tile and columns past 2^20 included."""
    import torch
    _lib, lib, s = _lib_and_stream()
    L0, _, _ = _factor(96, seed=96)
    Lc = L0.cpu().numpy()
    B = torch.randn((96, 5), dtype=torch.float64, device="cuda", generator=_gen(0))
    B0 = B.clone()
    assert lib.scasml_trsm_lower(_lib.ptr(L0), 96, _lib.ptr(B), 0, 0, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(B), _bits(B0))
    del B, B0
    nrhs = (1 << 21) - 1
    B = torch.randn((96, nrhs), dtype=torch.float64, device="cuda", generator=_gen(1))
    S = sample(nrhs, 5)
    S = torch.from_numpy(np.union1d(S, [1 << 20, (1 << 20) + 63, nrhs - 64, nrhs - 65])).cuda()
    prev = B[:, S].cpu().numpy()
    for trans in (0, 1):
        _trsm(L0, B, trans)
        Xs = B[:, S].cpu().numpy()
        _check_solve(Lc, trans, Xs, prev, "nrhs=2^21-1 trans=%d" % trans)
        prev = Xs


# ------------------------------------------------------------------------------------------------------------------ C. scasml_cholesky_inverse
@pytest.mark.parametrize("M", [32, 288, 4384, 8160, 8192 + 96])
def test_cholesky_inverse(M):
    """Symmetric bit for bit and a small residual; M <= 4384 matches np.linalg.inv.  4384: the backward sweep's group updates on the WS = 4
    tile; 8160: the largest without look-ahead; 8288: look-ahead groups of 512 rows, the last one 96."""
    L0, A, kappa = _factor(M, seed=M + 3)
    X = _inverse(L0)
    Ac = _check_inverse(X, A, kappa, seed=M)
    if M <= 4384:
        want = np.linalg.inv(Ac)
        assert np.abs(X.cpu().numpy() - want).max() <= SAFETY * gamma(M) * kappa * np.abs(want).max()


def test_cholesky_inverse_register_staged_tile_equals_dma_tile(monkeypatch):
    import torch
    L0, A, kappa = _factor(4384, seed=4384 + 3)
    X_dma = _inverse(L0)
    monkeypatch.setenv(REG_KNOB, "1")
    X_reg = _inverse(L0)
    monkeypatch.delenv(REG_KNOB)
    _check_inverse(X_reg, A, kappa, seed=2)
    assert torch.equal(_bits(X_dma), _bits(X_reg))


# ------------------------------------------------------------------------------------------------------------------ D. dist_linalg.hip
def _gemm(C0, A, B, K, tri=(0, 0, 0)):
    import torch
    _lib, lib, s = _lib_and_stream()
    Cm = C0.clone()
    rows, cols = A.shape[0], B.shape[0]
    assert lib.scasml_gemm_nt_sub(_lib.ptr(Cm), Cm.shape[1], rows, cols, _lib.ptr(A), A.shape[1], _lib.ptr(B), B.shape[1], K, *tri, s) == 0, \
        lib.scasml_last_error()
    torch.cuda.synchronize()
    return Cm


def _check_gemm(Cm, C0, A, B, K, cols, seed):
    """C = C0 - A B^T within gamma_{K+1} (|C0| + |A||B|^T) on sampled rows; columns of C beyond `cols` untouched."""
    import torch
    S = torch.from_numpy(sample(A.shape[0], seed)).cuda()
    As, Bc = A[S, :K].cpu().numpy(), B[:, :K].cpu().numpy()
    c0 = C0[S, :cols].cpu().numpy()
    res = np.abs(Cm[S, :cols].cpu().numpy() - (c0 - As @ Bc.T))
    bound = SAFETY * gamma(K + 1) * (np.abs(c0) + np.abs(As) @ np.abs(Bc).T)
    assert np.all(res <= bound), "worst ratio %g" % (res / bound).max()
    assert torch.equal(_bits(Cm[:, cols:]), _bits(C0[:, cols:]))


# (rows, cols, K, lda, ldb, ldc pads): WS = 2 below 4096 or K < 256; 4096 x 4100 x 256: WS = 4 on the DMA tile, with an odd lda the
# register-staged WS = 4 tile
@pytest.mark.parametrize("rows,cols,K,pa,pb,pc", [(1, 1, 32, 3, 0, 5), (63, 65, 32, 1, 3, 7), (200, 130, 96, 32, 5, 3),
                                                  (4096, 4100, 224, 32, 2, 4), (4096, 4100, 256, 32, 2, 4), (4096, 4100, 256, 33, 2, 4)])
def test_gemm_nt_sub(rows, cols, K, pa, pb, pc):
    import torch
    g = _gen(rows + K + pa)
    A = torch.randn((rows, K + pa), dtype=torch.float64, device="cuda", generator=g)
    B = torch.randn((cols, K + pb), dtype=torch.float64, device="cuda", generator=g)
    C0 = torch.randn((rows, cols + pc), dtype=torch.float64, device="cuda", generator=g)
    A[:, K:] = float("nan")            # beyond K: never read
    B[:, K:] = float("nan")
    _check_gemm(_gemm(C0, A, B, K), C0, A, B, K, cols, seed=rows)


@pytest.mark.parametrize("nlb,K", [(5, 96), (16, 256)])
@pytest.mark.parametrize("row0,stride,col0", [(0, 1, 0), (1, 2, 0), (3, 4, 1), (0, 8, 0)])
def test_gemm_nt_sub_block_triangular_map(nlb, K, row0, stride, col0):
    """C laid out as dist_gp.py lays out block rows: local block lb (256 rows; a 17-row partial one last) is global block row
    row0 + lb * stride, C's columns start at global block column col0.  Tiles above the block diagonal keep their sentinel bit for bit;
    the others equal the stride-0 call bit for bit and the product bound.  nlb = 5, K = 96: WS = 2; nlb = 16, K = 256: the WS = 4 DMA tile."""
    import torch
    BLK = 256
    rows = nlb * BLK + 17
    cols = (row0 + nlb * stride + 1) * BLK
    g = _gen(nlb * 100 + stride)
    A = torch.randn((rows, K), dtype=torch.float64, device="cuda", generator=g)
    B = torch.randn((cols, K), dtype=torch.float64, device="cuda", generator=g)
    C0 = torch.randn((rows, cols), dtype=torch.float64, device="cuda", generator=g)
    lim = []                                                  # per local block row: the first column above its block diagonal
    for lb in range(nlb + 1):
        lim.append(min(cols, max(0, (row0 + lb * stride - col0 + 1) * BLK)))
        C0[lb * BLK:(lb + 1) * BLK, lim[-1]:] = 12345.0625
    full = _gemm(C0, A, B, K)
    _check_gemm(full, C0, A, B, K, cols, seed=nlb)
    tri = _gemm(C0, A, B, K, (row0, stride, col0))
    for lb in range(nlb + 1):
        r = slice(lb * BLK, (lb + 1) * BLK)
        assert torch.equal(_bits(tri[r, :lim[lb]]), _bits(full[r, :lim[lb]])), lb
        assert bool(torch.all(tri[r, lim[lb]:] == 12345.0625)), lb


@pytest.mark.parametrize("nb", [32, 256, 512])
@pytest.mark.parametrize("rows", [1, 255, 257, 5000])
def test_trsm_right_lt(nb, rows):
    """X <- X L^-T with ldl > nb, ldx > nb: the residual X' L^T - X within gamma_nb |X'||L^T|; L beyond nb columns never read, X beyond them untouched."""
    import scipy.linalg
    import torch
    _lib, lib, s = _lib_and_stream()
    L0, _, _ = _factor(nb, seed=nb)
    L = torch.full((nb, nb + 3), float("nan"), dtype=torch.float64, device="cuda")
    L[:, :nb] = L0
    X0 = torch.randn((rows, nb + 5), dtype=torch.float64, device="cuda", generator=_gen(rows))
    X = X0.clone()
    assert lib.scasml_trsm_right_lt(_lib.ptr(L), nb + 3, nb, _lib.ptr(X), nb + 5, rows, s) == 0, lib.scasml_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(X[:, nb:]), _bits(X0[:, nb:]))
    Lc, x0, x = L0.cpu().numpy(), X0[:, :nb].cpu().numpy(), X[:, :nb].cpu().numpy()
    res = np.abs(x @ Lc.T - x0)
    assert np.all(res <= SAFETY * gamma(nb) * (np.abs(x) @ np.abs(Lc).T))
    want = scipy.linalg.solve_triangular(Lc, x0.T, lower=True).T
    assert np.abs(x - want).max() <= SAFETY * gamma(nb) * 16 * np.abs(want).max()       # kappa(L0) <= 4


_GEMV_COLS_MAX, _GEMV_PAD = 3000, 5


@pytest.fixture(scope="module")
def gemv_operands():
    """Per row count: one rows x 3005 matrix on the GPU and its copy on the host; every column count below is a view with lda = 3005."""
    import torch
    out = {}
    for rows in (1, 3, 1024, 1025, 4096, 4097, 70001):
        A = torch.randn((rows, _GEMV_COLS_MAX + _GEMV_PAD), dtype=torch.float64, device="cuda", generator=_gen(rows))
        out[rows] = (A, A.cpu().numpy())
    return out


def _gemv_sub(A, cols, x, y, trans):
    import torch
    _lib, lib, s = _lib_and_stream()
    assert lib.scasml_gemv_sub(_lib.ptr(A), A.shape[1], A.shape[0], cols, _lib.ptr(x), _lib.ptr(y), trans, s) == 0, lib.scasml_last_error()
    torch.cuda.synchronize()


def _check_gemv(got, y0, Ac, x, n):
    want = y0 - Ac @ x
    res = np.abs(got - want)
    bound = SAFETY * gamma(n + 1) * (np.abs(y0) + np.abs(Ac) @ np.abs(x))
    assert np.all(res <= bound), "worst ratio %g" % (res / bound).max()


@pytest.mark.parametrize("rows", [1, 3, 1024, 1025, 70001])
@pytest.mark.parametrize("cols", [1, 63, 65, 3000])
@pytest.mark.parametrize("trans", [0, 1])
def test_gemv_sub(gemv_operands, rows, cols, trans):
    """y -= A x and y -= A^T x with lda > cols.  trans = 1 up to 1024 rows is a single writer per column: two runs are bitwise equal."""
    import torch
    A, Ac = gemv_operands[rows]
    Ac = Ac[:, :cols]
    g = _gen(rows + cols)
    x = torch.randn((cols if not trans else rows,), dtype=torch.float64, device="cuda", generator=g)
    y0 = torch.randn((rows if not trans else cols,), dtype=torch.float64, device="cuda", generator=g)
    y = y0.clone()
    _gemv_sub(A, cols, x, y, trans)
    _check_gemv(y.cpu().numpy(), y0.cpu().numpy(), Ac.T if trans else Ac, x.cpu().numpy(), rows if trans else cols)
    if trans and rows <= 1024:
        y2 = y0.clone()
        _gemv_sub(A, cols, x, y2, trans)
        assert torch.equal(_bits(y), _bits(y2))


def _gemv_t_ordered(A, lda, rows, cols, x, y, tri=None):
    import torch
    _lib, lib, s = _lib_and_stream()
    n = lib.scasml_gemv_t_ordered_scratch(rows, cols)
    scratch = torch.full((max(n, 1),), float("nan"), dtype=torch.float64, device="cuda")
    if tri is None:
        rc = lib.scasml_gemv_t_sub_ordered(_lib.ptr(A), lda, rows, cols, _lib.ptr(x), _lib.ptr(y), _lib.ptr(scratch), n, s)
    else:
        rc = lib.scasml_gemv_t_sub_ordered_tri(_lib.ptr(A), lda, rows, cols, _lib.ptr(x), _lib.ptr(y), _lib.ptr(scratch), n, tri[0], tri[1], s)
    assert rc == 0, lib.scasml_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows", [1, 4096, 4097, 70001])
@pytest.mark.parametrize("cols", [65, 3000])
def test_gemv_t_sub_ordered(gemv_operands, rows, cols):
    """Row groups of 64 up to 4096 rows, 65 at 4097, 1094 at 70001: the product bound, and two runs bitwise equal."""
    import torch
    A, Ac = gemv_operands[rows]
    g = _gen(rows * 7 + cols)
    x = torch.randn((rows,), dtype=torch.float64, device="cuda", generator=g)
    y0 = torch.randn((cols,), dtype=torch.float64, device="cuda", generator=g)
    out = []
    for _ in range(2):
        y = y0.clone()
        _gemv_t_ordered(A, A.shape[1], rows, cols, x, y)
        out.append(y)
    assert torch.equal(_bits(out[0]), _bits(out[1]))
    _check_gemv(out[0].cpu().numpy(), y0.cpu().numpy(), Ac[:, :cols].T, x.cpu().numpy(), rows)


@pytest.mark.parametrize("nlb", [6, 17])
@pytest.mark.parametrize("row0", [0, 2])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_gemv_tri_sweeps(nlb, row0, stride):
    """Block-row panels as dist_gp.py stores them (local block lb of 256 rows, the last one 17 rows, is global block row row0 + lb * stride;
    nothing beyond its diagonal block is stored).  With zeros above the block diagonal both sweeps equal the plain entries: the row sweep bit
    for bit (its lanes walk the same columns and only stop early); the transposed sweep bit for bit while the row groups are 64 rows
    (nlb = 6, 1297 rows), since skipping whole 256-row blocks keeps every row in the same accumulator.  At nlb = 17 (4113 rows) the groups
    are 65 rows, a group's first row moves by a non-multiple of 16 when its leading zero blocks are skipped, so its rows land in other
    accumulators: a legitimate change of association, checked against the product bound instead.  Filling the region with NaN changes
    nothing, bit for bit: it is never read."""
    import torch
    BLK = 256
    rows = (nlb - 1) * BLK + 17
    cols = (row0 + (nlb - 1) * stride + 1) * BLK
    lda = cols + 3
    g = _gen(nlb * 10 + row0 * 3 + stride)
    A = torch.randn((rows, lda), dtype=torch.float64, device="cuda", generator=g)
    above = []
    for lb in range(nlb):
        c = (row0 + lb * stride + 1) * BLK
        above.append((slice(lb * BLK, min(rows, (lb + 1) * BLK)), c))
        A[lb * BLK:(lb + 1) * BLK, c:] = 0.0
    xr = torch.randn((cols,), dtype=torch.float64, device="cuda", generator=g)
    xt = torch.randn((rows,), dtype=torch.float64, device="cuda", generator=g)
    yr0 = torch.randn((rows,), dtype=torch.float64, device="cuda", generator=g)
    yt0 = torch.randn((cols,), dtype=torch.float64, device="cuda", generator=g)
    _lib, lib, s = _lib_and_stream()

    def tri_pair():
        yr, yt = yr0.clone(), yt0.clone()
        assert lib.scasml_gemv_sub_tri(_lib.ptr(A), lda, rows, cols, _lib.ptr(xr), _lib.ptr(yr), row0, stride, s) == 0, lib.scasml_last_error()
        _gemv_t_ordered(A, lda, rows, cols, xt, yt, (row0, stride))
        return yr, yt

    yr_plain, yt_plain = yr0.clone(), yt0.clone()
    _gemv_sub(A, cols, xr, yr_plain, 0)
    _gemv_t_ordered(A, lda, rows, cols, xt, yt_plain)
    yr, yt = tri_pair()
    assert torch.equal(yr, yr_plain)
    if rows <= 4096:
        assert torch.equal(yt, yt_plain)
    Ac = A[:, :cols].cpu().numpy()
    _check_gemv(yt.cpu().numpy(), yt0.cpu().numpy(), Ac.T, xt.cpu().numpy(), rows)
    _check_gemv(yr.cpu().numpy(), yr0.cpu().numpy(), Ac, xr.cpu().numpy(), cols)
    for r, c in above:
        A[r, c:] = float("nan")
    yr_nan, yt_nan = tri_pair()
    assert torch.equal(_bits(yr_nan), _bits(yr)) and torch.equal(_bits(yt_nan), _bits(yt))


# ------------------------------------------------------------------------------------------------------------------ E. scasml_gemv, Newton kernels
@pytest.mark.parametrize("M", [1, 5, 4225])
def test_gemv_with_a_leading_dimension(M):
    """y = A x with lda = M + 7; the padding holds NaN and must not be read."""
    import torch
    _lib, lib, s = _lib_and_stream()
    g = _gen(M)
    A = torch.randn((M, M + 7), dtype=torch.float64, device="cuda", generator=g)
    A[:, M:] = float("nan")
    x = torch.randn((M,), dtype=torch.float64, device="cuda", generator=g)
    y = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.scasml_gemv(_lib.ptr(A), M, M + 7, _lib.ptr(x), _lib.ptr(y), s) == 0, lib.scasml_last_error()
    torch.cuda.synchronize()
    _check_gemv(y.cpu().numpy(), np.zeros(M), -A[:, :M].cpu().numpy(), x.cpu().numpy(), M)


def _newton_reference(eq, sol, g, N, Nb, A):
    """b, the dense Jacobian J = db/dsol ((4N + Nb) x 3N), the Hessian pieces of F and a magnitude per point for the tolerances."""
    z1, z3, z5 = sol[:N], sol[N:2 * N], sol[2 * N:]
    F, (d1, d3, d5), (F11, F15, F55) = eq.F_parts(z1, z3, z5)
    M, k = 4 * N + Nb, np.arange(N)
    b = np.concatenate([z1, g, z3, F, z5])
    J = np.zeros((M, 3 * N))
    J[k, k] = 1.0
    J[N + Nb + k, N + k] = 1.0
    J[2 * N + Nb + k, k], J[2 * N + Nb + k, N + k], J[2 * N + Nb + k, 2 * N + k] = d1, d3, d5
    J[3 * N + Nb + k, 2 * N + k] = 1.0
    mag = 10.0 * (1.0 + np.abs(z1) + np.abs(z3) + np.abs(z5)) ** 3      # bounds |F|, its derivatives and the terms inside them
    Jmag = np.abs(J)
    Jmag[2 * N + Nb + k, k] = Jmag[2 * N + Nb + k, N + k] = Jmag[2 * N + Nb + k, 2 * N + k] = mag
    return b, J, Jmag, (F11, F15, F55), mag


def _second(N, w, parts):
    """sum_i w_i Hess(F_i) as a 3N x 3N matrix (F depends on z1_i and z5_i only)."""
    F11, F15, F55 = parts
    H = np.zeros((3 * N, 3 * N))
    k = np.arange(N)
    H[k, k] = w * F11
    H[k, 2 * N + k] = H[2 * N + k, k] = w * F15
    H[2 * N + k, 2 * N + k] = w * F55
    return H


@pytest.mark.parametrize("eq_id", [0, 1])
@pytest.mark.parametrize("N", [1, 7, 300])
@pytest.mark.parametrize("Nb", [0, 1, 45])
def test_newton_kernels_against_the_oracle(eq_id, N, Nb):
    """scasml_gp_newton_b, _jv, _jtv (Ab, v NULL and set) and _system (Gauss-Newton and full, ldh = 3N, 3N + 5, the next multiple of 32)
    against b, J, 2 J^T A b, 2 J^T A J and 2 J^T A J + 2 sum_i (A b)_{F_i} Hess F_i built from the oracle's F_parts, with lda > 4N + Nb (the
    padding of A holds NaN); the padding of H is exactly the identity."""
    import torch
    from oracle.equation import CubicReactionDiffusion, GradDependentNonlinear
    _lib, lib, s = _lib_and_stream()
    d = 20
    eq = (GradDependentNonlinear if eq_id == 0 else CubicReactionDiffusion)(d + 1)
    sig, mu = float(eq.sigma()), float(eq.mu())
    M, n3 = 4 * N + Nb, 3 * N
    g = _gen(eq_id * 1000 + N * 10 + Nb)
    dev = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda", generator=g)
    sol_d = dev(n3)
    if eq_id == 1:
        sol_d[:N] = 0.5 + 0.5 * sol_d[:N]                     # u around the logistic's range, where every factor of f matters
    bdy_d = dev(max(Nb, 1))
    R = dev(M, M)
    lda = M + 3
    A_d = torch.full((M, lda), float("nan"), dtype=torch.float64, device="cuda")
    A_d[:, :M] = (R + R.T) / 2
    sol, bdy, A = sol_d.cpu().numpy(), bdy_d[:Nb].cpu().numpy(), A_d[:, :M].cpu().numpy()
    b, J, Jmag, parts, mag = _newton_reference(eq, sol, bdy, N, Nb, A)
    rF = slice(2 * N + Nb, 3 * N + Nb)
    tol = 1e-13

    out = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.scasml_gp_newton_b(eq_id, d, sig, mu, _lib.ptr(sol_d), _lib.ptr(bdy_d) if Nb else None, N, Nb, _lib.ptr(out), s) == 0
    torch.cuda.synchronize()
    bmag = np.abs(b)
    bmag[rF] = mag
    assert np.all(np.abs(out.cpu().numpy() - b) <= tol * bmag)

    v_d = dev(n3)
    v = v_d.cpu().numpy()
    out.fill_(float("nan"))
    assert lib.scasml_gp_newton_jv(eq_id, d, sig, mu, _lib.ptr(sol_d), _lib.ptr(v_d), N, Nb, _lib.ptr(out), s) == 0
    torch.cuda.synchronize()
    assert np.all(np.abs(out.cpu().numpy() - J @ v) <= tol * (Jmag @ np.abs(v)))

    w_d, Ab_d = dev(M), torch.from_numpy(A @ b).cuda()
    w, Ab = w_d.cpu().numpy(), A @ b
    o = torch.full((n3,), float("nan"), dtype=torch.float64, device="cuda")
    for with_second in (False, True):
        assert lib.scasml_gp_newton_jtv(eq_id, d, sig, mu, _lib.ptr(sol_d), _lib.ptr(w_d), _lib.ptr(Ab_d) if with_second else None,
                                        _lib.ptr(v_d) if with_second else None, 2.0, N, Nb, _lib.ptr(o), s) == 0
        torch.cuda.synchronize()
        want, wmag = 2.0 * (J.T @ w), 2.0 * (Jmag.T @ np.abs(w))
        if with_second:
            want = want + 2.0 * _second(N, Ab[rF], parts) @ v
            wmag = wmag + 2.0 * _second(N, np.abs(Ab[rF]) * mag, (1, 1, 1)) @ np.abs(v)
        assert np.all(np.abs(o.cpu().numpy() - want) <= tol * wmag), with_second

    grad_want, grad_mag = 2.0 * (J.T @ Ab), 2.0 * (Jmag.T @ np.abs(Ab))
    H_gn, H_gn_mag = 2.0 * (J.T @ A @ J), 2.0 * (Jmag.T @ np.abs(A) @ Jmag)
    H2, H2_mag = 2.0 * _second(N, Ab[rF], parts), 2.0 * _second(N, np.abs(Ab[rF]) * mag, (1, 1, 1))
    for ldh in sorted({n3, n3 + 5, (n3 + 31) // 32 * 32}):
        for gn in (1, 0):
            H = torch.full((ldh, ldh), float("nan"), dtype=torch.float64, device="cuda")
            grad = torch.full((n3,), float("nan"), dtype=torch.float64, device="cuda")
            assert lib.scasml_gp_newton_system(eq_id, d, sig, mu, _lib.ptr(A_d), lda, N, Nb, _lib.ptr(sol_d), _lib.ptr(Ab_d), _lib.ptr(grad),
                                               _lib.ptr(H), ldh, gn, s) == 0, lib.scasml_last_error()
            torch.cuda.synchronize()
            Hc = H.cpu().numpy()
            assert np.array_equal(Hc[n3:], np.eye(ldh)[n3:]) and np.array_equal(Hc[:, n3:], np.eye(ldh)[:, n3:]), (ldh, gn)
            assert np.all(np.abs(grad.cpu().numpy() - grad_want) <= tol * grad_mag)
            want, wmag = (H_gn, H_gn_mag) if gn else (H_gn + H2, H_gn_mag + H2_mag)
            assert np.all(np.abs(Hc[:n3, :n3] - want) <= tol * wmag), (ldh, gn)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) == 3 and sys.argv[1] == "outer":
        _forced_outer(int(sys.argv[2]))
    else:
        sys.exit("usage: test_gpu_f64_linalg.py outer <rows>")
