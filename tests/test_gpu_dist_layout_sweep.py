"""The COMPOSITION of the block-row distributed Gram / Cholesky / substitutions / fit (scasml_gp_amd/dist_gp.py) at every layout its
index arithmetic distinguishes, against float64 NumPy on the host.  The six device building blocks are swept one by one in
tests/test_gpu_f64_linalg.py (section D); here it is owned_blocks / _slot0, the all-gather reorder of _panel, the (first block, world,
col0) arguments of the triangular map, the last-pair split of factor(), the groups of four block rows of the substitutions and the
identity padding of build() that are under test.

Layouts (n_dom, n_bdy) -> M = 4 n_dom + n_bdy, d = 20, `a` and the nugget of GP_Grad_Dependent_Nonlinear:
  M = 255 (1 block row, one padding row), 256 (1, none), 257 (2, the last holds ONE real row), 512 (2, none), 700 (3, part real), 1024
  (4: exactly one substitution group), 1025 (5: groups of 4 and 1), 2000 (8: two full groups), 2100 (9: 4 + 4 + 1).
Worlds: 1 in process; 2, 3 and 4 as ranks sharing the GPU over gloo (tests/_dist_ranks.py), ONE launch per world whose ranks walk all nine
layouts and then the fits -- so block rows < ranks (a rank with an empty panel) occurs at every world above 1.

Per layout and world, two matrices:
  (G) what build() makes: the documented Gram, and the Gram as coded by the reference (five Hutchinson indices) without and with the float16
      diagonal (round_diag);
  (S) a synthetic well-conditioned A = L0 L0^T, L0 = D + N as `_factor` of tests/test_gpu_f64_linalg.py (D in [1, 2], N strictly lower, |N|_F
      < 0.9: kappa_2(A) <= ((2 + |N|_F) / (1 - |N|_F))^2), made with NumPy from a fixed seed, identity-padded, written over the panels:
      layout errors apart from the Gram's conditioning.
Checks (SAFETY and gamma(n) = n eps / (1 - n eps) of tests/test_gpu_f64_linalg.py; every reference is NumPy float64 on the host):
  (a) build, on every (G): the owned block rows up to their diagonal block equal the rows of the single-GPU Gram (+ nugget, or
      scasml_round16_diag) bit for bit, zeros to the right, padding rows e_i; memory_bytes() = 8 R.numel() = budget()["panel_R"]; the owned
      block rows of all ranks add up to nblk.
  (b) factor, on (G) documented, both (G) as coded, and (S): |L L^T - A| <= SAFETY gamma_{M+1} |L||L^T| entrywise (a backward error: no
      condition number); on (S) also max |L - chol(A)| <= SAFETY gamma_{M+1} kappa max |L|; padding rows of R still e_i bit for bit;
      diag[k] = the diagonal block of gather_factor() on every rank, also one that owns nothing (to the sign of zeros: _digest_factor); a
      matrix that factor() refuses as not positive definite is a failed check.
  (c) modes, on (G) documented and (S): lookahead=False equals lookahead=True bit for bit in R and diag, for pair=True and pair=False; the
      pair=False factor meets (b) too.
  (d) solve and matvec, on (S) and (G) documented, b and v seeded normals:
        |x - x_ref|_inf <= SAFETY gamma_{3M+1} kappa_inf(A) |x_ref|_inf       (x_ref = numpy.linalg.solve, kappa_inf = numpy.linalg.cond(A, inf))
        |A x - b| <= the same factor times |A||x| entrywise
        |matvec(v) - A v| <= SAFETY gamma_{3M} |L||L^T||v| entrywise
      two calls return the same bits; every rank returns the bits of rank 0.
  (e) recorded, not asserted (nothing promises it): whether the factor has the same bits at every world.
The heavy host products are formed by rank 0 alone; the other ranks report SHA-256 digests of the (replicated) factor, x and K_p v, which must
equal rank 0's.

DistributedGP.fit, in the same launches: the documented operators on equation 0 and on equation 1 (Cubic_Reaction_Diffusion, F11 != 0: the only
one that reaches the second-derivative term of scasml_gp_newton_jtv inside the CG loop) at d = 20, 120 + 40 points (M = 520, 3 block rows),
worlds 1, 2 and 4, against OracleGP.GPsolver on the CPU: same number of Newton steps, losses to rtol 1e-8, right_vector to 1e-6 of its
largest entry, the same right_vector bits on every rank, gauss_newton_steps = the single-GPU GPsolver's count.

The Gauss-Newton fallback.  A search on the CPU oracle (equation 1, d in {6, 20}, n_dom in {20, 40, 80, 120, 150} with n_bdy = n_dom // 3,
seeds 0 .. 39, points of oracle.equation.sample_points) for fits in which H + 1e-4 I is not positive definite at some Newton iterate found
149 of the 400; in all but a handful the oracle's plain Newton then diverges (smallest eigenvalue -1e5 .. -1e18).  FALLBACK_CASE is the
mildest: d = 6, 80 + 26 points, seed 27 -- ONE indefinite iterate, smallest eigenvalue -0.0125.  The oracle has no fallback (it takes the
LU step regardless, as the reference does): from that iterate on its losses are another sequence (4.58 against 3.55 one step later; both
end after six steps at 2.9769339, right_vector 1.3e-5 apart).  So that case is compared with the single-GPU GPsolver, which falls back too
(its Cholesky factorisation of H + 1e-4 I fails; the distributed fit's CG meets p^T H p <= 0): see test_fit_fallback_case.

Measured on an MI355X (profiles/dist_layout_sweep.json; SCASML_DIST_LAYOUT_SWEEP_JSON=path writes such a record): no check uses more than
0.015 of its bound -- factor residual <= 0.015 (G) and 0.010 (S), |L - chol(A)| 1.7e-4, solve error and residual on (S) 5.1e-4 (the explicit
group inverses cost nothing measurable at kappa(L_GG) ~ 5; on (G) the bound is loose, kappa_inf ~ 1e7), K_p v 3.5e-3; the fits use 4.5e-4 of
the loss tolerance and 1.4e-7 of the right_vector bound, the fallback case 9.1e-3 and 8.3e-8.  The factor has the same bits at every world,
up to the sign of zeros (_digest_factor).  A launch of all ranks of one world takes 8 .. 10 s, the module 33 s.  Ten mutants of the index
arithmetic (that file's table): eight fail here; `s0 = _slot0(k)` in _update_pair and `nxt = step` in factor() change no behaviour -- what
they add to a launch lies above the block diagonal, where the update tile returns before its first load."""
import hashlib
import json
import os
import time

import numpy as np
import pytest

from test_gpu_dist_gp import _problem
from test_gpu_f64_linalg import SAFETY, gamma

pytestmark = pytest.mark.gpu

D = 20
LAYOUTS = [(60, 15), (60, 16), (60, 17), (120, 32), (150, 100), (240, 64), (240, 65), (450, 200), (500, 100)]
NBLK = {255: 1, 256: 1, 257: 2, 512: 2, 700: 3, 1024: 4, 1025: 5, 2000: 8, 2100: 9}
WORLDS = (2, 3, 4)
HUTCHINSON = (11, 17, 12, 6, 4)
FIT = dict(d=20, nd=120, nb=40, seed=2)                                          # M = 520, 3 block rows
FIT_WORLDS = (1, 2, 4)
FALLBACK_CASE = dict(d=6, nd=80, nb=26, seed=27)                                 # M = 346, 2 block rows
RANK_TIMEOUT = 120           # seconds a rank waits in one gloo collective
LAUNCH_TIMEOUT = 420         # seconds the launcher waits for the results of one world
MEASURED = {"layouts": {}, "fit": {}, "seconds": {}}


def _key(nd, nb):
    return "M=%d" % (4 * nd + nb)


def _bits_equal(x, y):
    import torch
    return x.shape == y.shape and bool(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)))


def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def _digest_factor(L):
    """Of gather_factor(): above one rank it is an all-reduce (a sum with the other ranks' zeros), which turns the factor's -0.0 entries -- the
    Gram has them: -a r_t kappa at r_t = 0, float16(-tiny) -- into +0.0; x + 0.0 does the same to the copy of one rank."""
    return _digest(L + 0.0)


def _worst(res, bound):
    """Largest res / bound over the entries (0 where res is 0)."""
    return float(np.max(np.where(res == 0.0, 0.0, res / np.maximum(bound, 1e-300))))


def _synthetic(M):
    """L0 = D + N, A = L0 L0^T exactly symmetric, kappa bound; NumPy, seeded by M."""
    rng = np.random.default_rng(1000 + M)
    N = np.tril(rng.standard_normal((M, M)), -1) * (0.6 / M)
    nF = float(np.linalg.norm(N))
    assert nF < 0.9
    L0 = N + np.diag(1.0 + rng.random(M))
    A = L0 @ L0.T
    A = np.tril(A) + np.tril(A, -1).T
    return A, ((2 + nF) / (1 - nF)) ** 2


def _single_gpu_gram(a, dom, bdy, nugget, compat_idx, round_diag):
    """K + nugget I as the single-GPU path makes it (models/GP.py kernel_phi_phi): the full Gram in one call, then the diagonal."""
    import ctypes as C
    import torch
    from scasml_gp_amd import _lib
    lib, s = _lib.load(), _lib.stream_ptr()
    xd = torch.from_numpy(np.ascontiguousarray(dom, dtype=np.float32)).cuda()
    xb = torch.from_numpy(np.ascontiguousarray(bdy, dtype=np.float32)).cuda()
    nd, nb = xd.shape[0], xb.shape[0]
    M = 4 * nd + nb
    K = torch.empty((M, M), dtype=torch.float64, device="cuda")
    if compat_idx is None:
        _lib.check(lib.scasml_gp_gram(D, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, _lib.ptr(K), s), "gp_gram")
    else:
        idx = np.ascontiguousarray(compat_idx, dtype=np.int32)
        _lib.check(lib.scasml_gp_gram_compat(D, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, idx.ctypes.data_as(C.c_void_p), _lib.ROUND16_ENTRIES, _lib.ptr(K), s),
                   "gp_gram_compat")
    if round_diag:
        _lib.check(lib.scasml_round16_diag(_lib.ptr(K), M, M, float(nugget), s), "round16_diag")
    else:
        K.diagonal().add_(nugget)
    torch.cuda.synchronize()
    return K


def _padding_is_identity(ch):
    """The rows beyond M of this rank's panel are e_i, bit for bit, over the full width."""
    import torch
    from scasml_gp_amd.dist_gp import BLK
    ok = True
    for slot, i in enumerate(ch.mine):
        first = max(ch.M, i * BLK)
        if first < (i + 1) * BLK:
            want = torch.zeros(((i + 1) * BLK - first, ch.Mp), dtype=torch.float64, device="cuda")
            want[torch.arange(want.shape[0]), torch.arange(first, (i + 1) * BLK)] = 1.0
            ok = ok and _bits_equal(ch.R[slot * BLK + first - i * BLK:(slot + 1) * BLK], want)
    return ok


def _check_build(ch, K, out, tag):
    """(a) on this rank's panel against the single-GPU matrix K (M x M, diagonal already moved)."""
    import torch
    from scasml_gp_amd.dist_gp import BLK, DistCholesky
    Kp = torch.eye(ch.Mp, dtype=torch.float64, device="cuda")
    Kp[:ch.M, :ch.M] = K
    rows_ok = right_ok = True
    for slot, i in enumerate(ch.mine):
        rows, c1 = ch.R[slot * BLK:(slot + 1) * BLK], (i + 1) * BLK
        rows_ok = rows_ok and _bits_equal(rows[:, :c1], Kp[i * BLK:(i + 1) * BLK, :c1])
        right_ok = right_ok and int(rows[:, c1:].contiguous().view(torch.int64).count_nonzero()) == 0
    budget = DistCholesky.budget(D, ch.n_dom, ch.n_bdy, ch.comm.world, ch.comm.rank)
    flags = out["flags"]
    flags["a %s rows = single-GPU Gram, bit for bit" % tag] = rows_ok
    flags["a %s zeros right of the diagonal block" % tag] = right_ok
    flags["a %s padding rows are e_i" % tag] = _padding_is_identity(ch)
    flags["a %s memory_bytes = 8 R.numel = budget panel_R" % tag] = ch.memory_bytes() == ch.R.numel() * 8 == budget["panel_R"]
    flags["a %s shape of R" % tag] = tuple(ch.R.shape) == (len(ch.mine) * BLK, ch.Mp) and ch.R.is_contiguous()
    out["owned"] = budget["owned_block_rows"]
    flags["a %s owned block rows" % tag] = budget["owned_block_rows"] == len(ch.mine) and budget["block_rows"] == ch.nblk


def _load(ch, Ap):
    """Write the identity-padded host matrix Ap over the panels as build() lays a matrix out: rows [i B, (i + 1) B), columns [0, (i + 1) B) of
    every owned block row i, zeros beyond."""
    import torch
    from scasml_gp_amd.dist_gp import BLK
    ch.R = torch.zeros((len(ch.mine) * BLK, ch.Mp), dtype=torch.float64, device="cuda")
    for slot, i in enumerate(ch.mine):
        ch.R[slot * BLK:(slot + 1) * BLK, :(i + 1) * BLK] = torch.from_numpy(np.ascontiguousarray(Ap[i * BLK:(i + 1) * BLK, :(i + 1) * BLK])).cuda()
    return ch


def _factored(ch, out, tag, lookahead=True, pair=True):
    """factor() on a built ch; a matrix refused as not positive definite (every rank raises together) is a failed check, not the end of the
    rank's walk: -> None."""
    import torch
    name = "b %s: factor() accepts the matrix" % tag
    try:
        ch.factor(lookahead=lookahead, pair=pair)
    except ValueError as e:
        if "not positive definite" not in str(e):
            raise
        out["flags"][name] = False
        return None
    torch.cuda.synchronize()
    out["flags"].setdefault(name, True)
    return ch


def _with_panel(ch, R0):
    ch.R = R0.clone()
    return ch


def _check_factor(ch, A, out, tag, heavy, kappa=None):
    """(b) on a factored ch against the host matrix A (M x M, symmetric); -> the gathered factor (device), and on the heavy rank as NumPy."""
    import torch
    from scasml_gp_amd.dist_gp import BLK
    M = ch.M
    Lg = ch.gather_factor()
    flags, ratios = out["flags"], out["ratios"]
    flags["b %s padding rows still e_i" % tag] = _padding_is_identity(ch)
    same = all(t is not None for t in ch.diag)
    for k in range(ch.nblk if same else 0):
        r = min(BLK, M - k * BLK)
        same = same and _bits_equal(torch.tril(ch.diag[k])[:r, :r] + 0.0, Lg[k * BLK:k * BLK + r, k * BLK:k * BLK + r] + 0.0)      # (+ 0.0: see _digest_factor)
    flags["b %s diag[k] = diagonal block of the factor" % tag] = same
    out["digests"]["L %s" % tag] = _digest_factor(Lg)
    L = None
    if heavy:
        L = Lg.cpu().numpy()
        absLLt = np.abs(L) @ np.abs(L).T
        ratios["b %s |L L^T - A| / bound" % tag] = _worst(np.abs(L @ L.T - A), SAFETY * gamma(M + 1) * absLLt)
        flags["b %s factor finite, diagonal positive" % tag] = bool(np.isfinite(L).all() and (np.diag(L) > 0).all())
        if kappa is not None:
            ratios["b %s max |L - chol(A)| / bound" % tag] = float(np.abs(L - np.linalg.cholesky(A)).max() / (SAFETY * gamma(M + 1) * kappa * np.abs(L).max()))
        L = (L, absLLt)
    return L


def _check_modes(make, R0, A, out, tag, heavy, kappa=None):
    """(c): the four factor() modes from the same panel; -> the default-mode object and its host factor."""
    keep = (None, None)
    for pair in (True, False):
        ahead = _factored(_with_panel(make(), R0), out, "%s pair=%s" % (tag, pair), True, pair)
        plain = _factored(_with_panel(make(), R0), out, "%s pair=%s" % (tag, pair), False, pair)
        if ahead is None or plain is None:
            continue
        same = _bits_equal(ahead.R, plain.R) and all(_bits_equal(x, y) for x, y in zip(ahead.diag, plain.diag))
        out["flags"]["c %s pair=%s: lookahead=False has the bits of lookahead=True" % (tag, pair)] = same
        del plain
        L = _check_factor(ahead, A, out, "%s pair=%s" % (tag, pair), heavy, kappa)
        if pair:
            keep = (ahead, L)
    return keep


def _check_solves(ch, A, L, out, tag, heavy):
    """(d) on the default-mode factor."""
    import torch
    if ch is None:
        return
    M = ch.M
    b, v = np.random.default_rng(7).standard_normal(M), np.random.default_rng(8).standard_normal(M)
    bd, vd = torch.from_numpy(b).cuda(), torch.from_numpy(v).cuda()
    x, x2 = ch.solve(bd), ch.solve(bd)
    mv, mv2 = ch.matvec(vd), ch.matvec(vd)
    torch.cuda.synchronize()
    flags, ratios = out["flags"], out["ratios"]
    flags["d %s two solves, the same bits" % tag] = _bits_equal(x, x2) and tuple(x.shape) == (M,)
    flags["d %s two matvecs, the same bits" % tag] = _bits_equal(mv, mv2) and tuple(mv.shape) == (M,)
    out["digests"]["x %s" % tag], out["digests"]["Kv %s" % tag] = _digest(x), _digest(mv)
    if heavy:
        x, mv = x.cpu().numpy(), mv.cpu().numpy()
        x_ref = np.linalg.solve(A, b)
        c = SAFETY * gamma(3 * M + 1) * float(np.linalg.cond(A, np.inf))
        ratios["d %s |x - x_ref|_inf / bound" % tag] = float(np.abs(x - x_ref).max() / (c * np.abs(x_ref).max()))
        ratios["d %s |A x - b| / bound" % tag] = _worst(np.abs(A @ x - b), c * (np.abs(A) @ np.abs(x)))
        ratios["d %s |K_p v - A v| / bound" % tag] = _worst(np.abs(mv - A @ v), SAFETY * gamma(3 * M) * (L[1] @ np.abs(v)))


def sweep_layout(nd, nb, comm, heavy):
    """Every check of one layout on this rank -> {"flags": name -> bool, "ratios": name -> share of the bound used (heavy rank only),
    "digests": name -> SHA-256 of a replicated result, "owned": block rows of this rank, "seconds"}."""
    import torch
    from scasml_gp_amd.dist_gp import DistCholesky
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    t0 = time.perf_counter()
    eq, dom, bdy = _problem(D, nd, nb)
    gp = GP_Grad_Dependent_Nonlinear(eq, compat=None)
    a, nugget = 1.0 / float(gp.sigma) ** 2, gp.nugget
    M = 4 * nd + nb
    out = {"flags": {}, "ratios": {}, "digests": {}}

    def host(K):
        K = K.cpu().numpy()
        return np.tril(K) + np.tril(K, -1).T

    # (G) as coded: build layout and the default factor
    for round_diag in (False, True):
        tag = "G as coded, float16 diagonal" if round_diag else "G as coded"
        K = _single_gpu_gram(a, dom, bdy, nugget, HUTCHINSON, round_diag)
        ch = DistCholesky(D, a, dom, bdy, nugget, comm, compat_idx=HUTCHINSON, round_diag=round_diag).build()
        _check_build(ch, K, out, tag)
        if _factored(ch, out, tag) is not None:
            _check_factor(ch, host(K) if heavy else None, out, tag, heavy)
        del ch, K
    # (G) documented: build layout, the four modes, the solves
    K = _single_gpu_gram(a, dom, bdy, nugget, None, False)
    make = lambda: DistCholesky(D, a, dom, bdy, nugget, comm)
    ch = make().build()
    out["flags"]["layout: M, block rows, owned block rows"] = (ch.M == M and ch.nblk == NBLK[M] and ch.Mp == 256 * NBLK[M]
                                                                 and ch.mine == list(range(comm.rank, NBLK[M], comm.world)))
    _check_build(ch, K, out, "G documented")
    A = host(K) if heavy else None
    fac, L = _check_modes(make, ch.R, A, out, "G documented", heavy)
    _check_solves(fac, A, L, out, "G documented", heavy)
    del ch, fac, K
    # (S) synthetic
    A, kappa = _synthetic(M)
    Ap = np.eye(256 * NBLK[M])
    Ap[:M, :M] = A
    ch = _load(make(), Ap)
    fac, L = _check_modes(make, ch.R, A, out, "S", heavy, kappa)
    _check_solves(fac, A, L, out, "S", heavy)
    del ch, fac
    torch.cuda.synchronize()
    out["seconds"] = time.perf_counter() - t0
    return out


# ------------------------------------------------------------------------------------------------------------------ fits
def _equations(eq_id, d):
    from oracle.equation import CubicReactionDiffusion, GradDependentNonlinear
    from scasml_gp_amd.equations.equations import Cubic_Reaction_Diffusion, Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Cubic_Reaction_Diffusion, GP_Grad_Dependent_Nonlinear
    return ((Grad_Dependent_Nonlinear, GP_Grad_Dependent_Nonlinear, GradDependentNonlinear),
            (Cubic_Reaction_Diffusion, GP_Cubic_Reaction_Diffusion, CubicReactionDiffusion))[eq_id]


def _fit_points(case):
    from oracle.equation import sample_points
    return sample_points(np.random.default_rng(case["seed"]), case["d"], case["nd"], case["nb"])


_REFERENCES = {}


def fit_reference(eq_id, case, oracle=True):
    """Computed once per session in the launching process: the oracle's fit on the CPU (loss history, right_vector) and the single-GPU
    GPsolver's (loss history, right_vector, gauss_newton_steps)."""
    key = (eq_id, tuple(sorted(case.items())))
    if key not in _REFERENCES:
        Eq, Gp, Oeq = _equations(eq_id, case["d"])
        dom, bdy = _fit_points(case)
        ref = {}
        if oracle:
            from oracle.gp import OracleGP
            ogp = OracleGP(Oeq(case["d"] + 1))
            ogp.GPsolver(dom, bdy, GN_steps=20)
            ref.update(oracle_loss=[float(v) for v in ogp.loss_history], oracle_rv=np.asarray(ogp.right_vector, dtype=np.float64).reshape(-1))
        one = Gp(Eq(case["d"] + 1), compat=None)
        one.GPsolver(dom, bdy, GN_steps=20)
        ref.update(single_loss=[float(v) for v in one.loss_history], single_rv=np.asarray(one.right_vector, dtype=np.float64).reshape(-1),
                   single_gauss_newton_steps=int(getattr(one, "gauss_newton_steps", 0)))
        _REFERENCES[key] = ref
    return _REFERENCES[key]


def fit_numbers(eq_id, case, comm):
    """DistributedGP.fit of the documented operators on this rank -> what the assertions need."""
    from scasml_gp_amd.dist_gp import DistributedGP
    t0 = time.perf_counter()
    Eq, Gp, _ = _equations(eq_id, case["d"])
    dom, bdy = _fit_points(case)
    gp = Gp(Eq(case["d"] + 1), compat=None)
    fit = DistributedGP(gp, comm)
    fit.fit(dom, bdy, GN_steps=20)
    rv = np.asarray(gp.right_vector, dtype=np.float64).reshape(-1)
    return dict(loss=[float(v) for v in gp.loss_history], rv=rv, rv_digest=hashlib.sha256(rv.tobytes()).hexdigest()[:16],
                gauss_newton_steps=int(fit.gauss_newton_steps), cg_iterations=list(fit.cg_iterations), block_rows=fit.chol.nblk,
                owned=len(fit.chol.mine), seconds=time.perf_counter() - t0)


FIT_JOBS = {1: [(0, FIT), (1, FIT), (1, FALLBACK_CASE)], 2: [(0, FIT), (1, FIT), (1, FALLBACK_CASE)], 3: [], 4: [(0, FIT), (1, FIT)]}


def _fit_name(eq_id, case):
    return "eq %d, d=%d, %d+%d points, seed %d" % (eq_id, case["d"], case["nd"], case["nb"], case["seed"])


# ------------------------------------------------------------------------------------------------------------------ ranks
def _sweep_worker(rank, world, port, q):
    import datetime
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=RANK_TIMEOUT))
    try:
        from scasml_gp_amd.dist_gp import Comm
        comm = Comm()
        assert comm.world == world and comm.rank == rank and comm.host
        res = {"layouts": {}, "fit": {}}
        for nd, nb in LAYOUTS:
            res["layouts"][_key(nd, nb)] = sweep_layout(nd, nb, comm, heavy=rank == 0)
        for eq_id, case in FIT_JOBS[world]:
            res["fit"][_fit_name(eq_id, case)] = fit_numbers(eq_id, case, comm)
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


_LAUNCHED = {}


def _ranks(world):
    """The results of all ranks of ``world`` (one launch per world and session)."""
    if world not in _LAUNCHED:
        from _dist_ranks import run_ranks
        _LAUNCHED[world] = None                       # a launch that failed is not repeated
        t0 = time.perf_counter()
        _LAUNCHED[world] = [r for _, r in run_ranks(world, _sweep_worker, (), LAUNCH_TIMEOUT)]
        MEASURED["seconds"]["launch of world %d" % world] = time.perf_counter() - t0
    assert _LAUNCHED[world] is not None, "the launch of world %d failed earlier in this session" % world
    return _LAUNCHED[world]


_WORLD1 = {}


def _world1(nd, nb):
    if (nd, nb) not in _WORLD1:
        from scasml_gp_amd.dist_gp import Comm
        comm = Comm()
        assert comm.world == 1 and not comm.active
        _WORLD1[(nd, nb)] = sweep_layout(nd, nb, comm, heavy=True)
    return _WORLD1[(nd, nb)]


def _layout_failures(key, world, per_rank):
    """Every check of one layout that did not hold, as text; the shares of the bounds go on record."""
    bad = []
    nblk = NBLK[int(key[2:])]
    for rank, r in enumerate(per_rank):
        bad += ["%s world %d rank %d: %s" % (key, world, rank, name) for name, ok in sorted(r["flags"].items()) if not ok]
        bad += ["%s world %d rank %d: %s = %.3g > 1" % (key, world, rank, name, v) for name, v in sorted(r["ratios"].items()) if not v <= 1.0]
        for name, dg in sorted(r["digests"].items()):
            if dg != per_rank[0]["digests"].get(name):
                bad.append("%s world %d rank %d: %s differs from rank 0's bits" % (key, world, rank, name))
    if sum(r["owned"] for r in per_rank) != nblk:
        bad.append("%s world %d: owned block rows add up to %d, not %d" % (key, world, sum(r["owned"] for r in per_rank), nblk))
    if not per_rank[0]["ratios"]:
        bad.append("%s world %d: rank 0 formed no host checks" % (key, world))
    rec = MEASURED["layouts"].setdefault(key, {})
    rec["world %d" % world] = dict(share_of_bound=per_rank[0]["ratios"], factor_digests={k: v for k, v in per_rank[0]["digests"].items() if k.startswith("L ")},
                                   checks=sum(len(r["flags"]) + len(r["digests"]) for r in per_rank) + len(per_rank[0]["ratios"]),
                                   seconds_on_rank_0=per_rank[0]["seconds"])
    return bad


@pytest.mark.parametrize("nd,nb", LAYOUTS, ids=[_key(*p) for p in LAYOUTS])
def test_one_rank_in_process(nd, nb):
    bad = _layout_failures(_key(nd, nb), 1, [_world1(nd, nb)])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("world", WORLDS)
def test_ranks_sharing_the_gpu_walk_every_layout(world):
    res = _ranks(world)
    assert len(res) == world
    bad = []
    for nd, nb in LAYOUTS:
        bad += _layout_failures(_key(nd, nb), world, [r["layouts"][_key(nd, nb)] for r in res])
    assert not bad, "\n".join(bad)
    assert any(r["layouts"][_key(60, 15)]["owned"] == 0 for r in res)              # one block row: a rank with an empty panel took part


def _fit_results(world, eq_id, case):
    if world == 1:
        from scasml_gp_amd.dist_gp import Comm
        return [fit_numbers(eq_id, case, Comm())]
    return [r["fit"][_fit_name(eq_id, case)] for r in _ranks(world)]


def _fit_failures(world, got, want_loss, want_rv, want_gn, what):
    bad = []
    shares = dict(loss=0.0, rv=0.0)
    for rank, g in enumerate(got):
        where = "world %d rank %d" % (world, rank)
        if len(g["loss"]) != len(want_loss):
            bad.append("%s: %d Newton losses, %s has %d" % (where, len(g["loss"]), what, len(want_loss)))
        else:
            rel = float(np.max(np.abs(np.asarray(g["loss"]) - np.asarray(want_loss)) / np.abs(want_loss)))
            shares["loss"] = max(shares["loss"], rel / 1e-8)
            if not np.allclose(g["loss"], want_loss, rtol=1e-8):
                bad.append("%s: losses differ from %s's by %.3g (relative)" % (where, what, rel))
        err = float(np.abs(g["rv"] - want_rv).max() / np.abs(want_rv).max())
        shares["rv"] = max(shares["rv"], err / 1e-6)
        if not err <= 1e-6:
            bad.append("%s: right_vector is %.3g of its largest entry from %s's" % (where, err, what))
        if g["rv_digest"] != got[0]["rv_digest"]:
            bad.append("%s: right_vector has not the bits of rank 0" % where)
        if g["gauss_newton_steps"] != want_gn:
            bad.append("%s: %d Gauss-Newton steps, the single-GPU GPsolver took %d" % (where, g["gauss_newton_steps"], want_gn))
    return bad, shares


@pytest.mark.parametrize("eq_id", [0, 1])
@pytest.mark.parametrize("world", FIT_WORLDS)
def test_fit_matches_the_oracle_on_both_equations(world, eq_id):
    ref = fit_reference(eq_id, FIT)
    got = _fit_results(world, eq_id, FIT)
    assert len(got) == world and all(g["block_rows"] == 3 for g in got) and sum(g["owned"] for g in got) == 3
    bad, shares = _fit_failures(world, got, ref["oracle_loss"], ref["oracle_rv"], ref["single_gauss_newton_steps"], "the oracle")
    MEASURED["fit"]["%s, world %d" % (_fit_name(eq_id, FIT), world)] = dict(
        share_of_loss_rtol=shares["loss"], share_of_right_vector_bound=shares["rv"], newton_steps=len(got[0]["loss"]) - 1,
        gauss_newton_steps=got[0]["gauss_newton_steps"], cg_products=sum(got[0]["cg_iterations"]), seconds_on_rank_0=got[0]["seconds"])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("world", [1, 2])
def test_fit_fallback_case(world):
    """The one small case of the oracle search with an indefinite Newton iterate (module docstring).  The oracle takes the LU step of the
    indefinite system; the single-GPU GPsolver (Cholesky fails -> Gauss-Newton operator) and the distributed fit (CG meets p^T H p <= 0 ->
    Gauss-Newton operator) do not, so the reference is the single-GPU GPsolver: the same number of fallback steps, at least one; the same
    number of Newton steps, losses to rtol 1e-8, right_vector to 1e-6; the same bits on every rank."""
    ref = fit_reference(1, FALLBACK_CASE)
    got = _fit_results(world, 1, FALLBACK_CASE)
    bad, shares = _fit_failures(world, got, ref["single_loss"], ref["single_rv"], ref["single_gauss_newton_steps"], "the single-GPU GPsolver")
    print("fallback case, world %d: losses %s\n single-GPU %s\n oracle %s\n right_vector from the oracle's: %.3g of its largest entry" % (
        world, got[0]["loss"], ref["single_loss"], ref["oracle_loss"], np.abs(got[0]["rv"] - ref["oracle_rv"]).max() / np.abs(ref["oracle_rv"]).max()))
    MEASURED["fit"]["fallback: %s, world %d" % (_fit_name(1, FALLBACK_CASE), world)] = dict(
        oracle_newton_steps=len(ref["oracle_loss"]) - 1, oracle_last_loss=ref["oracle_loss"][-1], last_loss=got[0]["loss"][-1],
        right_vector_from_the_oracles=float(np.abs(got[0]["rv"] - ref["oracle_rv"]).max() / np.abs(ref["oracle_rv"]).max()),
        share_of_loss_rtol=shares["loss"], share_of_right_vector_bound=shares["rv"], newton_steps=len(got[0]["loss"]) - 1,
        gauss_newton_steps=got[0]["gauss_newton_steps"], single_gpu_gauss_newton_steps=ref["single_gauss_newton_steps"],
        single_gpu_newton_steps=len(ref["single_loss"]) - 1, cg_products=sum(got[0]["cg_iterations"]), seconds_on_rank_0=got[0]["seconds"])
    assert ref["single_gauss_newton_steps"] >= 1, "the single-GPU GPsolver took no Gauss-Newton step on the case the oracle search found"
    assert not bad, "\n".join(bad)


@pytest.fixture(scope="module", autouse=True)
def _write_measured():
    """SCASML_DIST_LAYOUT_SWEEP_JSON=path: the shares of the bounds, observation (e) and the seconds of this run."""
    yield
    path = os.environ.get("SCASML_DIST_LAYOUT_SWEEP_JSON")
    if not path or not MEASURED["layouts"]:
        return
    same = {}
    for key, worlds in sorted(MEASURED["layouts"].items()):        # (e): the factor's bits, world against world
        names = sorted(set.intersection(*[set(w["factor_digests"]) for w in worlds.values()]))
        same[key] = {n: len({w["factor_digests"][n] for w in worlds.values()}) == 1 for n in names}
        same[key]["worlds"] = sorted(worlds)
    doc = dict(safety=SAFETY, layouts={k: {w: {kk: vv for kk, vv in r.items() if kk != "factor_digests"} for w, r in v.items()}
                                       for k, v in MEASURED["layouts"].items()},
               largest_share_of_any_bound=max([s for v in MEASURED["layouts"].values() for r in v.values() for s in r["share_of_bound"].values()] or [0.0]),
               factor_bits_equal_across_worlds=same, fit=MEASURED["fit"], seconds=MEASURED["seconds"])
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
