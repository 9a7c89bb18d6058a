"""Monte-Carlo standard errors of the Picard solvers' u (``return_stderr=True``, scasml_picard_tree_stderr in include/scasml_hip.h).

Expected values come from the unchanged CPU oracle on bit-identical normals: ``PicardOracle.uz_solve(..., rank=0, world=2, owner=owner)``
with ONE summand's units marked 0 and every other unit 1 returns that summand's unclipped Y in float64 (column 0), so the formula of the
header -- Var = sum over terms of N / (N - 1) sum_i (Y_i - mean)^2 -- is applied to the oracle's own summands.  Unit order: the terminal
samples m = 0 .. mg - 1, then for l = 0 .. n - 1, m = 0 .. mc - 1, k = 0 .. q - 1 the "+" addend and, for l > 0, the "-" addend.

Tolerance: |se - se_oracle| <= 2 (ATOL + RTOL max(|u_unclipped|, se_oracle)) with the ATOL / RTOL of tests/test_gpu_mlp.py (2e-5 / 1e-4) and
tests/test_gpu_scasml.py (5e-5 / 2e-4): the error of se is at most sqrt(N / (N - 1)) <= sqrt(2) times the summed errors of the summands,
which the tolerance on u already bounds.  Every case also asserts that the median oracle se is at least ten times the tolerance.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MLP_TOL = (2e-5, 1e-4)
SCASML_TOL = (5e-5, 2e-4)


def _points(d, B, seed):
    from oracle.equation import sample_points
    dom, bdy = sample_points(np.random.default_rng(seed), d, B - B // 4, B // 4)
    return np.concatenate([dom, bdy])


def _groups(variant, n, par, T=0.5):
    """[(N_j, [units of summand 0, units of summand 1, ...])] of the root call: the terminal term, then the level terms."""
    from oracle.tables import approx_parameters
    if variant == "quad":
        Mf, Mg, Q, _, _ = approx_parameters(par, T)
        mg = int(Mg[par - 1, n])
        terms = [(int(Q[par - 1, n - l - 1]), int(Mf[par - 1, n - l - 1])) for l in range(n)]
    else:
        mg = par ** n
        terms = [(1, par ** (n - l)) for l in range(n)]
    groups = [(mg, [[m] for m in range(mg)])]
    unit = mg
    for l, (q, mc) in enumerate(terms):
        per = q * (2 if l else 1)
        groups.append((mc, [list(range(unit + m * per, unit + (m + 1) * per)) for m in range(mc)]))
        unit += mc * per
    return groups, unit


def _oracle_se(ora, variant, n, par, xt):
    """(se, unclipped u) per row in float64 from the oracle's own summands."""
    import oracle.mlp as O
    groups, units = _groups(variant, n, par)
    var = np.zeros(xt.shape[0])
    u = np.zeros(xt.shape[0])
    # every one of the calls below replays the root call's sample paths (a quadrature path advances on every rank): the oracle's normals
    # are a pure function of (seed, stream, roots, site, d) and its tables one of (par, T), so the same arrays are handed back instead of
    # being computed once per summand; the oracle's code runs unchanged
    draw, memo = O.philox.normals, {}

    def normals(seed, stream, roots, site, d):
        key = (int(seed), int(stream), roots.tobytes(), int(site), int(d))
        if key not in memo:
            memo[key] = draw(seed, stream, roots, site, d)
            memo[key].setflags(write=False)
        return memo[key]
    tables, tab_memo = O.approx_parameters, {}

    def approx_parameters(par_, T):                      # the oracle rebuilds its tables in every call
        if (par_, T) not in tab_memo:
            tab_memo[(par_, T)] = tables(par_, T)
        return tab_memo[(par_, T)]
    O.philox.normals, O.approx_parameters = normals, approx_parameters
    try:
        for N, summands in groups:
            Y = []
            for mine in summands:
                owner = np.ones(units, dtype=np.uint8)
                owner[mine] = 0
                Y.append(ora.uz_solve(n, par, xt, rank=0, world=2, owner=owner)[:, 0])
            Y = np.stack(Y)
            assert Y.shape[0] == N
            u += Y.sum(axis=0)
            var += N / (N - 1.0) * ((Y - Y.mean(axis=0)) ** 2).sum(axis=0)
    finally:
        O.philox.normals, O.approx_parameters = draw, tables
    return np.sqrt(var), u


def _check(got_se, ora, variant, n, par, xt, tol):
    want, u = _oracle_se(ora, variant, n, par, xt)
    got_se = np.asarray(got_se, dtype=np.float64)[:, 0]
    bound = 2.0 * (tol[0] + tol[1] * np.maximum(np.abs(u), want))
    dev = np.abs(got_se - want)
    print("stderr case %s n=%d par=%d d=%d B=%d: se %.3e..%.3e, max |dev| %.3e, max dev/bound %.3f"
          % (variant, n, par, xt.shape[1] - 1, xt.shape[0], want.min(), want.max(), dev.max(), (dev / bound).max()))
    assert np.median(want) >= 10.0 * bound.max(), (np.median(want), bound.max())      # the comparison cannot pass vacuously
    assert np.all(dev <= bound), (dev.max(), (dev / bound).max())


def _mlp(d, variant, seed, eq_pair=None):
    from oracle.equation import GradDependentNonlinear
    from oracle.mlp import PicardOracle
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    from scasml_gp_amd.solvers.MLP_full_history import MLP_full_history
    hip_eq, ora_eq = eq_pair or (Grad_Dependent_Nonlinear, GradDependentNonlinear)
    eq = hip_eq(d + 1)
    hip = MLP(eq, seed=seed) if variant == "quad" else MLP_full_history(eq, seed=seed)
    return hip, PicardOracle(ora_eq(d + 1), variant, seed=seed, stream=0)


def _same_bits(a, b):
    """Bit for bit, NaNs included (z is NaN where the reference's quadrature weight is: SURVEY.md Appendix B)."""
    a, b = (np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v, dtype=np.float32) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _solve(hip, variant, n, par, xt, **kw):
    return hip.uz_solve(n, par, xt, **kw) if variant == "quad" else hip.uz_solve(n, None, xt, par, **kw)


# ---- 1. expected values from the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,rho,B", [(20, 1, 3, 16), (7, 2, 4, 9), (20, 2, 3, 16), (20, 3, 3, 8), (100, 3, 3, 4), (250, 2, 3, 3), (20, 4, 4, 2)])
def test_mlp_quadrature_stderr_matches_oracle_summands(d, n, rho, B):
    """Lane-group widths 4 (d = 7), 8 (d = 20), 32 (d = 100) and 64 (d = 250); n = 4 runs the deep translation unit.
    Largest deviation observed on an MI355X over all cases of this file that compare with the oracle: |se - se_oracle| = 4.3e-7 (equation 2,
    full history, se up to 2.5); largest share of the tolerance 0.001 (n = 1, rho = 3, |dev| 3.6e-8).  The calibration ratio below
    came out at 0.980."""
    hip, ora = _mlp(d, "quad", seed=3)
    xt = _points(d, B, 10 + d)
    uz, se = hip.uz_solve(n, rho, xt, return_stderr=True)
    assert se.shape == (B, 1) and se.dtype == np.float32 and uz.shape == (B, d + 1)
    _check(se, ora, "quad", n, rho, xt, MLP_TOL)


@pytest.mark.parametrize("d,n,M,B", [(20, 2, 3, 16), (11, 2, 2, 7), (100, 3, 3, 4), (12, 5, 2, 3)])
def test_mlp_full_history_stderr_matches_oracle_summands(d, n, M, B):
    hip, ora = _mlp(d, "fh", seed=11)
    xt = _points(d, B, 20 + d)
    uz, se = hip.uz_solve(n, None, xt, M, return_stderr=True)
    assert se.shape == (B, 1) and se.dtype == np.float32
    _check(se, ora, "fh", n, M, xt, MLP_TOL)


@pytest.mark.parametrize("eq_id,variant,d,n,par,B", [(1, "quad", 20, 3, 3, 6), (2, "fh", 20, 3, 2, 6)])
def test_stderr_on_the_other_registered_equations(eq_id, variant, d, n, par, B):
    from oracle.equation import CubicReactionDiffusion, QuadraticGradientReactionDiffusion
    from scasml_gp_amd.equations.equations import Cubic_Reaction_Diffusion, Quadratic_Gradient_Reaction_Diffusion
    pair = {1: (Cubic_Reaction_Diffusion, CubicReactionDiffusion), 2: (Quadratic_Gradient_Reaction_Diffusion, QuadraticGradientReactionDiffusion)}[eq_id]
    hip, ora = _mlp(d, variant, seed=3, eq_pair=pair)
    assert hip.equation.eq_id == eq_id
    xt = _points(d, B, 11)
    _, se = _solve(hip, variant, n, par, xt, return_stderr=True)
    _check(se, ora, variant, n, par, xt, MLP_TOL)


_SCASML = {}


def _scasml(variant, seed):
    """The 60 + 20 point surrogate of tests/test_gpu_scasml.py (compat=None), fitted once and shared by the cases, never modified."""
    if seed not in _SCASML:
        from oracle.equation import GradDependentNonlinear, sample_points
        from oracle.gp import OracleGP
        from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
        from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
        d = 20
        dom, bdy = sample_points(np.random.default_rng(seed), d, 60, 20)
        oeq = GradDependentNonlinear(d + 1)
        ogp = OracleGP(oeq)
        ogp.GPsolver(dom, bdy, GN_steps=20)
        eq = Grad_Dependent_Nonlinear(d + 1)
        gp = GP_Grad_Dependent_Nonlinear(eq, compat=None)
        gp.GPsolver(dom, bdy, GN_steps=20)
        _SCASML[seed] = (eq, gp, oeq, ogp)
    from oracle.mlp import PicardOracle
    from scasml_gp_amd.solvers.ScaSML import ScaSML
    from scasml_gp_amd.solvers.ScaSML_full_history import ScaSML_full_history
    eq, gp, oeq, ogp = _SCASML[seed]
    hip = ScaSML(eq, gp, seed=seed) if variant == "quad" else ScaSML_full_history(eq, gp, seed=seed)
    return hip, PicardOracle(oeq, variant, gp=ogp, seed=seed, stream=0)


def _scasml_points(d, B, seed):
    from oracle.equation import sample_points
    return np.concatenate(sample_points(np.random.default_rng(seed), d, B - B // 4, B // 4))


@pytest.mark.parametrize("variant,n,par,B", [("quad", 2, 3, 12), ("quad", 3, 3, 6), ("fh", 2, 3, 10)])
def test_scasml_stderr_matches_oracle_summands(variant, n, par, B):
    hip, ora = _scasml(variant, seed=7)
    xt = _scasml_points(20, B, 30)
    uz, se = _solve(hip, variant, n, par, xt, return_stderr=True)
    assert se.shape == (B, 1) and se.dtype == np.float32
    _check(se, ora, variant, n, par, xt, SCASML_TOL)


# ---- 2. (u, z) is that of the plain call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,d,n,par,B", [("quad", 20, 3, 3, 37), ("quad", 100, 3, 3, 5), ("quad", 20, 4, 4, 3), ("fh", 20, 3, 3, 37), ("fh", 12, 5, 2, 3)])
def test_mlp_uz_with_stderr_is_bit_identical_to_the_plain_call(variant, d, n, par, B):
    hip, _ = _mlp(d, variant, seed=5)
    xt = _points(d, B, 40)
    plain = _solve(hip, variant, n, par, xt)                                   # call 0
    hip._engine.calls = 0
    uz, se = _solve(hip, variant, n, par, xt, return_stderr=True)              # call 0 again
    assert _same_bits(plain, uz) and hip._engine.calls == 1
    # mixing: the call after a standard-error call is on the stream a plain call would have left it
    after = _solve(hip, variant, n, par, xt)
    hip._engine.calls = 1
    assert _same_bits(after, _solve(hip, variant, n, par, xt)) and not _same_bits(after, plain)
    u, se_u = (hip.u_solve(n, par, xt, return_stderr=True) if variant == "quad" else hip.u_solve(n, None, xt, par, return_stderr=True))
    assert u.shape == (B, 1) and se_u.shape == (B, 1) and hip._engine.calls == 3


@pytest.mark.parametrize("variant,n,par", [("quad", 3, 3), ("fh", 2, 3)])
def test_scasml_uz_and_u_with_stderr_are_bit_identical_to_the_plain_calls(variant, n, par):
    hip, _ = _scasml(variant, seed=7)
    xt = _scasml_points(20, 21, 41)
    plain = _solve(hip, variant, n, par, xt)
    count = hip.evaluation_counter
    hip._engine.calls = 0
    uz, se = _solve(hip, variant, n, par, xt, return_stderr=True)
    assert _same_bits(plain, uz) and hip.evaluation_counter == 2 * count
    args = (n, par, xt) if variant == "quad" else (n, None, xt, par)
    hip._engine.calls = 0
    u_plain = hip.u_solve(*args)
    hip._engine.calls = 0
    u, se_u = hip.u_solve(*args, return_stderr=True)
    assert _same_bits(u_plain, u) and _same_bits(se, se_u) and se_u.shape == (21, 1)     # the se of the correction


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,n,par", [("quad", 3, 3), ("fh", 2, 3)])
def test_terminal_time_rows_level_zero_empty_batch_and_device_tensors(variant, n, par):
    import torch
    hip, _ = _mlp(20, variant, seed=1)
    xt = _points(20, 12, 5)
    xt[::3, -1] = 0.5                                    # t = T: every sample of g coincides, every weight is 0
    uz, se = _solve(hip, variant, n, par, xt, return_stderr=True)
    assert np.all(se[::3, 0] == 0.0) and np.all(se[1::3, 0] > 0.0) and np.all(np.isfinite(se))
    uz0, se0 = _solve(hip, variant, 0, par, xt, return_stderr=True)
    assert np.array_equal(uz0, np.zeros((12, 21), dtype=np.float32)) and np.array_equal(se0, np.zeros((12, 1), dtype=np.float32))
    uze, see = _solve(hip, variant, n, par, xt[:0], return_stderr=True)
    assert uze.shape == (0, 21) and see.shape == (0, 1)
    xd = torch.from_numpy(xt.astype(np.float32)).cuda()
    hip._engine.calls = 0
    uzd, sed = _solve(hip, variant, n, par, xd, return_stderr=True)
    assert isinstance(uzd, torch.Tensor) and isinstance(sed, torch.Tensor) and uzd.is_cuda and sed.is_cuda
    assert sed.dtype == torch.float32 and tuple(sed.shape) == (12, 1)
    assert _same_bits(sed, se) and _same_bits(uzd, uz)


# ---- 4. calibration on the device ----------------------------------------------------------------------------------------------------
def test_reported_stderr_is_calibrated_against_the_spread_of_replicates():
    """One point repeated 4096 times: the root index is a Philox counter word, so the rows are independent replicates.  The oracle gives
    sqrt(mean se^2) / std(u) = 1.017 .. 1.027 at this shape; the sampling error of the ratio is about 1.5 %; u stays far inside the clip."""
    hip, _ = _mlp(20, "quad", seed=2)
    xt = np.repeat(_points(20, 1, 6), 4096, axis=0)
    uz, se = hip.uz_solve(2, 3, xt, return_stderr=True)
    assert np.abs(uz[:, 0]).max() < 0.9 * hip.equation.norm_estimation
    ratio = float(np.sqrt(np.mean(se[:, 0].astype(np.float64) ** 2)) / np.std(uz[:, 0].astype(np.float64), ddof=1))
    print("calibration ratio %.4f" % ratio)
    assert 0.9 <= ratio <= 1.1, ratio


# ---- 5. chunking -------------------------------------------------------------------------------------------------------------------------
def test_chunked_scasml_solve_returns_the_same_stderr_bits(monkeypatch):
    import scasml_gp_amd.solvers._picard as P
    hip, _ = _scasml("quad", seed=7)
    xt = _scasml_points(20, 50, 33)
    hip._engine.calls = 0
    one_uz, one_se = hip.uz_solve(2, 3, xt, return_stderr=True)
    ppr = int(P._lib.load().scasml_points_per_root(C.byref(hip._engine.plan(2, 3))))
    monkeypatch.setattr(P, "POINT_BUFFER_BYTES", ppr * 32 * 4 * 7)             # 7 roots per chunk (point rows of d = 20 are 32 floats)
    hip._engine.calls = 0
    uz, se = hip.uz_solve(2, 3, xt, return_stderr=True)
    assert _same_bits(one_se, se) and _same_bits(one_uz, uz)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_plans_with_a_one_sample_term_are_refused_before_anything_moves():
    hip, _ = _mlp(20, "quad", seed=1)
    xt = _points(20, 4, 5)
    for n, rho in ((2, 2), (1, 2)):
        assert hip._engine.stderr_supported(n, rho)[0] is False
        with pytest.raises(ValueError, match="no estimable variance"):
            hip.uz_solve(n, rho, xt, return_stderr=True)
    assert hip._engine.calls == 0 and hip.evaluation_counter == 0
    fh, _ = _mlp(20, "fh", seed=1)
    with pytest.raises(ValueError, match="no estimable variance"):
        fh.u_solve(2, None, xt, M=1, return_stderr=True)
    assert fh._engine.calls == 0


def test_sharded_parity_mode_and_callback_solves_are_refused():
    import torch
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    xt = _points(20, 4, 5)
    eq = Grad_Dependent_Nonlinear(21)
    with pytest.raises(_lib.ScasmlError):
        MLP(eq)._engine.solve(3, 3, xt, rank=0, world=2, stderr=True)
    for kw in (dict(compat_crn=True), dict(compat_f16=True), dict(compat_rng="jax")):
        solver = MLP(eq, **kw)
        with pytest.raises(_lib.ScasmlError):
            solver.uz_solve(3, 3, xt, return_stderr=True)
        assert solver._engine.calls == 0

    class Callback(Grad_Dependent_Nonlinear):
        eq_id = None
        torch_callbacks = True

        def f(self, x_t, u, z):
            return self.sigma() * u * z.sum(dim=1, keepdim=True)

        def g(self, x_t):
            return 1 - 1 / (1 + torch.exp(x_t[:, -1:] + x_t[:, :-1].sum(dim=1, keepdim=True)))
    with pytest.raises(NotImplementedError):
        MLP(Callback(21)).uz_solve(3, 3, xt, return_stderr=True)


def test_c_entry_refusals_through_ctypes():
    import torch
    from scasml_gp_amd import _lib, tables
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    lib = _lib.load()
    eng = MLP(Grad_Dependent_Nonlinear(21))._engine
    prob = eng.problem()
    good, one_sample = eng.plan(3, 3), eng.plan(2, 2)
    x = torch.from_numpy(_points(20, 4, 5).astype(np.float32)).cuda()
    out = torch.zeros((4, 21), dtype=torch.float32, device="cuda")
    se = torch.zeros((4,), dtype=torch.float32, device="cuda")
    pts = torch.zeros((4 * int(lib.scasml_points_per_root(C.byref(good))), 32), dtype=torch.float32, device="cuda")

    def call(plan, mode, world, se_ptr, points=None):
        rng = _lib.Rng(0, 0, 0, 0, world, 0, 0, None, None)
        return lib.scasml_picard_tree_stderr(C.byref(prob), C.byref(plan), mode, _lib.ptr(x), 4, 0, rng, _lib.ptr(points), None, _lib.ptr(out), None, se_ptr, None)
    ERR_ARG, ERR_UNSUPPORTED = -1, -2                       # include/scasml_hip.h
    assert call(good, _lib.MODE_MLP, 2, _lib.ptr(se)) == ERR_UNSUPPORTED and b"world" in lib.scasml_last_error()
    assert call(one_sample, _lib.MODE_MLP, 1, _lib.ptr(se)) == ERR_UNSUPPORTED and b"term [2][1]" in lib.scasml_last_error()
    assert call(good, _lib.MODE_GENERATE, 1, _lib.ptr(se), pts) == ERR_ARG and len(lib.scasml_last_error()) > 0
    assert call(good, _lib.MODE_MLP, 1, None) == ERR_ARG and b"out_se" in lib.scasml_last_error()
    flagged = _lib.Rng(0, 0, 0, 0, 1, _lib.RNG_COMPAT_CRN, 0, None, None)
    assert lib.scasml_picard_tree_stderr(C.byref(prob), C.byref(good), _lib.MODE_MLP, _lib.ptr(x), 4, 0, flagged, None, None, _lib.ptr(out), None,
                                         _lib.ptr(se), None) == ERR_UNSUPPORTED and b"flags" in lib.scasml_last_error()
    assert call(good, _lib.MODE_MLP, 1, _lib.ptr(se)) == 0
    torch.cuda.synchronize()
    assert bool((se > 0).all())
