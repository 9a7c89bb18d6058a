"""Monte-Carlo standard errors of the Picard solvers' u AND z (``return_stderr="uz"``, scasml_picard_tree_stderr_uz in include/scasml_hip.h).

Expected values come from the unchanged CPU oracle on bit-identical normals, as in tests/test_gpu_picard_stderr.py: with ONE summand's
units marked 0 and every other unit 1, ``PicardOracle.uz_solve(..., rank=0, world=2, owner=owner)`` returns that summand's unclipped
contribution to (u, z_1 .. z_d) in float64, and the formula of the header -- Var = sum over terms of N / (N - 1) sum_m (Y_m - mean)^2,
component by component -- is applied to all 1 + d columns.

Tolerance per component: |se - se_oracle| <= 2 (ATOL + RTOL max(|unclipped value|, se_oracle)) with the project's ATOL / RTOL (2e-5 / 1e-4
for MLP, 5e-5 / 2e-4 for ScaSML).  Every case asserts that no component passes vacuously: its oracle se is at least ten times its bound.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_picard_stderr import MLP_TOL, SCASML_TOL, _groups, _mlp, _points, _same_bits, _scasml, _scasml_points, _solve

pytestmark = pytest.mark.gpu


def _oracle_se_uz(ora, variant, n, par, xt):
    """(se, unclipped value), each (B, 1 + d) float64, from the oracle's own summands."""
    import oracle.mlp as O
    groups, units = _groups(variant, n, par)
    var = np.zeros((xt.shape[0], xt.shape[1]))
    total = np.zeros_like(var)
    # the oracle's normals are a pure function of (seed, stream, roots, site, d) and its tables one of (par, T): the same arrays are handed
    # back instead of being computed once per summand; the oracle's code runs unchanged (tests/test_gpu_picard_stderr.py)
    draw, memo = O.philox.normals, {}

    def normals(seed, stream, roots, site, d):
        key = (int(seed), int(stream), roots.tobytes(), int(site), int(d))
        if key not in memo:
            memo[key] = draw(seed, stream, roots, site, d)
            memo[key].setflags(write=False)
        return memo[key]
    tables, tab_memo = O.approx_parameters, {}

    def approx_parameters(par_, T):
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
                Y.append(ora.uz_solve(n, par, xt, rank=0, world=2, owner=owner))
            Y = np.stack(Y)
            assert Y.shape == (N,) + var.shape
            total += Y.sum(axis=0)
            var += N / (N - 1.0) * ((Y - Y.mean(axis=0)) ** 2).sum(axis=0)
    finally:
        O.philox.normals, O.approx_parameters = draw, tables
    return np.sqrt(var), total


def _check(got, ora, variant, n, par, xt, tol):
    """Every component whose unclipped oracle value is finite: inside the tolerance, and not vacuously.  A component whose unclipped value
    is NOT finite has no number to compare with: its se must not be finite either (the header's rule).  That is every z of a quadrature
    solve at n >= 4, whose level-0 rule has q = 5 nodes that are not increasing (sqrt of a negative step: SURVEY.md Appendix B) -- there u,
    which is finite, is compared as everywhere; no other case may have such a component."""
    B, d = xt.shape[0], xt.shape[1] - 1
    assert got.shape == (B, d + 1) and got.dtype == np.float32
    want, val = _oracle_se_uz(ora, variant, n, par, xt)
    fin = np.isfinite(val) & np.isfinite(want)
    assert np.all(fin[:, 0]) and (np.all(fin) or (variant == "quad" and n >= 4 and not np.any(fin[:, 1:])))
    assert not np.any(np.isfinite(got[~fin]))
    want, val, got = want[fin], val[fin], got.astype(np.float64)[fin]
    bound = 2.0 * (tol[0] + tol[1] * np.maximum(np.abs(val), want))
    dev = np.abs(got - want)
    print("se_uz case %s n=%d par=%d d=%d B=%d: %d of %d components finite, se %.3e..%.3e (median %.3e), max |dev| %.3e, max dev/bound %.4f, min se/bound %.0f"
          % (variant, n, par, d, B, fin.sum(), fin.size, want.min(), want.max(), np.median(want), dev.max(), (dev / bound).max(), (want / bound).min()))
    assert np.all(want >= 10.0 * bound), (want / bound).min()                  # no component can pass vacuously
    assert np.all(dev <= bound), (dev.max(), (dev / bound).max())


# ---- 1. expected values from the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,rho,B", [(7, 2, 4, 5), (20, 1, 3, 8), (20, 2, 3, 8), (43, 2, 3, 4), (100, 3, 3, 3), (250, 2, 3, 2), (20, 4, 4, 2)])
def test_mlp_quadrature_se_uz_matches_oracle_summands(d, n, rho, B):
    """Lane-group widths 4 (d = 7), 8 (d = 20), 16 with idle lanes (d = 43), 32 (d = 100) and 64 (d = 250); n = 4 runs the deep unit
    (its z, and so its se_z, is NaN: _check).  On an MI355X, over all cases of this file that compare with the oracle: largest share of the
    tolerance 0.0047 (d = 100, n = rho = 3), largest |se - se_oracle| 1.7e-5 at se up to 42 (d = 7); smallest se / bound 11."""
    hip, ora = _mlp(d, "quad", seed=3)
    xt = _points(d, B, 10 + d)
    uz, se = hip.uz_solve(n, rho, xt, return_stderr="uz")
    assert uz.shape == (B, d + 1)
    _check(se, ora, "quad", n, rho, xt, MLP_TOL)


@pytest.mark.parametrize("d,n,M,B", [(20, 2, 3, 8), (11, 2, 2, 7), (100, 3, 3, 3), (12, 5, 2, 3)])
def test_mlp_full_history_se_uz_matches_oracle_summands(d, n, M, B):
    hip, ora = _mlp(d, "fh", seed=11)
    xt = _points(d, B, 20 + d)
    _, se = hip.uz_solve(n, None, xt, M, return_stderr="uz")
    _check(se, ora, "fh", n, M, xt, MLP_TOL)


@pytest.mark.parametrize("eq_id,variant,d,n,par,B", [(1, "quad", 20, 3, 3, 4), (2, "fh", 20, 3, 2, 4)])
def test_se_uz_on_the_other_registered_equations(eq_id, variant, d, n, par, B):
    from oracle.equation import CubicReactionDiffusion, QuadraticGradientReactionDiffusion
    from scasml_gp_amd.equations.equations import Cubic_Reaction_Diffusion, Quadratic_Gradient_Reaction_Diffusion
    pair = {1: (Cubic_Reaction_Diffusion, CubicReactionDiffusion), 2: (Quadratic_Gradient_Reaction_Diffusion, QuadraticGradientReactionDiffusion)}[eq_id]
    hip, ora = _mlp(d, variant, seed=3, eq_pair=pair)
    assert hip.equation.eq_id == eq_id
    xt = _points(d, B, 11)
    _, se = _solve(hip, variant, n, par, xt, return_stderr="uz")
    _check(se, ora, variant, n, par, xt, MLP_TOL)


@pytest.mark.parametrize("variant,n,par,B", [("quad", 2, 3, 8), ("quad", 3, 3, 4), ("fh", 2, 3, 6)])
def test_scasml_se_uz_matches_oracle_summands(variant, n, par, B):
    """The 60 + 20 point surrogate of tests/test_gpu_scasml.py: the standard errors of the correction (u_breve, z_breve)."""
    hip, ora = _scasml(variant, seed=7)
    xt = _scasml_points(20, B, 30)
    _, se = _solve(hip, variant, n, par, xt, return_stderr="uz")
    _check(se, ora, variant, n, par, xt, SCASML_TOL)


# ---- 2. (u, z) is that of the plain call, column 0 that of return_stderr=True --------------------------------------------------------------
@pytest.mark.parametrize("variant,d,n,par,B", [("quad", 20, 3, 3, 37), ("quad", 100, 3, 3, 5), ("quad", 20, 4, 4, 3), ("fh", 20, 3, 3, 37), ("fh", 12, 5, 2, 3)])
def test_mlp_uz_and_se_u_are_bit_identical_to_the_plain_and_the_u_only_calls(variant, d, n, par, B):
    hip, _ = _mlp(d, variant, seed=5)
    xt = _points(d, B, 40)
    plain = _solve(hip, variant, n, par, xt)                                   # call 0
    count = hip.evaluation_counter
    hip._engine.calls = 0
    _, se_u = _solve(hip, variant, n, par, xt, return_stderr=True)             # call 0 again
    hip._engine.calls = 0
    uz, se = _solve(hip, variant, n, par, xt, return_stderr="uz")              # and again
    assert se.shape == (B, d + 1) and se.dtype == np.float32
    assert _same_bits(plain, uz) and _same_bits(se_u, se[:, 0:1])
    assert hip._engine.calls == 1 and hip.evaluation_counter == 3 * count and count > 0
    # mixing: the call after a "uz" call is on the stream a plain call would have left it
    after = _solve(hip, variant, n, par, xt)
    hip._engine.calls = 1
    assert _same_bits(after, _solve(hip, variant, n, par, xt)) and not _same_bits(after, plain)


@pytest.mark.parametrize("variant,n,par", [("quad", 3, 3), ("fh", 2, 3)])
def test_scasml_uz_and_se_u_are_bit_identical_and_chunking_changes_no_bit(variant, n, par, monkeypatch):
    import scasml_gp_amd.solvers._picard as P
    hip, _ = _scasml(variant, seed=7)
    xt = _scasml_points(20, 50, 41)
    plain = _solve(hip, variant, n, par, xt)
    count = hip.evaluation_counter
    hip._engine.calls = 0
    _, se_u = _solve(hip, variant, n, par, xt, return_stderr=True)
    hip._engine.calls = 0
    uz, se = _solve(hip, variant, n, par, xt, return_stderr="uz")
    assert se.shape == (50, 21) and se.dtype == np.float32
    assert _same_bits(plain, uz) and _same_bits(se_u, se[:, 0:1])
    assert hip._engine.calls == 1 and hip.evaluation_counter == 3 * count and count > 0
    ppr = int(P._lib.load().scasml_points_per_root(C.byref(hip._engine.plan(n, par))))
    monkeypatch.setattr(P, "POINT_BUFFER_BYTES", ppr * 32 * 4 * 7)             # 7 roots per chunk (point rows of d = 20 are 32 floats)
    hip._engine.calls = 0
    uz7, se7 = _solve(hip, variant, n, par, xt, return_stderr="uz")
    assert _same_bits(uz, uz7) and _same_bits(se, se7)


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,n,par", [("quad", 3, 3), ("fh", 2, 3)])
def test_terminal_time_and_nan_rows_level_zero_empty_batch_and_device_tensors(variant, n, par):
    import torch
    hip, _ = _mlp(20, variant, seed=1)
    xt = _points(20, 12, 5)
    xt[::3, -1] = 0.5                                    # t = T: every sample of g coincides, every weight of a level term is 0
    xt[4, :] = np.nan
    uz, se = _solve(hip, variant, n, par, xt, return_stderr="uz")
    assert se.shape == (12, 21) and se.dtype == np.float32
    assert np.all(se[::3, 0] == 0.0)
    if variant == "quad":                                # the terminal scale is 1 / (mg 1e-6): large and finite
        assert np.all(np.isfinite(se[::3, 1:])) and np.all(se[::3, 1:] > 0.0)
    else:                                                # the terminal scale is 1 / 0
        assert not np.any(np.isfinite(se[::3, 1:]))
    assert np.all(np.isnan(se[4]))
    rest = np.setdiff1d(np.arange(12), np.r_[np.arange(0, 12, 3), 4])
    assert np.all(np.isfinite(se[rest])) and np.all(se[rest] > 0.0)
    uz0, se0 = _solve(hip, variant, 0, par, xt, return_stderr="uz")
    assert np.array_equal(uz0, np.zeros((12, 21), dtype=np.float32)) and np.array_equal(se0, np.zeros((12, 21), dtype=np.float32))
    assert se0.dtype == np.float32
    uze, see = _solve(hip, variant, n, par, xt[:0], return_stderr="uz")
    assert uze.shape == (0, 21) and see.shape == (0, 21)
    xd = torch.from_numpy(xt.astype(np.float32)).cuda()
    hip._engine.calls = 0
    uzd, sed = _solve(hip, variant, n, par, xd, return_stderr="uz")
    assert isinstance(uzd, torch.Tensor) and isinstance(sed, torch.Tensor) and uzd.is_cuda and sed.is_cuda
    assert sed.dtype == torch.float32 and tuple(sed.shape) == (12, 21)
    assert _same_bits(sed, se) and _same_bits(uzd, uz)


# ---- 4. calibration on the device ----------------------------------------------------------------------------------------------------
def test_reported_se_z_is_calibrated_against_the_spread_of_replicates():
    """One point repeated 4096 times (the root index is a Philox counter word: the rows are independent replicates), with the clip raised
    to 100 so that the returned z is the unclipped one.  Pooled over the 20 components, sqrt(mean se_z^2) / sqrt(mean var(z_i)) must lie in
    the band the project uses for u, 0.9 .. 1.1; 1024 replicates of the CPU oracle gave 1.0035 (per component 0.936 .. 1.056) and no
    component on the clip.  On an MI355X: pooled 1.0005, per component 0.961 .. 1.028, largest |z| 32.2, median se_z 1.62."""
    hip, _ = _mlp(20, "quad", seed=2)
    hip.equation.norm_estimation = 100.0
    xt = np.repeat(_points(20, 1, 6), 4096, axis=0)
    uz, se = hip.uz_solve(2, 3, xt, return_stderr="uz")
    z, se_z = uz[:, 1:].astype(np.float64), se[:, 1:].astype(np.float64)
    assert np.abs(uz).max() < 100.0                      # no component on the clip: the spread below is that of the unclipped sum
    var_z = z.var(axis=0, ddof=1)
    per = np.sqrt((se_z ** 2).mean(axis=0) / var_z)
    ratio = float(np.sqrt((se_z ** 2).mean() / var_z.mean()))
    print("se_z calibration: pooled ratio %.4f, per component %.3f..%.3f, median se_z %.3f, max |z| %.2f" % (ratio, per.min(), per.max(), np.median(se_z), np.abs(z).max()))
    assert 0.9 <= ratio <= 1.1, ratio


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_u_only_estimate_holds_and_moves_nothing():
    import torch
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    hip, _ = _mlp(20, "quad", seed=1)
    xt = _points(20, 4, 5)
    for n, rho in ((2, 2), (1, 2)):
        with pytest.raises(ValueError, match="no estimable variance"):
            hip.uz_solve(n, rho, xt, return_stderr="uz")
    assert hip._engine.calls == 0 and hip.evaluation_counter == 0
    fh, _ = _mlp(20, "fh", seed=1)
    with pytest.raises(ValueError, match="no estimable variance"):
        fh.uz_solve(2, None, xt, 1, return_stderr="uz")
    assert fh._engine.calls == 0 and fh.evaluation_counter == 0
    eq = Grad_Dependent_Nonlinear(21)
    sharded = MLP(eq)
    with pytest.raises(_lib.ScasmlError):
        sharded._engine.solve(3, 3, xt, rank=0, world=2, stderr="uz")
    assert sharded._engine.calls == 0
    for kw in (dict(compat_crn=True), dict(compat_f16=True), dict(compat_rng="jax")):
        solver = MLP(eq, **kw)
        with pytest.raises(_lib.ScasmlError):
            solver.uz_solve(3, 3, xt, return_stderr="uz")
        assert solver._engine.calls == 0 and solver.evaluation_counter == 0

    class Callback(Grad_Dependent_Nonlinear):
        eq_id = None
        torch_callbacks = True

        def f(self, x_t, u, z):
            return self.sigma() * u * z.sum(dim=1, keepdim=True)

        def g(self, x_t):
            return 1 - 1 / (1 + torch.exp(x_t[:, -1:] + x_t[:, :-1].sum(dim=1, keepdim=True)))
    staged = MLP(Callback(21))
    with pytest.raises(NotImplementedError):
        staged.uz_solve(3, 3, xt, return_stderr="uz")
    assert staged._engine.calls == 0 and staged.evaluation_counter == 0


def test_c_entry_refuses_what_the_u_only_entry_refuses_with_the_same_codes():
    import torch
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    lib = _lib.load()
    eng = MLP(Grad_Dependent_Nonlinear(21))._engine
    prob = eng.problem()
    good, one_sample = eng.plan(3, 3), eng.plan(2, 2)
    x = torch.from_numpy(_points(20, 4, 5).astype(np.float32)).cuda()
    out = torch.zeros((4, 21), dtype=torch.float32, device="cuda")
    se = torch.zeros((4,), dtype=torch.float32, device="cuda")
    se_uz = torch.full((4, 21), -1.0, dtype=torch.float32, device="cuda")
    pts = torch.zeros((4 * int(lib.scasml_points_per_root(C.byref(good))), 32), dtype=torch.float32, device="cuda")
    keys = torch.zeros((64,), dtype=torch.int32, device="cuda")

    def both(plan, mode, world=1, flags=0, null_out=False, points=None):
        """(code of scasml_picard_tree_stderr, code of scasml_picard_tree_stderr_uz) for the same arguments."""
        rng = _lib.Rng(0, 0, 0, 0, world, flags, 0, None, keys.data_ptr() if flags & _lib.RNG_JAX_STREAM else None)
        args = (C.byref(prob), C.byref(plan), mode, _lib.ptr(x), 4, 0, rng, _lib.ptr(points), None, _lib.ptr(out), None)
        rc_u = lib.scasml_picard_tree_stderr(*args, None if null_out else _lib.ptr(se), None)
        rc_uz = lib.scasml_picard_tree_stderr_uz(*args, None if null_out else _lib.ptr(se_uz), None)
        assert len(lib.scasml_last_error()) > 0
        return rc_u, rc_uz
    ERR_ARG, ERR_UNSUPPORTED = -1, -2                       # include/scasml_hip.h
    assert both(good, _lib.MODE_MLP, null_out=True) == (ERR_ARG, ERR_ARG) and b"out_se_uz" in lib.scasml_last_error()
    assert both(good, _lib.MODE_GENERATE, points=pts) == (ERR_ARG, ERR_ARG)
    assert both(good, _lib.MODE_MLP, world=2) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED) and b"world" in lib.scasml_last_error()
    for flag in (_lib.RNG_COMPAT_CRN, _lib.RNG_COMPAT_F16, _lib.RNG_JAX_STREAM):
        assert both(good, _lib.MODE_MLP, flags=flag) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED) and b"flags" in lib.scasml_last_error()
    assert both(one_sample, _lib.MODE_MLP) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED) and b"term [2][1]" in lib.scasml_last_error()
    torch.cuda.synchronize()
    assert bool((se_uz == -1.0).all())                      # a refused call has written nothing
    rng = _lib.Rng(0, 0, 0, 0, 1, 0, 0, None, None)
    assert lib.scasml_picard_tree_stderr_uz(C.byref(prob), C.byref(good), _lib.MODE_MLP, _lib.ptr(x), 4, 0, rng, None, None, _lib.ptr(out), None,
                                            _lib.ptr(se_uz), None) == 0
    torch.cuda.synchronize()
    assert bool((se_uz > 0).all())
