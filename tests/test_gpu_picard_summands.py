"""The table of the root call's summands (``PicardEngine.solve(..., summands=...)``, scasml_picard_tree_summands in include/scasml_hip.h) and the
standard errors closed from it (``finalize_summands``, scasml_picard_summands_stderr): what a sample-sharded solve's error bars are made of.

Expected values are ``PicardOracle.root_summands(..., with_z=True)``: ONE float64 walk of the tree on bit-identical normals that records every
summand of (u, z) -- the CPU statement of the table, computed once per case (``_reference``) and shared, unchanged, by the tests.

Bounds.  An entry of the table is a rank's partial sum under an owner mask, which tests/test_gpu_picard_sweep.py already holds to
ATOL + RTOL |value|: here |Y - Y_or| <= ATOL + RTOL max(|Y_or|, |u_unclipped|), with the (ATOL, RTOL) of tests/test_gpu_picard_stderr.py (2e-5 / 1e-4
for MLP, 5e-5 / 2e-4 with a surrogate).  A standard error is held to that file's ``_check`` bound, 2 (ATOL + RTOL max(|unclipped value|, se_or)),
by its derivation (the error of se is at most sqrt(N / (N - 1)) <= sqrt(2) times the summed errors of the summands); the world - 1 extra
float32 roundings of a sharded summand (2^-24 relative each) are far inside it.  No comparison may pass vacuously: the median oracle se is at
least ten times the bound.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_picard_stderr import MLP_TOL, SCASML_TOL, _mlp, _points, _same_bits, _scasml, _scasml_points, _solve

pytestmark = pytest.mark.gpu

QUAD = [(7, 2, 4, 9), (20, 3, 3, 8), (100, 3, 3, 4), (250, 2, 3, 3), (20, 4, 4, 2)]        # lane groups 4, 8, 32, 64; the deep unit
FH = [(11, 2, 2, 7), (12, 5, 2, 3)]
MLP_CASES = [("quad", 0) + c for c in QUAD] + [("fh", 0) + c for c in FH] + [("quad", 1, 20, 3, 3, 6), ("fh", 2, 20, 3, 2, 6)]
SCASML_CASES = [("quad", 2, 3, 12), ("quad", 3, 3, 6), ("fh", 2, 3, 10)]
WORLDS = (2, 3, 8)

_REF = {}


def _mlp_case(variant, eq_id, d, n, par, B):
    """(solver, x_t, tolerance, oracle summands (S, B, 1 + d) float64, counts per term) of an MLP / MLP_full_history case."""
    key = ("mlp", variant, eq_id, d, n, par, B)
    pair = None
    if eq_id:
        from oracle.equation import CubicReactionDiffusion, QuadraticGradientReactionDiffusion
        from scasml_gp_amd.equations.equations import Cubic_Reaction_Diffusion, Quadratic_Gradient_Reaction_Diffusion
        pair = {1: (Cubic_Reaction_Diffusion, CubicReactionDiffusion), 2: (Quadratic_Gradient_Reaction_Diffusion, QuadraticGradientReactionDiffusion)}[eq_id]
    hip, ora = _mlp(d, variant, seed=3 if variant == "quad" else 11, eq_pair=pair)
    xt = _points(d, B, (10 if variant == "quad" else 20) + d)
    return (hip, xt, MLP_TOL) + _reference(key, ora, n, par, xt)


def _scasml_case(variant, n, par, B):
    hip, ora = _scasml(variant, seed=7)
    xt = _scasml_points(20, B, 30)
    return (hip, xt, SCASML_TOL) + _reference(("scasml", variant, n, par, B), ora, n, par, xt)


def _reference(key, ora, n, par, xt):
    if key not in _REF:
        Y = ora.root_summands(n, par, xt, with_z=True)
        table = np.concatenate(Y, axis=0)
        table.setflags(write=False)
        _REF[key] = (table, tuple(y.shape[0] for y in Y))
    return _REF[key]


def _se_of(table, counts):
    """The header's definition on a float64 table: sum over terms of N / (N - 1) sum_m (Y_m - mean)^2, per column; sqrt."""
    var, j = np.zeros(table.shape[1:]), 0
    with np.errstate(invalid="ignore", over="ignore"):
        for N in counts:
            Y = table[j:j + N]
            var += N / (N - 1.0) * ((Y - Y.mean(axis=0)) ** 2).sum(axis=0)
            j += N
        return np.sqrt(var)


def _check_table(got, want, tol, what):
    """Every entry inside ATOL + RTOL max(|Y_or|, |u_unclipped|); where the oracle's entry is not finite (every z of a quadrature solve at
    n >= 4, whose level-0 rule has nodes that are not increasing: SURVEY.md Appendix B) the kernel's is not finite either."""
    got = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.all(fin[:, :, 0]) and not np.any(np.isfinite(got[~fin]))
    u = want[:, :, 0].sum(axis=0)                                             # the unclipped u of every root
    bound = (tol[0] + tol[1] * np.maximum(np.abs(np.where(fin, want, 0.0)), np.abs(u)[None, :, None]))[fin]
    dev = np.abs(got[fin] - want[fin])
    print("summands %s: %d x %d x %d, max |dev| %.3e, max dev/bound %.4f" % ((what,) + want.shape + (dev.max(), (dev / bound).max())))
    assert np.all(dev <= bound), (what, dev.max(), (dev / bound).max())
    du = np.abs(got[:, :, 0].sum(axis=0) - u)                                # column 0 over the summands: the unclipped u
    assert np.all(du <= tol[0] + tol[1] * np.abs(u)), (what, du.max())


def _check_se(got, want_table, counts, tol, what):
    """tests/test_gpu_picard_stderr.py's _check, per column: inside 2 (ATOL + RTOL max(|unclipped value|, se_or)) wherever the oracle's value
    is finite, not finite where it is not, and not vacuously."""
    got = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got, dtype=np.float64)
    ncol = got.shape[1]
    want, val = _se_of(want_table, counts)[:, :ncol], want_table.sum(axis=0)[:, :ncol]
    fin = np.isfinite(want) & np.isfinite(val)
    assert got.shape == want.shape and np.all(fin[:, 0]) and not np.any(np.isfinite(got[~fin]))
    bound = 2.0 * (tol[0] + tol[1] * np.maximum(np.abs(val[fin]), want[fin]))
    dev = np.abs(got[fin] - want[fin])
    bound_u = 2.0 * (tol[0] + tol[1] * np.maximum(np.abs(val[:, 0]), want[:, 0]))
    print("se %s: %d columns, se %.3e..%.3e, max |dev| %.3e, max dev/bound %.4f, median se/bound %.0f"
          % (what, ncol, want[fin].min(), want[fin].max(), dev.max(), (dev / bound).max(), np.median(want[fin] / bound)))
    assert np.median(want[:, 0]) >= 10.0 * bound_u.max() and np.median(want[fin] / bound) >= 10.0      # the comparison cannot pass vacuously
    assert np.all(dev <= bound), (what, dev.max(), (dev / bound).max())


def _tables(eng, n, par, xt, world, form="uz"):
    """The ranks' (partial uz, table) of one solve, launched in turn in this process under the engine's dealing (stream 0)."""
    got = [eng.solve(n, par, xt, rank=r, world=world, stream_id=0, summands=form) for r in range(world)]
    return [g[0] for g in got], [g[-1] for g in got]


def _total(tables):
    """The ranks' tables added one after another in float32, as a reduction adds them."""
    acc = tables[0].clone()
    for t in tables[1:]:
        acc += t
    return acc


# ---- 3. the table against the oracle, one rank ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,eq_id,d,n,par,B", MLP_CASES)
def test_mlp_table_matches_the_oracle_summands_and_uz_is_the_plain_call(variant, eq_id, d, n, par, B):
    hip, xt, tol, want, counts = _mlp_case(variant, eq_id, d, n, par, B)
    eng = hip._engine
    assert eng.root_summands(n, par) == want.shape[0] == sum(counts)
    plain = eng.solve(n, par, xt, stream_id=0)[0]
    uz, _, _, table = eng.solve(n, par, xt, stream_id=0, summands="uz")
    assert tuple(table.shape) == want.shape and table.is_cuda and str(table.dtype) == "torch.float32" and eng.calls == 0
    assert _same_bits(uz, plain)
    _check_table(table, want, tol, (variant, eq_id, d, n, par))
    uz1, _, _, table_u = eng.solve(n, par, xt, stream_id=0, summands="u")                  # the u-only kernels: column 0, bit for bit
    assert tuple(table_u.shape) == want.shape[:2] + (1,) and _same_bits(uz1, plain) and _same_bits(table_u, table[:, :, :1])


@pytest.mark.parametrize("variant,n,par,B", SCASML_CASES)
def test_scasml_table_matches_the_oracle_summands_and_chunking_changes_no_bit(variant, n, par, B, monkeypatch):
    import scasml_gp_amd.solvers._picard as P
    hip, xt, tol, want, counts = _scasml_case(variant, n, par, B)
    eng = hip._engine
    plain, uhat_plain, _ = eng.solve(n, par, xt, stream_id=0)
    uz, uhat, _, table = eng.solve(n, par, xt, stream_id=0, summands="uz")
    assert _same_bits(uz, plain) and _same_bits(uhat, uhat_plain)
    _check_table(table, want, tol, ("scasml", variant, n, par))
    table_u = eng.solve(n, par, xt, stream_id=0, summands="u")[-1]
    assert _same_bits(table_u, table[:, :, :1])
    ppr = int(P._lib.load().scasml_points_per_root(C.byref(eng.plan(n, par))))
    monkeypatch.setattr(P, "POINT_BUFFER_BYTES", ppr * 32 * 4 * 5)            # 5 roots per chunk: every chunk writes its slice through ldy
    uz5, uhat5, _, table5 = eng.solve(n, par, xt, stream_id=0, summands="uz")
    assert _same_bits(uz5, plain) and _same_bits(uhat5, uhat_plain) and _same_bits(table5, table)


# ---- 4. the ranks' tables add up --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,eq_id,d,n,par,B", MLP_CASES)
def test_mlp_rank_tables_add_up_to_the_oracle_summands(variant, eq_id, d, n, par, B):
    hip, xt, tol, want, counts = _mlp_case(variant, eq_id, d, n, par, B)
    eng = hip._engine
    for world in WORLDS:
        parts, tables = _tables(eng, n, par, xt, world)
        for r in range(world):
            assert _same_bits(parts[r], eng.solve(n, par, xt, rank=r, world=world, stream_id=0)[0]), (world, r)
        _check_table(_total(tables), want, tol, (variant, eq_id, d, n, par, "world %d" % world))


@pytest.mark.parametrize("variant,n,par,B", SCASML_CASES)
def test_scasml_rank_tables_add_up_to_the_oracle_summands(variant, n, par, B):
    hip, xt, tol, want, counts = _scasml_case(variant, n, par, B)
    eng = hip._engine
    for world in WORLDS:
        parts, tables = _tables(eng, n, par, xt, world)
        for r in range(world):
            assert _same_bits(parts[r], eng.solve(n, par, xt, rank=r, world=world, stream_id=0)[0]), (world, r)
        _check_table(_total(tables), want, tol, ("scasml", variant, n, par, "world %d" % world))


def _launch(eng, n, par, x, rank, world, owner, ncol, fill=None):
    """scasml_picard_tree_summands through ctypes in MLP mode under a given owner table (None: unit % world) -> (partial uz, table)."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    B, d = x.shape[0], x.shape[1] - 1
    S = eng.root_summands(n, par)
    out = torch.empty((B, d + 1), dtype=torch.float32, device="cuda")
    table = torch.empty((S, B, ncol), dtype=torch.float32, device="cuda") if fill is None else torch.full((S, B, ncol), fill, dtype=torch.float32, device="cuda")
    rng = _lib.Rng(eng.seed, 0, 0, rank, world, 0, 0, owner.data_ptr() if owner is not None else None, None)
    plan, prob = eng.plan(n, par), eng.problem()
    rc = lib.scasml_picard_tree_summands(C.byref(prob), C.byref(plan), _lib.MODE_MLP, _lib.ptr(x), B, 0, rng, None, None, _lib.ptr(out), None,
                                         _lib.ptr(table), ncol, 0, None)
    assert rc == 0, lib.scasml_last_error()
    torch.cuda.synchronize()
    return out, table


def _summand_units(counts, plan, n):
    """Units of every summand in the enumeration of scasml_plan_deal_units: a terminal sample is one unit, a path of level l its q (l = 0)
    or 2 q (l > 0) addends."""
    per = [1] + [int(plan.term[n][l].q) * (2 if l else 1) for l in range(n)]
    return [p for N, p in zip(counts, per) for _ in range(N)]


@pytest.mark.parametrize("variant,d,n,par,B", [("quad", 20, 3, 3, 8), ("fh", 11, 2, 2, 7)])
def test_round_robin_dealing_and_whole_summands_on_one_rank(variant, d, n, par, B):
    import torch
    hip, xt, tol, want, counts = _mlp_case(variant, 0, d, n, par, B)
    eng = hip._engine
    x = torch.from_numpy(xt.astype(np.float32)).cuda()
    x[1, :] = float("nan")                                                    # a NaN root: NaN summands on the rank that owns them
    one = _launch(eng, n, par, x, 0, 1, None, d + 1)[1].cpu().numpy()
    assert np.all(np.isnan(one[:counts[0], 1, :])) and np.all(np.isfinite(np.delete(one, 1, axis=1)))     # g of a NaN point: every terminal summand
    # owner = NULL: unit % world, which splits the addends of a path across ranks; a poisoned table shows that every entry is written
    got = [_launch(eng, n, par, x, r, 3, None, d + 1, fill=float("inf")) for r in range(3)]
    left = [np.argwhere(np.isinf(g[1].cpu().numpy()))[:6].tolist() for g in got]
    assert not any(left), "entries (summand, root, column) a rank left unwritten: %s" % left
    total = _total([g[1] for g in got]).cpu().numpy()
    assert np.array_equal(np.isnan(total), np.isnan(one))                     # NaN where the one-rank table has NaN, and nowhere else
    keep = np.arange(B) != 1
    _check_table(total[:, keep], want[:, keep], tol, (variant, "owner NULL, world 3"))
    # every summand whole on one rank: the other ranks hold exact zeros there, and the sum is the one-rank table as numbers
    units = _summand_units(counts, eng.plan(n, par), n)
    for world in (2, 3):
        rank_of = np.arange(len(units)) % world
        owner = torch.from_numpy(np.repeat(rank_of, units).astype(np.uint8)).cuda()
        tabs = [_launch(eng, n, par, x, r, world, owner, d + 1)[1].cpu().numpy() for r in range(world)]
        for r in range(world):
            assert np.all(tabs[r][rank_of != r] == 0.0), (world, r)
            assert np.array_equal(tabs[r][rank_of == r], one[rank_of == r], equal_nan=True), (world, r)
        assert np.array_equal(sum(tabs[1:], tabs[0]), one, equal_nan=True)


# ---- 5. end to end: the standard errors from the summed tables ------------------------------------------------------------------------
def _end_to_end(hip, variant, n, par, xt, tol, want, counts, what):
    eng = hip._engine
    unsharded = {}
    for form, flag in (("u", True), ("uz", "uz")):
        eng.calls = 0
        unsharded[form] = _solve(hip, variant, n, par, xt, return_stderr=flag)[1]
    for world in (1,) + WORLDS:
        for form in ("u", "uz"):
            table = _total(_tables(eng, n, par, xt, world, form)[1])
            se = eng.finalize_summands(table, n, par)
            assert tuple(se.shape) == (xt.shape[0], 1 if form == "u" else xt.shape[1]) and str(se.dtype) == "torch.float32"
            _check_se(se, want, counts, tol, what + (form, "world %d" % world))
            # against the fused, unsharded estimate under the same bound
            a, b = se.cpu().numpy().astype(np.float64), np.asarray(unsharded[form], dtype=np.float64)
            fin = np.isfinite(b)
            assert not np.any(np.isfinite(a[~fin]))
            val = want.sum(axis=0)[:, :a.shape[1]]
            with np.errstate(invalid="ignore"):
                ok = np.abs(a - b)[fin] <= 2.0 * (tol[0] + tol[1] * np.maximum(np.abs(val[fin]), b[fin]))
            assert np.all(ok), (what, form, world)


@pytest.mark.parametrize("variant,eq_id,d,n,par,B", MLP_CASES)
def test_mlp_stderr_from_summed_tables_matches_the_oracle_and_the_unsharded_estimate(variant, eq_id, d, n, par, B):
    hip, xt, tol, want, counts = _mlp_case(variant, eq_id, d, n, par, B)
    _end_to_end(hip, variant, n, par, xt, tol, want, counts, (variant, eq_id, d, n, par))


@pytest.mark.parametrize("variant,n,par,B", SCASML_CASES)
def test_scasml_stderr_from_summed_tables_matches_the_oracle_and_the_unsharded_estimate(variant, n, par, B):
    hip, xt, tol, want, counts = _scasml_case(variant, n, par, B)
    _end_to_end(hip, variant, n, par, xt, tol, want, counts, ("scasml", variant, n, par))


@pytest.mark.parametrize("variant,n,par", [("quad", 3, 3), ("fh", 2, 3)])
def test_terminal_time_rows_give_exactly_zero_and_nan_rows_nan_at_every_world(variant, n, par):
    hip, _ = _mlp(20, variant, seed=1)
    eng = hip._engine
    xt = _points(20, 12, 5)
    xt[::3, -1] = 0.5                                    # t = T: every sample of g coincides, every weight of a level term is 0
    xt[4, :] = np.nan
    rest = np.setdiff1d(np.arange(12), np.r_[np.arange(0, 12, 3), 4])
    for world in (1,) + WORLDS:
        for form in ("u", "uz"):
            se = eng.finalize_summands(_total(_tables(eng, n, par, xt, world, form)[1]), n, par).cpu().numpy()
            assert np.all(se[::3, 0] == 0.0), (world, form)
            assert np.all(np.isnan(se[4])), (world, form)
            assert np.all(np.isfinite(se[rest])) and np.all(se[rest] > 0.0)
            if form == "uz" and variant == "fh":         # the terminal scale is 1 / 0 (scasml_picard_tree_stderr_uz)
                assert not np.any(np.isfinite(se[::3, 1:]))
    # level 0: no summand, zeros; the empty batch
    uz0, _, _, t0 = eng.solve(0, par, xt, stream_id=0, summands="uz")
    assert tuple(t0.shape) == (0, 12, 21) and not uz0.cpu().numpy().any()
    assert not eng.finalize_summands(t0, 0, par).cpu().numpy().any()
    uze, _, _, te = eng.solve(n, par, xt[:0], stream_id=0, summands="u")
    assert tuple(uze.shape) == (0, 21) and tuple(te.shape) == (eng.root_summands(n, par), 0, 1)
    assert tuple(eng.finalize_summands(te, n, par).shape) == (0, 1)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_summands_refusals_come_before_a_counter_moves():
    import torch
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    xt = _points(20, 4, 5)
    eq = Grad_Dependent_Nonlinear(21)
    for kw in (dict(compat_crn=True), dict(compat_f16=True), dict(compat_rng="jax")):
        solver = MLP(eq, **kw)
        for world in (1, 2):
            with pytest.raises(_lib.ScasmlError):
                solver._engine.solve(3, 3, xt, rank=0, world=world, summands="u")
        assert solver._engine.calls == 0 and solver._engine.jax_splits == 0
    plain = MLP(eq)
    for n, rho in ((2, 2), (1, 2)):
        with pytest.raises(ValueError, match="no estimable variance"):
            plain._engine.solve(n, rho, xt, rank=1, world=2, summands="uz")
    with pytest.raises(ValueError):
        plain._engine.solve(3, 3, xt, summands="z")
    with pytest.raises(ValueError):
        plain._engine.solve(3, 3, xt, summands="u", stderr=True)
    with pytest.raises(_lib.ScasmlError):                                     # stderr= at world != 1 keeps raising
        plain._engine.solve(3, 3, xt, rank=0, world=2, stderr=True)
    assert plain._engine.calls == 0

    class Callback(Grad_Dependent_Nonlinear):
        eq_id = None
        torch_callbacks = True
        staged_stderr = True

        def f(self, x_t, u, z):
            return self.sigma() * u * z.sum(dim=1, keepdim=True)

        def g(self, x_t):
            return 1 - 1 / (1 + torch.exp(x_t[:, -1:] + x_t[:, :-1].sum(dim=1, keepdim=True)))
    staged = MLP(Callback(21))
    with pytest.raises(NotImplementedError):
        staged._engine.solve(3, 3, xt, summands="u")
    assert staged._engine.calls == 0


def test_c_entries_refuse_with_the_codes_of_the_fused_estimate_and_accept_a_world():
    import torch
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.MLP import MLP
    lib = _lib.load()
    eng = MLP(Grad_Dependent_Nonlinear(21))._engine
    prob = eng.problem()
    good, one_sample, level0 = eng.plan(3, 3), eng.plan(2, 2), eng.plan(0, 3)
    S = eng.root_summands(3, 3)
    x = torch.from_numpy(_points(20, 4, 5).astype(np.float32)).cuda()
    out = torch.full((4, 21), -1.0, dtype=torch.float32, device="cuda")
    y = torch.full((S, 4, 21), -1.0, dtype=torch.float32, device="cuda")
    se = torch.full((4, 21), -1.0, dtype=torch.float32, device="cuda")
    pts = torch.zeros((4 * int(lib.scasml_points_per_root(C.byref(good))), 32), dtype=torch.float32, device="cuda")
    keys = torch.zeros((64,), dtype=torch.int32, device="cuda")

    def call(plan, mode=_lib.MODE_MLP, world=1, flags=0, y_ptr=_lib.ptr(y), ncol=21, ldy=0, points=None, B=4):
        rng = _lib.Rng(0, 0, 0, 0, world, flags, 0, None, keys.data_ptr() if flags & _lib.RNG_JAX_STREAM else None)
        return lib.scasml_picard_tree_summands(C.byref(prob), C.byref(plan), mode, _lib.ptr(x), B, 0, rng, _lib.ptr(points), None, _lib.ptr(out), None,
                                               y_ptr, ncol, ldy, None)
    ERR_ARG, ERR_UNSUPPORTED = -1, -2                       # include/scasml_hip.h
    assert call(good, mode=_lib.MODE_GENERATE, points=pts) == ERR_ARG and b"mode" in lib.scasml_last_error()
    assert call(good, y_ptr=None) == ERR_ARG and b"out_y" in lib.scasml_last_error()
    for ncol in (0, 2, 20, 22):
        assert call(good, ncol=ncol) == ERR_ARG and b"ncol" in lib.scasml_last_error()
    assert call(good, ldy=3) == ERR_ARG and b"ldy" in lib.scasml_last_error()
    for flag in (_lib.RNG_COMPAT_CRN, _lib.RNG_COMPAT_F16, _lib.RNG_JAX_STREAM):
        assert call(good, flags=flag) == ERR_UNSUPPORTED and b"flags" in lib.scasml_last_error()
    assert call(one_sample) == ERR_UNSUPPORTED and b"term [2][1]" in lib.scasml_last_error()
    assert lib.scasml_picard_summands_stderr(C.byref(one_sample), _lib.ptr(y), 4, 0, 21, _lib.ptr(se), None) == ERR_UNSUPPORTED
    assert b"no estimable variance" in lib.scasml_last_error()
    assert lib.scasml_picard_summands_stderr(C.byref(good), None, 4, 0, 21, _lib.ptr(se), None) == ERR_ARG and b"y is null" in lib.scasml_last_error()
    assert lib.scasml_picard_summands_stderr(C.byref(good), _lib.ptr(y), 4, 0, 21, None, None) == ERR_ARG and b"out_se" in lib.scasml_last_error()
    assert lib.scasml_picard_summands_stderr(C.byref(good), _lib.ptr(y), 4, 3, 21, _lib.ptr(se), None) == ERR_ARG and b"ldy" in lib.scasml_last_error()
    assert call(good, B=0) == 0 and lib.scasml_picard_summands_stderr(C.byref(good), _lib.ptr(y), 0, 0, 21, _lib.ptr(se), None) == 0
    torch.cuda.synchronize()
    assert bool((y == -1.0).all()) and bool((out == -1.0).all()) and bool((se == -1.0).all())      # a refused call has written nothing
    assert call(level0) == 0                                # n = 0: zeros in out_uz, nothing else touched
    torch.cuda.synchronize()
    assert bool((out == 0.0).all()) and bool((y == -1.0).all())
    assert call(good, world=1, ncol=1) == 0                 # the u form writes the S x 4 x 1 table and no float beyond it
    torch.cuda.synchronize()
    assert bool((y.view(-1)[:S * 4] != -1.0).all()) and bool((y.view(-1)[S * 4:] == -1.0).all())
    assert call(good, world=2) == 0                         # the point: a sharded rank is accepted, and writes every entry
    torch.cuda.synchronize()
    assert bool((y != -1.0).all())
