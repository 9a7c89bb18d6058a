"""Every compiled K-step count of the three GP evaluation kernels against the float64 statements (oracle/gp_compat.py, oracle/gp.py).

Each kernel is a switch over KS = kp / 16 with kp = scasml_point_stride(d) = ceil((d + 4) / 16) * 16: sixteen instantiations, whose
launch geometry (workgroups per CU, waves per SIMD, LDS slots, prefetch) and register allocation change with KS.  The sweep takes, for
every KS, the smallest and the largest d that map to it (at the smallest the last real coordinate lies alone in the last K-step), plus
the reference's own sizes by name, and checks at each of them, with the bounds the other modules hold at a few d:

* the as-coded matrix-core kernel (scasml_gp_eval_compat_sites, entry rounding on; tests/test_gpu_compat_mfma.py): outputs and Laplacian
  to 2e-5 of the magnitude plus rounding flips, float16 outputs, every site form and a shuffled site list bitwise equal to the full form;
* its geometry forms (round16 bits 0 and 4): the factored sums in every site form, one plane within its stated approximation;
* the documented operators (scasml_gp_eval) in splits 22 (float32 and float16 collocation points), 3, 2 and 0, each called with its mode
  set explicitly, so that no demotion or fallback tests something else;
* both gradients (scasml_gp_gradient, scasml_gp_gradient_compat).

Every case also has ragged edges: collocation counts N = 0, 1, 31 mod 32 (some without boundary points), a batch whose last workgroup is
partly empty, and prefixes of 1, 31 and 33 rows that give the same bits on their own.  Coefficients are random of realistic size, not a fit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_compat_mfma import _magnitudes, _raw, _setup, _test_points

gpu = pytest.mark.gpu

# smallest and largest d of every KS (16 KS - 19 and 16 KS - 4; the documented operators start at d = 1, the as-coded form at d = 5), and the
# reference's sizes 20, 40, 60, 80, 100, 250 by name.  test_the_sweep_reaches_every_k_step_count_at_both_ends checks this list against the library.
D_SWEEP = [1, 5, 12, 13, 20, 28, 29, 40, 44, 45, 60, 61, 76, 77, 80, 92, 93, 100, 108, 109, 124, 125, 140, 141, 156, 157, 172, 173, 188,
           189, 204, 205, 220, 221, 236, 237, 250, 252]
AS_CODED_MIN_D = 5          # five Hutchinson indices (models/GP.py:30)
NAMED_D = (20, 40, 60, 80, 100, 250)
AS_CODED_D = [d for d in D_SWEEP if d >= AS_CODED_MIN_D]
# (n_dom, n_bdy), dealt round the sweep: N = n_dom + n_bdy is 0, 1 or 31 mod 32, with and without boundary points, and a tile that holds
# domain and boundary rows together
COLLOC = [(100, 28), (70, 27), (40, 23), (64, 0), (33, 0), (95, 0), (31, 33)]
N_INF = 4 * 128 + 33        # the last workgroup of every kernel's launch is partly empty
PREFIXES = (1, 31, 33)


def _ks(d):
    return -(-(d + 4) // 16)


def _ids(ds):
    return ["ks%02d-d%d" % (_ks(d), d) for d in ds]


def _colloc(d):
    return COLLOC[D_SWEEP.index(d) % len(COLLOC)]


def _hutch(d):
    """Five distinct Hutchinson indices that include 0 and d - 1: the last K-step feeds the Laplacian too."""
    mid = np.random.default_rng(d).choice(np.arange(1, d - 1), 3, replace=False)
    return [d - 1, int(mid[0]), 0, int(mid[1]), int(mid[2])]


def test_the_sweep_reaches_every_k_step_count_at_both_ends():
    """The sweep against the library's own point stride: all sixteen KS, both ends of each within the kernels' d range, the named sizes."""
    from scasml_gp_amd import _lib
    lib = _lib.load()
    stride = lambda d: int(lib.scasml_point_stride(d))
    for lo, sweep in ((1, D_SWEEP), (AS_CODED_MIN_D, AS_CODED_D)):
        assert sorted({stride(d) // 16 for d in sweep}) == list(range(1, 17))
        for ks in range(1, 17):
            d_min, d_max = max(16 * ks - 19, lo), min(16 * ks - 4, _lib.MAX_DIM)
            assert stride(d_min) == stride(d_max) == 16 * ks
            assert d_min == lo or stride(d_min - 1) == 16 * (ks - 1)
            assert d_max == _lib.MAX_DIM or stride(d_max + 1) == 16 * (ks + 1)
            assert d_min in sweep and d_max in sweep, (ks, d_min, d_max)
        assert set(NAMED_D) <= set(sweep)
    assert all(_ks(d) == stride(d) // 16 for d in D_SWEEP)
    assert {(nd + nb) % 32 for nd, nb in COLLOC} == {0, 1, 31} and any(nb == 0 for _, nb in COLLOC)


def _flip(ogp, X, mag):
    """a rounding decided on float32 here and on float64 there moves one term by 2^-11 of itself: a few of the largest per point"""
    return {op: 4 * 2.0 ** -11 * (np.abs(ogp._features(op, X)) * np.abs(ogp.right_vector)[:, 0][None, :]).max(1) for op in mag}


def _prefixes_are_bitwise(run, X):
    whole = run(X)
    for n in PREFIXES:
        part = run(X[:n])
        assert all(np.array_equal(p, w[:n]) for p, w in zip(part, whole)), n


# ---------------------------------------------------------------------------------------------------- the as-coded matrix-core kernel
@gpu
@pytest.mark.parametrize("d", AS_CODED_D, ids=_ids(AS_CODED_D))
def test_as_coded_rounded_entries_match_the_float64_statement(d):
    nd, nb = _colloc(d)
    gp, ogp, _ = _setup(d, _hutch(d), nd, nb, seed=d, round16=True)
    X = _test_points(d, N_INF, seed=d + 1)
    out4, lap = _raw(gp, X, round16=1)
    ogp.round_out = False
    mag = _magnitudes(ogp, X)
    flip = _flip(ogp, X, mag)
    dt, div, lp = ogp.pde_parts(X)
    err_rounded = np.abs(out4[:, 0] - ogp.predict(X)[:, 0])
    assert np.all(err_rounded <= 2e-5 * mag["I"] + flip["I"])
    assert np.all(np.abs(out4[:, 3] - dt[:, 0]) <= 2e-5 * mag["dt"] + flip["dt"])
    assert np.all(np.abs(out4[:, 1] - div[:, 0]) <= 2e-5 * mag["div"] + flip["div"])
    assert np.all(np.abs(lap - lp[:, 0]) <= 2e-5 * mag["lap"] + flip["lap"])
    # the rounding is there at all (the R16 instantiation ran): the unrounded statement is much further away
    ogp.round16 = False
    assert np.abs(out4[:, 0] - ogp.predict(X)[:, 0]).mean() > 3 * err_rounded.mean()
    # float16 outputs (bit 1)
    out4r, _ = _raw(gp, X, round16=3)
    assert np.array_equal(out4r[:, 0].astype(np.float16).astype(np.float64), out4r[:, 0])
    assert np.array_equal(out4r[:, 2].astype(np.float16).astype(np.float64), out4r[:, 2])
    assert np.all(np.abs(out4r[:, 0] - out4[:, 0]) <= 2.0 ** -11 * np.abs(out4[:, 0]) + 1e-7)
    _prefixes_are_bitwise(lambda x: _raw(gp, x, round16=3), X)


def _site_list(gp, X, round16, kinds, rows, order):
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    pts = gp._points_device(X)[0]
    kd = torch.from_numpy(np.asarray(kinds, dtype=np.uint8)).cuda()
    od = torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda()
    out4 = torch.full((pts.shape[0], 4), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.scasml_gp_eval_compat_site_list(
        gp.d, 1.0 / float(gp.sigma) ** 2, float(gp.equation.sigma()), float(gp.equation.mu()), int(gp.equation.eq_id), _lib.ptr(gp._compat_model),
        gp.N_domain, gp.N_boundary, gp.laplacian_idx.ctypes.data_as(C.c_void_p), round16, 0.0, _lib.ptr(pts), pts.shape[0], rows,
        _lib.ptr(kd), _lib.ptr(od), len(order), _lib.ptr(out4), None, _lib.stream_ptr()), "gp_eval_compat_site_list")
    return out4.cpu().numpy().astype(np.float64)


def _consumed_bits_agree(got, full, k, where):
    """what a site of kind k consumes has the bits of the full form: u_hat always, div u_hat for kinds 0 and 4, everything for kind 0"""
    assert np.array_equal(got[:, 0], full[:, 0]), where
    if k in (0, 4):
        assert np.array_equal(got[:, 1], full[:, 1]), where
    if k == 0:
        assert np.array_equal(got, full), where


@gpu
@pytest.mark.parametrize("d", AS_CODED_D, ids=_ids(AS_CODED_D))
def test_as_coded_site_forms_and_site_list_give_the_full_forms_bits(d):
    nd, nb = _colloc(d)
    gp, _, _ = _setup(d, _hutch(d), nd, nb, seed=d + 2)
    X = _test_points(d, N_INF, seed=d + 3)
    full, _ = _raw(gp, X, round16=3)
    # one workgroup per 128-row site, so each form runs on its own; the last site is partly filled
    rows, kinds = 128, [1, 4, 2, 0, 3]
    part, _ = _raw(gp, X, round16=3, kinds=kinds, rows_per_site=rows)
    for s, k in enumerate(kinds):
        sl = slice(s * rows, (s + 1) * rows)
        if k == 2:                                        # another rank's site: untouched
            assert not part[sl].any()
        else:
            _consumed_bits_agree(part[sl], full[sl], k, (s, k))
    # 32-row sites listed in shuffled order: a workgroup gathers sites that are neighbours in the list only
    n_sites = (N_INF // 32)
    kinds32 = [(0, 1, 3, 4, 2)[s % 5] for s in range(n_sites)]
    listed = [s for s, k in enumerate(kinds32) if k != 2]
    order = list(np.random.default_rng(d).permutation(listed))
    got = _site_list(gp, X[:32 * n_sites], 3, kinds32, 32, order)
    for s, k in enumerate(kinds32):
        sl = slice(s * 32, (s + 1) * 32)
        if k == 2:
            assert (got[sl] == -7.0).all(), s             # not listed: not written
        else:
            _consumed_bits_agree(got[sl], full[sl], k, (s, k))


# ---------------------------------------------------------------------------------------------------- its geometry forms
@gpu
@pytest.mark.parametrize("d", AS_CODED_D, ids=_ids(AS_CODED_D))
def test_geometry_forms_match_the_float64_statement(d):
    """round16 bit 0 off (factored epilogue), two point planes (bit 4 off) and one: tests/test_gpu_compat_mfma.py's bounds, in every site form."""
    nd, nb = _colloc(d)
    gp, ogp, _ = _setup(d, _hutch(d), nd, nb, seed=d + 4, round16=False)
    rows, kinds = 128, [1, 4, 0, 3, 0]
    X = _test_points(d, N_INF, seed=d + 5, spread=0.7)
    mag = _magnitudes(ogp, X)
    dt, div, lp = ogp.pde_parts(X)
    u = ogp.predict(X)[:, 0]
    a = 1.0 / float(gp.sigma) ** 2
    ycol = np.concatenate([ogp.x_t_domain, ogp.x_t_boundary])
    # one plane: the point enters x.y rounded to float16: |delta Lambda| <= 1.45 a 2^-12 sum_k |x_k y_k| per pair, relative in kappa
    loose = 1.0 * a * 2.0 ** -12 * float((np.abs(X).astype(np.float64) @ np.abs(ycol).T).max())
    for bits in (0, 4):
        tol = 2e-5 + (0.0 if bits == 0 else loose)
        full, lap = _raw(gp, X, round16=bits)
        part, _ = _raw(gp, X, round16=bits, kinds=kinds, rows_per_site=rows)
        assert np.all(np.abs(full[:, 0] - u) <= tol * mag["I"]), bits
        assert np.all(np.abs(full[:, 3] - dt[:, 0]) <= tol * mag["dt"]), bits
        assert np.all(np.abs(full[:, 1] - div[:, 0]) <= tol * mag["div"]), bits
        assert np.all(np.abs(lap - lp[:, 0]) <= tol * mag["lap"]), bits
        if bits == 0:                                     # tests/test_gpu_compat_mfma.py: formulas without rounding
            eps = ogp.compute_PDE_loss(X)[:, 0]
            s2 = ogp.sigma_eq ** 2
            assert np.all(np.abs(full[:, 2] - eps) <= 2e-5 * (mag["dt"] + (abs(ogp.eq.mu()) + s2) * mag["div"] + 0.5 * s2 * mag["lap"] + mag["I"]))
        for s, k in enumerate(kinds):
            sl = slice(s * rows, (s + 1) * rows)
            assert np.all(np.abs(part[sl, 0] - u[sl]) <= tol * mag["I"][sl]), (bits, s, k)
            if k in (0, 4):
                assert np.all(np.abs(part[sl, 1] - div[sl, 0]) <= tol * mag["div"][sl]), (bits, s, k)
            if k == 0:
                assert np.all(np.abs(part[sl, 3] - dt[sl, 0]) <= tol * mag["dt"][sl]), (bits, s, k)
    two, _ = _raw(gp, X, round16=0)
    one, _ = _raw(gp, X, round16=4)
    assert np.all(np.abs(one[:, 0] - two[:, 0]) <= loose * mag["I"] + 1e-6)
    assert np.abs(one[:, 0] - two[:, 0]).max() > 0.0
    for bits in (2, 6):
        _prefixes_are_bitwise(lambda x: _raw(gp, x, round16=bits), X)


# ---------------------------------------------------------------------------------------------------- the documented operators
# split -> bound on u_hat, relative to sum_j |kappa_j c_j| (tests/test_gpu_gp.py: test_evaluation_arithmetic_modes_agree for float32
# collocation points, test_fused_evaluation_and_gradient_match_oracle for float16 ones), and on the derivative rows relative to that times
# (1 + a (1 + d)); split 2 (two truncated bf16 planes, ~2^-16 per product) keeps its own looser bound
DOC_MODES = {"split22": (22, False, 4e-6, 2e-5), "split22-f16colloc": (22, True, 2e-5, 2e-5), "split3": (3, False, 2e-6, 2e-5),
             "split2": (2, False, 1e-4, 1e-4), "split0": (0, False, 2e-6, 2e-5)}
DOC_CASES = [(d, mode) for d in D_SWEEP for mode in DOC_MODES]


@functools.lru_cache(maxsize=2)
def _doc_setup(d, f16_colloc):
    from oracle.equation import GradDependentNonlinear, sample_points
    from oracle.gp import OracleGP
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    nd, nb = _colloc(d)
    dom, bdy = sample_points(np.random.default_rng(d + 6), d, nd, nb)
    if f16_colloc:
        dom, bdy = dom.astype(np.float16).astype(np.float32), bdy.astype(np.float16).astype(np.float32)
    gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)
    ora = OracleGP(GradDependentNonlinear(d + 1))
    M = 4 * nd + nb
    rv = np.random.default_rng(d + 7).normal(size=M) * np.concatenate([np.full(nd, 1.0), np.full(nb, 1.0), np.full(nd, 0.05), np.full(nd, 0.3),
                                                                        np.full(nd, 0.3)])
    ora.x_t_domain, ora.x_t_boundary = dom.astype(np.float64), bdy.astype(np.float64)
    ora.N_domain, ora.N_boundary, ora.phi_dim = nd, nb, M
    ora.right_vector = rv[:, None]
    gp.load_right_vector(dom, bdy, rv)
    assert gp._colloc_is_f16 == f16_colloc
    X = np.random.default_rng(d + 8).uniform(-0.6, 0.6, (N_INF, d + 1)).astype(np.float32)
    X[:, -1] = np.abs(X[:, -1])
    mag = (np.abs(ora._features("I", X)) @ np.abs(ora.right_vector))[:, 0] + 1e-3
    want = dict(zip(("dt", "div", "lap"), (v[:, 0] for v in ora.pde_parts(X))), u=ora.predict(X)[:, 0], eps=ora.compute_PDE_loss(X)[:, 0])
    return gp, ora, X, mag, want


@functools.lru_cache(maxsize=2)
def _doc_lap_magnitude(d, f16_colloc):
    """What a rounding error of the Laplacian is relative to: the absolute values of the terms its epilogue adds (gp_eval.hip:10-15),
    sum_j kappa (|L| |E|_abs + 2 a (|cL| (2 |L| + a d) + |cS s|)) with |L| = a^2 rho^2 + a d and |E|_abs = |c0| + |cL| |L| + |ct p| + |cS s|."""
    _, ora, X, _, _ = _doc_setup(d, f16_colloc)
    a, N, Nb = ora.a, ora.N_domain, ora.N_boundary
    rv = np.abs(ora.right_vector[:, 0])
    c0, cb, cL, ct, cS = rv[:N], rv[N:N + Nb], rv[N + Nb:2 * N + Nb], rv[2 * N + Nb:3 * N + Nb], rv[3 * N + Nb:]
    kap, rho2, S, rt = ora._pairs(X, ora.x_t_domain)
    L, p, s = a * a * rho2 + a * d, np.abs(a * rt), np.abs(a * S)
    E = c0[None, :] + cL[None, :] * L + ct[None, :] * p + cS[None, :] * s
    magL = (kap * (L * E + 2 * a * (cL[None, :] * (2 * L + a * d) + cS[None, :] * s))).sum(1)
    if Nb:
        kap, rho2, _, _ = ora._pairs(X, ora.x_t_boundary)
        magL = magL + (kap * (a * a * rho2 + a * d) * cb[None, :]).sum(1)
    return magL


def _doc_raw(gp, X, split, f16_colloc):
    """(out4, lap) straight from scasml_gp_eval with the model's split set explicitly: the mode asked for is the mode that runs (the
    library refuses a split it cannot serve rather than demoting it)."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    m = gp._device_model()
    m.split = split
    assert m.split == split and m.colloc_is_f16 == int(f16_colloc) and m.x_bound == 0.0
    pts = gp._points_device(X)[0]
    out4 = torch.zeros((pts.shape[0], 4), dtype=torch.float32, device="cuda")
    lap = torch.zeros((pts.shape[0],), dtype=torch.float32, device="cuda")
    _lib.check(lib.scasml_gp_eval(C.byref(m), _lib.ptr(pts), pts.shape[0], _lib.ptr(out4), _lib.ptr(lap), _lib.stream_ptr()), "gp_eval")
    return out4.cpu().numpy().astype(np.float64), lap.cpu().numpy().astype(np.float64)


@gpu
@pytest.mark.parametrize("d,mode", DOC_CASES, ids=["ks%02d-d%d-%s" % (_ks(d), d, m) for d, m in DOC_CASES])
def test_documented_operators_match_the_float64_statement(d, mode):
    split, f16_colloc, tol_u, tol_p = DOC_MODES[mode]
    gp, ora, X, mag, want = _doc_setup(d, f16_colloc)
    out4, lap = _doc_raw(gp, X, split, f16_colloc)
    magp = mag * (1 + ora.a * (1 + d))                    # derivative features carry factors of a, a d
    assert np.all(np.abs(out4[:, 0] - want["u"]) <= tol_u * mag), np.max(np.abs(out4[:, 0] - want["u"]) / mag)
    assert np.all(np.abs(out4[:, 1] - want["div"]) <= tol_p * magp)
    assert np.all(np.abs(out4[:, 2] - want["eps"]) <= tol_p * magp)
    assert np.all(np.abs(out4[:, 3] - want["dt"]) <= tol_p * magp)
    magL = _doc_lap_magnitude(d, f16_colloc)
    assert np.all(np.abs(lap - want["lap"]) <= tol_p * magL), np.max(np.abs(lap - want["lap"]) / magL)
    _prefixes_are_bitwise(lambda x: _doc_raw(gp, x, split, f16_colloc), X)


# ---------------------------------------------------------------------------------------------------- gradients
@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_gradients_match_the_float64_statement(d):
    """scasml_gp_gradient (LDS of 4 (kp + 64) floats) and, from d = 5, scasml_gp_gradient_compat: tests/test_gpu_gp.py's and
    tests/test_gpu_compat_mfma.py's bounds."""
    gp, ora, X, mag, _ = _doc_setup(d, False)
    magp = mag * (1 + ora.a * (1 + d))
    g = gp.compute_gradient(X).astype(np.float64)
    assert g.shape == (N_INF, d + 1)
    assert np.all(np.abs(g - ora.compute_gradient(X)) <= 2e-5 * magp[:, None])
    out4, _ = _doc_raw(gp, X, 22, False)
    assert np.all(np.abs(g[:, :-1].sum(1) - out4[:, 1]) <= 4e-5 * magp * np.sqrt(d))
    _prefixes_are_bitwise(lambda x: (gp.compute_gradient(x),), X)
    if d < AS_CODED_MIN_D:
        return
    nd, nb = _colloc(d)
    gpc, ogp, _ = _setup(d, _hutch(d), nd, nb, seed=d + 9)
    Xc = _test_points(d, N_INF, seed=d + 10)
    got = gpc.compute_gradient(Xc).astype(np.float64)
    want = ogp.compute_gradient(Xc)
    assert np.array_equal(got, got.astype(np.float16).astype(np.float64))
    assert np.all(np.abs(got - want) <= 2.0 ** -10 * np.abs(want) + 1e-6)
    out4c, _ = _raw(gpc, Xc, round16=1)
    magc = _magnitudes(ogp, Xc)
    assert np.all(np.abs(got[:, :d].sum(1) - out4c[:, 1]) <= 2.0 ** -9 * magc["div"])
    assert np.all(np.abs(got[:, d] - out4c[:, 3]) <= 2.0 ** -9 * magc["dt"])
    _prefixes_are_bitwise(lambda x: (gpc.compute_gradient(x),), Xc)
