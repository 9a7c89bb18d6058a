"""Pathwise GP posterior draws on the device: scasml_gp_rff_functionals and scasml_gp_rff_noise (csrc/gp_rff.hip), GP.sample_functions and
GPFunctionDraws against the NumPy statement of tests/_gp_rff_ref.py (features from oracle.philox, sums in np.longdouble, a dense float64 solve).

* The kernel: errors are counted in units of 2^-53 F^-1/2 sum_f |mult_f| (|wc_f| + |ws_f|) (1 + (d + 2) sum_k |omega_fk x_k|) of every output -- the
  scale of the sum times the absolute error with which theta enters the sine.  The ratios are asserted at 16 times the largest measured on the MI355X
  per shape (profiles/gp_rff_accuracy.json; the margin is for other points and other boxes), and that bound must itself stay under the a-priori
  2 (F + d + 8) units.
* Everything in which the device solves with K_p is asserted at the cap 256 cond(K_p) 2^-53 of the quantity's own scale (tests/_gp_evidence_ref.py).
* Statistics: six empirical standard errors on every entry of the sample mean and covariance at a fixed seed (MOMENT_SEED: the NumPy statement alone
  -- oracle normals, dense solve -- gives 1.98 and 2.98 standard errors there; seeds 0 .. 5 give 1.7 .. 2.7 and 3.0 .. 3.8)."""
import functools

import numpy as np
import pytest

import _gp_loo_ref as lref
import _gp_rff_ref as ref

pytestmark = pytest.mark.gpu

# (d, n, F, ld_x - (d + 1)): every edge of every axis once -- K = d + 1 = 2, 4, 32, 34, 101 (d = 31: wc and ws lie past the last 32-column stage),
# n = 1, 63, 65, 130 (three point tiles), F = 1, 63, 64, 65, 200 (four feature tiles, the last ragged) -- and (100, 130, 200) in full
KERNEL_CASES = [(1, 1, 1, 0), (3, 63, 63, 0), (31, 65, 64, 3), (33, 130, 65, 0), (100, 130, 200, 0), (1, 130, 200, 0), (100, 1, 1, 0), (3, 65, 64, 0)]
# 16 x the largest ratio measured on the MI355X at each case (profiles/gp_rff_accuracy.json), in the units above
KERNEL_BOUND = {(1, 1, 1): 16.0 * 0.2147, (3, 63, 63): 16.0 * 0.0696, (31, 65, 64): 16.0 * 0.0049, (33, 130, 65): 16.0 * 0.0061,
                (100, 130, 200): 16.0 * 0.0009, (1, 130, 200): 16.0 * 0.1019, (100, 1, 1): 16.0 * 0.0016, (3, 65, 64): 16.0 * 0.0533}
MOMENT_SEED = 3
bits = lambda a: np.ascontiguousarray(a).view(np.int64)


def _gp(d):
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    return GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)


def _a(d):
    return 1.0 / float(_gp(d).sigma) ** 2


def _rff(d, a, X, F, seed, sample0, S, ld_extra=0):
    """scasml_gp_rff_functionals on the rows of X (host float32), the rows laid out with leading dimension d + 1 + ld_extra: (S, n, 4) float64."""
    import torch
    from scasml_gp_amd import _lib
    n = X.shape[0]
    buf = torch.full((max(n, 1), d + 1 + ld_extra), 7.0, dtype=torch.float32, device="cuda")       # the padding holds a value that must not be read
    buf[:n, :d + 1] = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    out = torch.full((S, n, 4), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().scasml_gp_rff_functionals(d, a, _lib.ptr(buf), n, d + 1 + ld_extra, F, seed, sample0, S, _lib.ptr(out), _lib.stream_ptr()),
               "gp_rff_functionals")
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _kernel_points(d):
    X = lref.points(d, 130, 0)[0]
    return X


# ------------------------------------------------------------------------------------------------ 1. the kernel against the statement
@pytest.mark.parametrize("d,n,F,ld_extra", KERNEL_CASES)
def test_kernel_matches_the_statement(d, n, F, ld_extra):
    a, seed, sample0, S = _a(d), 0xF00D + d, 3, 2
    X = _kernel_points(d)[:n]
    got = _rff(d, a, X, F, seed, sample0, S, ld_extra)
    assert got.shape == (S, n, 4) and np.isfinite(got).all()
    worst = 0.0
    for s in range(S):
        want, unit = ref.functionals(d, a, F, seed, sample0 + s, X, with_unit=True)
        worst = max(worst, float((np.abs(got[s].astype(np.longdouble) - want) / unit).max()))
    print("gp_rff kernel d=%d n=%d F=%d ld_x=%d: largest error %.4f units" % (d, n, F, d + 1 + ld_extra, worst))
    bound = KERNEL_BOUND[(d, n, F)]
    assert bound <= 2.0 * (F + d + 8), "the measured bound left the a-priori one"
    assert worst <= bound


# ------------------------------------------------------------------------------------------------ 2. a point's values are a function of the point
def test_values_do_not_depend_on_where_the_point_stands():
    d, F, seed = 33, 200, 77
    a = _a(d)
    X = _kernel_points(d)
    full = _rff(d, a, X, F, seed, 5, 3)
    assert np.array_equal(bits(_rff(d, a, X[97:98], F, seed, 5, 3)), bits(full[:, 97:98]))         # alone; inside 130 points
    perm = np.random.default_rng(1).permutation(130)
    assert np.array_equal(bits(_rff(d, a, X[perm], F, seed, 5, 3)), bits(full[:, perm]))
    assert np.array_equal(bits(_rff(d, a, X, F, seed, 5, 3, ld_extra=5)), bits(full))
    for s in range(3):                                                                              # the split of the draws over calls
        assert np.array_equal(bits(_rff(d, a, X, F, seed, 5 + s, 1)), bits(full[s:s + 1]))
    assert not np.array_equal(bits(full[0]), bits(full[1]))


# ------------------------------------------------------------------------------------------------ 3. the noise
@pytest.mark.parametrize("M", [1, 5, 109])
def test_noise_is_the_oracles_normals(M):
    import torch
    from scasml_gp_amd import _lib
    seed, sample0, S, ld = 0xABCDEF0123, 2 ** 32 - 3, 3, M + 2
    out = torch.full((S, ld), 7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().scasml_gp_rff_noise(M, seed, sample0, S, _lib.ptr(out), ld, _lib.stream_ptr()), "gp_rff_noise")
    got = out.cpu().numpy()
    assert (got[:, M:] == 7.0).all()
    for s in range(S):
        assert np.array_equal(bits(got[s, :M]), bits(ref.noise(seed, sample0 + s, M)))


# ------------------------------------------------------------------------------------------------ 4. - 6. the class
CLASS_SHAPES = [(6, 20, 29), (3, 50, 20)]
CLASS_F, CLASS_S, CLASS_SEED, CLASS_SAMPLE0 = 65, 3, 0xC1A55, 4


@functools.lru_cache(maxsize=None)
def _case(d, nd, nb):
    """One shape's NumPy side and its loaded GP, computed once and left unchanged: points, z, K_p, cond, 33 off-collocation points and their cross rows."""
    from oracle.equation import sample_points
    dom, bdy = lref.points(d, nd, nb)
    gp = _gp(d)
    og = lref.oracle(d, float(gp.sigma))
    M = 4 * nd + nb
    z = lref.z_of(d, M)
    Kp = og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64)) + gp.nugget * np.eye(M)
    alpha = np.linalg.solve(Kp, z)
    gp.load_right_vector(dom, bdy, alpha)
    X = sample_points(np.random.default_rng(4242), d, 33, 1)[0]
    case = dict(d=d, nd=nd, nb=nb, M=M, dom=dom, bdy=bdy, gp=gp, og=og, z=z, Kp=Kp, alpha=alpha, X=X, rows=ref.cross_rows(og, X),
                cap=lref.cap(float(np.linalg.cond(Kp))))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _class_draws(d, nd, nb):
    c = _case(d, nd, nb)
    return c["gp"].sample_functions(CLASS_S, seed=CLASS_SEED, n_features=CLASS_F, sample0=CLASS_SAMPLE0, z=c["z"])


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("d,nd,nb", CLASS_SHAPES)
def test_class_matches_the_dense_statement(d, nd, nb):
    import torch
    c = _case(d, nd, nb)
    draws = _class_draws(d, nd, nb)
    assert c["gp"]._L_pad.shape[0] == (128 if (d, nd, nb) == (6, 20, 29) else 224)
    rv = draws.right_vectors
    assert isinstance(rv, torch.Tensor) and rv.is_cuda and rv.dtype == torch.float64 and tuple(rv.shape) == (CLASS_S, c["M"])
    pred, fun = draws.predict(c["X"]), draws.functionals(c["X"])
    assert isinstance(pred, np.ndarray) and pred.shape == (CLASS_S, 33) and pred.dtype == np.float64
    assert isinstance(fun, np.ndarray) and fun.shape == (CLASS_S, 33, 4) and fun.dtype == np.float64
    assert np.array_equal(bits(pred), bits(fun[:, :, 0]))
    for s in range(CLASS_S):
        want_rv, _, _, want = ref.posterior_draw(c["og"], c["Kp"], c["z"], c["gp"].nugget, CLASS_F, CLASS_SEED, CLASS_SAMPLE0 + s, c["X"], c["rows"])
        errs = [_rel(rv[s].cpu().numpy(), want_rv)] + [_rel(fun[s, :, k], want[:, k]) for k in range(4)]
        print("draw %d of (%d, %d, %d): rv, u, Lap, dt, div relative errors %s, cap %.3e" % (s, d, nd, nb, ["%.2e" % e for e in errs], c["cap"]))
        assert max(errs) <= c["cap"]
    # CUDA tensor in, CUDA tensor out; split and permuted points; the draws continued by sample0: the same bits
    xt = torch.from_numpy(c["X"].copy()).cuda()
    ft = draws.functionals(xt)
    assert isinstance(ft, torch.Tensor) and ft.is_cuda and np.array_equal(bits(ft.cpu().numpy()), bits(fun))
    perm = np.random.default_rng(2).permutation(33)
    assert np.array_equal(bits(draws.functionals(c["X"][perm])), bits(fun[:, perm]))
    assert np.array_equal(bits(np.concatenate([draws.predict(c["X"][:7]), draws.predict(c["X"][7:])], axis=1)), bits(pred))
    later = c["gp"].sample_functions(1, seed=CLASS_SEED, n_features=CLASS_F, sample0=CLASS_SAMPLE0 + 2, z=c["z"])
    assert np.array_equal(bits(later.predict(c["X"])), bits(pred[2:3]))
    cap_bytes = c["gp"].variance_buffer_bytes
    try:                                              # chunks of 5 points
        c["gp"].variance_buffer_bytes = 5 * 8 * c["gp"]._L_pad.shape[0]
        assert np.array_equal(bits(draws.functionals(c["X"])), bits(fun))
    finally:
        c["gp"].variance_buffer_bytes = cap_bytes


@pytest.mark.parametrize("d,nd,nb", CLASS_SHAPES)
def test_draws_interpolate_their_noisy_data(d, nd, nb):
    """K rv_s + phi_s = z - sqrt(eta) eps_s - eta rv_s: the draw's functionals at the collocation points, in the Gram's order."""
    c = _case(d, nd, nb)
    draws = _class_draws(d, nd, nb)
    eta = c["gp"].nugget
    fd, fb = draws.functionals(c["dom"]), draws.functionals(c["bdy"])
    rv = draws.right_vectors.cpu().numpy()
    for s in range(CLASS_S):
        got = ref.gram_order(fd[s], fb[s])
        want = c["z"] - np.sqrt(eta) * ref.noise(CLASS_SEED, CLASS_SAMPLE0 + s, c["M"]) - eta * rv[s]
        err = _rel(got, want)
        print("draw %d of (%d, %d, %d): interpolation identity %.2e, cap %.3e" % (s, d, nd, nb, err, c["cap"]))
        assert err <= c["cap"]


def test_moments_are_the_posterior_mean_and_covariance():
    c = _case(6, 20, 29)
    gp = c["gp"]
    draws = gp.sample_functions(4096, seed=MOMENT_SEED, n_features=64)          # z = None: K_p right_vector of the loaded model
    got = draws.predict(c["X"])
    assert got.shape == (4096, 33)
    r_mean, r_cov = ref.moment_ratios(got, c["rows"][0] @ c["alpha"], gp.predict_covariance(c["X"]))
    print("4096 draws, F = 64: mean within %.2f, covariance within %.2f standard errors" % (r_mean, r_cov))
    assert r_mean <= 6.0 and r_cov <= 6.0


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_and_empty_calls():
    import torch
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    c = _case(6, 20, 29)
    gp = c["gp"]
    as_coded = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(7), compat="reference", laplacian_idx=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="compat=None"):
        as_coded.sample_functions(2)
    with pytest.raises(_lib.ScasmlError, match="no collocation points"):
        _gp(6).sample_functions(2)
    only_points = _gp(6)
    only_points.kernel_phi_phi(c["dom"], c["bdy"])
    with pytest.raises(_lib.ScasmlError, match="no feature values"):
        only_points.sample_functions(2)
    with pytest.raises(ValueError, match="n_features"):
        gp.sample_functions(2, n_features=0)
    with pytest.raises(ValueError, match="negative"):
        gp.sample_functions(2, sample0=-1)
    with pytest.raises(ValueError, match="negative"):
        gp.sample_functions(-1)
    with pytest.raises(ValueError, match="2\\^32"):
        gp.sample_functions(2, sample0=2 ** 32 - 1)
    with pytest.raises(ValueError, match="shape"):
        _class_draws(6, 20, 29).predict(np.zeros((3, 6), dtype=np.float32))
    none = gp.sample_functions(0, n_features=8)
    assert tuple(none.right_vectors.shape) == (0, c["M"])
    assert none.predict(c["X"]).shape == (0, 33) and none.functionals(c["X"]).shape == (0, 33, 4)
    draws = _class_draws(6, 20, 29)
    empty = np.zeros((0, 7), dtype=np.float32)
    assert draws.predict(empty).shape == (CLASS_S, 0) and draws.functionals(empty).shape == (CLASS_S, 0, 4)
    et = draws.functionals(torch.zeros((0, 7), device="cuda"))
    assert isinstance(et, torch.Tensor) and tuple(et.shape) == (CLASS_S, 0, 4)
    last = gp.sample_functions(1, n_features=8, sample0=2 ** 32 - 1)          # the last draw index there is
    assert np.isfinite(last.predict(c["X"])).all()
