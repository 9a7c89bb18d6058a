"""Per-component gradients of the pathwise GP posterior draws on the device: scasml_gp_rff_gradient (csrc/gp_rff_grad.hip),
GPFunctionDraws.gradient and GP.posterior_mean_gradient against the NumPy statement of tests/_gp_rff_grad_ref.py (features from oracle.philox, sums
in np.longdouble, the dense alpha form, a dense float64 solve).

* The kernel: errors are counted in units of 2^-53 F^-1/2 sum_f |omega_fk| (|wc_f| + |ws_f|) (1 + (d + 2) sum_j |omega_fj x_j|) of every component --
  the scale of the sum times the absolute error with which theta enters the sine.  The ratios are asserted at 16 times the largest measured on the
  MI355X per shape (profiles/gp_rff_gradient_accuracy.json; the margin is for other points and other boxes), and that bound must itself stay under the
  a-priori 2 (F + d + 8) units.
* Everything in which the device solves with K_p is asserted at the cap 256 cond(K_p) 2^-53 of the quantity's own scale (tests/_gp_evidence_ref.py).
* Statistics: six empirical standard errors on every entry of the sample mean and of the 28 x 28 sample covariance at seed 1 (the NumPy statement
  alone -- oracle normals, dense solve -- gives 1.92 and 2.86 standard errors there; seeds 0 .. 5 give 1.9 .. 2.8 and 2.9 .. 4.0)."""
import numpy as np
import pytest

import _gp_rff_grad_ref as gref
import _gp_rff_ref as ref
from test_gpu_gp_rff import CLASS_F, CLASS_S, CLASS_SAMPLE0, CLASS_SEED, CLASS_SHAPES, _a, _case, _class_draws, _gp, _kernel_points, _rel, _rff, bits

pytestmark = pytest.mark.gpu

# (d, n, F, ld_x - (d + 1), ld_out - (d + 1)): K = d + 1 = 2, 4, 32, 34, 101 as in test_gpu_gp_rff.py; d + 1 = 64 is exactly one component tile, at
# d = 64 the second tile holds one component, d = 252 is the most component tiles (four) the kernel serves; the last case has padded output rows
KERNEL_CASES = [(1, 1, 1, 0, 0), (3, 63, 63, 0, 0), (31, 65, 64, 3, 0), (33, 130, 65, 0, 0), (63, 65, 64, 0, 0), (64, 65, 65, 0, 0), (100, 130, 200, 0, 0),
                (252, 65, 65, 0, 0), (100, 1, 1, 0, 0), (33, 65, 64, 0, 5)]
# 16 x the largest ratio measured on the MI355X at each case (profiles/gp_rff_gradient_accuracy.json), in the units above
KERNEL_BOUND = {(1, 1, 1, 0): 16.0 * 0.2147, (3, 63, 63, 0): 16.0 * 0.1136, (31, 65, 64, 0): 16.0 * 0.0091, (33, 130, 65, 0): 16.0 * 0.0110,
                (63, 65, 64, 0): 16.0 * 0.0046, (64, 65, 65, 0): 16.0 * 0.0046, (100, 130, 200, 0): 16.0 * 0.0036, (252, 65, 65, 0): 16.0 * 0.0009,
                (100, 1, 1, 0): 16.0 * 0.0010, (33, 65, 64, 5): 16.0 * 0.0104}
MOMENT_SEED = 1


def _grad(d, a, X, F, seed, sample0, S, ld_extra=0, ld_out_extra=0):
    """scasml_gp_rff_gradient on the rows of X (host float32): (S, n, d + 1 + ld_out_extra) float64, the padding of both sides pre-filled with 7."""
    import torch
    from scasml_gp_amd import _lib
    n = X.shape[0]
    buf = torch.full((max(n, 1), d + 1 + ld_extra), 7.0, dtype=torch.float32, device="cuda")       # the padding holds a value that must not be read
    buf[:n, :d + 1] = torch.from_numpy(np.array(X, dtype=np.float32)).cuda()
    out = torch.full((S, n, d + 1 + ld_out_extra), 7.0, dtype=torch.float64, device="cuda")
    out[:, :, :d + 1] = float("nan")
    _lib.check(_lib.load().scasml_gp_rff_gradient(d, a, _lib.ptr(buf), n, d + 1 + ld_extra, F, seed, sample0, S, _lib.ptr(out), d + 1 + ld_out_extra,
                                                  _lib.stream_ptr()), "gp_rff_gradient")
    return out.cpu().numpy()


def _kernel_errors(d, n, F, ld_extra, ld_out_extra):
    """(values (S, n, d+1), largest error in units, the units (S, n, d+1)) of one kernel case."""
    a, seed, sample0, S = _a(d), 0xF00D + d, 3, 2
    X = _kernel_points(d)[:n]
    got = _grad(d, a, X, F, seed, sample0, S, ld_extra, ld_out_extra)
    assert got.shape == (S, n, d + 1 + ld_out_extra) and (got[:, :, d + 1:] == 7.0).all()          # the padding of the output comes back untouched
    got = got[:, :, :d + 1]
    assert np.isfinite(got).all()
    worst, units = 0.0, []
    for s in range(S):
        want, unit = gref.prior_gradient(d, a, F, seed, sample0 + s, X, with_unit=True)
        worst = max(worst, float((np.abs(got[s].astype(np.longdouble) - want) / unit).max()))
        units.append(unit)
    return got, worst, np.stack(units)


# ------------------------------------------------------------------------------------------------ 1. the kernel against the statement
@pytest.mark.parametrize("d,n,F,ld_extra,ld_out_extra", KERNEL_CASES)
def test_kernel_matches_the_statement(d, n, F, ld_extra, ld_out_extra):
    _, worst, _ = _kernel_errors(d, n, F, ld_extra, ld_out_extra)
    print("gp_rff_gradient kernel d=%d n=%d F=%d ld_x=%d ld_out=%d: largest error %.4f units" % (d, n, F, d + 1 + ld_extra, d + 1 + ld_out_extra, worst))
    bound = KERNEL_BOUND[(d, n, F, ld_out_extra)]
    assert bound <= 2.0 * (F + d + 8), "the measured bound left the a-priori one"
    assert worst <= bound


# ------------------------------------------------------------------------------------------------ 2. the same draw as the functionals kernel
@pytest.mark.parametrize("d,n,F,ld_extra,ld_out_extra", KERNEL_CASES[:-1])
def test_time_component_is_dt_and_spatial_sum_is_div(d, n, F, ld_extra, ld_out_extra):
    """Against scasml_gp_rff_functionals at the same (seed, sample0): both kernels are within their bound of the statement, whose two forms agree to
    2^-64 -- so they differ by at most the sum of the two units times the bound (the spatial sum: the units summed over the components; the d - 1
    float64 additions of the sum itself are 2^-53 of partial sums that the units dominate)."""
    a, seed, sample0, S = _a(d), 0xF00D + d, 3, 2
    X = _kernel_points(d)[:n]
    got, _, unit = _kernel_errors(d, n, F, ld_extra, ld_out_extra)
    fun = _rff(d, a, X, F, seed, sample0, S, ld_extra)
    bound = KERNEL_BOUND[(d, n, F, ld_out_extra)]
    for s in range(S):
        funit = ref.functionals(d, a, F, seed, sample0 + s, X, with_unit=True)[1]
        r_dt = float((np.abs(got[s, :, d] - fun[s, :, 2]) / (unit[s, :, d] + funit[:, 2])).max())
        r_div = float((np.abs(got[s, :, :d].sum(1) - fun[s, :, 3]) / (unit[s, :, :d].sum(1) + funit[:, 3])).max())
        print("d=%d n=%d F=%d draw %d: time component against dt %.4f, spatial sum against div %.4f of the summed units" % (d, n, F, s, r_dt, r_div))
        assert r_dt <= bound and r_div <= bound


# ------------------------------------------------------------------------------------------------ 3. a point's values are a function of the point
def test_values_do_not_depend_on_where_the_point_stands():
    d, F, seed = 100, 200, 77                                                                        # two component tiles, four feature tiles
    a = _a(d)
    X = _kernel_points(d)
    full = _grad(d, a, X, F, seed, 5, 3)
    assert np.array_equal(bits(_grad(d, a, X[97:98], F, seed, 5, 3)), bits(full[:, 97:98]))          # alone; inside 130 points
    perm = np.random.default_rng(1).permutation(130)
    assert np.array_equal(bits(_grad(d, a, X[perm], F, seed, 5, 3)), bits(full[:, perm]))
    assert np.array_equal(bits(_grad(d, a, X, F, seed, 5, 3, ld_extra=5)), bits(full))
    assert np.array_equal(bits(_grad(d, a, X, F, seed, 5, 3, ld_out_extra=3)[:, :, :d + 1]), bits(full))
    for s in range(3):                                                                              # the split of the draws over calls
        assert np.array_equal(bits(_grad(d, a, X, F, seed, 5 + s, 1)), bits(full[s:s + 1]))
    assert not np.array_equal(bits(full[0]), bits(full[1]))


# ------------------------------------------------------------------------------------------------ 4. the class against the dense statement
@pytest.mark.parametrize("d,nd,nb", CLASS_SHAPES)
def test_class_matches_the_dense_statement(d, nd, nb):
    import torch
    c = _case(d, nd, nb)
    gp, X = c["gp"], c["X"]
    draws = _class_draws(d, nd, nb)
    G = gref.gradient_rows(c["og"], X)
    grad = draws.gradient(X)
    assert isinstance(grad, np.ndarray) and grad.shape == (CLASS_S, 33, d + 1) and grad.dtype == np.float64
    for s in range(CLASS_S):
        rv = ref.posterior_draw(c["og"], c["Kp"], c["z"], gp.nugget, CLASS_F, CLASS_SEED, CLASS_SAMPLE0 + s)[0]
        want = gref.prior_gradient(d, c["og"].a, CLASS_F, CLASS_SEED, CLASS_SAMPLE0 + s, X).astype(np.float64) + gref.data_gradient(c["og"], X, rv, G)
        err = _rel(grad[s], want)
        print("draw %d of (%d, %d, %d): gradient relative error %.2e, cap %.3e" % (s, d, nd, nb, err, c["cap"]))
        assert err <= c["cap"]
    # the float64 gradient of the mean: the data-term routine on right_vector; compute_gradient is its float32 kernel
    mean = gp.posterior_mean_gradient(X)
    assert isinstance(mean, np.ndarray) and mean.shape == (33, d + 1) and mean.dtype == np.float64
    want = gref.data_gradient(c["og"], X, c["alpha"], G)
    e64 = _rel(mean, want)
    # compute_gradient's own float32 tolerance (test_gpu_gp.py): 2e-5 of sum_j |kappa_j c_j| times the derivative features' factor 1 + a (1 + d)
    magp = (np.abs(c["rows"][0]) @ np.abs(c["alpha"]) + 1e-3) * (1 + c["og"].a * (1 + d))
    e32 = float((np.abs(gp.compute_gradient(X).astype(np.float64) - mean) / magp[:, None]).max())
    print("mean gradient of (%d, %d, %d): %.2e of G alpha (cap %.3e), compute_gradient %.2e of its magnitude away" % (d, nd, nb, e64, c["cap"], e32))
    assert e64 <= c["cap"]
    assert e32 <= 2e-5
    # CUDA tensor in, CUDA tensor out; split and permuted points; 5-point chunks; the draws continued by sample0: the same bits
    xt = torch.from_numpy(X.copy()).cuda()
    gt, mt = draws.gradient(xt), gp.posterior_mean_gradient(xt)
    assert isinstance(gt, torch.Tensor) and gt.is_cuda and gt.dtype == torch.float64 and np.array_equal(bits(gt.cpu().numpy()), bits(grad))
    assert isinstance(mt, torch.Tensor) and mt.is_cuda and mt.dtype == torch.float64 and np.array_equal(bits(mt.cpu().numpy()), bits(mean))
    perm = np.random.default_rng(2).permutation(33)
    assert np.array_equal(bits(draws.gradient(X[perm])), bits(grad[:, perm]))
    assert np.array_equal(bits(gp.posterior_mean_gradient(X[perm])), bits(mean[perm]))
    assert np.array_equal(bits(np.concatenate([draws.gradient(X[:7]), draws.gradient(X[7:])], axis=1)), bits(grad))
    assert np.array_equal(bits(np.concatenate([gp.posterior_mean_gradient(X[:7]), gp.posterior_mean_gradient(X[7:])])), bits(mean))
    later = gp.sample_functions(1, seed=CLASS_SEED, n_features=CLASS_F, sample0=CLASS_SAMPLE0 + 2, z=c["z"])
    assert np.array_equal(bits(later.gradient(X)), bits(grad[2:3]))
    cap_bytes = gp.variance_buffer_bytes
    try:                                              # chunks of 5 points
        gp.variance_buffer_bytes = 5 * 8 * gp._L_pad.shape[0]
        assert np.array_equal(bits(draws.gradient(X)), bits(grad))
        assert np.array_equal(bits(gp.posterior_mean_gradient(X)), bits(mean))
    finally:
        gp.variance_buffer_bytes = cap_bytes
    # the draw's own functionals: the time component is dt, the spatial sum div, both data term included
    fun = draws.functionals(X)
    scale = np.abs(grad).max()
    assert np.abs(grad[:, :, d] - fun[:, :, 2]).max() <= c["cap"] * scale and np.abs(grad[:, :, :d].sum(2) - fun[:, :, 3]).max() <= c["cap"] * d * scale


# ------------------------------------------------------------------------------------------------ 5. moments
def test_moments_are_the_posterior_mean_and_covariance_of_the_gradient():
    """4096 draws, F = 64, the first 4 of the 33 points (28 components), seed 1: the NumPy statement alone gives 1.92 and 2.86 standard errors."""
    c = _case(6, 20, 29)
    gp, X = c["gp"], c["X"][:4]
    draws = gp.sample_functions(4096, seed=MOMENT_SEED, n_features=64)          # z = None: K_p right_vector of the loaded model
    got = draws.gradient(X)
    assert got.shape == (4096, 4, 7)
    G = gref.gradient_rows(c["og"], X)
    mean, cov = (G @ c["alpha"]).reshape(-1), gref.posterior_gradient_covariance(c["og"], c["Kp"], X, G)
    r_mean, r_cov = ref.moment_ratios(got.reshape(4096, 28), mean, cov)
    print("4096 draws, F = 64: gradient mean within %.2f, covariance within %.2f standard errors" % (r_mean, r_cov))
    assert r_mean <= 6.0 and r_cov <= 6.0


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_and_empty_calls():
    import torch
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear, GPFunctionDraws
    c = _case(6, 20, 29)
    gp, draws = c["gp"], _class_draws(6, 20, 29)
    as_coded = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(7), compat="reference", laplacian_idx=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="compat=None"):
        as_coded.posterior_mean_gradient(c["X"])
    with pytest.raises(ValueError, match="compat=None"):
        GPFunctionDraws(as_coded, torch.zeros((2, c["M"]), dtype=torch.float64, device="cuda"), 8, 0, 0).gradient(c["X"])
    with pytest.raises(_lib.ScasmlError, match="not trained"):
        _gp(6).posterior_mean_gradient(c["X"])
    with pytest.raises(ValueError, match="shape"):
        draws.gradient(np.zeros((3, 6), dtype=np.float32))
    with pytest.raises(ValueError, match="shape"):
        gp.posterior_mean_gradient(np.zeros((3, 6), dtype=np.float32))
    none = gp.sample_functions(0, n_features=8)
    assert none.gradient(c["X"]).shape == (0, 33, 7)
    empty = np.zeros((0, 7), dtype=np.float32)
    assert draws.gradient(empty).shape == (CLASS_S, 0, 7) and gp.posterior_mean_gradient(empty).shape == (0, 7)
    et = draws.gradient(torch.zeros((0, 7), device="cuda"))
    assert isinstance(et, torch.Tensor) and tuple(et.shape) == (CLASS_S, 0, 7)
    last = gp.sample_functions(1, n_features=8, sample0=2 ** 32 - 1)          # the last draw index there is
    assert np.isfinite(last.gradient(c["X"])).all()
    # the ABI: refusals as codes on device pointers, empty calls leave the output alone
    lib = _lib.load()
    x = torch.zeros((4, 7), dtype=torch.float32, device="cuda")
    out = torch.full((2, 4, 7), 7.0, dtype=torch.float64, device="cuda")
    call = lambda **kw: lib.scasml_gp_rff_gradient(*[dict(dict(d=6, a=0.5, x=_lib.ptr(x), n=4, ld_x=7, F=8, seed=1, sample0=0, S=2, out=_lib.ptr(out), ld_out=7,
                                                               stream=_lib.stream_ptr()), **kw)[k]
                                                     for k in ("d", "a", "x", "n", "ld_x", "F", "seed", "sample0", "S", "out", "ld_out", "stream")])
    assert call(ld_out=6) == -1 and call(ld_x=6) == -1 and call(F=0) == -1 and call(d=253) == -1 and call(sample0=2 ** 32 - 1) == -2
    assert call(n=0) == 0 and call(S=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0 and bool(torch.isfinite(out).all())
