"""GP posterior variance: GP.predict_variance / predict_std and the C entry point scasml_gp_variance (csrc/gp_variance.hip)

    var(x) = 1 - | L^-1 K(x, phi) |^2 ,   L L^T = K(phi, phi) + nugget I   (all float64)

against float64 NumPy written out here.  Tolerances are not tuned to the device: two float64 host evaluations of the same quantity at the same
conditioning (route A: Cholesky + solve with the factor; route B: one solve with K_p) disagree by ``delta_host``; the device, a third backward-stable
evaluation with another summation order (4-wide MFMA chunks, blocked solve), must agree with route A within max(32 * delta_host, 1e-13).  A float32
slip anywhere in the path shows as >= 1e-7, so every case also asserts 32 * delta_host <= 1e-9.  The figures go to profiles/gp_variance_accuracy.json."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "gp_variance_accuracy.json")
NUGGET = 1e-2


def _record(key, **figures):
    try:
        with open(ACCURACY_JSON) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc[key] = {k: float(v) for k, v in figures.items()}
    with open(ACCURACY_JSON, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _idx(d):
    return [d - 1, 0, d // 2, 2, 1]


def _pair(d, compat, nd, nb, seed, equation=None):
    """(GP, oracle) of one surrogate on one sampled collocation set; the as-coded one on float16 points, as the reference's are."""
    from oracle.equation import GradDependentNonlinear, sample_points
    from oracle.gp import OracleGP
    from oracle.gp_compat import OracleGPCompat
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    dom, bdy = sample_points(np.random.default_rng(seed), d, nd, nb)
    if compat == "reference":
        dom, bdy = dom.astype(np.float16).astype(np.float32), bdy.astype(np.float16).astype(np.float32)
        gp = GP_Grad_Dependent_Nonlinear(equation or Grad_Dependent_Nonlinear(d + 1), compat="reference", laplacian_idx=_idx(d))
        ogp = OracleGPCompat(GradDependentNonlinear(d + 1), _idx(d), round16=True, round_factor=False)
    else:
        gp = GP_Grad_Dependent_Nonlinear(equation or Grad_Dependent_Nonlinear(d + 1), compat=None)
        ogp = OracleGP(GradDependentNonlinear(d + 1))
    return gp, ogp, dom, bdy


def _sampler_points(d, n, seed):
    X = np.random.default_rng(seed).uniform(-0.6, 0.6, (n, d + 1)).astype(np.float32)
    X[:, -1] = np.abs(X[:, -1]) * 0.8
    return X


def _host_routes(K, k):
    """Routes A and B.  Every factorisation of the product reads the LOWER triangle of K (the as-coded blocks are built separately and need not
    mirror exactly), so that triangle is mirrored first."""
    Kp = np.tril(K) + np.tril(K, -1).T + NUGGET * np.eye(K.shape[0])
    Lh = np.linalg.cholesky(Kp)
    y = np.linalg.solve(Lh, k.T)
    var_a = 1.0 - (y * y).sum(0)
    var_b = 1.0 - np.einsum("ij,ji->i", k, np.linalg.solve(Kp, k.T))
    return var_a, var_b


def _tolerance(delta_host):
    assert 32.0 * delta_host <= 1e-9, "the case is too ill-conditioned to expose a float32 slip: delta_host = %.3e" % delta_host
    return max(32.0 * delta_host, 1e-13)


# ------------------------------------------------------------------------------------------------ 1. against float64 NumPy, both surrogates
@pytest.mark.parametrize("compat", [None, "reference"])
@pytest.mark.parametrize("d", [6, 20, 100])
def test_variance_matches_float64_numpy(d, compat):
    """M = 4 * 37 + 9 = 157 (not a multiple of 32: five block columns of 32 after padding, the last block column of the kernel 32 wide), n = 131
    (two full point tiles and three rows): sampler points, the collocation points themselves, six points far outside the box."""
    nd, nb = 37, 9
    gp, ogp, dom, bdy = _pair(d, compat, nd, nb, seed=100 + d)
    far = _sampler_points(d, 6, seed=3) + np.float32(4.0) * np.array([1, -1, 2, -2, 3, -3], dtype=np.float32)[:, None]
    X = np.concatenate([_sampler_points(d, 131 - nd - nb - 6, seed=d), dom, bdy, far]).astype(np.float32)
    assert X.shape == (131, d + 1)
    K = ogp.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64))
    k = ogp._features("I", X.astype(np.float64))
    var_a, var_b = _host_routes(K, k)
    delta_host = float(np.abs(var_a - var_b).max())
    gp.kernel_phi_phi(dom, bdy)
    got = gp.predict_variance(X)
    assert got.shape == (131, 1) and got.dtype == np.float64
    err = float(np.abs(got[:, 0] - var_a).max())
    # the same host routes on the DEVICE's own matrices (the Gram and the feature rows are older kernels with tests of their own): tells an error
    # of the new solve from last-bit differences of the inputs
    Kd = gp.kernel_phi_phi(dom, bdy).cpu().numpy()
    Kd[np.diag_indices_from(Kd)] = np.diag(K)              # kernel_phi_phi returns K + nugget I (as coded: that diagonal rounded to float16)
    kd = np.asarray(gp.kernel_x_t_phi(X, dom, bdy), dtype=np.float64)
    err_inputs = float(np.abs(got[:, 0] - _host_routes(Kd, kd)[0]).max())
    print("d=%d compat=%s delta_host=%.3e device-vs-A=%.3e (host routes on the device's matrices: %.3e; entries differ by K %.3e, k %.3e)" % (
        d, compat, delta_host, err, err_inputs, np.abs(np.tril(Kd - K)).max(), np.abs(kd - k).max()))
    _record("numpy d=%d %s" % (d, compat or "documented"), delta_host=delta_host, device_max_abs_error=err, device_max_abs_error_on_device_matrices=err_inputs)
    assert err <= _tolerance(delta_host)


# ------------------------------------------------------------------------------------------------ 2. rows in, rows out: the entry point alone
@functools.lru_cache(maxsize=None)
def _factor_case(Mp):
    rng = np.random.default_rng(Mp)
    L = np.tril(rng.normal(size=(Mp, Mp)), -1) * (0.3 / np.sqrt(Mp))
    L[np.diag_indices(Mp)] = rng.uniform(1.0, 2.0, Mp)
    R = rng.normal(size=(1000, Mp))
    Xa = np.linalg.solve(L, R.T).T
    Xb = R @ np.linalg.inv(L).T
    va, vb = 0.75 - (Xa * Xa).sum(1), 0.75 - (Xb * Xb).sum(1)
    return L, R, Xa, va, float(np.abs(Xa - Xb).max()), float(np.abs(va - vb).max())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("Mp", [32, 64, 96, 4224])
def test_entry_point_rows_in_rows_out(Mp, n):
    """One 32-wide block column, one 64-wide, one of each, 66 of them; a single row, both sides of the 64-row tile edge, a ragged last tile.  Rows
    beyond n and columns beyond Mp of a wider buffer (ld = Mp + 8 at n = 65) are not touched."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    L, R, Xa, va, delta_rows, delta_var = _factor_case(Mp)
    ld = Mp + 8 if n == 65 else Mp
    buf = np.full((n + 3, ld), 7.0)
    buf[:n, :Mp] = R[:n]
    rows = torch.from_numpy(buf).cuda()
    Ld = torch.from_numpy(L).cuda()
    var = torch.full((n + 3,), 7.0, dtype=torch.float64, device="cuda")
    rc = lib.scasml_gp_variance(_lib.ptr(Ld), Mp, _lib.ptr(rows), ld, n, 0.75, _lib.ptr(var), _lib.stream_ptr())
    assert rc == 0, lib.scasml_last_error()
    torch.cuda.synchronize()
    out, v = rows.cpu().numpy(), var.cpu().numpy()
    assert np.all(out[n:] == 7.0) and np.all(out[:, Mp:] == 7.0) and np.all(v[n:] == 7.0)
    err_rows, err_var = float(np.abs(out[:n, :Mp] - Xa[:n]).max()), float(np.abs(v[:n] - va[:n]).max())
    print("Mp=%d n=%d rows: delta_host=%.3e device=%.3e   var: delta_host=%.3e device=%.3e" % (Mp, n, delta_rows, err_rows, delta_var, err_var))
    _record("entry Mp=%d n=%d" % (Mp, n), delta_host_rows=delta_rows, device_max_abs_error_rows=err_rows, delta_host_var=delta_var,
            device_max_abs_error_var=err_var)
    assert err_rows <= _tolerance(delta_rows) and err_var <= _tolerance(delta_var)


# ------------------------------------------------------------------------------------------------ 3. properties
def test_variance_properties_of_the_documented_surrogate():
    d, nd, nb = 20, 200, 50
    gp, _, dom, bdy = _pair(d, None, nd, nb, seed=7)
    gp.kernel_phi_phi(dom, bdy)
    X = _sampler_points(d, 500, seed=8)
    far = X[:64].copy()
    far[:, :d] += np.float32(10.0 * gp.sigma)              # every spatial coordinate by 10 sigma: the point moves by 10 sigma sqrt(d)
    var = gp.predict_variance(np.concatenate([X, dom, bdy, far]))[:, 0]
    assert np.all(var >= -1e-10) and np.all(var <= 1.0 + 1e-10), (var.min(), var.max())
    assert np.all(var[-64:] >= 1.0 - 1e-6), var[-64:].min()
    # u(x_bdy_j) is one of the observed functionals.  With observation noise eta the posterior covariance of the observed functionals is
    # K - K (K + eta I)^-1 K = eta (I - eta (K + eta I)^-1), whose diagonal is below eta by eta^2 [(K + eta I)^-1]_jj >= eta^2 / (lambda_max + eta)
    # -- orders of magnitude above float64 rounding, so the bound is asserted as it stands
    at_bdy = var[500 + nd:500 + nd + nb]
    assert np.all(at_bdy <= gp.nugget), at_bdy.max()
    # predict_std is sqrt(max(var, 0)) exactly; squaring a square root returns var only up to its last bits, which is all that is asked of std^2
    std = gp.predict_std(np.concatenate([X, dom, bdy, far]))
    assert std.shape == (len(var), 1) and np.array_equal(std[:, 0], np.sqrt(np.maximum(var, 0.0)))
    assert np.all(np.abs(std[:, 0] ** 2 - np.maximum(var, 0.0)) <= 4 * np.finfo(np.float64).eps * np.maximum(var, 0.0))


# ------------------------------------------------------------------------------------------------ 4. determinism / chunk invariance
@pytest.mark.parametrize("compat", [None, "reference"])
def test_every_point_is_a_function_of_that_point_alone(compat):
    """One call, a call walked in chunks of 7 points, reversed order, a CUDA tensor in: bit-identical values point by point."""
    import torch
    d = 20
    gp, _, dom, bdy = _pair(d, compat, 60, 17, seed=11)
    gp.kernel_phi_phi(dom, bdy)
    X = _sampler_points(d, 3000, seed=12)
    one = gp.predict_variance(X)
    gp.variance_buffer_bytes = 7 * 8 * gp._L_pad.shape[0]
    chunked = gp.predict_variance(X)
    del gp.variance_buffer_bytes
    assert gp.variance_buffer_bytes == 1 << 30
    backwards = gp.predict_variance(X[::-1].copy())[::-1]
    t = gp.predict_variance(torch.from_numpy(X).cuda())
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.shape == (3000, 1)
    for other in (chunked, backwards, t.cpu().numpy()):
        assert np.array_equal(one.view(np.int64), other.view(np.int64))
    assert np.array_equal(one[:5], gp.predict_variance(X[:5]))
    assert gp.predict_variance(X[:0]).shape == (0, 1)


# ------------------------------------------------------------------------------------------------ 5. full size, device against device
def _composed_route(gp, X):
    """What the ABI allowed before scasml_gp_variance: feature rows, transposed, one blocked solve with n right-hand sides, torch square-sum."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    L = gp._L_pad
    Mp, M = L.shape[0], gp.phi_dim
    k = gp.kernel_x_t_phi(torch.from_numpy(X).cuda(), gp.x_t_domain, gp.x_t_boundary).to(torch.float64)
    B = torch.zeros((Mp, X.shape[0]), dtype=torch.float64, device="cuda")
    B[:M] = k.t()
    _lib.check(lib.scasml_trsm_lower(_lib.ptr(L), Mp, _lib.ptr(B), X.shape[0], 0, _lib.stream_ptr()), "trsm_lower")
    return (1.0 - (B * B).sum(0)).cpu().numpy()


@pytest.mark.parametrize("compat", [None, "reference"])
def test_full_size_against_the_composed_route(compat):
    d, nd, nb, n = 100, 1000, 200, 16384
    gp, ogp, dom, bdy = _pair(d, compat, nd, nb, seed=21)
    gp.kernel_phi_phi(dom, bdy)
    X = _sampler_points(d, n, seed=22)
    got = gp.predict_variance(X)[:, 0]
    composed = _composed_route(gp, X)
    sub = np.arange(0, n, n // 64)[:64]
    K = ogp.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64))
    var_a, _ = _host_routes(K, ogp._features("I", X[sub].astype(np.float64)))
    delta = float(np.abs(composed[sub] - var_a).max())
    err = float(np.abs(got - composed).max())
    print("d=100 M=4200 n=16384 compat=%s: composed route vs host route A on 64 points %.3e, new path vs composed route %.3e, new path vs route A %.3e" % (
        compat, delta, err, np.abs(got[sub] - var_a).max()))
    _record("full size %s" % (compat or "documented"), composed_vs_host_route_a_64_points=delta, new_path_vs_composed_route=err,
            new_path_vs_host_route_a_64_points=float(np.abs(got[sub] - var_a).max()))
    assert err <= _tolerance(delta)


# ------------------------------------------------------------------------------------------------ 6. lazy factor
def test_factor_is_rebuilt_after_load_and_needs_no_fit(tmp_path):
    from scasml_gp_amd import _lib
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear, Quadratic_Gradient_Reaction_Diffusion
    from scasml_gp_amd.models.GP import GP, GP_Grad_Dependent_Nonlinear
    d = 20
    gp, _, dom, bdy = _pair(d, "reference", 40, 10, seed=31)
    gp.GPsolver(dom, bdy, GN_steps=5)
    X = _sampler_points(d, 150, seed=32)
    before = gp.predict_variance(X)
    path = str(tmp_path / "gp.npz")
    gp.save(path)
    fresh = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat="reference", laplacian_idx=_idx(d))
    fresh.load(path)
    assert getattr(fresh, "_L_pad", None) is None
    u0 = fresh.predict(X)
    after = fresh.predict_variance(X)
    assert np.array_equal(before.view(np.int64), after.view(np.int64))
    assert np.array_equal(u0, fresh.predict(X)) and np.array_equal(u0, gp.predict(X))
    L1 = fresh._L_pad
    fresh.predict_variance(X[:3])
    assert fresh._L_pad is L1                                 # kept, not rebuilt per call
    assert "_L_pad" not in fresh.state_dict() and set(fresh.state_dict()) == set(gp.state_dict())
    # an equation GPsolver has no Newton kernels for: the variance needs the points, sigma and nugget only
    other = GP(Quadratic_Gradient_Reaction_Diffusion(d + 1), compat=None)
    with pytest.raises(NotImplementedError):
        other.GPsolver(dom, bdy)
    other.kernel_phi_phi(dom, bdy)
    same = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)
    same.kernel_phi_phi(dom, bdy)
    v = other.predict_variance(X)
    assert np.all(v >= -1e-10) and np.all(v <= 1.0 + 1e-10)
    if float(other.sigma) == float(same.sigma):
        assert np.array_equal(v, same.predict_variance(X))
    untrained = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1))
    with pytest.raises(_lib.ScasmlError):
        untrained.predict_variance(X)
    with pytest.raises(_lib.ScasmlError):
        untrained.predict_std(X)
