"""Posterior covariance of [u, Lap u, dt u, div u] and the delta-method variance of the PDE residual: GP.predict_functional_covariance,
GP.predict_residual_variance / predict_residual_std and the C entry point scasml_gp_functional_covariance (csrc/gp_functional_cov.hip)

    cov(x) = P - (L^-1 k(x)^T)^T (L^-1 k(x)^T),   L L^T = K(phi, phi) + nugget I,   k(x) the four feature rows of x   (all float64)

against the float64 NumPy of _gp_functional_cov_ref.py.  Tolerances follow test_gpu_gp_variance.py and are not tuned to the device: two host
evaluations of the same quantity (route A: Cholesky + solve; route B: one solve with K_p) disagree by ``delta_host``; the device must agree with route
A within max(32 * delta_host, 1e-13), and every case asserts 32 * delta_host <= 1e-9 (a float32 slip shows as >= 1e-7).  All of it in scaled units:
entry (o, p) over sqrt(P_oo P_pp).  The figures go to profiles/gp_functional_covariance_accuracy.json."""
import functools
import json
import os

import numpy as np
import pytest

import _gp_evidence_ref as eref
import _gp_functional_cov_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "gp_functional_covariance_accuracy.json")
NUGGET = ref.NUGGET
ND, NB, N_POINTS = 37, 9, 35        # M = 157, Mp = 160: the last block column 32 wide; 140 rows: two full tiles and a 12-row tile
bits = lambda a: np.ascontiguousarray(a).view(np.int64)


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


def _sampler_points(d, n, seed):
    X = np.random.default_rng(seed).uniform(-0.6, 0.6, (n, d + 1)).astype(np.float32)
    X[:, -1] = np.abs(X[:, -1]) * 0.8
    return X


EQUATIONS = {"Grad_Dependent_Nonlinear": ("GradDependentNonlinear", "GP_Grad_Dependent_Nonlinear"),
             "Cubic_Reaction_Diffusion": ("CubicReactionDiffusion", "GP_Cubic_Reaction_Diffusion")}


@functools.lru_cache(maxsize=None)
def _case(d, equation="Grad_Dependent_Nonlinear", fit=False):
    """One dimension's GP on 37 + 9 sampled collocation points and its NumPy side, computed once and left unchanged: 35 points -- sampler points,
    five domain and three boundary collocation points, six points far outside the box -- their feature rows, K_p, both host routes."""
    import oracle.equation as oeq
    import scasml_gp_amd.equations.equations as eqs
    import scasml_gp_amd.models.GP as models
    oname, gname = EQUATIONS[equation]
    dom, bdy = oeq.sample_points(np.random.default_rng(100 + d), d, ND, NB)
    far = _sampler_points(d, 6, seed=3) + np.float32(4.0) * np.array([1, -1, 2, -2, 3, -3], dtype=np.float32)[:, None]
    X = np.concatenate([_sampler_points(d, N_POINTS - 14, seed=d), dom[3:8], bdy[2:5], far]).astype(np.float32)
    assert X.shape == (N_POINTS, d + 1)
    gp = getattr(models, gname)(getattr(eqs, equation)(d + 1), compat=None)
    oeqn = getattr(oeq, oname)(d + 1)
    og = eref.oracle(d, float(gp.sigma))
    og.eq = oeqn
    Kp = og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64)) + NUGGET * np.eye(4 * ND + NB)
    if fit:
        gp.GPsolver(dom, bdy)
    else:
        gp.kernel_phi_phi(dom, bdy)
    P = ref.prior_block(d, og.a)
    k = ref.rows(og, X)
    cov_a, cov_b = ref.route_a(Kp, k, P), ref.route_b(Kp, k, P)
    case = dict(d=d, gp=gp, og=og, oeqn=oeqn, dom=dom, bdy=bdy, X=X, Kp=Kp, P=P, k=k, cov_a=cov_a, cov_b=cov_b, delta=ref.delta_host(cov_a, cov_b, P))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


# ------------------------------------------------------------------------------------------------ 1. against float64 NumPy
@pytest.mark.parametrize("d", [1, 6, 100])
def test_covariance_matches_float64_numpy(d):
    c = _case(d)
    gp = c["gp"]
    assert gp._variance_factor().shape[0] == 160
    got = gp.predict_functional_covariance(c["X"])
    assert isinstance(got, np.ndarray) and got.shape == (N_POINTS, 4, 4) and got.dtype == np.float64
    err = float((np.abs(got - c["cov_a"]) / ref.scale(c["P"])).max())
    print("d=%d scaled delta_host=%.3e device-vs-A=%.3e" % (d, c["delta"], err))
    _record("numpy d=%d" % d, scaled_delta_host=c["delta"], device_scaled_max_error=err)
    assert err <= ref.tolerance(c["delta"])


# ------------------------------------------------------------------------------------------------ 2. rows in, block out: the entry point alone
@functools.lru_cache(maxsize=None)
def _factor_case(Mp):
    """The synthetic factor and rows of test_gpu_gp_variance.py's _factor_case, 140 rows = 35 points; the prior block is the table at d = 6."""
    rng = np.random.default_rng(Mp)
    L = np.tril(rng.normal(size=(Mp, Mp)), -1) * (0.3 / np.sqrt(Mp))
    L[np.diag_indices(Mp)] = rng.uniform(1.0, 2.0, Mp)
    R = rng.normal(size=(4 * N_POINTS, Mp))
    Xa = np.linalg.solve(L, R.T).T
    Xb = R @ np.linalg.inv(L).T
    P = ref.prior_block(6, 16.0 / 6.0)
    cov = [P[None] - np.einsum("iom,ipm->iop", V.reshape(N_POINTS, 4, Mp), V.reshape(N_POINTS, 4, Mp)) for V in (Xa, Xb)]
    return L, R, Xa, P, cov[0], float(np.abs(Xa - Xb).max()), ref.delta_host(cov[0], cov[1], P)


@pytest.mark.parametrize("n_points", [1, 16, 17, 35])
@pytest.mark.parametrize("Mp", [32, 64, 96, 160])
def test_entry_point_rows_in_block_out(Mp, n_points):
    """One 32-wide block column, one 64-wide, one of each, two and a 32-wide one; one point (a 4-row tile), a full tile, one point more, two tiles and
    three points.  ld = Mp + 8: the guard columns, the rows beyond 4 n_points and the blocks beyond n_points are not touched."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    L, R, Xa, P, cov_a, delta_rows, delta_cov = _factor_case(Mp)
    n, ld = 4 * n_points, Mp + 8
    buf = np.full((n + 3, ld), 7.0)
    buf[:n, :Mp] = R[:n]
    rows = torch.from_numpy(buf).cuda()
    Ld = torch.from_numpy(L).cuda()
    cov = torch.full((n_points + 1, 16), 7.0, dtype=torch.float64, device="cuda")
    prior = np.ascontiguousarray(P)
    rc = lib.scasml_gp_functional_covariance(_lib.ptr(Ld), Mp, _lib.ptr(rows), ld, n_points, prior.ctypes.data, _lib.ptr(cov), _lib.stream_ptr())
    assert rc == 0, lib.scasml_last_error()
    torch.cuda.synchronize()
    out, cv = rows.cpu().numpy(), cov.cpu().numpy()
    assert np.all(out[n:] == 7.0) and np.all(out[:, Mp:] == 7.0) and np.all(cv[n_points:] == 7.0)
    err_rows = float(np.abs(out[:n, :Mp] - Xa[:n]).max())
    err_cov = float((np.abs(cv[:n_points].reshape(-1, 4, 4) - cov_a[:n_points]) / ref.scale(P)).max())
    print("Mp=%d n_points=%d rows: delta_host=%.3e device=%.3e   scaled block: delta_host=%.3e device=%.3e" % (
        Mp, n_points, delta_rows, err_rows, delta_cov, err_cov))
    _record("entry Mp=%d n_points=%d" % (Mp, n_points), delta_host_rows=delta_rows, device_max_abs_error_rows=err_rows, scaled_delta_host=delta_cov,
            device_scaled_max_error=err_cov)
    assert err_rows <= ref.tolerance(delta_rows) and err_cov <= ref.tolerance(delta_cov)


# ------------------------------------------------------------------------------------------------ 3. bit identities
def _interleaved_rows(gp, X):
    """The (n, 4, Mp) row buffer of the class, built by its own calls."""
    import torch
    xi = gp._rows_device(X)[0]
    Mp = gp._variance_factor().shape[0]
    buf = torch.zeros((len(X), 4, Mp), dtype=torch.float64, device="cuda")
    for o in range(4):
        gp._cross_rows(gp._xd, gp._xb, o, xi, buf[:, o, :], 4 * Mp, 0)
    return buf


def test_bit_identities():
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    c = _case(6)
    gp, X, P = c["gp"], c["X"], c["P"]
    n = len(X)
    cov = gp.predict_functional_covariance(X)
    assert np.array_equal(bits(cov[:, 0, 0]), bits(gp.predict_variance(X)[:, 0]))
    assert np.array_equal(bits(cov), bits(cov.transpose(0, 2, 1)))
    # the entry point and scasml_gp_variance on copies of the same 4 n rows: the same solved rows, prior - ssq the diagonal entries
    L = gp._variance_factor()
    Mp = L.shape[0]
    raw = _interleaved_rows(gp, X)
    solved, blocks = raw.clone(), torch.empty((n, 16), dtype=torch.float64, device="cuda")
    prior = np.ascontiguousarray(P)
    _lib.check(lib.scasml_gp_functional_covariance(_lib.ptr(L), Mp, _lib.ptr(solved), Mp, n, prior.ctypes.data, _lib.ptr(blocks), _lib.stream_ptr()),
               "gp_functional_covariance")
    assert np.array_equal(bits(blocks.cpu().numpy().reshape(n, 4, 4)), bits(cov))
    for o in range(4):
        again, var = raw.clone(), torch.empty(4 * n, dtype=torch.float64, device="cuda")
        _lib.check(lib.scasml_gp_variance(_lib.ptr(L), Mp, _lib.ptr(again), Mp, 4 * n, float(P[o, o]), _lib.ptr(var), _lib.stream_ptr()), "gp_variance")
        assert np.array_equal(bits(again.cpu().numpy()), bits(solved.cpu().numpy()))
        assert np.array_equal(bits(var.cpu().numpy()[o::4]), bits(cov[:, o, o]))
    # a point's block is a function of that point alone: permuted, sub-selected, walked in three chunks, a CUDA tensor in
    perm = np.random.default_rng(5).permutation(n)
    assert np.array_equal(bits(gp.predict_functional_covariance(X[perm])), bits(cov[perm]))
    assert np.array_equal(bits(gp.predict_functional_covariance(X[17:18])), bits(cov[17:18]))
    assert np.array_equal(bits(gp.predict_functional_covariance(X[3:30:4])), bits(cov[3:30:4]))
    try:
        gp.variance_buffer_bytes = 12 * 32 * Mp                      # chunks of 12 points: 12 + 12 + 11
        assert np.array_equal(bits(gp.predict_functional_covariance(X)), bits(cov))
    finally:
        del gp.variance_buffer_bytes
    assert gp.variance_buffer_bytes == 1 << 30
    t = gp.predict_functional_covariance(torch.from_numpy(X.copy()).cuda())
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (n, 4, 4)
    assert np.array_equal(bits(t.cpu().numpy()), bits(cov))


# ------------------------------------------------------------------------------------------------ 4. an identity that does not pass through the prior table
@pytest.mark.parametrize("d", [6, 100])
def test_block_at_a_collocation_point_is_the_noise_identity(d):
    """The four functionals at the domain collocation point j are observed with noise eta: their posterior covariance is
    K_JJ - K_J K_p^-1 K_J^T = eta I - eta^2 [K_p^-1]_JJ,  J = {j, N + Nb + j, 2 N + Nb + j, 3 N + Nb + j}.  The right side never sees the prior table: a
    wrong constant in it -- the (d^2 + 2 d) a^2 entry, say -- fails here.  K_p^-1 on the device: scasml_cholesky_inverse."""
    import torch
    from scasml_gp_amd import _lib
    c = _case(d)
    gp, og, P = c["gp"], c["og"], c["P"]
    M = 4 * ND + NB
    js = np.array([0, 5, 17, 36])
    J = np.stack([js, ND + NB + js, 2 * ND + NB + js, 3 * ND + NB + js], axis=1)                   # (4 points, 4 operators)
    k = ref.rows(og, c["dom"][js])
    host_a = ref.route_a(c["Kp"], k, P)
    Ah = np.linalg.inv(c["Kp"])
    host_id = np.stack([NUGGET * np.eye(4) - NUGGET ** 2 * Ah[np.ix_(j4, j4)] for j4 in J])
    delta = float((np.abs(host_a - host_id) / ref.scale(P)).max())
    L = gp._variance_factor()
    Mp = L.shape[0]
    A = torch.empty((Mp, Mp), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().scasml_cholesky_inverse(_lib.ptr(L), Mp, _lib.ptr(A), _lib.stream_ptr()), "cholesky_inverse")
    Ad = A.cpu().numpy()[:M, :M]
    Ad = np.tril(Ad) + np.tril(Ad, -1).T
    want = np.stack([NUGGET * np.eye(4) - NUGGET ** 2 * Ad[np.ix_(j4, j4)] for j4 in J])
    got = gp.predict_functional_covariance(c["dom"][js])
    err = float((np.abs(got - want) / ref.scale(P)).max())
    wrong = P.copy()
    wrong[1, 1] = (d * d + 2 * d + 1) * og.a ** 2
    teeth = float((np.abs(ref.route_a(c["Kp"], k, wrong) - host_id) / ref.scale(P)).max())
    print("d=%d noise identity: scaled delta_host=%.3e device=%.3e (a table with (d + 1)^2 a^2: %.3e)" % (d, delta, err, teeth))
    _record("noise identity d=%d" % d, scaled_delta_host=delta, device_scaled_max_error=err)
    tol = ref.tolerance(delta)
    assert teeth > 100.0 * tol
    assert err <= tol


# ------------------------------------------------------------------------------------------------ 5. residual variance
@pytest.mark.parametrize("equation", sorted(EQUATIONS))
def test_residual_variance_matches_the_reference_formula(equation):
    """After GPsolver: means, c and c^T cov c against the oracle's features, F_parts and route A at the device's right_vector.  Means and c relative to
    their largest magnitude, the variance relative to c^T P c.  The check has teeth: zeroing any one component of c in the reference moves the variance
    by more than 100 tolerances -- any component that is not identically zero: the cubic equation's F does not depend on div u, its c_div is 0."""
    import torch
    c = _case(6, equation, True)
    gp, X, P = c["gp"], c["X"], c["P"]
    rv = np.asarray(gp.right_vector, dtype=np.float64).reshape(-1)
    m, cc, res, var = ref.residual_parts(c["oeqn"], c["k"], rv, c["cov_a"])
    var_b = ref.residual_parts(c["oeqn"], c["k"], rv, c["cov_b"])[3]
    unit = np.einsum("io,op,ip->i", cc, P, cc)
    delta = max(c["delta"], float((np.abs(var - var_b) / unit).max()))
    tol = ref.tolerance(delta)
    got, parts = gp.predict_residual_variance(X, return_parts=True)
    assert isinstance(got, np.ndarray) and got.shape == (N_POINTS, 1) and got.dtype == np.float64
    assert parts["mean"].shape == (N_POINTS, 4) and parts["c"].shape == (N_POINTS, 4) and parts["residual"].shape == (N_POINTS, 1)
    errs = dict(mean=float(np.abs(parts["mean"] - m).max() / np.abs(m).max()), c=float(np.abs(parts["c"] - cc).max() / np.abs(cc).max()),
                residual=float(np.abs(parts["residual"][:, 0] - res).max() / max(np.abs(m).max(), np.abs(res).max())),
                variance=float((np.abs(got[:, 0] - var) / unit).max()))
    moved = []
    for o in range(4):
        c0 = cc.copy()
        c0[:, o] = 0.0
        moved.append(float((np.abs(np.einsum("io,iop,ip->i", c0, c["cov_a"], c0) - var) / unit).max()))
    print("%s: delta_host=%.3e errors %s; zeroing a component of c moves the variance by %s" % (
        equation, delta, {k: "%.2e" % v for k, v in errs.items()}, ["%.2e" % v for v in moved]))
    _record("residual %s" % equation, delta_host=delta, **{"device_error_" + k: v for k, v in errs.items()})
    live = [o for o in range(4) if np.any(cc[:, o] != 0.0)]
    assert live == ([0, 1, 2] if equation == "Cubic_Reaction_Diffusion" else [0, 1, 2, 3])
    assert all(moved[o] > 100.0 * tol for o in live)
    assert max(errs.values()) <= tol
    std = gp.predict_residual_std(X)
    assert std.shape == (N_POINTS, 1) and np.array_equal(std, np.sqrt(np.maximum(got, 0.0)))
    assert np.array_equal(bits(gp.predict_residual_variance(X)), bits(got))
    perm = np.random.default_rng(6).permutation(N_POINTS)
    assert np.array_equal(bits(gp.predict_residual_variance(X[perm])), bits(got[perm]))
    t, tp = gp.predict_residual_variance(torch.from_numpy(X.copy()).cuda(), return_parts=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in [t] + list(tp.values()))
    assert np.array_equal(bits(t.cpu().numpy()), bits(got)) and np.array_equal(bits(tp["mean"].cpu().numpy()), bits(parts["mean"]))


# ------------------------------------------------------------------------------------------------ 6. agreement with the pathwise draws
@functools.lru_cache(maxsize=None)
def _moment_case():
    """_gp_functional_cov_ref.moment_case and a GP for it (every test loads the right_vector K_p^-1 z it needs)."""
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    mc = dict(ref.moment_case())
    mc["gp"] = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(mc["d"] + 1), compat=None)
    assert mc["gp"].a == mc["og"].a and mc["gp"].nugget == NUGGET
    return mc


def test_closed_forms_agree_with_the_pathwise_draws():
    mc = _moment_case()
    gp, X = mc["gp"], mc["X"]
    gp.load_right_vector(mc["dom"], mc["bdy"], mc["alpha"])
    draws = gp.sample_functions(ref.MOMENT_DRAWS, seed=ref.MOMENT_SEED, n_features=ref.MOMENT_FEATURES)     # z = None: K_p right_vector of the loaded model
    fun = draws.functionals(X)
    assert fun.shape == (4096, 8, 4)
    cov = gp.predict_functional_covariance(X)
    var, parts = gp.predict_residual_variance(X, return_parts=True)
    r_cov, r_var = ref.moment_ratios(fun, parts["mean"], cov, parts["c"], var[:, 0])
    print("4096 draws, F = 64: functional covariance within %.2f, residual variance within %.2f standard errors" % (r_cov, r_var))
    assert r_cov <= 6.0 and r_var <= 6.0


# ------------------------------------------------------------------------------------------------ 7. refusals and empty calls
def test_refusals_and_empty_calls():
    import torch
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear, Quadratic_Gradient_Reaction_Diffusion
    from scasml_gp_amd.models.GP import GP, GP_Grad_Dependent_Nonlinear
    mc = _moment_case()
    d, X = mc["d"], mc["X"]
    as_coded = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(7), compat="reference", laplacian_idx=[0, 1, 2, 3, 4])
    for call in (as_coded.predict_functional_covariance, as_coded.predict_residual_variance, as_coded.predict_residual_std):
        with pytest.raises(ValueError, match="compat=None: the as-coded matrix is not the Gram of one kernel"):
            call(np.zeros((2, 7), dtype=np.float32))
    untrained = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)
    untrained.kernel_phi_phi(mc["dom"], mc["bdy"])
    assert untrained.predict_functional_covariance(X).shape == (8, 4, 4)       # the covariance needs the points alone
    with pytest.raises(NotImplementedError, match="GPsolver"):
        untrained.predict_residual_variance(X)
    with pytest.raises(NotImplementedError):
        untrained.predict_residual_std(X)

    class NoOperator(Grad_Dependent_Nonlinear):
        F_parts = None
    for equation in (NoOperator(d + 1), Quadratic_Gradient_Reaction_Diffusion(d + 1)):
        other = GP(equation, compat=None)
        other.load_right_vector(mc["dom"], mc["bdy"], mc["alpha"])
        with pytest.raises(NotImplementedError):
            other.predict_residual_variance(X)
        assert other.predict_functional_covariance(X).shape == (8, 4, 4)
    gp = mc["gp"]
    gp.load_right_vector(mc["dom"], mc["bdy"], mc["alpha"])
    with pytest.raises(ValueError, match="shape"):
        gp.predict_functional_covariance(np.zeros((3, d + 2), dtype=np.float32))
    empty = gp.predict_functional_covariance(np.zeros((0, d + 1), dtype=np.float32))
    assert isinstance(empty, np.ndarray) and empty.shape == (0, 4, 4) and empty.dtype == np.float64
    et = gp.predict_functional_covariance(torch.zeros((0, d + 1), device="cuda"))
    assert isinstance(et, torch.Tensor) and et.is_cuda and tuple(et.shape) == (0, 4, 4)
    v, parts = gp.predict_residual_variance(np.zeros((0, d + 1), dtype=np.float32), return_parts=True)
    assert v.shape == (0, 1) and parts["mean"].shape == (0, 4) and parts["c"].shape == (0, 4) and parts["residual"].shape == (0, 1)
