"""Float64 NumPy statement of the posterior covariance of the four functionals [u, Lap u, dt u, div u] of the GP surrogate at a point
(GP.predict_functional_covariance, scasml_gp_functional_covariance) and of the delta-method variance of the PDE residual
(GP.predict_residual_variance), on oracle.gp.OracleGP; shared by test_gp_functional_cov_host.py and test_gpu_gp_functional_cov.py.

    cov(x) = P - k(x) K_p^-1 k(x)^T,   k(x) the (4, M) rows K_o(x, phi), o in OPS,   K_p = K(phi, phi) + eta I
    P = prior_block(d, a): the 4 x 4 table of L_x^o L_y^p kappa at y = x (Appendix C of SURVEY.md at rho^2 = S = r_t = 0)
Route A: Cholesky of K_p, solve, P - V V^T.  Route B: one solve with K_p.  Every comparison is in SCALED units: entry (o, p) over
sqrt(P_oo P_pp) -- the four functionals differ by powers of a d, and an absolute tolerance would test the Laplacian alone."""
import functools

import numpy as np

OPS = ("I", "lap", "dt", "div")     # scasml_gp_cross_rows' op 0 .. 3
NUGGET = 1e-2
# The seed of the moment tests, chosen on the CPU: at this seed the NumPy statement alone (posterior_functional_draws: oracle normals, dense solves,
# 4096 draws of 64 features) puts the sample covariance of the four functionals within 1.67 and the sample variance of c . functionals within 1.29
# standard errors of the closed forms (test_gp_functional_cov_host.py asserts the cap of 6 for it); seeds 0 .. 5 give 1.67 .. 3.41 and 1.12 .. 2.25.
MOMENT_SEED, MOMENT_DRAWS, MOMENT_FEATURES = 4, 4096, 64


def prior_block(d, a):
    P = np.zeros((4, 4))
    P[0, 0] = 1.0
    P[0, 1] = P[1, 0] = -a * d
    P[1, 1] = (d * d + 2 * d) * a * a
    P[2, 2] = a
    P[3, 3] = a * d
    return P


def scale(P):
    """(4, 4): sqrt(P_oo P_pp)."""
    s = np.sqrt(np.diag(P))
    return s[:, None] * s[None, :]


def rows(og, X):
    """(n, 4, M): the four feature rows of every point, og having seen kernel_phi_phi(dom, bdy)."""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([og._features(op, X) for op in OPS], axis=1)


def route_a(Kp, k, P):
    """(n, 4, 4) by the factor: V_i = L^-1 k_i^T, P - V_i^T V_i."""
    n, _, M = k.shape
    V = np.linalg.solve(np.linalg.cholesky(Kp), k.reshape(4 * n, M).T).T.reshape(n, 4, M)
    return P[None] - np.einsum("iom,ipm->iop", V, V)


def route_b(Kp, k, P):
    """(n, 4, 4) by one solve with K_p."""
    n, _, M = k.shape
    W = np.linalg.solve(Kp, k.reshape(4 * n, M).T).T.reshape(n, 4, M)
    return P[None] - np.einsum("iom,ipm->iop", k, W)


def delta_host(cov_a, cov_b, P):
    """The largest scaled disagreement of the two host routes."""
    return float((np.abs(cov_a - cov_b) / scale(P)).max())


def tolerance(delta):
    """The rule of test_gpu_gp_variance.py: a float32 slip shows as >= 1e-7, so the case must resolve 1e-9; the device, a third backward-stable
    evaluation in another summation order, must agree with route A within max(32 delta_host, 1e-13)."""
    assert 32.0 * delta <= 1e-9, "the case is too ill-conditioned to expose a float32 slip: delta_host = %.3e" % delta
    return max(32.0 * delta, 1e-13)


def residual_parts(eq, k, rv, cov):
    """(means (n, 4), c (n, 4), residual mean (n,), variance (n,)) of r = dt u - F(u, Lap u, div u) linearised at the posterior-mean functionals
    m_o = k_o . rv:  c = [-dF/dz1, -dF/dz3, 1, -dF/dz5],  variance = c^T cov c."""
    m = k @ np.asarray(rv, dtype=np.float64).reshape(-1)
    F, (d1, d3, d5) = eq.F_parts(m[:, 0], m[:, 1], m[:, 3])[:2]
    ones = np.ones(len(m))
    c = np.stack([-d1 * ones, -d3 * ones, ones, -d5 * ones], axis=1)
    return m, c, m[:, 2] - F, np.einsum("io,iop,ip->i", c, cov, c)


def posterior_functional_draws(og, Kp, z, eta, F, seed, draws, X):
    """(len(draws), n, 4) float64: the four functionals of many pathwise posterior draws at the rows of X -- _gp_rff_ref.posterior_draw vectorised over
    the draws in plain float64 (statistics over thousands of draws: choosing the seed of the moment test on the CPU)."""
    import _gp_rff_ref as rff
    from oracle import philox
    d, a = og.d, og.a
    dom, bdy = og.x_t_domain, og.x_t_boundary
    draws = np.asarray(draws, dtype=np.uint64)
    fd = rff.prior_draws(d, a, F, seed, draws, dom)
    fb = rff.prior_draws(d, a, F, seed, draws, bdy)
    phi = np.concatenate([fd[:, :, 0], fb[:, :, 0], fd[:, :, 1], fd[:, :, 2], fd[:, :, 3]], axis=1)          # (S, M)
    eps = np.stack([philox.normals(seed, rff.STREAM_GP_RFF_NOISE, np.array([r], dtype=np.uint64), 0, len(z))[0] for r in draws]).astype(np.float64)
    rv = np.linalg.solve(Kp, (z[None, :] - phi - np.sqrt(eta) * eps).T).T                                    # (S, M)
    k = rows(og, X)                                                                                          # (n, 4, M)
    return rff.prior_draws(d, a, F, seed, draws, X) + np.einsum("nom,sm->sno", k, rv)


@functools.lru_cache(maxsize=None)
def moment_case():
    """The NumPy side of the moment tests, computed once and left unchanged: d = 3, 20 + 8 collocation points, z, K_p, alpha = K_p^-1 z, 8 points."""
    import _gp_loo_ref as lref
    from oracle.equation import sample_points
    d, nd, nb = 3, 20, 8
    dom, bdy = lref.points(d, nd, nb)
    og = lref.oracle(d)
    M = 4 * nd + nb
    z = lref.z_of(d, M)
    Kp = og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64)) + NUGGET * np.eye(M)
    case = dict(d=d, og=og, dom=dom, bdy=bdy, z=z, Kp=Kp, alpha=np.linalg.solve(Kp, z), X=sample_points(np.random.default_rng(4242), d, 8, 1)[0])
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def moment_ratios(fun, mean, cov, c, var):
    """The largest |sample - closed form| / standard error over the points (_gp_rff_ref.moment_ratios' standard errors) of (S, n, 4) draws of the
    functionals: (their covariance per point against cov (n, 4, 4), the variance of c . functionals against var (n,))."""
    import _gp_rff_ref as rff
    n = fun.shape[1]
    r_cov = max(rff.moment_ratios(fun[:, i, :], mean[i], cov[i])[1] for i in range(n))
    lin = (fun * c[None]).sum(-1)
    r_var = max(rff.moment_ratios(lin[:, i:i + 1], (mean[i] * c[i]).sum(keepdims=True), var[i].reshape(1, 1))[1] for i in range(n))
    return r_cov, r_var
