"""Float64 NumPy statement of GP leave-one-out cross-validation (Rasmussen & Williams 5.4.2), shared by test_gp_loo_host.py and test_gpu_gp_loo.py.

With K_p = K(a) + eta I, a = 1 / sigma^2, A = K_p^-1, alpha = A z:
    mean_i = z_i - alpha_i / A_ii,   var_i = 1 / A_ii,   resid_i = alpha_i / sqrt(A_ii),   logp_i = 1/2 log A_ii - alpha_i^2 / (2 A_ii) - 1/2 log 2 pi
    dLOO/dtheta = sum_i [ alpha_i (Z alpha)_i - 1/2 (1 + alpha_i^2 / A_ii) (Z A)_ii ] / A_ii,   Z = A dK_p/dtheta
The points, z and K_a = dK/da are those of _gp_evidence_ref."""
import numpy as np

from _gp_evidence_ref import SHAPES, U, cap, gram_da, oracle, points      # noqa: F401  (re-exported: the GPU tests take them from here)

NUGGET = 1e-2
BLOCKS = ("u_dom", "u_bdy", "lap_dom", "dt_dom", "div_dom")                # the Gram's block order


def z_of(d, M):
    """The feature values every test of a shape uses (those of the evidence tests)."""
    return np.random.default_rng(2000 + d).standard_normal(M)


def blocks(nd, nb):
    edges = [0, nd, nd + nb, 2 * nd + nb, 3 * nd + nb, 4 * nd + nb]
    return {name: slice(lo, hi) for name, lo, hi in zip(BLOCKS, edges[:-1], edges[1:])}


def inverse(Kp, z):
    """(A = K_p^-1 symmetrised, alpha = K_p^-1 z)."""
    A = np.linalg.inv(Kp)
    return 0.5 * (A + A.T), np.linalg.solve(Kp, z)


def loo_values(A, alpha, z):
    """The closed forms: {"mean", "variance", "residual", "log_predictive"} and the three terms of every log_predictive_i (an (M, 3) array)."""
    dA = np.diag(A)
    terms = np.stack([0.5 * np.log(dA), -alpha * alpha / (2.0 * dA), np.full_like(dA, -0.5 * np.log(2.0 * np.pi))], axis=1)
    return {"mean": z - alpha / dA, "variance": 1.0 / dA, "residual": alpha / np.sqrt(dA), "log_predictive": terms.sum(1)}, terms


def brute_force(Kp, z):
    """(mean, variance) of z_i predicted from the other M - 1 values, row and column i of K_p deleted, for every i."""
    M = len(z)
    mean, var = np.empty(M), np.empty(M)
    for i in range(M):
        keep = np.arange(M) != i
        k = Kp[keep, i]
        sol = np.linalg.solve(Kp[np.ix_(keep, keep)], np.stack([z[keep], k], axis=1))
        mean[i] = k @ sol[:, 0]
        var[i] = Kp[i, i] - k @ sol[:, 1]
    return mean, var


def grad_terms(A, alpha, Za, ZA_diag):
    """(t1_i, t2_i) of dLOO/dtheta = sum_i t1_i + t2_i from (Z alpha)_i and (Z A)_ii."""
    dA = np.diag(A)
    return alpha * Za / dA, -0.5 * (1.0 + alpha * alpha / dA) * ZA_diag / dA


def loo_and_grad(d, dom, bdy, sigma, nugget, z, drop=None):
    """NumPy statement: (LOO, the (M, 3) terms of the value, {"log_sigma": (t1, t2), "log_nugget": (t1, t2)} as arrays over i, cond(K_p)); a gradient
    is (t1 + t2).sum().  drop: the operator pair whose derivative gram_da zeroes."""
    og = oracle(d, sigma)
    M = 4 * len(dom) + len(bdy)
    z = np.asarray(z, dtype=np.float64)
    Kp = og.kernel_phi_phi(np.asarray(dom, dtype=np.float64), np.asarray(bdy, dtype=np.float64)) + nugget * np.eye(M)
    A, alpha = inverse(Kp, z)
    vals, terms = loo_values(A, alpha, z)
    Ka = gram_da(og, dom, bdy, drop)
    a = og.a
    q = ((A @ Ka) * A).sum(1)                         # (Z A)_ii for theta = a
    ta = grad_terms(A, alpha, A @ (Ka @ alpha), q)
    te = grad_terms(A, alpha, A @ alpha, (A * A).sum(1))
    grads = {"log_sigma": (-2 * a * ta[0], -2 * a * ta[1]), "log_nugget": (nugget * te[0], nugget * te[1])}
    return float(vals["log_predictive"].sum()), terms, grads, float(np.linalg.cond(Kp))


def loo_value(d, dom, bdy, sigma, nugget, z):
    """The value alone (the central differences of the host test step this)."""
    og = oracle(d, sigma)
    M = 4 * len(dom) + len(bdy)
    Kp = og.kernel_phi_phi(np.asarray(dom, dtype=np.float64), np.asarray(bdy, dtype=np.float64)) + nugget * np.eye(M)
    A, alpha = inverse(Kp, np.asarray(z, dtype=np.float64))
    return float(loo_values(A, alpha, z)[0]["log_predictive"].sum())
