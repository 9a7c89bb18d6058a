"""NumPy statement of the per-component gradients of the pathwise GP posterior draws (scasml_gp_rff_gradient, GPFunctionDraws.gradient,
GP.posterior_mean_gradient), shared by test_gp_rff_gradient_host.py and test_gpu_gp_rff_gradient.py.  Built on _gp_rff_ref: the same features,
the same Q_f = ws_f cos theta_f - wc_f sin theta_f.

Prior term (sums in np.longdouble):      d_k u(x) = F^-1/2 sum_f omega_fk Q_f(x),   k = 0 .. d, time last.
Data term, the gradient of k(x, phi)^T v: with K0 the op-0 cross rows, r = x_i - y_j, and the collocation functional of column m,
    u_j:   alpha = -a K0[i,u_j]                          Lap_j: alpha = a (2a K0[i,u_j] - K0[i,Lap_j])
    dt_j:  alpha = -a K0[i,dt_j]                         div_j: alpha = -a K0[i,div_j], plus a K0[i,u_j] in every spatial component
    d_k K0[i,m] = r_k alpha   (k < d)                    d_t K0[i,m] = the op-2 ("dt") cross row
which is the alpha form of GP._data_gradient written column by column (gradient_rows), dense: (n, d+1, M).
Posterior covariance of the gradients: cov(d_k u(x_i), d_l u(x_j)) = kappa(x_i, x_j) (a delta_kl - a^2 r_k r_l) - G K_p^-1 G^T, G = gradient_rows."""
import numpy as np

import _gp_rff_ref as ref

U = ref.U


def prior_gradient(d, a, F, seed, draw, X, feats=None, with_unit=False):
    """(n, d+1) np.longdouble: the gradient of prior draw `draw` at the rows of X (float32 values).  with_unit: also the (n, d+1) error unit
    2^-53 F^-1/2 sum_f |omega_fk| (|wc_f| + |ws_f|) (1 + (d + 2) sum_j |omega_fj x_j|) -- the scale of the sum times the absolute error with which
    theta enters the sine."""
    L = np.longdouble
    feats = feats if feats is not None else ref.features(d, a, F, seed, draw)
    omega, wc, ws = (v.astype(L) for v in feats)
    X64 = np.asarray(X, dtype=np.float64)
    theta = X64.astype(L) @ omega.T                                        # (n, F)
    Q = ws * np.cos(theta) - wc * np.sin(theta)
    scale = 1 / np.sqrt(L(F))
    out = (Q @ omega) * scale
    if not with_unit:
        return out
    om, c, s = feats
    theta_err = 1.0 + (d + 2) * (np.abs(X64) @ np.abs(om).T)               # (n, F)
    unit = U * float(scale) * ((theta_err * (np.abs(c) + np.abs(s))) @ np.abs(om))
    return out, unit


def gradient_rows(og, X):
    """(n, d+1, M): the gradient in x of every op-0 cross row of X against the collocation sets og.kernel_phi_phi was given, by the alpha form."""
    d, a = og.d, og.a
    X = np.asarray(X, dtype=np.float64)
    dom, bdy = og.x_t_domain, og.x_t_boundary
    N, Nb = len(dom), len(bdy)
    K0 = og._features("I", X)                                              # (n, M)
    ku, kb = K0[:, :N], K0[:, N:N + Nb]
    kL, kt, kS = (K0[:, k * N + Nb:(k + 1) * N + Nb] for k in (1, 2, 3))
    alpha = np.concatenate([-a * ku, -a * kb, a * (2 * a * ku - kL), -a * kt, -a * kS], axis=1)          # (n, M)
    Y = np.concatenate([dom, bdy, dom, dom, dom])[:, :d]                   # the point of every column
    G = np.empty((len(X), d + 1, K0.shape[1]))
    G[:, :d, :] = (X[:, None, :d] - Y[None, :, :]).transpose(0, 2, 1) * alpha[:, None, :]
    G[:, :d, 3 * N + Nb:] += a * ku[:, None, :]
    G[:, d, :] = og._features("dt", X)
    return G


def data_gradient(og, X, v, G=None):
    """(n, d+1): the gradient of k(x, phi)^T v at the rows of X."""
    return (gradient_rows(og, X) if G is None else G) @ v


def posterior_gradient_covariance(og, Kp, X, G=None):
    """(n (d+1), n (d+1)), point-major: the posterior covariance of the gradient components at the rows of X."""
    d, a = og.d, og.a
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    G = (gradient_rows(og, X) if G is None else G).reshape(n * (d + 1), -1)
    r = X[:, None, :] - X[None, :, :]                                      # (n, n, d+1)
    kap = np.exp(-0.5 * a * (r * r).sum(-1))
    prior = kap[:, :, None, None] * (a * np.eye(d + 1)[None, None] - a * a * r[:, :, :, None] * r[:, :, None, :])    # (n, n, d+1, d+1)
    prior = prior.transpose(0, 2, 1, 3).reshape(n * (d + 1), n * (d + 1))
    return prior - G @ np.linalg.solve(Kp, G.T)


def prior_gradient_draws(d, a, F, seed, draws, X):
    """(len(draws), n, d+1) float64: the prior gradients of many draws at once, plain float64 sums -- for statistics over thousands of draws, not
    for rounding-level comparisons (as _gp_rff_ref.prior_draws)."""
    v = ref.feature_normals(d, seed, draws, F).astype(np.float64)           # (S, F, d + 3)
    omega, wc, ws = np.sqrt(np.float64(a)) * v[:, :, :d + 1], v[:, :, d + 1:d + 2], v[:, :, d + 2:d + 3]
    theta = omega @ np.asarray(X, dtype=np.float64).T                       # (S, F, n)
    Q = ws * np.cos(theta) - wc * np.sin(theta)
    return np.einsum("sfn,sfk->snk", Q, omega) / np.sqrt(F)


def posterior_gradient_draws(og, Kp, z, eta, F, seed, draws, X, G=None):
    """(len(draws), n, d+1) float64: the gradients of posterior draws by the dense statement (prior_gradient_draws, _gp_rff_ref.prior_draws and noise,
    a dense float64 solve)."""
    d, a = og.d, og.a
    fd = ref.prior_draws(d, a, F, seed, draws, og.x_t_domain)
    fb = ref.prior_draws(d, a, F, seed, draws, og.x_t_boundary) if len(og.x_t_boundary) else np.zeros((len(draws), 0, 4))
    phi = np.concatenate([fd[:, :, 0], fb[:, :, 0], fd[:, :, 1], fd[:, :, 2], fd[:, :, 3]], axis=1)      # (S, M)
    eps = np.stack([ref.noise(seed, r, len(z)) for r in draws])
    rv = np.linalg.solve(Kp, (z - phi - np.sqrt(eta) * eps).T)              # (M, S)
    G = gradient_rows(og, X) if G is None else G
    return prior_gradient_draws(d, a, F, seed, draws, X) + (G @ rv).transpose(2, 0, 1)
