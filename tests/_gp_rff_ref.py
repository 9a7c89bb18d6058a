"""NumPy statement of the pathwise GP posterior draws (GP.sample_functions, scasml_gp_rff_functionals, scasml_gp_rff_noise), shared by
test_gp_rff_host.py and test_gpu_gp_rff.py.

kappa(x, y) = exp(-a |x - y|^2 / 2) on (x_1 .. x_d, t) has the spectral measure omega ~ N(0, a I_{d+1}).  A prior draw with F features of its own:
    theta_f = omega_f . x (time last)      P_f = wc_f cos theta_f + ws_f sin theta_f      Q_f = ws_f cos theta_f - wc_f sin theta_f
    u = F^-1/2 sum P_f     Lap = F^-1/2 sum -|omega_f,x|^2 P_f     dt = F^-1/2 sum omega_f,t Q_f     div = F^-1/2 sum (sum_k omega_f,k) Q_f
Feature f of draw r: v = oracle.philox.normals(seed, STREAM_GP_RFF, [r], site = f, d + 3)[0]; omega_f = sqrt(a) * float64(v[0 : d+1]), wc_f = v[d+1],
ws_f = v[d+2].  Noise of draw r: normals(seed, STREAM_GP_RFF_NOISE, [r], site = 0, M)[0].  The sums are taken in np.longdouble.
A posterior draw: rv_s = K_p^-1 (z - Phi[f_s] - sqrt(eta) eps_s) by a dense float64 solve, post_s(x) = f_s(x) + k(x, phi)^T rv_s."""
import numpy as np

from oracle import philox

STREAM_GP_RFF = 0x47505246          # "GPRF" (include/scasml_hip.h: SCASML_STREAM_GP_RFF)
STREAM_GP_RFF_NOISE = 0x4750524E    # "GPRN" (SCASML_STREAM_GP_RFF_NOISE)
U = 2.0 ** -53
OPS = ("I", "lap", "dt", "div")     # the order of the four functionals, and of scasml_gp_cross_rows' op 0 .. 3


def feature_normals(d, seed, draws, F):
    """(len(draws), F, d + 3) float32: row [r, f] is oracle.philox.normals(seed, STREAM_GP_RFF, [draws[r]], site = f, d + 3)[0] (test_gp_rff_host.py
    checks that it is), every block of every feature and draw in one vectorised pass."""
    nq = (d + 3 + 3) // 4
    q = np.arange(nq, dtype=np.uint64)[None, None, :]
    f = np.arange(F, dtype=np.uint64)[None, :, None]
    r = np.asarray(draws, dtype=np.uint64)[:, None, None]
    words = philox.philox4x32_10(q, f, r, np.uint64(STREAM_GP_RFF), np.uint64(seed) & np.uint64(0xFFFFFFFF), np.uint64(seed) >> np.uint64(32))
    return np.stack([philox.icdf_normal(w) for w in words], axis=-1).reshape(len(r), F, 4 * nq)[:, :, :d + 3]


def features(d, a, F, seed, draw):
    """(omega (F, d+1) float64, wc (F,), ws (F,)) of one draw."""
    v = feature_normals(d, seed, [draw], F)[0].astype(np.float64)
    return np.sqrt(np.float64(a)) * v[:, :d + 1], v[:, d + 1], v[:, d + 2]


def multipliers(omega, d):
    """(F, 4): what P (columns 0, 1) and Q (columns 2, 3) of a feature are multiplied by in u, Lap, dt, div."""
    return np.stack([np.ones(len(omega)), -(omega[:, :d] ** 2).sum(1), omega[:, d], omega[:, :d].sum(1)], axis=1)


def per_feature(d, feats, X, dtype=np.longdouble):
    """(n, F, 4): the four functionals of every single feature at the rows of X, not yet summed or scaled."""
    omega, wc, ws = (v.astype(dtype) for v in feats)
    theta = np.asarray(X, dtype=np.float64).astype(dtype) @ omega.T     # (n, F)
    c, s = np.cos(theta), np.sin(theta)
    P, Q = wc * c + ws * s, ws * c - wc * s
    mult = multipliers(omega, d)
    return np.stack([P * mult[:, 0], P * mult[:, 1], Q * mult[:, 2], Q * mult[:, 3]], axis=-1)


def functionals(d, a, F, seed, draw, X, feats=None, with_unit=False):
    """(n, 4) np.longdouble: u, Lap, dt, div of prior draw `draw` at the rows of X (float32 values).  with_unit: also the (n, 4) error unit
    2^-53 F^-1/2 sum_f |mult_f| (|wc_f| + |ws_f|) (1 + (d + 2) sum_k |omega_fk x_k|) -- the second factor is the absolute error of theta entering
    the sine."""
    feats = feats if feats is not None else features(d, a, F, seed, draw)
    scale = 1 / np.sqrt(np.longdouble(F))
    out = per_feature(d, feats, X).sum(1) * scale
    if not with_unit:
        return out
    omega, wc, ws = feats
    theta_err = 1.0 + (d + 2) * (np.abs(np.asarray(X, dtype=np.float64)) @ np.abs(omega).T)           # (n, F)
    unit = U * float(scale) * (theta_err @ (np.abs(multipliers(omega, d)) * (np.abs(wc) + np.abs(ws))[:, None]))
    return out, unit


def gram_order(fd, fb):
    """phi = [u(dom), u(bdy), Lap(dom), dt(dom), div(dom)] from the (N, 4) functionals at the domain points and the (Nb, 4) at the boundary points."""
    return np.concatenate([fd[:, 0], fb[:, 0], fd[:, 1], fd[:, 2], fd[:, 3]])


def noise(seed, draw, M):
    return philox.normals(seed, STREAM_GP_RFF_NOISE, np.array([draw], dtype=np.uint64), 0, M)[0].astype(np.float64)


def cross_rows(og, X):
    """(4, n, M): the operator-op feature rows of X against the collocation sets og.kernel_phi_phi was given, op in OPS order."""
    return np.stack([og._features(op, np.asarray(X, dtype=np.float64)) for op in OPS])


def posterior_draw(og, Kp, z, eta, F, seed, draw, X=None, rows=None):
    """(rv (M,), phi (M,), eps (M,), values (n, 4) or None) of posterior draw `draw`: the dense float64 statement.  og has seen kernel_phi_phi(dom, bdy);
    rows = cross_rows(og, X) may be handed in (it is the same for every draw)."""
    d, a = og.d, og.a
    dom, bdy = og.x_t_domain, og.x_t_boundary
    feats = features(d, a, F, seed, draw)
    fd = functionals(d, a, F, seed, draw, dom, feats)
    fb = functionals(d, a, F, seed, draw, bdy, feats) if len(bdy) else np.zeros((0, 4))
    phi = gram_order(fd, fb).astype(np.float64)
    eps = noise(seed, draw, len(z))
    rv = np.linalg.solve(Kp, z - phi - np.sqrt(eta) * eps)
    if X is None:
        return rv, phi, eps, None
    rows = cross_rows(og, X) if rows is None else rows
    vals = functionals(d, a, F, seed, draw, X, feats).astype(np.float64) + np.stack([rows[k] @ rv for k in range(4)], axis=1)
    return rv, phi, eps, vals


def prior_draws(d, a, F, seed, draws, X):
    """(len(draws), n, 4) float64: the four functionals of many prior draws at once, plain float64 sums -- for statistics over thousands of draws
    (choosing the seed of a moment test on the CPU), not for rounding-level comparisons."""
    v = feature_normals(d, seed, draws, F).astype(np.float64)            # (S, F, d + 3)
    omega, wc, ws = np.sqrt(np.float64(a)) * v[:, :, :d + 1], v[:, :, d + 1:d + 2], v[:, :, d + 2:d + 3]
    theta = omega @ np.asarray(X, dtype=np.float64).T                    # (S, F, n)
    c, s = np.cos(theta), np.sin(theta)
    P, Q = wc * c + ws * s, ws * c - wc * s
    mult = np.stack([np.ones(omega.shape[:2]), -(omega[:, :, :d] ** 2).sum(-1), omega[:, :, d], omega[:, :, :d].sum(-1)], axis=-1)   # (S, F, 4)
    return np.stack([np.einsum("sfn,sf->sn", P if k < 2 else Q, mult[:, :, k]) for k in range(4)], axis=-1) / np.sqrt(F)


def moment_ratios(draws, mean, cov):
    """(largest |sample mean - mean| / standard error, largest |sample covariance - cov| / standard error) of (S, n) draws; the standard errors come
    from the sample variance of the draws and of their products -- the draws are not Gaussian at finite F."""
    S = draws.shape[0]
    m = draws.mean(0)
    r_mean = np.abs(m - mean) / (draws.std(0, ddof=1) / np.sqrt(S))
    c = draws - m
    prod = c[:, :, None] * c[:, None, :]                                 # (S, n, n)
    r_cov = np.abs(prod.sum(0) / (S - 1) - cov) / (prod.std(0, ddof=1) / np.sqrt(S))
    return float(r_mean.max()), float(r_cov.max())
