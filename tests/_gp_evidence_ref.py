"""Float64 NumPy statement of the GP log marginal likelihood and its gradient, shared by test_gp_evidence_host.py and test_gpu_gp_evidence.py.

K_a = dK/da is written in OracleGP.block's variables (a, rho^2, S, r_t): an entry of K is P(ox, oy) kappa with kappa = exp(-a r^2 / 2),
r^2 = rho^2 + r_t^2, so the entry of K_a is (P_a - r^2 P / 2) kappa with P_a = dP/da at fixed geometry (the table of DESIGN.md section 4.10)."""
import functools

import numpy as np

SHAPES = [(1, 1, 0), (3, 50, 20), (5, 70, 0), (31, 64, 1), (33, 65, 63), (100, 130, 40)]      # (d, N_dom, N_bdy)
OPS = ("I", "lap", "dt", "div")
ROWS = (("I", "dom"), ("I", "bdy"), ("lap", "dom"), ("dt", "dom"), ("div", "dom"))           # the Gram's block order
U = 2.0 ** -53


def oracle(d, sigma=None):
    from oracle.equation import GradDependentNonlinear
    from oracle.gp import OracleGP
    og = OracleGP(GradDependentNonlinear(d + 1))
    if sigma is not None:
        og.s2 = float(sigma) ** 2
        og.a = 1.0 / og.s2
    return og


@functools.lru_cache(maxsize=None)
def points(d, nd, nb):
    """Collocation points of oracle.equation.sample_points rounded to float32 (one draw per shape, shared by every test)."""
    from oracle.equation import sample_points
    dom, bdy = sample_points(np.random.default_rng(1000 + d), d, nd, max(nb, 1))
    dom = np.ascontiguousarray(dom, dtype=np.float32)
    bdy = np.ascontiguousarray(bdy[:nb], dtype=np.float32).reshape(nb, d + 1)
    for arr in (dom, bdy):
        arr.setflags(write=False)
    return dom, bdy


def pair_polynomials(og, opx, opy, X, Y):
    """(P, P_a, kappa, r^2) of one operator pair on the point pairs (X_i, Y_j)."""
    a, d = og.a, og.d
    kap, rho2, S, rt = og._pairs(np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64))
    lap, lap_a = a * a * rho2 - a * d, 2 * a * rho2 - d
    one = np.ones_like(kap)
    sign = -1.0 if opx in ("dt", "div") and opy in ("I", "lap") else 1.0           # the x-side first derivative flips the sign
    key = frozenset((opx, opy))
    if key == {"I"}:
        P, Pa = one, 0 * one
    elif key == {"I", "lap"}:
        P, Pa = lap, lap_a
    elif key == {"I", "dt"}:
        P, Pa = a * rt, rt
    elif key == {"I", "div"}:
        P, Pa = a * S, S
    elif key == {"dt"}:
        P, Pa = a - a * a * rt * rt, 1 - 2 * a * rt * rt
    elif key == {"dt", "div"}:
        P, Pa = -a * a * rt * S, -2 * a * rt * S
    elif key == {"div"}:
        P, Pa = a * d - a * a * S * S, d - 2 * a * S * S
    elif key == {"lap", "dt"}:
        P, Pa = a * rt * lap, rt * lap + a * rt * lap_a
    elif key == {"lap", "div"}:
        P, Pa = a * S * lap - 2 * a * a * S, S * lap + a * S * lap_a - 4 * a * S
    elif key == {"lap"}:
        P = a ** 4 * rho2 ** 2 - (2 * d + 4) * a ** 3 * rho2 + (d * d + 2 * d) * a * a
        Pa = 4 * a ** 3 * rho2 ** 2 - 3 * (2 * d + 4) * a * a * rho2 + 2 * (d * d + 2 * d) * a
    else:
        raise KeyError((opx, opy))
    return sign * P, sign * Pa, kap, rho2 + rt * rt


def gram_da(og, dom, bdy, drop=None):
    """K_a on the collocation sets, in the Gram's block order.  drop = (opx, opy): that pair's derivative (and its mirror's) zeroed -- the mutation
    the gradient checks must be able to see."""
    pts = {"dom": np.asarray(dom, dtype=np.float64), "bdy": np.asarray(bdy, dtype=np.float64)}

    def blk(ox, px, oy, py):
        P, Pa, kap, r2 = pair_polynomials(og, ox, oy, pts[px], pts[py])
        out = (Pa - 0.5 * r2 * P) * kap
        return 0 * out if drop is not None and frozenset((ox, oy)) == frozenset(drop) else out

    return np.block([[blk(ox, px, oy, py) for (oy, py) in ROWS] for (ox, px) in ROWS])


def lml_terms(K, nugget, z):
    """(value, its three terms, alpha, K_p^-1, K_p) of the log marginal likelihood."""
    M = K.shape[0]
    Kp = K + nugget * np.eye(M)
    Lh = np.linalg.cholesky(Kp)
    alpha = np.linalg.solve(Kp, z)
    terms = (-0.5 * float(z @ alpha), -float(np.log(np.diag(Lh)).sum()), -0.5 * M * float(np.log(2 * np.pi)))
    A = np.linalg.inv(Kp)
    return sum(terms), terms, alpha, 0.5 * (A + A.T), Kp


def lml_and_grad(d, dom, bdy, sigma, nugget, z, drop=None):
    """NumPy statement: (LML, its terms, {"log_sigma": (term1, term2), "log_nugget": (term1, term2)}, cond(K_p)); a gradient is term1 + term2."""
    og = oracle(d, sigma)
    K = og.kernel_phi_phi(np.asarray(dom, dtype=np.float64), np.asarray(bdy, dtype=np.float64))
    value, terms, alpha, A, Kp = lml_terms(K, nugget, np.asarray(z, dtype=np.float64))
    Ka = gram_da(og, dom, bdy, drop)
    a = og.a
    grads = {"log_sigma": (-2 * a * 0.5 * float(alpha @ Ka @ alpha), 2 * a * 0.5 * float((A * Ka).sum())),
             "log_nugget": (nugget * 0.5 * float(alpha @ alpha), -nugget * 0.5 * float(np.trace(A)))}
    return value, terms, grads, float(np.linalg.cond(Kp))


def cap(cond):
    """The largest relative error a check here may allow: 256 cond(K_p) 2^-53.  Zeroing the derivative of any single operator pair moves the
    gradient by >= 4e-4 of |term1| + |term2| (asserted where the cap is used), four orders above it."""
    return 256.0 * cond * U
