"""GP leave-one-out cross-validation on the device: scasml_gp_gram_da_rows and scasml_gp_loo_da (csrc/gp_loo.hip), GP.loo, GP.loo_log_predictive and
GP.optimize_hyperparameters(objective="loo") against the float64 NumPy statement of tests/_gp_loo_ref.py.

Errors are counted in units of 2^-53 of the quantity's own scale.
* An entry of K_a: 2^-53 (|P_a| + r^2 |P| / 2) kappa.  Both sides form r^2 = |x|^2 + |y|^2 - 2 x.y in float64, which carries an ABSOLUTE error of order
  (d + 1) 2^-53 (|x|^2 + |y|^2) whatever the entry's size (on the diagonal the entry itself is -r^2 / 2 = 0), so the device is compared with K_a in
  np.longdouble from exact coordinate differences (the float32 inputs make every difference exact) and the first-order effect of that much error
  in r^2, |d entry / d r^2| (d + 1) 2^-53 (|x|^2 + |y|^2), is added to the unit (the derivative by a symmetric nudge of the longdouble table).
* q_i and v_i of scasml_gp_loo_da: 2^-53 sum |terms| of that row's own sum, the NumPy side summed in np.longdouble.  The kernel is fed NumPy's A and
  alpha, so only its arithmetic is measured.
These kernel-level ratios are asserted at 16 times the largest measured on the MI355X at these shapes (profiles/gp_loo_accuracy.json; the margin is
for other points and other boxes), and the bound of q_i and v_i must itself stay under the a-priori 2 Mp units and under 256 cond(K_p) units.
Everything in which the device solves with K_p itself is asserted at the cap 256 cond(K_p) 2^-53 (about 1e-8 here): zeroing the derivative of any
single operator pair moves dLOO/dlog sigma by four orders more (test_dropping_any_operator_pair_is_visible_far_above_the_cap)."""
import functools

import numpy as np
import pytest

import _gp_evidence_ref as eref
import _gp_loo_ref as ref

pytestmark = pytest.mark.gpu

# 16 x the largest ratios measured on the MI355X (profiles/gp_loo_accuracy.json).  The entries of K_a: the largest over SHAPES, 13.5 at (3, 50, 20) --
# a Lap-Lap entry whose polynomial nearly cancels; the float64 NumPy table is 24 of these units from the longdouble one there.  q_i and v_i: the
# largest of the two PER SHAPE, because the error of a sum grows with its length (0.41 units at M = 4, 8.3 at M = 560) and so does the a-priori bound
# 2 Mp it has to stay under: one bound for all shapes, 16 x 8.3, would be above 2 Mp = 64 at (1, 1, 0).
ROWS_BOUND = 16.0 * 13.55
LOO_DA_BOUND = {(1, 1, 0): 16.0 * 0.42, (3, 50, 20): 16.0 * 0.91, (5, 70, 0): 16.0 * 0.71, (31, 64, 1): 16.0 * 4.54, (33, 65, 63): 16.0 * 4.20,
                (100, 130, 40): 16.0 * 8.35}
NUGGET = ref.NUGGET
PANELS = (64, 128, 0)            # 64: (100, 130, 40) has nine panels, the last ragged, (3, 50, 20) four; 0: the library's default


def _gp(d, compat=None):
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    if compat == "reference":
        return GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat="reference", laplacian_idx=[0, 1, 2, 3, 4])
    return GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _case(d, nd, nb):
    """One shape's NumPy side, computed once: points, z, K_p, K_a, K_p^-1, alpha, cond(K_p) at the library's defaults, and the np.longdouble sums
    the kernel-level ratios are taken against."""
    dom, bdy = ref.points(d, nd, nb)
    sigma = float(_gp(d).sigma)
    og = ref.oracle(d, sigma)
    M = 4 * nd + nb
    z = ref.z_of(d, M)
    Kp = og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64)) + NUGGET * np.eye(M)
    A, alpha = ref.inverse(Kp, z)
    Ka = ref.gram_da(og, dom, bdy)
    L = np.longdouble
    Al, Kal = A.astype(L), Ka.astype(L)
    return _freeze(dict(d=d, nd=nd, nb=nb, M=M, dom=dom, bdy=bdy, sigma=sigma, a=og.a, z=z, Kp=Kp, A=A, alpha=alpha, Ka=Ka,
                        cond=float(np.linalg.cond(Kp)),
                        q=((Al @ Kal) * Al).sum(1), q_abs=((np.abs(A) @ np.abs(Ka)) * np.abs(A)).sum(1),
                        v=Kal @ alpha.astype(L), v_abs=np.abs(Ka) @ np.abs(alpha)))


class _ExactGeometry:
    """Stands in for OracleGP in _gp_evidence_ref.gram_da / pair_polynomials: the pair geometry in np.longdouble from exact coordinate differences,
    r^2 moved by nudge * (d + 1) 2^-53 (|x|^2 + |y|^2)."""

    def __init__(self, a, d, nudge=0.0):
        self.a, self.d, self.nudge = np.longdouble(a), d, nudge
        self._seen = {}                          # (id(X), id(Y)) -> (X, Y, geometry): the 25 blocks of a Gram share 4 pairs of point sets

    def _pairs(self, X0, Y0):
        hit = self._seen.get((id(X0), id(Y0)))
        if hit is not None and hit[0] is X0 and hit[1] is Y0:
            return hit[2]
        L = np.longdouble
        X, Y = np.asarray(X0, dtype=np.float64).astype(L), np.asarray(Y0, dtype=np.float64).astype(L)
        diff = X[:, None, :] - Y[None, :, :]
        r2 = (diff * diff).sum(-1) + self.nudge * (self.d + 1) * ref.U * ((X * X).sum(1)[:, None] + (Y * Y).sum(1)[None, :])
        rt = diff[..., -1]
        geometry = np.exp(-0.5 * self.a * r2), r2 - rt * rt, diff[..., :-1].sum(-1), rt
        self._seen[(id(X0), id(Y0))] = (X0, Y0, geometry)
        return geometry


@functools.lru_cache(maxsize=None)
def _rows_case(d, nd, nb):
    """(K_a in np.longdouble from exact differences, the unit of every entry as float64) -- see the module docstring."""
    c = _case(d, nd, nb)
    pts = {"dom": c["dom"].astype(np.float64), "bdy": c["bdy"].astype(np.float64)}
    exact = _ExactGeometry(c["a"], d)
    truth = eref.gram_da(exact, pts["dom"], pts["bdy"])

    def unit(ox, px, oy, py):
        P, Pa, kap, r2 = eref.pair_polynomials(exact, ox, oy, pts[px], pts[py])
        return (np.abs(Pa) + 0.5 * r2 * np.abs(P)) * kap

    scale = np.block([[unit(ox, px, oy, py) for (oy, py) in eref.ROWS] for (ox, px) in eref.ROWS])
    moved = eref.gram_da(_ExactGeometry(c["a"], d, 1.0), pts["dom"], pts["bdy"]) - eref.gram_da(_ExactGeometry(c["a"], d, -1.0), pts["dom"], pts["bdy"])
    # the floor: where r_t = S = 0 (a point against itself) the odd entries are exactly 0 on both sides, whatever r^2 is
    unit_all = (ref.U * scale + 0.5 * np.abs(moved)).astype(np.float64) + 1e-300
    unit_all.setflags(write=False)
    return truth, unit_all


def _cuda(x, dtype):
    import torch
    return torch.from_numpy(np.array(x, dtype=dtype)).cuda()


def _ragged_blocks(nd, nb):
    """[(row0, nrows, ncols)]: ragged row ranges that start inside one operator block and end inside the next -- u(dom) into its successor (u(bdy),
    or Lap(dom) without boundary points), u(bdy) into Lap(dom), dt(dom) into div(dom) -- each with fewer columns than M (a single point per block
    leaves no inside: whole blocks then)."""
    M, N = 4 * nd + nb, nd + nb
    cuts = [(nd // 2, nd + (nb + 1) // 2 if nb else N + (nd + 1) // 2, M - 1), (2 * nd + nb + nd // 2, 3 * nd + nb + (nd + 1) // 2, max(1, M - nd - 3))]
    if nb:
        cuts.append((nd + nb // 2, N + (nd + 1) // 2, N + 1))
    return [(lo, hi - lo, ncols) for lo, hi, ncols in cuts]


def gram_da_rows_ratio(d, nd, nb):
    """Largest |device - truth| / unit over the full matrix; the ragged blocks are asserted bit-equal to the same entries of the full matrix (an entry
    is a function of its pair of points alone) and to have written nothing outside themselves."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    c = _case(d, nd, nb)
    truth, unit = _rows_case(d, nd, nb)
    M = c["M"]
    xd, xb = _cuda(c["dom"], np.float32), _cuda(c["bdy"], np.float32)

    def rows(row0, nrows, ncols, ld):
        out = torch.full((nrows + 1, ld), float("nan"), dtype=torch.float64, device="cuda")       # one guard row, guard columns beyond ncols
        _lib.check(lib.scasml_gp_gram_da_rows(d, c["a"], _lib.ptr(xd), nd, _lib.ptr(xb) if nb else None, nb, row0, nrows, ncols, _lib.ptr(out), ld,
                                              _lib.stream_ptr()), "gp_gram_da_rows")
        got = out.cpu().numpy()
        assert np.isnan(got[nrows]).all() and np.isnan(got[:nrows, ncols:]).all()
        return got[:nrows, :ncols]

    full = rows(0, M, M, M + 3)
    assert np.isfinite(full).all() and np.array_equal(full, full.T)
    for row0, nrows, ncols in _ragged_blocks(nd, nb):
        assert nrows > 0 and row0 + nrows <= M and ncols < M
        assert np.array_equal(rows(row0, nrows, ncols, ncols + 5), full[row0:row0 + nrows, :ncols]), (row0, nrows, ncols)
    err = np.abs((full.astype(np.longdouble) - truth).astype(np.float64))
    return float((err / unit).max())


def loo_da_ratios(d, nd, nb):
    """(largest ratio of q_i, largest ratio of v_i, cap as a ratio) of scasml_gp_loo_da fed NumPy's A and alpha, at panel_rows = 64, 128 and the
    default, each run twice: the bits must be equal across all six runs, nothing beyond the M outputs and the stated workspace may be touched."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    c = _case(d, nd, nb)
    M = c["M"]
    xd, xb = _cuda(c["dom"], np.float32), _cuda(c["bdy"], np.float32)
    A, alpha = _cuda(c["A"], np.float64), _cuda(c["alpha"], np.float64)
    GUARD = 1024
    runs = []
    for panel_rows in PANELS:
        need = int(lib.scasml_gp_loo_da_doubles(nd, nb, panel_rows))
        assert need > 0
        for _ in range(2):
            q, v = (torch.full((M + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
            work = torch.full((need + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
            _lib.check(lib.scasml_gp_loo_da(d, c["a"], _lib.ptr(xd), nd, _lib.ptr(xb) if nb else None, nb, _lib.ptr(A), M, _lib.ptr(alpha), panel_rows,
                                            _lib.ptr(q), _lib.ptr(v), _lib.ptr(work), _lib.stream_ptr()), "gp_loo_da")
            assert bool(torch.isnan(work[need:]).all()) and bool(torch.isnan(q[M:]).all()) and bool(torch.isnan(v[M:]).all())
            runs.append((q[:M].cpu().numpy(), v[:M].cpu().numpy()))
    q0, v0 = runs[0]
    assert np.isfinite(q0).all() and np.isfinite(v0).all()
    for q, v in runs[1:]:
        assert np.array_equal(q, q0) and np.array_equal(v, v0)                     # the same bits on every run and for every panel_rows
    L = np.longdouble
    rq = np.abs(q0.astype(L) - c["q"]).astype(np.float64) / (ref.U * c["q_abs"])
    rv = np.abs(v0.astype(L) - c["v"]).astype(np.float64) / (ref.U * c["v_abs"])
    return float(rq.max()), float(rv.max()), 256.0 * c["cond"]


@pytest.mark.parametrize("d,nd,nb", ref.SHAPES)
def test_gram_da_rows_match_numpy_entry_by_entry(d, nd, nb):
    r = gram_da_rows_ratio(d, nd, nb)
    print("(%d, %d, %d): K_a rows off by at most %.2f units; asserted at %.0f" % (d, nd, nb, r, ROWS_BOUND))
    assert r <= ROWS_BOUND


@pytest.mark.parametrize("d,nd,nb", ref.SHAPES)
def test_loo_da_matches_numpy_and_is_the_same_bits_for_every_panel(d, nd, nb):
    rq, rv, cap_ratio = loo_da_ratios(d, nd, nb)
    Mp = (4 * nd + nb + 31) // 32 * 32
    bound = LOO_DA_BOUND[(d, nd, nb)]
    print("(%d, %d, %d): q off by %.2f, v by %.2f units of 2^-53 sum|terms| of the row; asserted at %.1f, a priori %d, cap %.3g" % (
        d, nd, nb, rq, rv, bound, 2 * Mp, cap_ratio))
    assert bound <= 2 * Mp and bound <= cap_ratio
    assert rq <= bound and rv <= bound


@pytest.mark.parametrize("d,nd,nb", ref.SHAPES)
def test_class_level_values_and_gradient_match_numpy(d, nd, nb):
    c = _case(d, nd, nb)
    value, terms, grads, cond = ref.loo_and_grad(d, c["dom"], c["bdy"], c["sigma"], NUGGET, c["z"])
    want, _ = ref.loo_values(c["A"], c["alpha"], c["z"])
    cap = ref.cap(cond)
    gp = _gp(d)
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    got = gp.loo(c["z"])
    assert set(got) == {"mean", "variance", "residual", "log_predictive", "blocks"} and got["blocks"] == ref.blocks(nd, nb)
    # Per-feature scales.  The device's A is (K_p + E)^-1 with |E| of order 2^-53 |K_p|, so dA = -A E A: A_ii moves by at most cond 2^-53 of ITSELF
    # (|A e_i|^2 <= |A| A_ii for a positive definite A) and the residual alpha_i / sqrt(A_ii) by cond 2^-53 of |resid_i| + sqrt(z^T alpha)
    # (|alpha|^2 <= |A| z^T alpha).  The other quantities are those two put together: mean_i - z_i = -resid_i / sqrt(A_ii), log_predictive_i =
    # 1/2 log A_ii - resid_i^2 / 2 - const.
    dA, resid = np.diag(c["A"]), np.abs(want["residual"])
    spread = resid + np.sqrt(float(c["z"] @ c["alpha"]))
    scales = {"mean": np.abs(c["z"]) + spread / np.sqrt(dA), "variance": 1.0 / dA, "residual": spread, "log_predictive": 0.5 + resid * spread}
    errs = {}
    for k, scale in scales.items():
        assert got[k].dtype == np.float64 and got[k].shape == (c["M"],)
        errs[k] = float((np.abs(got[k] - want[k]) / scale).max())
    v, grad = gp.loo_log_predictive(c["z"], return_grad=True)
    assert isinstance(v, float) and set(grad) == {"log_sigma", "log_nugget"}
    ev = abs(v - value) / float(np.abs(terms).sum())
    eg = {k: abs(grad[k] - float((t1 + t2).sum())) / float(np.abs(t1).sum() + np.abs(t2).sum()) for k, (t1, t2) in grads.items()}
    print("(%d, %d, %d): LOO %.6f off by %.2e, d/dlog sigma %.6g off by %.2e, d/dlog nugget %.6g off by %.2e (relative to sum |terms|); per-feature "
          "mean %.2e, variance %.2e, residual %.2e, log_predictive %.2e; cap %.2e" % (d, nd, nb, v, ev, grad["log_sigma"], eg["log_sigma"],
                                                                                   grad["log_nugget"], eg["log_nugget"], errs["mean"], errs["variance"],
                                                                                   errs["residual"], errs["log_predictive"], cap))
    assert ev <= cap and eg["log_sigma"] <= cap and eg["log_nugget"] <= cap
    assert max(errs.values()) <= cap
    assert gp.loo_log_predictive(c["z"]) == v                                             # the value alone: the same bits
    assert gp.loo_log_predictive(c["z"], return_grad=True) == (v, grad)                   # two calls: the same bits
    again = gp.loo(c["z"])
    assert all(np.array_equal(again[k], got[k]) for k in scales)
    assert abs(float(got["log_predictive"].sum()) - v) <= 4.0 * c["M"] * ref.U * float(np.abs(got["log_predictive"]).sum())      # two summation orders
    gp.loo_panel_rows = 64                                                                # the panel height does not reach the result
    assert gp.loo_log_predictive(c["z"], return_grad=True) == (v, grad)


@pytest.mark.parametrize("d,nd,nb", [(3, 50, 20), (5, 70, 0), (31, 64, 1), (33, 65, 63)])
def test_dropping_any_operator_pair_is_visible_far_above_the_cap(d, nd, nb):
    """NumPy only: what keeps the cap meaningful.  With the derivative of ANY single operator pair zeroed, dLOO/dlog sigma moves by at least 1e4 caps
    of sum_i |t1_i| + |t2_i| (1.7e-4 of it was the smallest move found when the formulas were derived; the cap is about 1e-8)."""
    c = _case(d, nd, nb)
    _, _, grads, cond = ref.loo_and_grad(d, c["dom"], c["bdy"], c["sigma"], NUGGET, c["z"])
    t1, t2 = grads["log_sigma"]
    whole, scale = float((t1 + t2).sum()), float(np.abs(t1).sum() + np.abs(t2).sum())
    pairs = [(ox, oy) for i, ox in enumerate(eref.OPS) for oy in eref.OPS[i:]]
    assert len(pairs) == 10
    moves = {}
    for pair in pairs:
        m1, m2 = ref.loo_and_grad(d, c["dom"], c["bdy"], c["sigma"], NUGGET, c["z"], drop=pair)[2]["log_sigma"]
        moves[pair] = abs(float((m1 + m2).sum()) - whole) / scale
    print("(%d, %d, %d): smallest move %.3e at %s; cap %.3e" % (d, nd, nb, min(moves.values()), min(moves, key=moves.get), ref.cap(cond)))
    assert min(moves.values()) >= 1e4 * ref.cap(cond)


def test_overrides_equal_a_fresh_gp_bit_for_bit_and_leave_the_object_alone():
    import torch
    d, nd, nb = 3, 50, 20
    c = _case(d, nd, nb)
    gp = _gp(d)
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    L, L_bits = gp._L_pad, gp._L_pad.clone()
    sigma2, nugget2 = 1.3 * c["sigma"], 3e-3
    got = gp.loo_log_predictive(c["z"], return_grad=True, sigma=sigma2, nugget=nugget2)
    got_loo = gp.loo(c["z"], sigma=sigma2, nugget=nugget2)
    assert (gp.sigma, gp.nugget) == (c["sigma"], NUGGET) and gp._L_pad is L and torch.equal(L, L_bits)
    fresh = _gp(d)
    fresh.sigma, fresh.nugget = sigma2, nugget2
    fresh.kernel_phi_phi(c["dom"], c["bdy"])
    assert fresh.loo_log_predictive(c["z"], return_grad=True) == got
    fresh_loo = fresh.loo(c["z"])
    assert all(np.array_equal(fresh_loo[k], got_loo[k]) for k in ("mean", "variance", "residual", "log_predictive"))
    own = gp.loo_log_predictive(c["z"], return_grad=True)
    assert own != got and gp.loo_log_predictive(c["z"], return_grad=True, sigma=c["sigma"], nugget=NUGGET) == own
    fresh.nugget = NUGGET                                                                 # one parameter overridden: the other is the object's
    assert gp.loo_log_predictive(c["z"], sigma=sigma2) == fresh.loo_log_predictive(c["z"])


def test_optimiser_maximises_the_loo_likelihood_of_a_prior_draw():
    d, nd, nb = 3, 50, 20
    c = _case(d, nd, nb)
    s_true, e_true, M = c["sigma"], NUGGET, c["M"]
    z = np.linalg.cholesky(c["Kp"]) @ np.random.default_rng(7).standard_normal(M)
    gp = _gp(d)
    gp.sigma, gp.nugget = 2.0 * s_true, 10.0 * e_true
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    rep = gp.optimize_hyperparameters(z, objective="loo")
    numpy_at = lambda s, e: ref.loo_and_grad(d, c["dom"], c["bdy"], s, e, z)
    v_end, _, g_end, cond = numpy_at(rep["sigma"], rep["nugget"])
    g_end = {k: float((t1 + t2).sum()) for k, (t1, t2) in g_end.items()}
    v_start, v_true = numpy_at(2.0 * s_true, 10.0 * e_true)[0], numpy_at(s_true, e_true)[0]
    gtol = 1e-4 * M
    print("optimiser: sigma %.4f sigma*, nugget %.4f eta*, LOO %.3f (NumPy %.3f; start %.3f, truth %.3f), NumPy gradient %.2e / %.2e, %d evaluations, "
          "%d iterations" % (rep["sigma"] / s_true, rep["nugget"] / e_true, rep["loo"], v_end, v_start, v_true, g_end["log_sigma"], g_end["log_nugget"],
                             rep["evaluations"], rep["iterations"]))
    assert set(rep) == {"objective", "sigma_start", "nugget_start", "loo_start", "sigma", "nugget", "loo", "grad", "evaluations", "iterations", "converged"}
    assert rep["objective"] == "loo" and rep["converged"] and rep["iterations"] <= 50
    assert v_end >= v_start and v_end >= v_true
    assert max(abs(g_end["log_sigma"]), abs(g_end["log_nugget"])) <= 2.0 * gtol
    assert (rep["sigma_start"], rep["nugget_start"]) == (2.0 * s_true, 10.0 * e_true) and abs(rep["loo_start"] - v_start) <= 1e-6 * abs(v_start)
    assert (gp.sigma, gp.nugget) == (rep["sigma"], rep["nugget"])
    X = np.random.default_rng(11).uniform(-0.5, 0.5, (70, d + 1)).astype(np.float32)
    fresh = _gp(d)
    fresh.sigma, fresh.nugget = rep["sigma"], rep["nugget"]
    fresh.kernel_phi_phi(c["dom"], c["bdy"])
    assert np.array_equal(gp.predict_variance(X), fresh.predict_variance(X))
    fresh.load_right_vector(c["dom"], c["bdy"], gp.right_vector)
    assert np.array_equal(gp.predict(X), fresh.predict(X))


def test_refusals_and_the_default_objective():
    from scasml_gp_amd import _lib
    d, nd, nb = 5, 70, 0
    c = _case(d, nd, nb)
    coded = _gp(d, compat="reference")
    for call in (lambda: coded.loo(c["z"]), lambda: coded.loo_log_predictive(c["z"]), lambda: coded.optimize_hyperparameters(c["z"], objective="loo")):
        with pytest.raises(ValueError):
            call()
    gp = _gp(d)
    for call in (lambda: gp.loo(c["z"]), lambda: gp.loo_log_predictive(c["z"]), lambda: gp.optimize_hyperparameters(c["z"], objective="loo")):
        with pytest.raises(_lib.ScasmlError):                                             # no collocation points
            call()
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    with pytest.raises(_lib.ScasmlError):
        gp.loo_log_predictive()                                                           # no fit and no right_vector: no default z
    for call in (lambda: gp.loo(c["z"][:-1]), lambda: gp.loo_log_predictive(c["z"][:-1]), lambda: gp.optimize_hyperparameters(c["z"], objective="cv"),
                 lambda: gp.loo_log_predictive(c["z"], nugget=0.0)):
        with pytest.raises(ValueError):
            call()
    # the keyword omitted and objective="lml": two otherwise identical GPs return identical reports
    reports = []
    for kw in ({}, {"objective": "lml"}):
        g = _gp(d)
        g.sigma, g.nugget = 1.5 * c["sigma"], 3.0 * NUGGET
        g.kernel_phi_phi(c["dom"], c["bdy"])
        reports.append(g.optimize_hyperparameters(c["z"], max_iter=3, **kw))
    assert reports[0] == reports[1] and "objective" not in reports[0] and "lml" in reports[0]
