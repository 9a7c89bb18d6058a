"""GP log marginal likelihood on the device: scasml_chol_logdet, scasml_gp_gram_da_contract (csrc/gp_evidence.hip), GP.log_marginal_likelihood and
GP.optimize_hyperparameters against the float64 NumPy statement of tests/_gp_evidence_ref.py.

Errors are counted in units of 2^-53 * sum |terms| of the sum being checked.  The kernels' own sums (the contraction, the log-determinant) are fed
NumPy's A = K_p^-1, alpha and factor, so that only their arithmetic is measured; they are asserted at 16 times the largest ratio measured on the
MI355X at these shapes (profiles/gp_evidence_accuracy.json; the margin is for other points and other boxes).  Everything in which the device solves
with K_p itself is asserted at the cap 256 cond(K_p) 2^-53 (about 1e-8 here), which the measured bounds must stay under as well: zeroing the
derivative of any single operator pair moves the gradient by four orders more (test_dropping_any_operator_pair_is_visible_far_above_the_cap)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _gp_evidence_ref as ref

pytestmark = pytest.mark.gpu

# 16 x the largest ratio |device - NumPy| / (2^-53 sum |terms|) measured over SHAPES on the MI355X (profiles/gp_evidence_accuracy.json)
CONTRACT_BOUND = 16.0 * 0.81      # largest: <A, K_a> at (3, 50, 20), 0.809
LOGDET_BOUND = 16.0 * 1.36        # largest: (1, 1, 0), 1.356 (four terms)
NUGGET = 1e-2


def _gp(d, compat=None):
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    if compat == "reference":
        return GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat="reference", laplacian_idx=[0, 1, 2, 3, 4])
    return GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat=None)


@functools.lru_cache(maxsize=None)
def _case(d, nd, nb):
    """One shape's NumPy side, computed once: points, z, K, K_a, K_p^-1, alpha, the likelihood's terms and cond(K_p), at the library's defaults."""
    dom, bdy = ref.points(d, nd, nb)
    sigma = float(_gp(d).sigma)
    og = ref.oracle(d, sigma)
    M = 4 * nd + nb
    z = np.random.default_rng(2000 + d).standard_normal(M)
    K = og.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64))
    value, terms, alpha, A, Kp = ref.lml_terms(K, NUGGET, z)
    case = dict(d=d, nd=nd, nb=nb, M=M, dom=dom, bdy=bdy, sigma=sigma, a=og.a, z=z, K=K, Ka=ref.gram_da(og, dom, bdy), A=A, alpha=alpha, Kp=Kp,
                value=value, terms=terms, cond=float(np.linalg.cond(Kp)))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _cuda(x, dtype):
    import torch
    return torch.from_numpy(np.array(x, dtype=dtype)).cuda()


def contraction_ratios(d, nd, nb):
    """(ratio of out[0], ratio of out[1], cap as a ratio) of scasml_gp_gram_da_contract fed NumPy's A and alpha; also run twice for the bits."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    c = _case(d, nd, nb)
    xd, xb = _cuda(c["dom"], np.float32), _cuda(c["bdy"], np.float32)
    A, alpha = _cuda(c["A"], np.float64), _cuda(c["alpha"], np.float64)
    outs = []
    for _ in range(2):
        out = torch.full((int(lib.scasml_gp_gram_da_contract_doubles(nd, nb)),), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.scasml_gp_gram_da_contract(d, c["a"], _lib.ptr(xd), nd, _lib.ptr(xb) if nb else None, nb, _lib.ptr(A), c["M"], _lib.ptr(alpha),
                                                  _lib.ptr(out), _lib.stream_ptr()), "gp_gram_da_contract")
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.isfinite(outs[0]).all()           # the same bits on every run, partial sums included
    tq = np.outer(c["alpha"], c["alpha"]) * c["Ka"]
    tt = c["A"] * c["Ka"]
    rq = abs(outs[0][0] - tq.sum()) / (ref.U * np.abs(tq).sum())
    rt = abs(outs[0][1] - tt.sum()) / (ref.U * np.abs(tt).sum())
    return float(rq), float(rt), 256.0 * c["cond"]


def logdet_ratio(d, nd, nb):
    """Ratio of scasml_chol_logdet on NumPy's own factor, identity-padded to a multiple of 32 as scasml_cholesky leaves it."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    c = _case(d, nd, nb)
    Lh = np.linalg.cholesky(c["Kp"])
    Mp = (c["M"] + 31) // 32 * 32
    Lp = np.eye(Mp)
    Lp[:c["M"], :c["M"]] = Lh
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.scasml_chol_logdet(_lib.ptr(_cuda(Lp, np.float64)), Mp, _lib.ptr(out), _lib.stream_ptr()), "chol_logdet")
    terms = 2.0 * np.log(np.diag(Lh))
    return float(abs(float(out.item()) - terms.sum()) / (ref.U * np.abs(terms).sum())), 256.0 * c["cond"]


@pytest.mark.parametrize("d,nd,nb", ref.SHAPES)
def test_contraction_matches_numpy(d, nd, nb):
    rq, rt, cap_ratio = contraction_ratios(d, nd, nb)
    print("(%d, %d, %d): alpha^T K_a alpha off by %.2f, <A, K_a> by %.2f units of 2^-53 sum|terms|; asserted at %.0f, cap %.3g" % (
        d, nd, nb, rq, rt, CONTRACT_BOUND, cap_ratio))
    assert CONTRACT_BOUND <= cap_ratio
    assert rq <= CONTRACT_BOUND and rt <= CONTRACT_BOUND


@pytest.mark.parametrize("d,nd,nb", ref.SHAPES)
def test_logdet_matches_numpy(d, nd, nb):
    r, cap_ratio = logdet_ratio(d, nd, nb)
    print("(%d, %d, %d): log det off by %.2f units of 2^-53 sum|terms|; asserted at %.0f, cap %.3g" % (d, nd, nb, r, LOGDET_BOUND, cap_ratio))
    assert LOGDET_BOUND <= cap_ratio
    assert r <= LOGDET_BOUND


@pytest.mark.parametrize("d,nd,nb", [(3, 50, 20), (5, 70, 0), (31, 64, 1), (33, 65, 63)])
def test_dropping_any_operator_pair_is_visible_far_above_the_cap(d, nd, nb):
    """NumPy only: what keeps the cap meaningful.  With the derivative of ANY single operator pair zeroed, dLML/dlog sigma moves by at least
    1e4 caps of |term1| + |term2| (4.3e-4 of it was the smallest move found when the table was derived; the cap is about 1e-8)."""
    c = _case(d, nd, nb)
    term = lambda Ka: (-c["a"] * float(c["alpha"] @ Ka @ c["alpha"]), c["a"] * float((c["A"] * Ka).sum()))
    t1, t2 = term(c["Ka"])
    og = ref.oracle(d, c["sigma"])
    pairs = [(ox, oy) for i, ox in enumerate(ref.OPS) for oy in ref.OPS[i:]]
    assert len(pairs) == 10
    moves = {}
    for pair in pairs:
        m1, m2 = term(ref.gram_da(og, c["dom"], c["bdy"], drop=pair))
        moves[pair] = abs((m1 + m2) - (t1 + t2)) / (abs(t1) + abs(t2))
    print("(%d, %d, %d): smallest move %.3e at %s; cap %.3e" % (d, nd, nb, min(moves.values()), min(moves, key=moves.get), ref.cap(c["cond"])))
    assert min(moves.values()) >= 1e4 * ref.cap(c["cond"])


@pytest.mark.parametrize("d,nd,nb", ref.SHAPES)
def test_likelihood_and_gradient_match_numpy(d, nd, nb):
    c = _case(d, nd, nb)
    _, _, grads, cond = ref.lml_and_grad(d, c["dom"], c["bdy"], c["sigma"], NUGGET, c["z"])
    gp = _gp(d)
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    value, grad = gp.log_marginal_likelihood(c["z"], return_grad=True)
    assert isinstance(value, float) and set(grad) == {"log_sigma", "log_nugget"}
    cap = ref.cap(cond)
    ev = abs(value - c["value"]) / sum(abs(t) for t in c["terms"])
    eg = {k: abs(grad[k] - sum(grads[k])) / (abs(grads[k][0]) + abs(grads[k][1])) for k in grads}
    print("(%d, %d, %d): LML %.6f off by %.2e, d/dlog sigma %.6g off by %.2e, d/dlog nugget %.6g off by %.2e (relative to sum |terms|); cap %.2e" % (
        d, nd, nb, value, ev, grad["log_sigma"], eg["log_sigma"], grad["log_nugget"], eg["log_nugget"], cap))
    assert ev <= cap and eg["log_sigma"] <= cap and eg["log_nugget"] <= cap
    assert gp.log_marginal_likelihood(c["z"]) == value                                   # the value alone: the same bits
    assert gp.log_marginal_likelihood(c["z"], return_grad=True) == (value, grad)         # two calls: the same bits


def test_overrides_equal_a_fresh_gp_bit_for_bit_and_leave_the_object_alone():
    import torch
    d, nd, nb = 3, 50, 20
    c = _case(d, nd, nb)
    gp = _gp(d)
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    L, L_bits = gp._L_pad, gp._L_pad.clone()
    sigma2, nugget2 = 1.3 * c["sigma"], 3e-3
    got = gp.log_marginal_likelihood(c["z"], return_grad=True, sigma=sigma2, nugget=nugget2)
    assert (gp.sigma, gp.nugget) == (c["sigma"], NUGGET) and gp._L_pad is L and torch.equal(L, L_bits)
    fresh = _gp(d)
    fresh.sigma, fresh.nugget = sigma2, nugget2
    fresh.kernel_phi_phi(c["dom"], c["bdy"])
    assert fresh.log_marginal_likelihood(c["z"], return_grad=True) == got
    own = gp.log_marginal_likelihood(c["z"], return_grad=True)
    assert own != got and gp.log_marginal_likelihood(c["z"], return_grad=True, sigma=c["sigma"], nugget=NUGGET) == own
    # one parameter overridden: the other is the object's
    fresh.nugget = NUGGET
    assert gp.log_marginal_likelihood(c["z"], sigma=sigma2) == fresh.log_marginal_likelihood(c["z"])


def test_default_z_is_the_fits_feature_vector():
    """After GPsolver z = None is b(sol) = [z1, g, z3, F(sol), z5]; after load_state_dict into a fresh object it is K_p right_vector."""
    import torch
    from scasml_gp_amd import _lib
    d, nd, nb = 3, 50, 20
    c = _case(d, nd, nb)
    gp = _gp(d)
    gp.GPsolver(c["dom"], c["bdy"])
    N = nd
    sol = gp._sol.cpu().numpy()
    g = gp.bdy_g(c["bdy"])
    b_dev = torch.empty(c["M"], dtype=torch.float64, device="cuda")                      # b(sol) by the library's own kernel
    _lib.check(_lib.load().scasml_gp_newton_b(int(gp.equation.eq_id), d, float(gp.equation.sigma()), float(gp.equation.mu()), _lib.ptr(gp._sol),
                                              _lib.ptr(_cuda(g, np.float64)), N, nb, _lib.ptr(b_dev), _lib.stream_ptr()), "gp_newton_b")
    trained = gp.log_marginal_likelihood(return_grad=True)
    assert trained == gp.log_marginal_likelihood(b_dev, return_grad=True)
    b_host = np.concatenate([sol[:N], g, sol[N:2 * N], gp.time_der_rep(sol, 0.0), sol[2 * N:]])      # ... and written out on the host
    value, terms, _, _, Kp = ref.lml_terms(c["K"], NUGGET, b_host)
    cap, scale = ref.cap(float(np.linalg.cond(Kp))), sum(abs(t) for t in terms)
    print("after GPsolver: LML(z = None) = %.6f, NumPy on b(sol) %.6f, cap %.2e" % (trained[0], value, cap))
    assert abs(trained[0] - value) <= cap * scale
    assert abs(gp.log_marginal_likelihood(b_host) - trained[0]) <= cap * scale
    fresh = _gp(d).load_state_dict(gp.state_dict())
    loaded = fresh.log_marginal_likelihood()
    print("after load_state_dict: LML(z = K_p right_vector) = %.6f, off by %.2e of sum |terms|" % (loaded, abs(loaded - trained[0]) / scale))
    assert abs(loaded - trained[0]) <= cap * scale


def test_optimiser_recovers_the_hyperparameters_of_a_prior_draw():
    d, nd, nb = 3, 50, 20
    c = _case(d, nd, nb)
    s_true, e_true, M = c["sigma"], NUGGET, c["M"]
    z = np.linalg.cholesky(c["Kp"]) @ np.random.default_rng(7).standard_normal(M)
    gp = _gp(d)
    gp.sigma, gp.nugget = 2.0 * s_true, 10.0 * e_true
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    rep = gp.optimize_hyperparameters(z)
    numpy_at = lambda s, e: ref.lml_and_grad(d, c["dom"], c["bdy"], s, e, z)
    v_end, _, g_end, cond = numpy_at(rep["sigma"], rep["nugget"])
    v_start, v_true = numpy_at(2.0 * s_true, 10.0 * e_true)[0], numpy_at(s_true, e_true)[0]
    gtol = 1e-4 * M
    print("optimiser: sigma %.4f sigma*, nugget %.4f eta*, LML %.3f (NumPy %.3f; start %.3f, truth %.3f), NumPy gradient %.2e / %.2e, %d evaluations, "
          "%d iterations" % (rep["sigma"] / s_true, rep["nugget"] / e_true, rep["lml"], v_end, v_start, v_true, sum(g_end["log_sigma"]),
                             sum(g_end["log_nugget"]), rep["evaluations"], rep["iterations"]))
    assert rep["converged"] and rep["iterations"] <= 50
    assert v_end >= v_start and v_end >= v_true
    assert max(abs(sum(g_end["log_sigma"])), abs(sum(g_end["log_nugget"]))) <= 2.0 * gtol
    assert 2.0 * s_true / 8.0 <= rep["sigma"] <= 2.0 * s_true * 8.0 and 1e-6 <= rep["nugget"] <= 1.0
    assert (rep["sigma_start"], rep["nugget_start"]) == (2.0 * s_true, 10.0 * e_true) and abs(rep["lml_start"] - v_start) <= 1e-6 * abs(v_start)
    assert (gp.sigma, gp.nugget) == (rep["sigma"], rep["nugget"])
    og = ref.oracle(d, rep["sigma"])
    Kp = og.kernel_phi_phi(c["dom"].astype(np.float64), c["bdy"].astype(np.float64)) + rep["nugget"] * np.eye(M)
    rv = np.linalg.solve(Kp, z)
    assert np.abs(gp.right_vector[:, 0] - rv).max() <= ref.cap(cond) * np.abs(rv).max()
    # the cached factor follows the scale: predict_variance is that of a fresh GP holding the returned hyperparameters, bit for bit
    X = np.random.default_rng(11).uniform(-0.5, 0.5, (70, d + 1)).astype(np.float32)
    fresh = _gp(d)
    fresh.sigma, fresh.nugget = rep["sigma"], rep["nugget"]
    fresh.kernel_phi_phi(c["dom"], c["bdy"])
    assert np.array_equal(gp.predict_variance(X), fresh.predict_variance(X))
    fresh.load_right_vector(c["dom"], c["bdy"], gp.right_vector)
    assert np.array_equal(gp.predict(X), fresh.predict(X))                               # ... and predict sees the re-packed model at once


def test_refusals_and_state_round_trip():
    from scasml_gp_amd import _lib
    d, nd, nb = 5, 70, 0
    c = _case(d, nd, nb)
    coded = _gp(d, compat="reference")
    with pytest.raises(ValueError):
        coded.log_marginal_likelihood(c["z"])
    with pytest.raises(ValueError):
        coded.optimize_hyperparameters(c["z"])
    gp = _gp(d)
    with pytest.raises(_lib.ScasmlError):
        gp.log_marginal_likelihood(c["z"])
    with pytest.raises(_lib.ScasmlError):
        gp.optimize_hyperparameters(c["z"])
    gp.kernel_phi_phi(c["dom"], c["bdy"])
    with pytest.raises(_lib.ScasmlError):
        gp.log_marginal_likelihood()                                                     # no fit and no right_vector: no default z
    with pytest.raises(ValueError):
        gp.log_marginal_likelihood(c["z"][:-1])
    with pytest.raises(ValueError):
        gp.optimize_hyperparameters(c["z"], which=("sigma", "length"))
    gp.sigma = 1.25 * c["sigma"]
    gp.load_right_vector(c["dom"], c["bdy"], c["alpha"])
    state = gp.state_dict()
    assert float(state["sigma"]) == gp.sigma
    fresh = _gp(d).load_state_dict(state)
    assert fresh.sigma == gp.sigma and fresh.nugget == gp.nugget
    old = {k: v for k, v in state.items() if k != "sigma"}                               # a state saved before the scale was carried
    assert _gp(d).load_state_dict(old).sigma == c["sigma"]
