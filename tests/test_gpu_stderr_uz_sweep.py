"""The z standard-error kernels (scasml_picard_tree_stderr_uz, picard_se_uz_kernel<VAR, MODE, N, EQ>: the walker under its SEZ flag) at every
lane-group width, level and mode, called through ctypes with the cases, batches, points and surrogate of tests/test_gpu_stderr_sweep.py.

out_se_uz holds rows (se_u, se_z_1 .. se_z_d).  Every output is prefilled with -3.0 and out_se_uz has one spare row after the batch (after the
site stride in a strided case); every launch asserts that the rows past B still hold -3.0.

Every (case, B) runs five checks:

(a) se_z against the float64 oracle's own summands in all 1 + d columns (PicardOracle.root_summands(with_z=True), one walk), within the project's
    bound per component, 2 (ATOL + RTOL max(|unclipped value|, se)) -- 2e-5 / 1e-4 in MLP mode, 5e-5 / 2e-4 in ACCUMULATE.  Guard 1: EVERY finite z
    component's oracle se is at least 10 x its bound (tests/test_gpu_picard_stderr_uz.py's rule; from the oracle alone the smallest is 18.9, MLP
    mode d = 252 quadrature (2, 3), medians 300 to 4000); column 0 carries the u-only entry's bits and keeps the u sweep's rule, the median root
    (single roots of it have an se_u below the bound: 0.5 x at d = 60).
    Guard 2 (test_dropping_any_z_term_would_be_noticed, from the oracle alone): for every required term j of every (variant, n, mode) some sweep
    case moves the median over all z components of |se - se without term j| / bound by >= 4.  The l = 0 term is exempt in MLP mode, where its
    z variance must be exactly 0, and required in ACCUMULATE.
(b) se_z against the DEVICE's own summands.  The sharded plain launches of the u sweep (world = 2, one summand's units owned) return that summand's
    unclipped float32 z in columns 1 .. d.  With Var and se64 formed from them per component in float64 as in the u sweep (per term j on the
    deviations dv from its first summand, S2_j = sum dv^2, v_j = N_j / (N_j - 1) (S2_j - S1_j^2 / N_j)), |Var32 - Var| <= B_var and
        |se_z - se64| <= max(sqrt(Var + B_var) - se64, se64 - sqrt(max(Var - B_var, 0))) + B_Y            (= B_var / (2 se64) + B_Y to first order)
        B_var = sum_j N_j / (N_j - 1) (3 N_j + 8) u S2_j + 2 u v_g + 4 u Var,      B_Y = u sqrt(sum_j k_j^2 N_j / (N_j - 1) sum_i Y_ji^2),  u = 2^-24,
        k_g = 6 for the terminal term and k_l = 4 for a level's.
    B_var is the u sweep's bound of SeTerm, which SeTerm4 repeats component by component, plus what SeTerm4 adds.  Per term, in units of
    u N / (N - 1) S2: the rounding of each dv moves S2 by 2 and S1^2 / N by 2 (|S1| sum |dv| / N <= S2); the N - 1 fmas into s2 add N - 1; the
    N - 2 additions into s1 move S1^2 / N by at most 2 (N - 1); -s1 / N, the closing fma, N / (N - 1) and the product with it add 4: 3 N + 5 of
    the 3 N + 8.  The spare 3 u v_j per term, 3 u Var in all, and the 4 u Var take the roundings of the sums into var (one per term after the
    first, at most 5, each at most u Var) and the final square root (u se, 2 u Var): 7 of 7.  close_into(var, N, scale) ends in ONE fma, the
    product with `scale` and the sum into var rounded together, so a level term (scale = 1, exact) has the roundings of SeTerm::close and no more.
    The terminal term accumulates the UNSCALED P_m = fl(g nrm_m) and closes with scale = fl(zs zs), zs = 1 / (mg (T - t + eps)): fl(zs zs) is
    zs^2 (1 + e), |e| <= u, and the product of the first fma into var = 0 is rounded once: 2 u v_g.  S2 of the P_m times zs^2 is S2 of the
    device's summands to a relative 2 u, of second order here.
    B_Y is the u sweep's allowance, 4 u |Y| (two ulps) by which a summand inside the kernel may differ from the sharded launch's, with the
    centring a projection: a perturbation e of a term's summands moves sqrt(v_j) by at most sqrt(N / (N - 1)) |e|_2, and se, the 2-norm of the
    sqrt(v_j), by at most the 2-norm of those.  The terminal term's summand in the sharded launch is fl(P_m zs), one rounding (u) that the kernel's
    zs^2 Var(P) does not make, and P_m = fl(g nrm_m) itself is a product that the u summand g / mg does not contain (u): k_g = 4 + 2.
    Derived, not fitted; tests/test_picard_stderr_uz_emulation.py shows on the CPU that a float32 emulation of SeTerm4 stays inside it.
    Where se64 = 0 the kernel's value is exactly 0; where se64 is not finite the kernel's is not finite either.
(c) out_uz and, in ACCUMULATE, out_uhat equal the plain launch's bit for bit; column 0 of out_se_uz equals the u-only entry's out_se bit for bit.
(d) a root's row of se_uz keeps its bits under every prefix batch and, in ACCUMULATE, under a site_stride past the batch with NaN in every
    padding row.
(e) quadrature at n >= 4: ACCUMULATE (4, 4) has a NaN u, so column 0 is NaN; MLP (4, 4) and DEEP_QUAD (5, 5) on its one root have a finite u
    and non-finite z (the q = 5 rule's nodes are not increasing: SURVEY.md Appendix B), so every se_z is non-finite, se_u is NaN exactly where
    the plain u is, and column 0 carries the u-only bits.  The expectation comes from check (b)'s device summands; the oracle, which walks these
    trees in 10 s and more, is consulted at one d and one root.

Beside the sweep: the table of all 50 instantiations, the read-back switch, the root counter wrap, a NaN coordinate, the solver classes, and
test_the_residual_addend_of_z_divides_by_its_own_step -- ScaSML's plans give the l = 0 term equal dplus and dminus tables, so only a plan in which
they differ can tell which of the two the residual addend's zm reads (a walker reading dplus there passed everything else in this file).

Measured on an MI355X (profiles/picard_stderr_uz_sweep.json, written when SCASML_STDERR_UZ_SWEEP_JSON names a file): check (b) reaches at most 0.161
of its bound (equation 1, table, quadrature n = 2) and 0.156 in the sweep (full history n = 1, MLP mode; 0.08 .. 0.15 elsewhere), 0.075 .. 0.126
at the roots near T and 0.11 .. 0.13 across the root counter wrap -- under half of it everywhere, as the u sweep's 0.14; check (a) at most 0.018
of its bound (full history n = 4, ACCUMULATE; 0.003 .. 0.005 near T).  Guard 1's smallest se / bound is 18.9, guard 2's best ratios per required
term 4.8 .. 3786.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_picard_stderr import _groups
from test_gpu_picard_sweep import D_SWEEP, FLAG_D, G_ENDS, IDLE, NEAR_T_D, SIGMA, _G, _ids, _near_t_points, _points, _ragged, _rpw
from test_gpu_stderr_sweep import (ACC, AMP, CASES, DEEP_QUAD, EPS, EPS_AMP, EPS_AMP_AT, MLP, NAN_BITS, TABLE_EQ_MODES, TABLE_MAX_SUMMANDS, _Case,
                                   _is_nan_case, _same, _scasml, _SeTree, _SweepSurrogate, _sweep_points, _sweep_tree, _table_par, bound_a, se_stats)

gpu = pytest.mark.gpu

K_TERMINAL, K_LEVEL = 6.0, 4.0            # B_Y's allowances in units of u |Y| (module docstring)


def _z_is_nan_case(variant, n, par):
    """Quadrature at n >= 4 meets q = 5: every z is non-finite in either mode (and u too in ACCUMULATE: _is_nan_case)."""
    return variant == "quad" and n >= 4


def test_the_z_stderr_sweep_reaches_every_width_level_and_mode():
    assert set(CASES[MLP]) == set(CASES[ACC]) == set(D_SWEEP)
    for g, (lo, hi) in G_ENDS.items():
        assert lo in D_SWEEP and hi in D_SWEEP
    for g, (lo, hi) in IDLE.items():
        assert any(lo <= d <= hi for d in D_SWEEP), g
    # the last lane of a root stores a partial float4 of standard errors at d mod 4 != 0: all four residues, d mod 4 = 1 at more than one G
    assert {d % 4 for d in D_SWEEP} == {0, 1, 2, 3}
    assert len({_G(d) for d in D_SWEEP if d % 4 == 1}) >= 3
    want = {("quad", 1, 3), ("quad", 2, 3), ("quad", 3, 3), ("quad", 4, 4), ("fh", 1, 3), ("fh", 2, 3), ("fh", 3, 2), ("fh", 4, 2), ("fh", 5, 2)}
    for mode in (MLP, ACC):
        assert {c for cases in CASES[mode].values() for c in cases} == want, mode
        for g in G_ENDS:
            ns = [n for d in D_SWEEP if _G(d) == g for _, n, _ in CASES[mode][d]]
            assert min(ns) <= 2 and max(ns) >= 3, (mode, g, ns)
        # every variant's every level with a finite z has a case with a live check (a) in each mode
        assert {(v, n) for v, n, par in want if not _z_is_nan_case(v, n, par)} == {("quad", 1), ("quad", 2), ("quad", 3)} | {("fh", n) for n in range(1, 6)}
    assert DEEP_QUAD[1] == ("quad", 5, 5) and DEEP_QUAD[0] in D_SWEEP
    assert sorted(_G(d) for d in FLAG_D) == [4, 8, 16, 32, 64] and set(NEAR_T_D) <= set(D_SWEEP)
    assert len({(v, n, eq, mode) for v in ("quad", "fh") for n in range(1, 6) for eq, mode in TABLE_EQ_MODES}) == 50
    # equation 1 in ACCUMULATE and every ACCUMULATE level below the read-back switch are in the table and the near-T test
    assert (1, ACC) in TABLE_EQ_MODES


# ------------------------------------------------------------------------------------------------------------- formulas (no GPU)
def se_stats_z(Ys):
    """Ys = [Y_g, Y_0, ...], float64 (N_j, B, 1 + d): se_stats component by component plus check (b)'s bound for the z columns (bound_z, b_var_z)."""
    st = se_stats(Ys)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        y2 = 0.0
        for j, Y in enumerate(Ys):
            N = Y.shape[0]
            y2 = y2 + (K_LEVEL if j else K_TERMINAL) ** 2 * N / (N - 1.0) * (Y * Y).sum(axis=0)
        var, se = st["var"], st["se"]
        b_var = st["b_var"] + 2 * EPS * st["terms"][0]
        up, down = np.sqrt(var + b_var) - se, se - np.sqrt(np.maximum(var - b_var, 0.0))
        st["b_var_z"], st["bound_z"] = b_var, np.maximum(up, down) + EPS * np.sqrt(y2)
    return st


def _finite(st):
    with np.errstate(invalid="ignore"):
        return np.isfinite(st["se"]) & np.isfinite(st["u"])


def drop_ratios_z(st, mode):
    """Guard 2: per term, the median over all z components of |se - se without term j| / bound (a)."""
    b, se, var = bound_a(st, mode)[:, 1:], st["se"][:, 1:], st["var"][:, 1:]
    return [float(np.median(np.abs(se - np.sqrt(np.maximum(var - v[:, 1:], 0.0))) / b)) for v in st["terms"]]


def emulate_float32_z(Ps, zs):
    """SeTerm4 of csrc/picard_tree.hpp in float32, component by component.  Ps = [P, Y_0, ...]: the terminal term's UNSCALED summands P_m = g nrm_m
    and the level terms' summands, (N_j, ...); zs: the terminal scale, float32, broadcastable.  add(): y0, s1 += dv, s2 = fma(dv, dv, s2);
    close_into(var, N, scale): var = fma(N / (N - 1) fma(-s1 / N, s1, s2), scale, var) with scale = fl(zs zs) for the terminal term and 1 for a
    level's.  (A product of two float32 is exact in float64; the one sum behind it is then rounded twice, which moves no bound here.)"""
    f32, f64 = np.float32, np.float64
    var = np.zeros(Ps[0].shape[1:], f32)
    for j, Y in enumerate(Ps):
        Y = Y.astype(f32)
        N = Y.shape[0]
        fn = f32(N)
        s1, s2 = np.zeros(Y.shape[1:], f32), np.zeros(Y.shape[1:], f32)
        for i in range(1, N):
            dv = (Y[i] - Y[0]).astype(f32)
            s1 = (s1 + dv).astype(f32)
            s2 = (dv.astype(f64) * dv.astype(f64) + s2.astype(f64)).astype(f32)
        m = (-s1 / fn).astype(f32)
        inner = (m.astype(f64) * s1.astype(f64) + s2.astype(f64)).astype(f32)
        closed = (f32(fn / (fn - f32(1))) * inner).astype(f32)
        scale = (np.asarray(zs, f32) * np.asarray(zs, f32)).astype(f32) if j == 0 else f32(1)
        var = (closed.astype(f64) * np.asarray(scale, f64) + var.astype(f64)).astype(f32)
    return var


# ------------------------------------------------------------------------------------------------------------- launches
class _UzCase(_Case):
    """_Case with the launch of scasml_picard_tree_stderr_uz and the sharded launches' whole rows."""

    def run_uz(self):
        """-> (out_uz, out_uhat or None, out_se_uz (B, 1 + d)), float32; asserts that the rows of out_se_uz past B were not written."""
        import torch
        from scasml_gp_amd import _lib
        lib, t, B = _lib.load(), self.t, self.B
        rows = max(self.stride, B) + 1
        out = torch.full((B, t.d + 1), -3.0, dtype=torch.float32, device="cuda")
        uh = torch.full((B,), -3.0, dtype=torch.float32, device="cuda") if t.mode == ACC else None
        s = torch.full((rows, t.d + 1), -3.0, dtype=torch.float32, device="cuda")
        mode = _lib.MODE_ACCUMULATE if t.mode == ACC else _lib.MODE_MLP
        _lib.check(lib.scasml_picard_tree_stderr_uz(C.byref(t.prob), C.byref(self.plan), mode, _lib.ptr(self.x), B, self.stride, self.rng(),
                                                    _lib.ptr(self.pts), _lib.ptr(self.vd), _lib.ptr(out), _lib.ptr(uh), _lib.ptr(s),
                                                    _lib.stream_ptr()), "picard_tree_stderr_uz")
        torch.cuda.synchronize()
        s = s.cpu().numpy()
        assert np.all(s[B:] == -3.0), ("out_se_uz was written past its B rows", self.t.d, B, self.stride)
        return out.cpu().numpy(), None if uh is None else uh.cpu().numpy(), s[:B]

    def summands_uz(self):
        """The device's own summands, all 1 + d columns: _Case.summands' launches.  -> [Y_g, Y_0, ...] float64 (N_j, B, 1 + d)."""
        import torch
        groups, units = _groups(self.t.variant, self.n, self.par)
        rows = [mine for _, summ in groups for mine in summ]
        own = np.ones((len(rows), units), dtype=np.uint8)
        for i, mine in enumerate(rows):
            own[i, mine] = 0
        owner = torch.from_numpy(own).cuda()
        out = torch.full((len(rows), self.B, self.t.d + 1), -3.0, dtype=torch.float32, device="cuda")
        for i in range(len(rows)):
            self._call(False, self.rng(owner=owner[i].data_ptr()), out[i], None, None)
        torch.cuda.synchronize()
        Y = out.cpu().numpy().astype(np.float64)
        Ys, at = [], 0
        for N, summ in groups:
            Ys.append(Y[at:at + N])
            at += N
        return Ys


# ------------------------------------------------------------------------------------------------------------- the checks
MEASURED = {}                  # "(variant) n=(n) (mode or edge)" -> a, b: largest dev / bound; s: smallest z se / bound (a); drops, guard2_best: guard 2
_ORACLE = {}                   # (mode, d, variant, n, par) -> se_stats_z of the oracle's summands at the largest batch; shared, never modified


def _record(key, **kw):
    m = MEASURED.setdefault("%s n=%d %s" % key, {})
    for k, v in kw.items():
        m[k] = min(m.get(k, float("inf")), float(v)) if k == "s" else max(m.get(k, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    """SCASML_STDERR_UZ_SWEEP_JSON=path: write what the checks measured (profiles/picard_stderr_uz_sweep.json is such a file)."""
    yield
    path = os.environ.get("SCASML_STDERR_UZ_SWEEP_JSON")
    if path and MEASURED:
        doc = dict(amp=AMP, eps_amp=EPS_AMP, eps_amp_at={str(k): v for k, v in EPS_AMP_AT.items()}, near_t_amp=0.3, k_terminal=K_TERMINAL,
                   k_level=K_LEVEL, checks={k: MEASURED[k] for k in sorted(MEASURED)})
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


def _freeze(st):
    for v in [st[k] for k in st if k != "terms"] + st["terms"]:
        v.setflags(write=False)
    return st


def _oracle_stats(mode, d, variant, n, par):
    key = (mode, d, variant, n, par)
    if key not in _ORACLE:
        assert not _z_is_nan_case(variant, n, par), "the oracle walks these trees in 10 s and more: check (e) consults it once"
        t = _sweep_tree(d, variant, mode)
        _ORACLE[key] = _freeze(se_stats_z(_summands_oracle(t, n, par, _sweep_points(d))))
    return _ORACLE[key]


def _summands_oracle(t, n, par, xt, root0=0):
    from oracle.mlp import PicardOracle
    return PicardOracle(t.oeq, t.variant, gp=t.sur, seed=t.seed, stream=t.stream).root_summands(n, par, xt, root0=root0, with_z=True)


def _rows(st, sel):
    return {k: (v[sel] if k != "terms" else [x[sel] for x in v]) for k, v in st.items()}


def check_a(se, st, mode, what, guard=True, key=None):
    """All 1 + d columns against se_stats_z of the oracle's summands for the same roots."""
    se = se.astype(np.float64)
    fin = _finite(st)
    assert not np.any(np.isfinite(se[~fin])), (what, "a finite se where the oracle's value or se is not finite")
    assert np.all(np.isfinite(se[fin])), (what, "se is not finite where the oracle's is")
    if not fin.any():
        return
    bound, dev, want = bound_a(st, mode)[fin], np.abs(se - st["se"])[fin], st["se"][fin]
    print("check (a) %s: se %.3e..%.3e, max |dev| %.3e, max dev/bound %.4f, min se/bound %.1f" % (what, want.min(), want.max(), dev.max(), (dev / bound).max(),
                                                                                                  (want / bound).min()))
    if key:
        _record(key, a=(dev / bound).max())
    if guard:                      # every z component; column 0, whose bits are the u-only entry's, under the u sweep's rule (the median root)
        zc = np.broadcast_to(np.arange(se.shape[1]) > 0, se.shape)[fin]
        if key:
            _record(key, s=(want / bound)[zc].min())
        assert np.all(want[zc] >= 10.0 * bound[zc]), (what, "guard 1", (want / bound)[zc].min())
        assert np.median(st["se"][:, 0]) >= 10.0 * bound[~zc].max(), (what, "guard 1, column 0")
    assert np.all(dev <= bound), (what, dev.max(), (dev / bound).max())


def check_b(se, dev_st, what, key=None):
    """The z columns against se_stats_z of the device's own summands."""
    se, se64, bound = se.astype(np.float64)[:, 1:], dev_st["se"][:, 1:], dev_st["bound_z"][:, 1:]
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(se64)
    assert np.array_equal(np.isfinite(se), fin), (what, "se_z is finite exactly where the device's own summands make it so")
    zero = fin & (se64 == 0)
    assert np.all(se[zero] == 0.0), (what, "se64 = 0 but the kernel's se_z is not")
    ok = fin & ~zero
    if not ok.any():
        return
    dev, bound, ref = np.abs(se - se64)[ok], bound[ok], se64[ok]
    print("check (b) %s: max |se_z - se64| %.3e, max / bound %.4f, bound / se %.2e..%.2e" % (what, dev.max(), (dev / bound).max(), (bound / ref).min(),
                                                                                           (bound / ref).max()))
    if key:
        _record(key, b=(dev / bound).max())
    assert np.all(dev <= bound), (what, dev.max(), (dev / bound).max(), int(np.argmax(dev / bound)))


def check_c(got, plain, u_only, what):
    assert _same(got[0], plain[0]), (what, "out_uz differs from the plain launch")
    if plain[1] is not None:
        assert _same(got[1], plain[1]) and _same(u_only[1], plain[1]), (what, "out_uhat differs from the plain launch")
    assert _same(got[2][:, 0], u_only[2]), (what, "column 0 of out_se_uz differs from the u-only entry's out_se")


def _three(c, what):
    """The z launch, checked (c) against the plain and the u-only launches of the same case.  -> (got, plain)."""
    got, plain = c.run_uz(), c.run(False)
    check_c(got, plain, c.run(True), what)
    return got, plain


def check_e(got, plain, mode, what):
    """Quadrature n >= 4 (module docstring (e))."""
    if mode == ACC:
        assert np.isnan(plain[0][:, 0]).all() and np.isnan(got[2][:, 0]).all(), (what, got[2][:, 0])
    assert not np.any(np.isfinite(plain[0][:, 1:])), (what, "a finite z behind a q = 5 rule")
    assert not np.any(np.isfinite(got[2][:, 1:])), (what, "a finite se_z where z is not finite")
    assert np.array_equal(np.isnan(got[2][:, 0]), np.isnan(plain[0][:, 0])), (what, "se_u is NaN exactly where u is")


@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_z_stderr_at_every_width_level_and_mode(d):
    """Checks (a) .. (e) of the module docstring at ragged batches; the roots of every batch are a prefix of the largest one."""
    Bs = _ragged(d)
    xt = _sweep_points(d)
    nan = np.frombuffer(np.uint32(NAN_BITS).tobytes(), dtype=np.float32)[0]
    for mode in (MLP, ACC):
        for variant, n, par in CASES[mode][d]:
            key, what = (variant, n, mode), (mode, variant, n, par, d)
            t = _sweep_tree(d, variant, mode)
            deep = _z_is_nan_case(variant, n, par)
            st = None if deep else _oracle_stats(mode, d, variant, n, par)
            assert deep or _finite(st).all()
            full = None
            for B in reversed(Bs):
                c = _UzCase(t, n, par, xt[:B])
                got, plain = _three(c, what + (B,))
                if deep:
                    check_e(got, plain, mode, what + (B,))
                else:
                    check_a(got[2], _rows(st, slice(0, B)), mode, what + (B,), guard=B == Bs[-1], key=key)
                if full is None:
                    full = got
                    check_b(got[2], se_stats_z(c.summands_uz()), what + (B,), key=key)
                    if mode == ACC:             # (d): a site stride past the batch, NaN in every padding row
                        S = (B + 31) // 32 * 32 + 32
                        padded = _UzCase(t, n, par, xt[:B], stride=S, pad=nan).run_uz()
                        assert all(_same(a, b) for a, b in zip(padded, got)), (what, "site_stride", S)
                else:
                    assert _same(got[2], full[2][:B]), (what, B, "se_uz of a root depends on the batch")          # (d)
            if not deep:
                MEASURED["%s n=%d %s" % key].setdefault("drops", {})["d=%d" % d] = drop_ratios_z(st, mode)


@gpu
def test_quadrature_level_four_has_a_finite_u_and_no_finite_z_in_the_oracle_too():
    """Check (e)'s expectation at one d and one root from the oracle: MLP mode (4, 4) at d = 13."""
    d, (variant, n, par) = 13, ("quad", 4, 4)
    assert (variant, n, par) in CASES[MLP][d]
    xt = _sweep_points(d)[:1]
    t = _sweep_tree(d, variant, MLP)
    st = se_stats_z(_summands_oracle(t, n, par, xt))
    fin = _finite(st)
    assert fin[:, 0].all() and not fin[:, 1:].any()
    c = _UzCase(t, n, par, xt)
    got, plain = _three(c, "quad (4, 4), one root")
    check_e(got, plain, MLP, "quad (4, 4), one root")
    check_a(got[2], st, MLP, "quad (4, 4), one root", guard=False)


@gpu
def test_quadrature_level_five_on_one_root():
    """Checks (c) and (e) on tests/golden/oracle_quad5_d13.npz's root; column 0's check (b) is the u sweep's, whose bits it carries."""
    from test_gpu_picard_sweep import _quad5
    d, (variant, n, par) = DEEP_QUAD
    c = _UzCase(_SeTree(0, d, variant, MLP), n, par, _quad5()["x_t"])
    got, plain = _three(c, "quad n=5")
    assert np.array_equal(np.isnan(plain[0]), np.isnan(_quad5()["uz"]))
    check_e(got, plain, MLP, "quad n=5")


def test_dropping_any_z_term_would_be_noticed():
    """Guard 2, from the oracle alone (no GPU), on the sweep's own cases (computed once per case and shared with the sweep)."""
    for mode in (MLP, ACC):
        for variant, n, par in sorted({c for cases in CASES[mode].values() for c in cases}):
            if _z_is_nan_case(variant, n, par):
                continue
            need = [j for j in range(n + 1) if not (mode == MLP and j == 1)]            # term 0 is the terminal one, term 1 + l the level l
            best = np.zeros(n + 1)
            for d in D_SWEEP:
                if (variant, n, par) not in CASES[mode][d]:
                    continue
                st = _oracle_stats(mode, d, variant, n, par)
                if mode == MLP:
                    assert np.all(st["terms"][1] == 0.0)            # the l = 0 term's variance is exactly 0 without a surrogate, for u and every z
                best = np.maximum(best, drop_ratios_z(st, mode))
                if all(best[j] >= 4.0 for j in need):
                    break
            print("guard 2 (z) %s %s n=%d: best drop ratios %s" % (mode, variant, n, np.round(best, 2).tolist()))
            MEASURED.setdefault("%s n=%d %s" % (variant, n, mode), {})["guard2_best"] = best.tolist()
            assert all(best[j] >= 4.0 for j in need), (mode, variant, n, best.tolist())


# ------------------------------------------------------------------------------------------------------------- the whole instantiation table
@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_every_z_instantiation_keeps_the_plain_and_the_u_only_bits(d):
    """Each of the 50 picard_se_uz_kernel instances (both variants, n = 1..5, equations 0 and 1 in MLP mode and ACCUMULATE, equation 2 in MLP
    mode) at one d per G, B = roots-per-wave + 1: check (c); se_z non-finite exactly where the plain launch's z is; check (b) on the equation 1
    and 2 entries of at most TABLE_MAX_SUMMANDS summands."""
    B = _rpw(d) + 1
    xt = _points(d, B, seed=1000 + d)
    for eq_id, mode in TABLE_EQ_MODES:
        for variant in ("quad", "fh"):
            t = _SeTree(eq_id, d, variant, mode)
            for n in range(1, 6):
                par = _table_par(variant, n)
                what = ("table", eq_id, mode, variant, n, par, d)
                # quadrature n = 5 walks 113 745 sites per root: two roots, and in ACCUMULATE (whose surrogate values come from the CPU) one
                rows = xt if not (variant == "quad" and n == 5) else xt[:1 if mode == ACC else 2]
                c = _UzCase(t, n, par, rows)
                got, plain = _three(c, what)
                assert np.array_equal(np.isfinite(got[2][:, 1:]), np.isfinite(plain[0][:, 1:])), what
                assert np.array_equal(np.isnan(got[2][:, 0]), np.isnan(plain[0][:, 0])), what
                assert _z_is_nan_case(variant, n, par) != bool(np.isfinite(got[2][:, 1:]).all()), what
                groups, _ = _groups(variant, n, par)
                if eq_id != 0 and sum(N for N, _ in groups) <= TABLE_MAX_SUMMANDS:
                    check_b(got[2], se_stats_z(c.summands_uz()), what, key=(variant, n, "%s equation %d, table" % (mode, eq_id)))


# ------------------------------------------------------------------------------------------------------------- edges
@gpu
@pytest.mark.parametrize("d", NEAR_T_D, ids=_ids(NEAR_T_D))
def test_z_stderr_on_both_sides_of_the_read_back_switch(d):
    """Roots at T - t = 0, one ulp, 1e-5, 1e-4, just below and above (kReadbackMinVol / sigma)^2 and 1e-2, ACCUMULATE, amp = 0.3: checks (a)
    (no guard 1: se_u goes to 0 with T - t) and (b) on both sides of the switch.  Quadrature at t = T: se_u is exactly 0 and every se_z finite
    and positive (the terminal scale is 1 / (mg 1e-6)).  Full history at t = T: the scale is 1 / 0 and every se_z of that root non-finite, and
    no other root of its wave changes a bit against the launch without that row."""
    xt = _near_t_points(d, seed=500 + d)
    taus = np.float64(0.5) - xt[:, d].astype(np.float64)
    assert taus[0] == 0 and np.all(SIGMA * np.sqrt(taus[:5]) < 1e-2) and np.all(SIGMA * np.sqrt(taus[5:]) > 1e-2)
    for variant, n, par in (("quad", 2, 3), ("quad", 3, 3), ("fh", 2, 3), ("fh", 3, 2)):
        what = (variant, n, "near T", d)
        t = _SeTree(0, d, variant, ACC, amp=0.3)
        c = _UzCase(t, n, par, xt)
        got, plain = _three(c, what)
        se = got[2]
        if variant == "quad":
            assert se[0, 0] == 0.0 and np.all(np.isfinite(se)) and np.all(se[0, 1:] > 0) and np.all(se[2:] > 0)
        else:
            assert not np.any(np.isfinite(se[0, 1:])) and np.all(np.isfinite(se[1:])) and np.all(se[2:] > 0)
            rest = _UzCase(t, n, par, xt[1:], root0=1)             # the same roots 1 .. B - 1 without the row at t = T
            got1, _ = _three(rest, what + ("without t = T",))
            assert all(_same(a[1:], b) for a, b in zip(got, got1)), (what, "a root at t = T moved a neighbour's bits")
        check_a(se, se_stats_z(_summands_oracle(t, n, par, xt)), ACC, what, guard=False, key=(variant, n, "acc near T"))
        check_b(se, se_stats_z(c.summands_uz()), what, key=(variant, n, "acc near T"))


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_z_stderr_root_counter_wraps(d):
    """root0 = 2^32 - 3, B = 8: checks (b) and (c) across the wrap; local root i >= 3 is root i - 3 of a launch that starts at 0."""
    root0, B = (1 << 32) - 3, 8
    xt = _points(d, B, seed=800 + d)
    for mode in (MLP, ACC):
        for variant, n, par in (("quad", 2, 3), ("fh", 3, 2)):
            t = _SeTree(0, d, variant, mode)
            c = _UzCase(t, n, par, xt, root0=root0)
            got, _ = _three(c, (mode, variant, "wrap"))
            check_b(got[2], se_stats_z(c.summands_uz()), (mode, variant, "wrap"), key=(variant, n, mode + " root counter wrap"))
            low = _UzCase(t, n, par, xt[3:]).run_uz()
            assert _same(got[2][3:], low[2]) and _same(got[0][3:], low[0]), (mode, variant, "wrapped roots")
            assert np.all(got[2] > 0)


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_a_nan_coordinate_makes_its_whole_row_nan_and_disturbs_no_other_root(d):
    """MLP mode, one coordinate of one row in the middle of a wave is NaN: that root's whole row of se_uz is NaN; every other root keeps the
    bits of the launch without it."""
    B = 4 * _rpw(d) + 1
    xt = _points(d, B, seed=1100 + d)
    bad = xt.copy()
    r = _rpw(d) // 2 if _rpw(d) > 1 else 1            # G = 64: one root per wave, the second wave's
    bad[r, d // 2] = np.nan
    others = np.arange(B) != r
    for variant, n, par in (("quad", 3, 3), ("fh", 4, 2)):
        t = _SeTree(0, d, variant, MLP)
        clean = _UzCase(t, n, par, xt).run_uz()
        got, _ = _three(_UzCase(t, n, par, bad), (variant, "NaN row"))
        assert np.isnan(got[2][r]).all() and np.isnan(got[0][r]).all(), (variant, got[2][r])
        assert _same(got[2][others], clean[2][others]) and _same(got[0][others], clean[0][others])
        assert np.all(np.isfinite(got[2][others])) and np.all(got[2][others] > 0)


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_the_residual_addend_of_z_divides_by_its_own_step(d):
    """ACCUMULATE at l = 0 emits the residual addend alone, and its z summand divides by the node's own step (dminus, ScaSML.py:274-280).  The
    term's other table, dplus, belongs to the "+" addend that is not emitted there, and ScaSML's plans set it equal to the first (tables.py), so
    a walker that read it for the residual addend's zm would pass every other test of this file.  With dplus of the root's l = 0 term doubled
    in a copy of the plan no bit of any output may change, and check (b) holds on the copy."""
    B = _rpw(d) + 1
    xt = _points(d, B, seed=1300 + d)
    for n, par in ((2, 3), (3, 3)):
        t = _SeTree(0, d, "quad", ACC)
        c = _UzCase(t, n, par, xt)
        got = c.run_uz()
        plan = type(c.plan).from_buffer_copy(c.plan)
        tm = plan.term[n][0]
        assert tm.q >= 1 and all(tm.dplus[k] == tm.cfrac[k] for k in range(tm.q))
        for k in range(tm.q):
            tm.dplus[k] = 2.0 * tm.dplus[k]
        c.plan = plan
        moved = c.run_uz()
        assert all(_same(a, b) for a, b in zip(moved, got)), (d, n, "the l = 0 term's dplus reached an ACCUMULATE output")
        check_b(moved[2], se_stats_z(c.summands_uz()), ("residual addend", n, d))


# ------------------------------------------------------------------------------------------------------------- through the solver classes
@gpu
@pytest.mark.parametrize("d", [43, 100])
def test_scasml_class_with_z_stderr_keeps_the_plain_bits_one_shot_and_chunked(d, monkeypatch):
    """G = 16 with idle lanes (d = 43) and G = 32 (d = 100): (u, z) of return_stderr="uz" is the plain call's, column 0 is return_stderr=True's,
    and a solve cut into chunks of 7 roots returns the se_uz bits of the one-shot solve."""
    import scasml_gp_amd.solvers._picard as P
    from oracle.equation import sample_points
    hip = _scasml(d)
    xt = np.concatenate(sample_points(np.random.default_rng(33), d, 38, 12))
    hip._engine.calls = 0
    plain = hip.uz_solve(2, 3, xt)
    hip._engine.calls = 0
    _, se_u = hip.uz_solve(2, 3, xt, return_stderr=True)
    hip._engine.calls = 0
    uz, se = hip.uz_solve(2, 3, xt, return_stderr="uz")
    assert se.shape == (50, d + 1) and se.dtype == np.float32 and np.all(np.isfinite(se)) and np.all(se > 0)
    assert _same(plain, uz) and _same(se[:, 0:1], se_u)
    ppr = int(P._lib.load().scasml_points_per_root(C.byref(hip._engine.plan(2, 3))))
    kp = int(P._lib.load().scasml_point_stride(d))
    monkeypatch.setattr(P, "POINT_BUFFER_BYTES", ppr * kp * 4 * 7)             # 7 roots per chunk
    hip._engine.calls = 0
    uz7, se7 = hip.uz_solve(2, 3, xt, return_stderr="uz")
    assert _same(se7, se) and _same(uz7, uz)
