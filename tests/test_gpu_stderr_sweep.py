"""The standard-error kernels (scasml_picard_tree_stderr, picard_tree_kernel<..., SE = true>) at every lane-group width, level and mode, called
through ctypes with the structs, batches and points of tests/test_gpu_picard_sweep.py.

Every (case, B) runs four checks:

(a) se against the float64 oracle's own summands (PicardOracle.root_summands, one walk) by the header's formula, within the project's bound
    2 (ATOL + RTOL max(|u_unclipped|, se)) -- 2e-5 / 1e-4 in MLP mode, 5e-5 / 2e-4 where points are read back.  Guard 1: the median oracle se is at
    least 10 x the bound.  Guard 2 (test_dropping_any_term_would_be_noticed, from the oracle alone): for every term j of every (variant, n, mode)
    some case moves the median root's oracle se by >= 4 x the bound when term j's variance is dropped.  The l = 0 term is exempt in MLP mode
    (f(0, 0) = 0 for the registered equations: its variance is exactly 0) and required in ACCUMULATE.
(b) se against the DEVICE's own summands: the plain kernel with world = 2 and an owner table that marks one summand's units returns that
    summand's unclipped float32 Y.  With Var and se64 formed from them in float64, per term on the deviations from its first summand
    (S2_j = sum dv^2), |se - se64| <= B_var / (2 se64) + B_Y,
        B_var = sum_j N_j / (N_j - 1) (3 N_j + 8) 2^-24 S2_j + 4 * 2^-24 Var,     B_Y = 4 * 2^-24 sqrt(sum_j N_j / (N_j - 1) sum_i Y_ji^2).
    B_var: the N - 1 float32 additions into S1 and S2, the rounding of each deviation, the closing fma and the square root (|S1| sum |dv| / N <= S2).
    B_Y: the one or two ulps by which a summand inside the kernel may differ from the sharded launch's (a contracted product; g * rcp(mg) rounded
    before, not after, the sum); centring is a projection, so a perturbation e of a term's summands moves its se by at most sqrt(N / (N - 1)) |e|_2.
    Derived, not fitted; tests/test_picard_stderr_host.py shows on the CPU that a float32 emulation of the accumulation stays inside B_var.
    Where se64 = 0 (t = T) the kernel's se is exactly 0; where it is NaN the kernel's is NaN.
(c) out_uz and, in ACCUMULATE, out_uhat equal the plain launch's bit for bit, NaNs included -- also over the whole table of 50 instantiations.
(d) a root's se bits do not depend on the batch (prefixes of one batch), on site_stride, or on what other rows or padding rows hold.

Surrogate of the ACCUMULATE cases: _Surrogate with amp = 0.05 and the residual eps_PDE scaled to 0.2 cos(.) (_SweepSurrogate).  The l = 0 term of
ACCUMULATE is the residual addend alone (f(u_hat, .) - f(u_hat, .) = 0 under a zero child), so `amp` does not reach it: at the 1e-3 residual of
_Surrogate dropping it moves se by 0.0 x the bound at every case, at 0.2 by up to 64 x (guard 2).  At d = 29 and d = 70 the residual is 0.1 and
0.05 (EPS_AMP_AT): at 0.2 it swamps the l = 1 term of full history (3, 2) and (2, 3) on the median root.  At amp = 1e-3 guard 1 fails too (se of
order 1e-4).  Quadrature (4, 4) in ACCUMULATE and quadrature (5, 5) in MLP mode are NaN at every root (a q = 5 rule, whose tabulated nodes are not
increasing, above a non-zero child): se must be NaN there, and they have no guards.

Measured on an MI355X (profiles/picard_stderr_sweep.json, written when SCASML_STDERR_SWEEP_JSON names a file): check (b) reaches at most 0.14 of its
bound (equation 1, table) and 0.11 in the sweep (quadrature n = 1, MLP mode; 0.05 .. 0.10 elsewhere), with the bound at 1e-6 .. 3e-4 of se (up to
5e-3 within 1e-4 of T); check (a) at most 0.0021 of its bound (full history n = 4, MLP mode).  Guard 2's ratios are 5.3 .. 556.
Before the final store let a NaN through (sqrtf(fmaxf(Var, 0)): fmaxf(NaN, 0) = 0) the NaN cases below reported se = 0.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_picard_stderr import _groups
from test_gpu_picard_sweep import (ATOL, ATOL_RB, D_SWEEP, FLAG_D, G_ENDS, IDLE, NEAR_T, NEAR_T_D, RTOL, RTOL_RB, SIGMA, _G, _ids, _near_t_points,
                                   _points, _ragged, _rpw, _Surrogate, _Tree)

gpu = pytest.mark.gpu

EPS = 2.0 ** -24
AMP, EPS_AMP = 0.05, 0.2                  # the surrogate of the ACCUMULATE cases (module docstring)
EPS_AMP_AT = {29: 0.1, 70: 0.05}          # full history (3, 2) and (2, 3): at 0.2 the residual term swamps their l = 1 term on the median root
MLP, ACC = "mlp", "acc"
TOL = {MLP: (ATOL, RTOL), ACC: (ATOL_RB, RTOL_RB)}
# plans with an estimable variance: quadrature rho >= 3, full history M >= 2
_Q = [(1, 3), (2, 3), (3, 3), (4, 4)]
_F = [(1, 3), (2, 3), (3, 2), (4, 2), (5, 2)]
CASES = {MLP: {d: [("quad",) + _Q[i % 4], ("fh",) + _F[i % 5]] for i, d in enumerate(D_SWEEP)},
         ACC: {d: [("quad",) + _Q[(i + 2) % 4], ("fh",) + _F[(i + 2) % 5]] for i, d in enumerate(D_SWEEP)}}
DEEP_QUAD = (13, ("quad", 5, 5))          # one root, MLP mode, checks (b) and (c): the oracle walks this tree in a minute or more
NAN_BITS = 0x7FC0BEEF
# the whole instantiation table: (eq, mode) x variant x n
TABLE_EQ_MODES = [(0, MLP), (0, ACC), (1, MLP), (1, ACC), (2, MLP)]
TABLE_MAX_SUMMANDS = 300                  # check (b) on the equation 1 and 2 entries, one launch per summand (quadrature n = 5 has 3224: DEEP_QUAD)


def _table_par(variant, n):
    return (max(n, 3) if variant == "quad" else (3 if n <= 2 else 2))


def _is_nan_case(variant, n, par, mode):
    return mode == ACC and variant == "quad" and n >= 4


def test_the_stderr_sweep_reaches_every_width_level_and_mode():
    assert set(CASES[MLP]) == set(CASES[ACC]) == set(D_SWEEP)
    for g, (lo, hi) in G_ENDS.items():
        assert lo in D_SWEEP and hi in D_SWEEP
    for g, (lo, hi) in IDLE.items():
        assert any(lo <= d <= hi for d in D_SWEEP), g
    assert {d % 4 for d in D_SWEEP} == {0, 1, 2, 3}
    want = {("quad",) + c for c in _Q} | {("fh",) + c for c in _F}
    for mode in (MLP, ACC):
        assert {c for cases in CASES[mode].values() for c in cases} == want, mode
    assert DEEP_QUAD[1] == ("quad", 5, 5) and DEEP_QUAD[0] in D_SWEEP
    # an estimable variance: rho >= 3, M >= 2, and rho >= n
    assert all((par >= 3 and par >= n) if v == "quad" else par >= 2 for v, n, par in want)
    # every G meets a shallow (n <= 2) and a deep (n >= 3) case in each mode
    for mode in (MLP, ACC):
        for g in G_ENDS:
            ns = [n for d in D_SWEEP if _G(d) == g for _, n, _ in CASES[mode][d]]
            assert min(ns) <= 2 and max(ns) >= 3, (mode, g, ns)
    assert sorted(_G(d) for d in FLAG_D) == [4, 8, 16, 32, 64] and set(NEAR_T_D) <= set(D_SWEEP)
    # the table: 2 variants x 5 levels x 5 (equation, mode) pairs = the 50 instantiations of the two translation units
    assert len({(v, n, eq, mode) for v in ("quad", "fh") for n in range(1, 6) for eq, mode in TABLE_EQ_MODES}) == 50
    for v in ("quad", "fh"):
        for n in range(1, 6):
            groups, _ = _groups(v, n, _table_par(v, n))
            assert all(N >= 2 for N, _ in groups)


# ------------------------------------------------------------------------------------------------------------- formulas (no GPU)
def se_stats(Ys):
    """Ys = [Y_g, Y_0, ...], float64 (N_j, B): the header's formula on the deviations from each term's first summand, and the bounds of check (b).
    -> dict(se, u, var, terms (per-term variances), bound_b, b_var)."""
    var = b_var = y2 = u = 0.0
    terms = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for Y in Ys:
            N = Y.shape[0]
            f = N / (N - 1.0)
            dv = Y - Y[0]
            S1, S2 = dv.sum(axis=0), (dv * dv).sum(axis=0)
            v = f * (S2 - S1 * S1 / N)
            terms.append(v)
            var = var + v
            b_var = b_var + f * (3 * N + 8) * EPS * S2
            y2 = y2 + f * (Y * Y).sum(axis=0)
            u = u + Y.sum(axis=0)
        b_var = b_var + 4 * EPS * var
        se = np.sqrt(np.maximum(var, 0.0))
        se = np.where(np.isnan(var), np.nan, se)
        bound_b = np.where(se > 0, b_var / (2 * np.where(se > 0, se, 1.0)), 0.0) + 4 * EPS * np.sqrt(y2)
    return dict(se=se, u=u, var=var, terms=terms, bound_b=bound_b, b_var=b_var)


def bound_a(st, mode):
    atol, rtol = TOL[mode]
    return 2.0 * (atol + rtol * np.maximum(np.abs(st["u"]), st["se"]))


def drop_ratios(st, mode):
    """Guard 2 on the median root: |se - se without term j| / bound (a), per term."""
    order = np.argsort(st["se"])
    r = order[len(order) // 2]
    b = bound_a(st, mode)[r]
    return [float(abs(st["se"][r] - np.sqrt(max(st["var"][r] - v[r], 0.0))) / b) for v in st["terms"]]


def emulate_float32(Ys):
    """SeTerm of csrc/picard_tree.hpp in float32 on float32(Y): y0, s1 += dv, s2 = fma(dv, dv, s2), N / (N - 1) fma(-s1 / N, s1, s2)."""
    f32 = np.float32
    var = f32(0) * Ys[0][0].astype(f32)
    for Y in Ys:
        Y = Y.astype(f32)
        N = Y.shape[0]
        fn = f32(N)
        s1 = np.zeros(Y.shape[1], f32)
        s2 = np.zeros(Y.shape[1], f32)
        for i in range(1, N):
            dv = (Y[i] - Y[0]).astype(f32)
            s1 = (s1 + dv).astype(f32)
            s2 = (dv.astype(np.float64) * dv.astype(np.float64) + s2.astype(np.float64)).astype(f32)       # dv * dv is exact in float64
        m = (-s1 / fn).astype(f32)
        close = (m.astype(np.float64) * s1.astype(np.float64) + s2.astype(np.float64)).astype(f32)
        var = (var + (f32(fn / (fn - f32(1))) * close).astype(f32)).astype(f32)
    return var


class _SweepSurrogate(_Surrogate):
    """_Surrogate with its residual scaled up: eps = eps_amp cos(c.x + e t) (module docstring)."""

    def __init__(self, d, amp=AMP, eps_amp=EPS_AMP):
        super().__init__(d, amp)
        self.eps_amp = eps_amp

    def compute_PDE_loss(self, P):
        x, t = self._split(P)
        return self.eps_amp * np.cos(x @ self.c + self.e * t)[:, None]


# ------------------------------------------------------------------------------------------------------------- launches
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class _SeTree(_Tree):
    def __init__(self, eq_id, d, variant, mode, amp=AMP, eps_amp=EPS_AMP):
        super().__init__(eq_id, d, variant, surrogate=mode == ACC, amp=amp)
        self.mode = mode
        if mode == ACC:
            self.sur = _SweepSurrogate(d, amp, eps_amp)          # the engine keeps the first one as a "there is a surrogate" marker only

    def summands_oracle(self, n, par, xt, root0=0):
        from oracle.mlp import PicardOracle
        return PicardOracle(self.oeq, self.variant, gp=self.sur, seed=self.seed, stream=self.stream).root_summands(n, par, xt, root0=root0)


class _Case:
    """One (tree, plan, batch): x_t on the device and, in ACCUMULATE, the points GENERATE emitted and the surrogate's values at them."""

    def __init__(self, t, n, par, xt, root0=0, stride=0, pad=0.0):
        import torch
        from scasml_gp_amd import _lib
        self.t, self.n, self.par, self.root0, self.stride = t, n, par, root0, stride
        self.plan = t.plan(n, par)
        self.B = xt.shape[0]
        self.x = torch.from_numpy(np.ascontiguousarray(xt, dtype=np.float32)).cuda()
        self.pts = self.vd = None
        if t.mode == ACC:
            lib = _lib.load()
            B, d, S = self.B, t.d, stride or self.B
            ppr = int(lib.scasml_points_per_root(C.byref(self.plan)))
            self.pts = torch.from_numpy(np.full((ppr * S, t.kp), pad, dtype=np.float32)).cuda()
            _lib.check(t.launch(_lib.MODE_GENERATE, self.plan, self.x, B, stride, self.rng(), pts=self.pts), "picard_tree(generate)")
            P = self.pts.cpu().numpy().reshape(ppr, S, t.kp)
            vals = np.full((ppr, S, 4), pad, dtype=np.float32)
            with np.errstate(all="ignore"):
                vals[:, :B] = t.sur.values(P[:, :B, :d + 1].reshape(-1, d + 1)).reshape(ppr, B, 4)
            self.vd = torch.from_numpy(vals.reshape(-1, 4)).cuda()

    def rng(self, owner=None):
        return self.t.rng(root0=self.root0, rank=0, world=2 if owner is not None else 1, owner=owner)

    def _call(self, se, rng, out, uh, s):
        from scasml_gp_amd import _lib
        lib, t = _lib.load(), self.t
        mode = _lib.MODE_ACCUMULATE if t.mode == ACC else _lib.MODE_MLP
        args = (C.byref(t.prob), C.byref(self.plan), mode, _lib.ptr(self.x), self.B, self.stride, rng, _lib.ptr(self.pts), _lib.ptr(self.vd),
                _lib.ptr(out), _lib.ptr(uh))
        if se:
            _lib.check(lib.scasml_picard_tree_stderr(*args, _lib.ptr(s), _lib.stream_ptr()), "picard_tree_stderr")
        else:
            _lib.check(lib.scasml_picard_tree(*args, _lib.stream_ptr()), "picard_tree")

    def run(self, se):
        """-> (out_uz, out_uhat or None, out_se or None), float32."""
        import torch
        out = torch.full((self.B, self.t.d + 1), -3.0, dtype=torch.float32, device="cuda")
        uh = torch.full((self.B,), -3.0, dtype=torch.float32, device="cuda") if self.t.mode == ACC else None
        s = torch.full((self.B,), -3.0, dtype=torch.float32, device="cuda") if se else None
        self._call(se, self.rng(), out, uh, s)
        torch.cuda.synchronize()
        return out.cpu().numpy(), None if uh is None else uh.cpu().numpy(), None if s is None else s.cpu().numpy()

    def summands(self):
        """The device's own summands: one sharded plain launch each (rank 0 of world 2 owns that summand's units and nothing else).
        -> [Y_g, Y_0, ...] float64 (N_j, B)."""
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
        Y = out[:, :, 0].cpu().numpy().astype(np.float64)
        Ys, at = [], 0
        for N, summ in groups:
            assert len(summ) == N
            Ys.append(Y[at:at + N])
            at += N
        return Ys


# ------------------------------------------------------------------------------------------------------------- the checks
MEASURED = {}                  # (variant, n, mode) -> dict(a=max |dev| / bound (a), b=max |se - se64| / bound (b), drops=[...]); dumped at the end
_ORACLE = {}                   # (mode, d, variant, n, par) -> se_stats of the oracle's summands at the largest batch; shared, never modified


def _record(key, **kw):
    m = MEASURED.setdefault("%s n=%d %s" % key, dict(a=0.0, b=0.0))
    for k, v in kw.items():
        m[k] = max(m[k], float(v))


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    """SCASML_STDERR_SWEEP_JSON=path: write what the checks measured (profiles/picard_stderr_sweep.json is such a file)."""
    yield
    path = os.environ.get("SCASML_STDERR_SWEEP_JSON")
    if path and MEASURED:
        doc = dict(amp=AMP, eps_amp=EPS_AMP, eps_amp_at={str(k): v for k, v in EPS_AMP_AT.items()}, near_t_amp=0.3, checks={k: MEASURED[k] for k in sorted(MEASURED)})
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


def _sweep_tree(d, variant, mode):
    return _SeTree(0, d, variant, mode, eps_amp=EPS_AMP_AT.get(d, EPS_AMP))


def _sweep_points(d):
    return _points(d, _ragged(d)[-1], seed=900 + d)


def _oracle_stats(mode, d, variant, n, par):
    key = (mode, d, variant, n, par)
    if key not in _ORACLE:
        t = _sweep_tree(d, variant, mode)
        st = se_stats(t.summands_oracle(n, par, _sweep_points(d)))
        for v in [st[k] for k in ("se", "u", "var", "bound_b", "b_var")] + st["terms"]:
            v.setflags(write=False)
        _ORACLE[key] = st
    return _ORACLE[key]


def check_a(se, st, mode, what, guard=True, key=None):
    """st: se_stats of the oracle's summands for the same roots."""
    se = se.astype(np.float64)
    nan = np.isnan(st["u"])
    assert np.array_equal(np.isnan(se), nan), (what, "se is NaN exactly where the oracle's unclipped u is")
    if nan.all():
        return
    ok = ~nan
    bound, dev = bound_a(st, mode)[ok], np.abs(se - st["se"])[ok]
    print("check (a) %s: se %.3e..%.3e, max |dev| %.3e, max dev/bound %.4f" % (what, st["se"][ok].min(), st["se"][ok].max(), dev.max(), (dev / bound).max()))
    if key:
        _record(key, a=(dev / bound).max())
    if guard:
        assert np.median(st["se"][ok]) >= 10.0 * bound.max(), (what, np.median(st["se"][ok]), bound.max())
    assert np.all(dev <= bound), (what, dev.max(), (dev / bound).max())


def check_b(se, dev_st, what, key=None):
    """dev_st: se_stats of the device's own summands."""
    se = se.astype(np.float64)
    se64 = dev_st["se"]
    nan = np.isnan(se64)
    assert np.array_equal(np.isnan(se), nan), (what, "se is NaN exactly where the device's own summands make it so")
    zero = (se64 == 0) & ~nan
    assert np.all(se[zero] == 0.0), (what, "se64 = 0 but the kernel's se is not")
    ok = ~nan & ~zero
    if not ok.any():
        return
    dev, bound = np.abs(se - se64)[ok], dev_st["bound_b"][ok]
    print("check (b) %s: max |se - se64| %.3e, max / bound %.4f, bound / se %.2e..%.2e" % (what, dev.max(), (dev / bound).max(), (bound / se64[ok]).min(),
                                                                                         (bound / se64[ok]).max()))
    if key:
        _record(key, b=(dev / bound).max())
    assert np.all(dev <= bound), (what, dev.max(), (dev / bound).max(), int(np.argmax(dev / bound)))


def check_c(with_se, plain, what):
    assert _same(with_se[0], plain[0]), (what, "out_uz differs from the plain launch")
    if plain[1] is not None:
        assert _same(with_se[1], plain[1]), (what, "out_uhat differs from the plain launch")


@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_stderr_at_every_width_level_and_mode(d):
    """Checks (a) .. (d) of the module docstring at ragged batches; the roots of every batch are a prefix of the largest one."""
    Bs = _ragged(d)
    xt = _sweep_points(d)
    nan = np.frombuffer(np.uint32(NAN_BITS).tobytes(), dtype=np.float32)[0]
    for mode in (MLP, ACC):
        for variant, n, par in CASES[mode][d]:
            key, what = (variant, n, mode), (mode, variant, n, par, d)
            t = _sweep_tree(d, variant, mode)
            st = _oracle_stats(mode, d, variant, n, par)
            assert np.isnan(st["u"]).all() == _is_nan_case(variant, n, par, mode) and (np.isnan(st["u"]).all() or np.isfinite(st["u"]).all())
            full = None
            for B in reversed(Bs):
                c = _Case(t, n, par, xt[:B])
                got, plain = c.run(True), c.run(False)
                check_c(got, plain, what + (B,))
                sub = {k: (v[:B] if k != "terms" else [x[:B] for x in v]) for k, v in st.items()}
                check_a(got[2], sub, mode, what + (B,), guard=B == Bs[-1], key=key)
                if full is None:
                    full = got
                    check_b(got[2], se_stats(c.summands()), what + (B,), key=key)
                    if mode == ACC:             # (d) and the padding edge: a site stride past the batch, NaN in every padding row
                        S = (B + 31) // 32 * 32 + 32
                        padded = _Case(t, n, par, xt[:B], stride=S, pad=nan).run(True)
                        assert all(_same(a, b) for a, b in zip(padded, got)), (what, "site_stride", S)
                else:
                    assert _same(got[2], full[2][:B]), (what, B, "se of a root depends on the batch")          # (d)
            if not _is_nan_case(variant, n, par, mode):
                MEASURED["%s n=%d %s" % key].setdefault("drops", {})["d=%d" % d] = drop_ratios(st, mode)


@gpu
def test_quadrature_level_five_on_one_root():
    """Checks (b) and (c) on tests/golden/oracle_quad5_d13.npz's root: 3224 summands, one launch each."""
    from test_gpu_picard_sweep import _quad5
    d, (variant, n, par) = DEEP_QUAD
    t = _SeTree(0, d, variant, MLP)
    c = _Case(t, n, par, _quad5()["x_t"])
    got = c.run(True)
    check_c(got, c.run(False), "quad n=5")
    # the root's u is NaN in the fixture (its l = 1 rule has q = 5, whose nodes are not increasing): se is NaN exactly where u is
    assert np.array_equal(np.isnan(got[2]), np.isnan(_quad5()["uz"][:, 0])) and np.array_equal(np.isnan(got[2]), np.isnan(got[0][:, 0]))
    check_b(got[2], se_stats(c.summands()), "quad n=5", key=(variant, n, MLP))


def test_dropping_any_term_would_be_noticed():
    """Guard 2, from the oracle alone (no GPU): the oracle's summands of the sweep's own cases, computed once per case and shared with the sweep."""
    for mode in (MLP, ACC):
        keys = sorted({c for cases in CASES[mode].values() for c in cases})
        for variant, n, par in keys:
            if _is_nan_case(variant, n, par, mode):
                continue
            need = [j for j in range(n + 1) if not (mode == MLP and j == 1)]            # term 0 is the terminal one, term 1 + l the level l
            best = np.zeros(n + 1)
            for d in D_SWEEP:
                if (variant, n, par) not in CASES[mode][d]:
                    continue
                best = np.maximum(best, drop_ratios(_oracle_stats(mode, d, variant, n, par), mode))
                if all(best[j] >= 4.0 for j in need):
                    break
            print("guard 2 %s %s n=%d: best drop ratios %s" % (mode, variant, n, np.round(best, 2).tolist()))
            assert all(best[j] >= 4.0 for j in need), (mode, variant, n, best.tolist())
            if mode == MLP:
                assert best[1] == 0.0            # the l = 0 term's variance is identically 0 without a surrogate


# ------------------------------------------------------------------------------------------------------------- the whole instantiation table
@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_every_instantiation_keeps_the_plain_bits(d):
    """Check (c) on each of the 50 kernels (both variants, n = 1..5, equations 0 and 1 in MLP mode and ACCUMULATE, equation 2 in MLP mode) at one d
    per G, B = roots-per-wave + 1; check (b) on the equation 1 and 2 entries (quadrature n = 5 apart: test_quadrature_level_five_on_one_root)."""
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
                c = _Case(t, n, par, rows)
                got = c.run(True)
                check_c(got, c.run(False), what)
                assert np.array_equal(np.isnan(got[2]), np.isnan(got[0][:, 0])), what        # se is NaN exactly where u is
                groups, _ = _groups(variant, n, par)
                if eq_id != 0 and sum(N for N, _ in groups) <= TABLE_MAX_SUMMANDS:
                    check_b(got[2], se_stats(c.summands()), what)


# ------------------------------------------------------------------------------------------------------------- edges
@gpu
@pytest.mark.parametrize("d", NEAR_T_D, ids=_ids(NEAR_T_D))
def test_stderr_on_both_sides_of_the_read_back_switch(d):
    """Roots at T - t = 0, one ulp, 1e-5, 1e-4, just below and above (kReadbackMinVol / sigma)^2 and 1e-2, ACCUMULATE, amp = 0.3: se finite
    everywhere and exactly 0 at t = T (quadrature; full history divides by T - t and skips that root, as the plain sweep does); checks (a) and (b)
    on both sides of the switch (no guard 1: se goes to 0 with T - t)."""
    xt = _near_t_points(d, seed=500 + d)
    taus = np.float64(0.5) - xt[:, d].astype(np.float64)
    assert taus[0] == 0 and np.all(SIGMA * np.sqrt(taus[:5]) < 1e-2) and np.all(SIGMA * np.sqrt(taus[5:]) > 1e-2)
    for variant, n, par in (("quad", 2, 3), ("quad", 3, 3), ("fh", 2, 3), ("fh", 3, 2)):
        rows = xt if variant == "quad" else xt[1:]
        t = _SeTree(0, d, variant, ACC, amp=0.3)
        c = _Case(t, n, par, rows)
        got = c.run(True)
        check_c(got, c.run(False), (variant, n, "near T"))
        se = got[2]
        assert np.all(np.isfinite(se)) and np.all(se >= 0)
        if variant == "quad":
            assert se[0] == 0.0 and np.all(se[2:] > 0)
        check_a(se, se_stats(t.summands_oracle(n, par, rows)), ACC, (variant, n, "near T"), guard=False)
        check_b(se, se_stats(c.summands()), (variant, n, "near T"))


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_stderr_root_counter_wraps(d):
    """root0 = 2^32 - 3, B = 8: check (b) across the wrap; local root i >= 3 is root i - 3 of a launch that starts at 0."""
    root0, B = (1 << 32) - 3, 8
    xt = _points(d, B, seed=800 + d)
    for mode in (MLP, ACC):
        for variant, n, par in (("quad", 2, 3), ("fh", 3, 2)):
            t = _SeTree(0, d, variant, mode)
            c = _Case(t, n, par, xt, root0=root0)
            got = c.run(True)
            check_c(got, c.run(False), (mode, variant, "wrap"))
            check_b(got[2], se_stats(c.summands()), (mode, variant, "wrap"))
            low = _Case(t, n, par, xt[3:]).run(True)
            assert _same(got[2][3:], low[2]) and _same(got[0][3:], low[0]), (mode, variant, "wrapped roots")
            assert np.all(got[2] > 0)


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_a_nan_row_reports_a_nan_standard_error_and_disturbs_no_other_root(d):
    """MLP mode, one coordinate of one row in the middle of a wave is NaN: that root's u and se are NaN (never 0, never finite); every other root
    keeps the bits of the launch without it."""
    B = 4 * _rpw(d) + 1
    xt = _points(d, B, seed=1100 + d)
    bad = xt.copy()
    r = _rpw(d) // 2 if _rpw(d) > 1 else 1            # G = 64: one root per wave, the second wave's
    bad[r, d // 2] = np.nan
    others = np.arange(B) != r
    for variant, n, par in (("quad", 3, 3), ("fh", 4, 2)):
        t = _SeTree(0, d, variant, MLP)
        clean = _Case(t, n, par, xt).run(True)
        c = _Case(t, n, par, bad)
        got = c.run(True)
        check_c(got, c.run(False), (variant, "NaN row"))
        assert np.isnan(got[0][r, 0]) and np.isnan(got[2][r]), (variant, got[0][r, 0], got[2][r])
        assert _same(got[2][others], clean[2][others]) and _same(got[0][others], clean[0][others])
        assert np.all(np.isfinite(got[2][others]))


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_a_nan_quadrature_rule_reports_nan_standard_errors(d):
    """ACCUMULATE quadrature (4, 4) around the surrogate: the oracle's unclipped u is NaN at every root (the q = 5 rule's nodes are not
    increasing: SURVEY.md Appendix B), so se is NaN at every root."""
    xt = _points(d, 2, seed=1200 + d)
    t = _SeTree(0, d, "quad", ACC)
    assert np.isnan(se_stats(t.summands_oracle(4, 4, xt))["u"]).all()
    c = _Case(t, 4, 4, xt)
    got = c.run(True)
    check_c(got, c.run(False), "quad (4, 4)")
    assert np.isnan(got[0][:, 0]).all() and np.isnan(got[2]).all(), got[2]


# ------------------------------------------------------------------------------------------------------------- through the solver classes
_FITS = {}


def _scasml(d, seed=7):
    """The 60 + 20 point surrogate of tests/test_gpu_picard_stderr.py at dimension d, fitted once per d and never modified."""
    from oracle.equation import sample_points
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers.ScaSML import ScaSML
    if d not in _FITS:
        dom, bdy = sample_points(np.random.default_rng(seed), d, 60, 20)
        eq = Grad_Dependent_Nonlinear(d + 1)
        gp = GP_Grad_Dependent_Nonlinear(eq, compat=None)
        gp.GPsolver(dom, bdy, GN_steps=20)
        _FITS[d] = (eq, gp)
    eq, gp = _FITS[d]
    return ScaSML(eq, gp, seed=seed)


@gpu
@pytest.mark.parametrize("d", [43, 100])
def test_scasml_class_with_stderr_keeps_the_plain_bits_one_shot_and_chunked(d, monkeypatch):
    """G = 16 with idle lanes (d = 43) and G = 32 (d = 100): (u, z) of return_stderr=True is the plain call's, and a solve cut into chunks of 7
    roots returns the se bits of the one-shot solve."""
    import scasml_gp_amd.solvers._picard as P
    from oracle.equation import sample_points
    hip = _scasml(d)
    xt = np.concatenate(sample_points(np.random.default_rng(33), d, 38, 12))
    hip._engine.calls = 0
    plain = hip.uz_solve(2, 3, xt)
    hip._engine.calls = 0
    uz, se = hip.uz_solve(2, 3, xt, return_stderr=True)
    assert se.shape == (50, 1) and se.dtype == np.float32 and np.all(np.isfinite(se)) and np.all(se > 0)
    assert _same(plain, uz)
    ppr = int(P._lib.load().scasml_points_per_root(C.byref(hip._engine.plan(2, 3))))
    kp = int(P._lib.load().scasml_point_stride(d))
    monkeypatch.setattr(P, "POINT_BUFFER_BYTES", ppr * kp * 4 * 7)             # 7 roots per chunk
    hip._engine.calls = 0
    uz7, se7 = hip.uz_solve(2, 3, xt, return_stderr=True)
    assert _same(se7, se) and _same(uz7, uz)
