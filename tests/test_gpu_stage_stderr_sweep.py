"""The standard-error form of the staged tree's root call (picard_stage_kernel<VAR, true>, csrc/picard_staged.hip, entry point
scasml_picard_stage_stderr) at every lane-group width, called through ctypes with float64 NumPy callbacks as tests/test_gpu_stage_sweep.py
calls the plain kernel.

The equation is _Steep: _WavyNP (tests/test_gpu_callback_equations.py) with the terminal function g = cos(2 sum x_i).  _WavyNP's own g is a
mean over the dims, whose spread over the terminal samples falls with d, and with it se_u against the bound of check (a).

out_se_uz holds rows (se_u, se_z_1 .. se_z_d).  Both outputs are prefilled with -3.0 and out_se_uz has one spare row after the batch, which every
launch asserts still holds -3.0.  Every case runs five checks:

(a) se_uz against the float64 oracle's own summands in all 1 + d columns (PicardOracle.root_summands(with_z=True), root0 = 77), within the
    project's rule for the standard-error sweeps with the staged path's parity bounds, 2 (ATOL_RB + RTOL_RB max(|unclipped value|, se)).  Guard,
    from the oracle alone: the median root's se_u and every finite z component's se are at least 10 x their bound.
(b) se_uz against the DEVICE's own summands.  The plain scasml_picard_stage is linear in `values`: launched at stage n with prob.clip the largest
    float32 and `values` zeroed except at the sites of ONE summand -- terminal sample m (site m, slot 0) or the q nodes of path m of term l (both
    slots; the kernel's own offsets, o = mg and then o += 1 + sites_l + sites_lm1 per node) -- its out_uz is that summand's unclipped float32
    (u, z), added up in the order the standard-error kernel adds ym and zm.  With all mg + sum mc summands in float64, se_stats_z
    (tests/test_gpu_stderr_uz_sweep.py) gives se64 and the derived bound bound_z; |se_uz - se64| <= bound_z per component, exactly 0 where
    se64 = 0, non-finite where se64 is.  The derivation is that sweep's: the accumulators are the same SeTerm / SeTerm4, closed the same way.
(c) out_uz of the new entry equals the plain last-stage launch bit for bit.
(d) a root's row of se_uz keeps its bits under every prefix batch, under a site_stride past the batch with SENTINEL NaNs in every padding row of
    points and values, and in chunks launched with their own root0.
(e) non-finite values: quadrature (4, 4) (the q = 5 rule's nodes are not increasing: SURVEY.md Appendix B), rows at t = T and one ulp below,
    a NaN coordinate.

Beside the sweep: staged against fused on equation 0 (a consistency check).  SCASML_STAGE_STDERR_SWEEP_JSON=path writes the largest observed
|diff| / bound per case (profiles/picard_stage_stderr_sweep.json is such a file).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_callback_equations import _WavyNP
from test_gpu_picard_sweep import ATOL, ATOL_RB, D_SWEEP, FLAG_D, G_ENDS, IDLE, RTOL, RTOL_RB, _G, _ids, _points, _ragged, _rpw
from test_gpu_stage_sweep import SENTINEL, _eq0, _nan, _Staged
from test_gpu_stderr_uz_sweep import se_stats_z

gpu = pytest.mark.gpu

_Q = [(1, 3), (2, 3), (3, 3)]
_F = [(1, 3), (2, 3), (3, 2), (4, 2)]
SE_CASES = {d: [("quad",) + _Q[i % 3], ("fh",) + _F[i % 4]] for i, d in enumerate(D_SWEEP)}
SE_CASES[13].append(("fh", 5, 2))
NEAR_T_D = [43, 139]                      # G = 16 and G = 64
SEED, STREAM, ROOT0 = 7, 3, 77


class _Steep(_WavyNP):
    """_WavyNP with a terminal function whose spread over the terminal samples does not average out with d."""

    def g(self, x_t):
        return np.cos(2.0 * np.sum(x_t[:, :-1], axis=1, keepdims=True))


def test_the_stage_stderr_sweep_reaches_every_width_residue_and_level():
    """Against the library's own point stride: both ends of every G, idle-lane d values of every G >= 16, all residues of d mod 4, quadrature
    n = 1..3 and full history n = 1..5; every plan has mg >= 2 and mc >= 2 (the entry refuses any other)."""
    from scasml_gp_amd import _lib, tables
    lib = _lib.load()
    stride = lambda d: int(lib.scasml_point_stride(d))
    G = lambda d: 1 << max(0, (stride(d) // 4 - 1).bit_length())
    assert set(SE_CASES) == set(D_SWEEP) and all(_G(d) == G(d) for d in D_SWEEP)
    for g, (lo, hi) in G_ENDS.items():
        assert G(lo) == G(hi) == g and (lo == 1 or G(lo - 1) == g // 2) and (hi == _lib.MAX_DIM or G(hi + 1) == 2 * g)
        assert lo in SE_CASES and hi in SE_CASES, g
    for g, (lo, hi) in IDLE.items():
        assert G(lo) == g and stride(lo) // 4 < g and any(lo <= d <= hi for d in SE_CASES), g
    assert {d % 4 for d in SE_CASES} == {0, 1, 2, 3} and {d % 4 for d in SE_CASES if G(d) >= 8} == {0, 1, 2, 3}
    got = {(v, n) for c in SE_CASES.values() for v, n, _ in c}
    assert got == {("quad", n) for n in range(1, 4)} | {("fh", n) for n in range(1, 6)}
    for v, n, par in {c for cases in SE_CASES.values() for c in cases} | {("quad", 4, 4)}:
        plan = tables.build_plan(v, n, par, 0.5, True)
        assert int(plan.mg[n]) >= 2 and all(int(plan.term[n][l].mc) >= 2 for l in range(n)), (v, n, par)
    assert sorted(G(d) for d in FLAG_D) == [4, 8, 16, 32, 64] and sorted(G(d) for d in NEAR_T_D) == [16, 64]
    assert all(1 in _ragged(d) and 4 * _rpw(d) + 1 in _ragged(d) for d in D_SWEEP)


# ------------------------------------------------------------------------------------------------------------- helpers
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def bound_a(st, atol=ATOL_RB, rtol=RTOL_RB):
    return 2.0 * (atol + rtol * np.maximum(np.abs(st["u"]), st["se"]))


def summand_sites(plan, n):
    """Per summand of the root call, in the order of root_summands: [(N_j, [sites of summand 0, sites of summand 1, ...])], by the stage
    kernel's own offsets."""
    mg = int(plan.mg[n])
    groups = [(mg, [[m] for m in range(mg)])]
    o = mg
    for l in range(n):
        tm = plan.term[n][l]
        paths = []
        for m in range(int(tm.mc)):
            nodes = []
            for k in range(int(tm.q)):
                nodes.append(o)
                o += 1 + int(tm.sites_l) + int(tm.sites_lm1)
            paths.append(nodes)
        groups.append((int(tm.mc), paths))
    assert o == int(plan.sites[n])
    return groups


class _StagedSe(_Staged):
    """_Staged with the launch of scasml_picard_stage_stderr for the last stage, on the points and values the plain walk left."""

    def _last(self, n, par, B, stride, root0, P, vals, se, prob=None):
        """One launch of the root call on host points (ppr, S, kp) and values (ppr, S, 2): the plain entry (se false) or the new one.
        -> out (B, 1 + d) float32, and with se the standard errors (B, 1 + d) float32."""
        import torch
        from scasml_gp_amd import _lib
        lib, d, plan = _lib.load(), self.d, self.plan(n, par)
        ent = torch.from_numpy(np.ascontiguousarray(self.lists(n, par)["subtrees"][n], dtype=np.int32)).cuda()
        pts = torch.from_numpy(np.ascontiguousarray(P.reshape(-1, self.kp))).cuda()
        vd = torch.from_numpy(np.ascontiguousarray(vals.reshape(-1, 2))).cuda()
        out = torch.full((B, d + 1), -3.0, dtype=torch.float32, device="cuda")
        rng = self.t.rng(root0=root0)
        head = (C.byref(prob or self.prob), C.byref(plan), n, _lib.ptr(ent), ent.shape[0], B, stride, rng, _lib.ptr(pts), _lib.ptr(vd))
        if not se:
            _lib.check(lib.scasml_picard_stage(*head, None, _lib.ptr(out), _lib.stream_ptr()), "picard_stage")
            torch.cuda.synchronize()
            return out.cpu().numpy()
        s = torch.full((B + 1, d + 1), -3.0, dtype=torch.float32, device="cuda")
        _lib.check(lib.scasml_picard_stage_stderr(*head, _lib.ptr(out), _lib.ptr(s), _lib.stream_ptr()), "picard_stage_stderr")
        torch.cuda.synchronize()
        s = s.cpu().numpy()
        assert np.all(s[B:] == -3.0), ("out_se_uz was written past its B rows", d, B, stride)
        return out.cpu().numpy(), s[:B]

    def solve_se(self, n, par, xt, root0=0, stride=0, pad=0.0):
        """The staged walk, then the new entry on what it left.  -> (out, se_uz) float32; out is asserted to carry the bits of the plain
        last-stage launch: check (c).  Keeps (par, P, vals) for the masked launches of check (b)."""
        out64, P, vals, _ = self.solve(n, par, xt, root0=root0, stride=stride, pad=pad)
        B = xt.shape[0]
        out, se = self._last(n, par, B, stride, root0, P, vals, True)
        assert _same(out, out64.astype(np.float32)), (self.d, self.variant, n, par, B, "out_uz differs from the plain launch")
        self.left = (par, P, vals)
        return out, se

    def huge_clip(self):
        from scasml_gp_amd import _lib
        p = self.prob
        return _lib.Problem(p.d, p.eq_id, p.T, p.mu, p.sigma, float(np.finfo(np.float32).max))

    def unclipped(self, n, B, root0=0, stride=0):
        """The plain launch of the root call under the largest float32 clip: the unclipped (u, z)."""
        par, P, vals = self.left
        return self._last(n, par, B, stride, root0, P, vals, False, prob=self.huge_clip())

    def summands(self, n, B, root0=0):
        """The device's own summands: one plain launch per summand with every other site's values zeroed.  -> [Y_g, Y_0, ...] float64
        (N_j, B, 1 + d)."""
        par, P, vals = self.left
        prob = self.huge_clip()
        Ys = []
        for N, summ in summand_sites(self.plan(n, par), n):
            rows = []
            for sites in summ:
                masked = np.zeros_like(vals)
                masked[sites] = vals[sites]
                rows.append(self._last(n, par, B, 0, root0, P, masked, False, prob=prob).astype(np.float64))
            Ys.append(np.stack(rows))
        return Ys

    def oracle_stats(self, n, par, xt, root0=0):
        from oracle.mlp import PicardOracle
        return se_stats_z(PicardOracle(self.oeq, self.variant, seed=self.t.seed, stream=self.t.stream).root_summands(n, par, xt, root0=root0, with_z=True))


def _staged(d, variant, oeq=None):
    return _StagedSe(d, variant, oeq or _Steep(d + 1), seed=SEED, stream=STREAM)


MEASURED = {}                  # "(variant) n=(n) (what)" -> a, b: largest dev / bound; s_u, s_z: smallest se / bound (a) of the guard


def _record(key, **kw):
    m = MEASURED.setdefault("%s n=%d %s" % key, {})
    for k, v in kw.items():
        m[k] = min(m.get(k, float("inf")), float(v)) if k.startswith("s") else max(m.get(k, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("SCASML_STAGE_STDERR_SWEEP_JSON")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump(dict(atol=ATOL_RB, rtol=RTOL_RB, checks={k: MEASURED[k] for k in sorted(MEASURED)}), f, indent=1, sort_keys=True)
            f.write("\n")


def _finite(st):
    with np.errstate(invalid="ignore"):
        return np.isfinite(st["se"]) & np.isfinite(st["u"])


def guard_a(st, what, key=None):
    """From the oracle alone: the median root's se_u and every finite z component's se are at least 10 x their bound of check (a)."""
    bound, se, fin = bound_a(st), st["se"], _finite(st)
    r = np.argsort(se[:, 0])[se.shape[0] // 2]
    zr = (se[:, 1:] / bound[:, 1:])[fin[:, 1:]]
    print("guard %s: median se_u / bound %.1f, smallest z se / bound %.1f" % (what, se[r, 0] / bound[r, 0], zr.min() if zr.size else np.inf))
    if key:
        _record(key, s_u=se[r, 0] / bound[r, 0], **({"s_z": zr.min()} if zr.size else {}))
    assert fin[r, 0] and se[r, 0] >= 10.0 * bound[r, 0], (what, "guard, se_u", se[r, 0] / bound[r, 0])
    assert np.all(zr >= 10.0), (what, "guard, se_z", zr.min())


def check_a(se, st, what, key=None):
    se, fin = se.astype(np.float64), _finite(st)
    assert not np.any(np.isfinite(se[~fin])), (what, "a finite se where the oracle's value or se is not finite")
    assert np.all(np.isfinite(se[fin])), (what, "se is not finite where the oracle's is")
    if not fin.any():
        return
    bound, dev = bound_a(st)[fin], np.abs(se - st["se"])[fin]
    print("check (a) %s: max |dev| %.3e, max dev / bound %.4f" % (what, dev.max(), (dev / bound).max()))
    if key:
        _record(key, a=(dev / bound).max())
    assert np.all(dev <= bound), (what, dev.max(), (dev / bound).max())


def check_b(se, dev_st, what, key=None):
    se, se64, bound = se.astype(np.float64), dev_st["se"], dev_st["bound_z"]
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(se64)
    assert np.array_equal(np.isfinite(se), fin), (what, "se is finite exactly where the device's own summands make it so")
    zero = fin & (se64 == 0)
    assert np.all(se[zero] == 0.0), (what, "se64 = 0 but the kernel's se is not")
    ok = fin & ~zero
    if not ok.any():
        return
    dev, bound = np.abs(se - se64)[ok], bound[ok]
    print("check (b) %s: max |se - se64| %.3e, max / bound %.4f, bound / se %.2e..%.2e" % (what, dev.max(), (dev / bound).max(), (bound / se64[ok]).min(),
                                                                                         (bound / se64[ok]).max()))
    if key:
        _record(key, b=(dev / bound).max())
    assert np.all(dev <= bound), (what, dev.max(), (dev / bound).max(), int(np.argmax(dev / bound)))


# ------------------------------------------------------------------------------------------------------------- the sweep
@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_stage_stderr_at_every_width_and_level(d):
    """Checks (a) .. (d) of the module docstring; the roots of every batch are a prefix of the largest one."""
    Bs = _ragged(d)
    B = Bs[-1]
    xt = _points(d, B, seed=3100 + d)
    for variant, n, par in SE_CASES[d]:
        key, what = (variant, n, "sweep"), (variant, n, par, d)
        s = _staged(d, variant)
        st = s.oracle_stats(n, par, xt, root0=ROOT0)
        assert _finite(st).all(), what
        guard_a(st, what, key=key)
        out, se = s.solve_se(n, par, xt, root0=ROOT0)                                  # (c) inside
        check_a(se, st, what, key=key)
        check_b(se, se_stats_z(s.summands(n, B, root0=ROOT0)), what, key=key)
        for b in Bs[:-1]:                                                              # (d): every prefix batch
            out_b, se_b = s.solve_se(n, par, xt[:b], root0=ROOT0)
            assert _same(se_b, se[:b]) and _same(out_b, out[:b]), (what, b, "se_uz of a root depends on the batch")
        S = B + 3                                                                      # (d): a site stride past the batch, NaN in every padding row
        out_p, se_p = s.solve_se(n, par, xt, root0=ROOT0, stride=S, pad=_nan())
        assert np.all(_bits(s.left[1][:, B:]) == SENTINEL) and np.all(_bits(s.left[2][:, B:]) == SENTINEL)
        assert _same(se_p, se) and _same(out_p, out), (what, "site_stride", S)


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_chunks_with_their_root0_give_the_standard_errors_of_the_whole_batch(d):
    """(d): rows r .. r + k launched with root0 = r are those rows of the whole batch, bit for bit (PicardEngine._solve_staged's root0 + b0)."""
    r = _rpw(d)
    B = 2 * r + 3
    xt = _points(d, B, seed=3300 + d)
    for variant, n, par in (("quad", 2, 3), ("fh", 3, 2)):
        s = _staged(d, variant)
        out, se = s.solve_se(n, par, xt)
        for r0, k in ((1, r), (r + 1, B - r - 1), (B - 1, 1)):
            out_c, se_c = s.solve_se(n, par, xt[r0:r0 + k], root0=r0)
            assert _same(se_c, se[r0:r0 + k]) and _same(out_c, out[r0:r0 + k]), (variant, r0, k)
        assert not _same(s.solve_se(n, par, xt[1:1 + r], root0=0)[1], se[1:1 + r])


# ------------------------------------------------------------------------------------------------------------- (e) non-finite values
@gpu
def test_quadrature_level_four_is_finite_exactly_where_the_unclipped_root_sum_is():
    """Quadrature (4, 4) at d = 6, B = 5, no oracle: se_z is finite exactly where the plain launch under the largest float32 clip has a finite
    unclipped z, and se_u is NaN exactly where that u is NaN.  (Check (b) is left out: a NaN point would leak through 0 * NaN in the masked
    launches.)"""
    d, B, (variant, n, par) = 6, 5, ("quad", 4, 4)
    s = _staged(d, variant)
    out, se = s.solve_se(n, par, _points(d, B, seed=3400))
    raw = s.unclipped(n, B)
    assert np.array_equal(np.isfinite(se[:, 1:]), np.isfinite(raw[:, 1:])), (se, raw)
    assert np.array_equal(np.isnan(se[:, 0]), np.isnan(raw[:, 0])), (se[:, 0], raw[:, 0])
    assert not np.isfinite(raw[:, 1:]).all(), "the q = 5 rule was expected to leave a non-finite z"


@gpu
@pytest.mark.parametrize("d", NEAR_T_D, ids=_ids(NEAR_T_D))
def test_rows_at_and_just_below_terminal_time(d):
    """Rows at t = T and one float32 ulp below, beside ordinary roots.  Quadrature: every se is finite (the terminal scale is 1 / (mg 1e-6)) and
    column 0 exactly 0 at t = T, where every sample of g coincides and every node's weight is 0.  Full history at t = T: the scale is 1 / 0
    and every se_z non-finite.  The ordinary roots keep the bits they have in the batch whose rows all lie at ordinary times."""
    T = np.float32(0.5)
    plain = _points(d, 6, seed=3500 + d)
    xt = plain.copy()
    xt[0, d], xt[1, d] = T, np.nextafter(T, np.float32(0))
    xt[3, d], xt[4, d] = np.nextafter(T, np.float32(0)), T
    for variant, n, par in (("quad", 2, 3), ("fh", 2, 3)):
        s = _staged(d, variant)
        out, se = s.solve_se(n, par, xt)
        if variant == "quad":
            assert np.all(np.isfinite(se)) and se[0, 0] == 0.0 and se[4, 0] == 0.0, (variant, se[:, 0])
        else:
            assert not np.any(np.isfinite(se[[0, 4], 1:])), (variant, "a finite se_z at t = T")
            assert np.all(np.isfinite(se[[2, 5]]))
        check_a(se, s.oracle_stats(n, par, xt), (variant, n, "near T", d), key=(variant, n, "near T"))
        out0, se0 = s.solve_se(n, par, plain)
        assert _same(se[[2, 5]], se0[[2, 5]]) and _same(out[[2, 5]], out0[[2, 5]]), (variant, "a root at t = T moved a neighbour's bits")


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_a_nan_coordinate_makes_its_whole_row_nan_and_disturbs_no_other_root(d):
    B = 4 * _rpw(d) + 1
    xt = _points(d, B, seed=3600 + d)
    bad = xt.copy()
    r = _rpw(d) // 2 if _rpw(d) > 1 else 1            # G = 64: one root per wave, the second wave's
    bad[r, d // 2] = np.nan
    others = np.arange(B) != r
    for variant, n, par in (("quad", 2, 3), ("fh", 3, 2)):
        s = _staged(d, variant)
        out0, se0 = s.solve_se(n, par, xt)
        out, se = s.solve_se(n, par, bad)
        assert np.isnan(se[r]).all() and np.isnan(out[r]).all(), (variant, se[r])
        assert _same(se[others], se0[others]) and _same(out[others], out0[others]), variant
        assert np.all(np.isfinite(se[others])) and np.all(se[others] > 0)


# ------------------------------------------------------------------------------------------------------------- staged against fused
@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_staged_standard_errors_agree_with_the_fused_kernel_on_equation_zero(d):
    """f and g of equation 0 as callbacks against scasml_picard_tree_stderr_uz in SCASML_MODE_MLP on the same stream.  Bound: the sum of the
    bounds of check (a) either side holds against the oracle (ATOL, RTOL fused; ATOL_RB, RTOL_RB staged), each formed from that side's own
    (u, z) and se.  A consistency check only: equation 0 saturates at large d, so it carries no guard."""
    import torch
    from scasml_gp_amd import _lib
    B = _ragged(d)[-1]
    xt = _points(d, B, seed=3700 + d)
    for variant, n, par in (("quad", 2, 3), ("fh", 2, 3)):
        s = _staged(d, variant, _eq0(d))
        out, se = s.solve_se(n, par, xt, root0=3)
        x = torch.from_numpy(np.ascontiguousarray(xt, dtype=np.float32)).cuda()
        fo = torch.full((B, d + 1), -3.0, dtype=torch.float32, device="cuda")
        fs = torch.full((B, d + 1), -3.0, dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().scasml_picard_tree_stderr_uz(C.byref(s.prob), C.byref(s.plan(n, par)), _lib.MODE_MLP, _lib.ptr(x), B, 0, s.t.rng(root0=3),
                                                            None, None, _lib.ptr(fo), None, _lib.ptr(fs), _lib.stream_ptr()), "picard_tree_stderr_uz")
        torch.cuda.synchronize()
        fo, fs = fo.cpu().numpy().astype(np.float64), fs.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isfinite(se), np.isfinite(fs)), variant
        fin = np.isfinite(fs)
        bound = bound_a(dict(u=out.astype(np.float64), se=se.astype(np.float64))) + bound_a(dict(u=fo, se=fs), ATOL, RTOL)
        dev = np.abs(se.astype(np.float64) - fs)
        print("staged vs fused %s d=%d: max dev / bound %.4f" % (variant, d, (dev[fin] / bound[fin]).max()))
        _record((variant, n, "staged vs fused"), a=(dev[fin] / bound[fin]).max())
        assert np.all(dev[fin] <= bound[fin]), (variant, (dev[fin] / bound[fin]).max())
