"""The stage kernel of the staged Picard tree (picard_stage_kernel<VAR>, csrc/picard_staged.hip, entry point scasml_picard_stage) at every
lane-group width, called through ctypes with float64 NumPy callbacks.

The kernel keeps its own copy of the lane mapping, the masks and the 32-bit row offsets of csrc/picard_tree.hpp, so the sweep of
tests/test_gpu_picard_sweep.py says nothing about it, and tests/test_gpu_callback_equations.py reaches it through the solver classes at
G = 4, 8 and 32 only, with float32 torch f and g between the kernel and the oracle.  Here _Staged restates PicardEngine._solve_staged with
the schedule of scasml_gp_amd.tables.stage_lists: GENERATE; g in float64 at the emitted terminal rows, cast to float32 once; for
S = 0 .. n-1 the stage-S kernel and then f in float64 on the gathered rows, cast once; the stage-n kernel into `out`.  No torch arithmetic
stands between kernel and oracle (oracle/mlp.py on the same Philox stream), so the bound is the tree sweep's where points are read back,
ATOL_RB + RTOL_RB |v| (tests/test_gpu_configs.py).  The near-T term of _atol_rb is not added: the terminal normals are replayed, not read
back (picard_staged.hip:68-71), and the read-back W_k = (X_k - x - mu c_k) / sigma carries one float32 rounding of O(1) numbers over
sigma (2.4e-7), which the z estimator multiplies by f w_k / (mc (c_k + 1e-6)) = O(f wfrac / cfrac): no division by T - t is left.

Checked: every d of D_SWEEP (both ends of every G, idle lanes, every d mod 4 -- which decides the float4 lane and component that hold u
in a uz row), both variants, stages 1..n of every level, ragged batches; the deepest quadrature level against the fused kernel's fixture;
staged against fused; the layout of a uz row; padding of a site stride > B; entries the kernel must skip; root0 and chunking; rows at T.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_callback_equations import _WavyNP
from test_gpu_picard_sweep import (ATOL, ATOL_RB, D_SWEEP, FLAG_D, G_ENDS, IDLE, RTOL, RTOL_RB, _close, _F4, _G, _ids, _kp, _points, _Q3, _ragged, _rpw,
                                   _Tree)

gpu = pytest.mark.gpu

# per d: (variant, n, par), dealt round the sweep; the deeper levels on small d (the oracle's cost is the tree's).  Quadrature n = 5 is one
# root against tests/golden/oracle_quad5_d13.npz.
STAGE_CASES = {d: [("quad",) + _Q3[(i + 1) % 3], ("fh",) + _F4[i % 4]] for i, d in enumerate(D_SWEEP)}
STAGE_CASES[6].append(("quad", 4, 4))
STAGE_CASES[13].append(("fh", 5, 2))
STAGE_CASES[125].append(("fh", 4, 2))
FUSED_CASES = {d: [("quad",) + _Q3[(i + 2) % 3], ("fh",) + _F4[(i + 2) % 4]] for i, d in enumerate(D_SWEEP)}
DEEP_QUAD = (13, ("quad", 5, 5))
NEAR_T_D = [43, 139]                      # G = 16 and G = 64
SENTINEL = np.uint32(0x7FC0BEEF)          # a NaN with a payload: what unwritten rows of `uz` and padding rows hold


def _nan():
    return np.float32(np.frombuffer(SENTINEL.tobytes(), dtype=np.float32)[0])


def test_the_sweep_reaches_every_width_stage_and_time_column():
    """Against the library's own point stride: both ends of every G, idle-lane d values of every G >= 16, all residues of d mod 4 (at
    G >= 8 too: the placements of u in a uz row), and stages 1..n of quadrature n = 1..4 (5: the fixture) and full history n = 1..5."""
    from scasml_gp_amd import _lib
    lib = _lib.load()
    stride = lambda d: int(lib.scasml_point_stride(d))
    G = lambda d: 1 << max(0, (stride(d) // 4 - 1).bit_length())
    assert all(_kp(d) == stride(d) and _G(d) == G(d) for d in range(1, _lib.MAX_DIM + 1))
    for cases in (STAGE_CASES, FUSED_CASES):
        assert set(cases) == set(D_SWEEP)
        for g, (lo, hi) in G_ENDS.items():
            assert G(lo) == G(hi) == g and (lo == 1 or G(lo - 1) == g // 2) and (hi == _lib.MAX_DIM or G(hi + 1) == 2 * g)
            assert lo in cases and hi in cases, g
        for g, (lo, hi) in IDLE.items():
            assert G(lo) == g and stride(lo) // 4 < g and {stride(d) for d in range(lo, hi + 1)} == {stride(lo)}
            assert any(lo <= d <= hi for d in cases), g
        assert {d % 4 for d in cases} == {0, 1, 2, 3} and {d % 4 for d in cases if G(d) >= 8} == {0, 1, 2, 3}
        assert all(n <= par for c in cases.values() for v, n, par in c if v == "quad")
    # a solve at level n runs stages 1..n
    got = {(v, n) for c in STAGE_CASES.values() for v, n, _ in c}
    assert got == {("quad", n) for n in range(1, 5)} | {("fh", n) for n in range(1, 6)} and DEEP_QUAD[1][:2] == ("quad", 5)
    assert sorted(G(d) for d in FLAG_D) == [4, 8, 16, 32, 64] and sorted(G(d) for d in NEAR_T_D) == [16, 64]
    assert any(lo <= d <= hi for d in FLAG_D for lo, hi in IDLE.values())
    assert all(1 in _ragged(d) and 4 * _rpw(d) + 1 in _ragged(d) for d in D_SWEEP)


# ------------------------------------------------------------------------------------------------------------- helpers
def _eq0(d):
    from oracle.equation import GradDependentNonlinear
    return GradDependentNonlinear(d + 1)


class _Staged:
    """PicardEngine._solve_staged restated: the launches through ctypes, f and g of ``oeq`` (the oracle's equation object) in float64."""

    def __init__(self, d, variant, oeq, seed=7, stream=3):
        from scasml_gp_amd import _lib
        self.d, self.variant, self.oeq = d, variant, oeq
        self.t = _Tree(0, d, variant, seed=seed, stream=stream)        # GENERATE evaluates neither f nor g: any registered id emits the same points
        self.kp = self.t.kp
        self.prob = _lib.Problem(d, _lib.EQ_GRAD_DEPENDENT_NONLINEAR, float(oeq.T), float(oeq.mu()), float(oeq.sigma()), float(oeq.norm_estimation))

    def plan(self, n, par):
        return self.t.plan(n, par)                                      # the MLP plan (stale delta_t), as PicardEngine(gp=None).plan

    def lists(self, n, par):
        from scasml_gp_amd import tables
        return tables.stage_lists(self.plan(n, par))

    def stage(self, S, plan, ent, B, stride, rng, pts, vals, uz, out):
        """One launch of the stage kernel.  -> the return code."""
        import torch
        from scasml_gp_amd import _lib
        e = torch.from_numpy(np.ascontiguousarray(ent, dtype=np.int32)).cuda()
        rc = _lib.load().scasml_picard_stage(C.byref(self.prob), C.byref(plan), S, _lib.ptr(e), e.shape[0], B, stride, rng, _lib.ptr(pts),
                                             _lib.ptr(vals), _lib.ptr(uz), _lib.ptr(out), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def solve(self, n, par, xt, root0=0, stride=0, pad=0.0, entries=None):
        """-> out (B, 1 + d) float64, and what the walk left: points (ppr, S, kp), values (ppr, S, 2), {stage: uz (ppr, S, kp) after it}.
        Padding rows (stride > B) of points and values hold ``pad``; every row of uz, padding included, starts as SENTINEL.  entries: {stage: list} to
        launch instead of the schedule's."""
        import torch
        from scasml_gp_amd import _lib
        lib = _lib.load()
        plan, lists = self.plan(n, par), self.lists(n, par)
        B, d, kp = xt.shape[0], self.d, self.kp
        S_ = stride or B
        ppr = int(lib.scasml_points_per_root(C.byref(plan)))
        rng = self.t.rng(root0=root0)
        x = torch.from_numpy(np.ascontiguousarray(xt, dtype=np.float32)).cuda()
        pts = torch.from_numpy(np.full((ppr * S_, kp), pad, dtype=np.float32)).cuda()
        _lib.check(self.t.launch(_lib.MODE_GENERATE, plan, x, B, stride, rng, pts=pts, prob=self.prob), "picard_tree(generate)")
        P = pts.cpu().numpy().reshape(ppr, S_, kp)
        vals = np.full((ppr, S_, 2), pad, dtype=np.float32)
        term = lists["terminals"]
        vals[term, :B, 0] = self.oeq.g(P[term, :B, :d + 1].reshape(-1, d + 1).astype(np.float64))[:, 0].reshape(len(term), B).astype(np.float32)
        uzh = np.full((ppr, S_, kp), _nan(), dtype=np.float32)
        uz = torch.from_numpy(uzh.reshape(-1, kp).copy()).cuda()
        out = torch.full((B, d + 1), -3.0, dtype=torch.float32, device="cuda")
        after = {}
        for S in range(n):
            if S >= 1:
                ent = lists["subtrees"][S] if entries is None or S not in entries else entries[S]
                vd = torch.from_numpy(vals.reshape(-1, 2).copy()).cuda()
                _lib.check(self.stage(S, plan, ent, B, stride, rng, pts, vd, uz, None), "picard_stage")
                after[S] = uz.cpu().numpy().reshape(ppr, S_, kp)
            node, child, slot = (lists["f_after"][S][:, j] for j in range(3))
            xf = P[node, :B, :d + 1].reshape(-1, d + 1).astype(np.float64)
            if S == 0:                                                   # the children are level-0 calls: (u, z) = 0 (MLP.py:205-207)
                u, z = np.zeros((xf.shape[0], 1)), np.zeros((xf.shape[0], d))
            else:                                                        # a uz row is (z_1 .. z_d, u, 0 ...)
                u = after[S][child, :B, d].reshape(-1, 1).astype(np.float64)
                z = after[S][child, :B, :d].reshape(-1, d).astype(np.float64)
            with np.errstate(all="ignore"):
                fv = np.asarray(self.oeq.f(xf, u, z), dtype=np.float64).reshape(len(node), B).astype(np.float32)
            vals[node, :B, slot] = fv
        vd = torch.from_numpy(vals.reshape(-1, 2).copy()).cuda()
        ent = lists["subtrees"][n] if entries is None or n not in entries else entries[n]
        _lib.check(self.stage(n, plan, ent, B, stride, rng, pts, vd, uz, out), "picard_stage")
        after[n] = uz.cpu().numpy().reshape(ppr, S_, kp)
        return out.cpu().numpy().astype(np.float64), P, vals, after

    def oracle(self, n, par, xt, root0=0):
        from oracle.mlp import PicardOracle
        return PicardOracle(self.oeq, self.variant, seed=self.t.seed, stream=self.t.stream).uz_solve(n, par, xt, root0=root0)

    def oracle_subtree(self, S, par, rows, root0, base):
        """(u, z) of the level-S call whose first site is ``base``, started at the point rows (x, t): PicardOracle.uz_call."""
        from oracle.mlp import PicardOracle
        return PicardOracle(self.oeq, self.variant, seed=self.t.seed, stream=self.t.stream).uz_call(S, par, rows, root0=root0, base=base)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- against the oracle
@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_staged_walk_matches_the_oracle_at_every_width_and_level(d):
    """An equation outside the registry (_WavyNP: f sees x, t and z component by component) through stages 1..n, ragged batches, root0 = 77:
    each launch compares with a prefix of the one oracle batch."""
    Bs = _ragged(d)
    xt = _points(d, Bs[-1], seed=2100 + d)
    for variant, n, par in STAGE_CASES[d]:
        s = _Staged(d, variant, _WavyNP(d + 1))
        want = s.oracle(n, par, xt, root0=77)
        for B in Bs:
            _close(s.solve(n, par, xt[:B], root0=77)[0], want[:B], ATOL_RB, RTOL_RB, (variant, n, par, B))


@gpu
def test_staged_walk_lands_on_the_quadrature_level_five_fixture():
    """Quadrature n = rho = 5 on one root at d = 13 with the closed forms of equation 0, seed 7 and stream 3: the fixture the fused kernel
    lands on (test_mlp_mode_quadrature_level_five_on_one_root).  That fixture is NaN in every component -- a level >= 4 call meets q = 5,
    whose tabulated nodes are not increasing, whatever the draws -- so the comparison of `out` pins where NaN goes
    and nothing else.  What is finite in this plan is checked beside it: the level-1..3 subtrees meet no q = 5, and the rows stages 1..3
    write for them are compared with the oracle's own (u, z) of those calls, at the first, a middle and the last subtree of each stage
    whose origin is a finite point."""
    d, (variant, n, par) = DEEP_QUAD
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_quad5_d13.npz"))
    assert np.isnan(g["uz"]).all()
    s = _Staged(d, variant, _eq0(d))
    assert (s.t.seed, s.t.stream) == (7, 3)
    out, P, vals, after = s.solve(n, par, g["x_t"])
    _close(out, g["uz"], ATOL_RB, RTOL_RB, "quad n=5")
    lists = s.lists(n, par)
    for S in (1, 2, 3):
        ent = lists["subtrees"][S]
        ent = ent[np.isfinite(P[ent[:, 1], 0]).all(axis=1)]
        assert len(ent) >= 3
        for base, origin in (ent[0], ent[len(ent) // 2], ent[-1]):
            want = s.oracle_subtree(S, par, P[origin, :1, :d + 1], 0, base)
            row = after[S][base, :1]
            assert np.isfinite(want).all() and np.all(row[:, d + 1:] == 0)
            _close(np.concatenate([row[:, d:d + 1], row[:, :d]], axis=1).astype(np.float64), want, ATOL_RB, RTOL_RB, ("quad n=5 stage", S, int(base)))


@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_staged_walk_matches_the_fused_kernel_on_equation_zero(d):
    """f and g of equation 0 as callbacks against SCASML_MODE_MLP on the same stream.  Bound: the sum of the two bounds each side holds
    against the oracle (ATOL, RTOL: tests/test_gpu_mlp.py; ATOL_RB, RTOL_RB: tests/test_gpu_configs.py)."""
    B = _ragged(d)[-1]
    xt = _points(d, B, seed=2200 + d)
    for variant, n, par in FUSED_CASES[d]:
        s = _Staged(d, variant, _eq0(d))
        fused = s.t.mlp(n, par, xt, s.t.rng(root0=3))
        _close(s.solve(n, par, xt, root0=3)[0], fused, ATOL + ATOL_RB, RTOL + RTOL_RB, (variant, n, par))


# ------------------------------------------------------------------------------------------------------------- the uz buffer
@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_uz_rows_hold_z_then_u_then_zeros_and_padding_is_left_alone(d):
    """After an intermediate stage every written row is (z_1 .. z_d, u, 0 ...): u in column d -- against the oracle's own (u, z) of that
    subtree -- and columns d + 1 .. kp - 1 exactly 0; rows of sites that are no subtree base of the stage, and padding rows of a site
    stride > B (NaN in points, values and uz), keep their bits, and the result is that of the unpadded walk bit for bit."""
    B = _rpw(d) + 1
    xt = _points(d, B, seed=2300 + d)
    stride = B + 3
    for variant, n, par in (("quad", 2, 2), ("fh", 3, 2)):
        s = _Staged(d, variant, _WavyNP(d + 1))
        plain = s.solve(n, par, xt, root0=9)
        out, P, vals, after = s.solve(n, par, xt, root0=9, stride=stride, pad=_nan())
        assert np.array_equal(_bits(out), _bits(plain[0])), (variant, "padding changed the result")
        assert np.all(_bits(P[:, B:]) == SENTINEL)
        lists = s.lists(n, par)
        written = np.zeros(P.shape[0], dtype=bool)
        for S in range(1, n):
            ent = lists["subtrees"][S]
            written[ent[:, 0]] = True
            U = after[S]
            assert np.all(_bits(U[:, B:]) == SENTINEL), (variant, S, "padding rows of uz")
            assert np.all(_bits(U[~written, :B]) == SENTINEL), (variant, S, "rows of other sites")
            rows = U[ent[:, 0], :B]
            assert np.array_equal(_bits(rows), _bits(plain[3][S][ent[:, 0]])), (variant, S)
            assert np.all(_bits(rows[:, :, d + 1:]) == 0) and np.all(np.isfinite(rows)), (variant, S, "columns past u")
            for base, origin in (ent[0], ent[len(ent) // 2], ent[-1]):
                want = s.oracle_subtree(S, par, P[origin, :B, :d + 1], 9, base)
                got = np.concatenate([rows[list(ent[:, 0]).index(base)][:, d:d + 1], rows[list(ent[:, 0]).index(base)][:, :d]], axis=1).astype(np.float64)
                _close(got, want, ATOL_RB, RTOL_RB, (variant, S, int(base)))
        assert np.array_equal(_bits(after[n]), _bits(after[n - 1])), (variant, "the last stage wrote to uz")


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_entries_that_are_no_subtree_are_skipped(d):
    """(-1, 0), (0, ppr) and a base one past ppr - 1 - sites[S] between the valid entries: the valid ones give the same bits as without
    them, nothing else in uz changes, and the result is the same."""
    from scasml_gp_amd import _lib
    B = 2 * _rpw(d) + 1
    xt = _points(d, B, seed=2400 + d)
    for variant, n, par in (("quad", 2, 2), ("fh", 2, 3)):
        s = _Staged(d, variant, _WavyNP(d + 1))
        plan = s.plan(n, par)
        ppr = int(_lib.load().scasml_points_per_root(C.byref(plan)))
        mixed = {}
        for S in range(1, n + 1):
            ent = s.lists(n, par)["subtrees"][S]
            bad = np.array([[-1, 0], [0, ppr], [ppr - int(plan.sites[S]), 0], [0, -1]], dtype=np.int32)
            assert S == n or 0 not in ent[:, 0]                          # site 0 is a terminal sample of the root call
            rows = []
            for i, e in enumerate(ent):
                rows += [bad[i % len(bad)], e]
            mixed[S] = np.array(rows + [bad[1], bad[2]], dtype=np.int32)
        mixed[n] = np.array([[-1, 0], [0, ppr], [1, ppr - 1]] + [list(e) for e in s.lists(n, par)["subtrees"][n]] + [[0, -1]], dtype=np.int32)
        plain = s.solve(n, par, xt)
        got = s.solve(n, par, xt, entries=mixed)
        assert np.array_equal(_bits(got[0]), _bits(plain[0])), variant
        for S in range(1, n + 1):
            assert np.array_equal(_bits(got[3][S]), _bits(plain[3][S])), (variant, S)


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_chunks_with_their_root0_give_the_bits_of_the_whole_batch(d):
    """Rows r .. r + k launched with root0 = r (more than one wave per entry among them) are those rows of the whole batch, bit for bit:
    the normals are independent of the chunking (PicardEngine._solve_staged's root0 + b0)."""
    r = _rpw(d)
    B = 2 * r + 3
    xt = _points(d, B, seed=2500 + d)
    for variant, n, par in (("quad", 2, 2), ("fh", 3, 2)):
        s = _Staged(d, variant, _WavyNP(d + 1))
        whole = s.solve(n, par, xt)[0]
        for r0, k in ((1, r), (r + 1, B - r - 1), (B - 1, 1)):
            part = s.solve(n, par, xt[r0:r0 + k], root0=r0)[0]
            assert np.array_equal(part.view(np.uint64), whole[r0:r0 + k].view(np.uint64)), (variant, r0, k)
        assert not np.array_equal(s.solve(n, par, xt[1:1 + r], root0=0)[0], whole[1:1 + r])


@gpu
@pytest.mark.parametrize("d", NEAR_T_D, ids=_ids(NEAR_T_D))
def test_rows_at_and_just_below_terminal_time(d):
    """T - t = 0 and one float32 ulp, beside ordinary roots: the horizon is zero (or rounds to it one call down), the terminal normals are
    replayed and the z estimator's scale is 1 / 1e-6 (quadrature) or 1 / 0 (full history: +-inf into the clip, as in the oracle)."""
    T = np.float32(0.5)
    xt = _points(d, 6, seed=2600 + d)
    xt[0, d], xt[1, d] = T, np.nextafter(T, np.float32(0))
    xt[3, d], xt[4, d] = np.nextafter(T, np.float32(0)), T
    for variant, n, par in (("quad", 2, 2), ("fh", 2, 3)):
        s = _Staged(d, variant, _WavyNP(d + 1))
        _close(s.solve(n, par, xt)[0], s.oracle(n, par, xt), ATOL_RB, RTOL_RB, (variant, "at T"))


# ------------------------------------------------------------------------------------------------------------- argument checks
@gpu
def test_stage_kernel_argument_checks_not_pinned_elsewhere():
    """What tests/test_gpu_callback_equations.py test_stage_kernel_validates_its_arguments leaves out: a site block too large for the 32-bit
    row offsets, B = 0 (returns 0 and touches nothing, whatever the pointers) and an intermediate stage without uz."""
    import torch
    from scasml_gp_amd import _lib, tables
    lib = _lib.load()
    plan = tables.build_plan("quad", 2, 2, 0.5, True)
    prob = _lib.Problem(10, 0, 0.5, 0.0, 0.25, 1.0)
    kp = int(lib.scasml_point_stride(10))
    ent = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    buf = torch.full((64,), 7.0, device="cuda")
    p, e, s = _lib.ptr(buf), _lib.ptr(ent), _lib.stream_ptr()
    rng = _lib.Rng(0, 0, 0, 0, 1, 0, 0)
    call = lambda *a: lib.scasml_picard_stage(C.byref(prob), C.byref(plan), *a, s)
    assert call(1, e, 1, 1, (1 << 32) // kp, rng, p, p, p, p) == -2 and b"32-bit row offsets" in lib.scasml_last_error()
    assert call(1, e, 1, 0, 0, rng, p, p, p, p) == 0 and call(2, e, 1, 0, 8, rng, None, None, None, None) == 0      # B = 0
    assert call(1, e, 1, 1, 0, rng, p, p, None, p) == -1 and b"needs uz" in lib.scasml_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((ent == 0).all())
