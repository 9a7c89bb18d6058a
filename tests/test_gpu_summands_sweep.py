"""The summand kernels (scasml_picard_tree_summands: picard_sum_kernel<VAR, MODE, N, EQ, SUM>, the walker under its SUM flavour) and the kernel that
closes the standard errors from a completed table (scasml_picard_summands_stderr) at every lane-group width, level and mode, called through ctypes
with the cases, batches, points and surrogate of tests/test_gpu_stderr_sweep.py.

The table is allocated as (S + 1, ldy, ncol) and prefilled with a NaN of a payload no arithmetic produces (FILL_BITS); out_uz and out_uhat have one
spare row and hold -3.0, out_se seven spare floats.  EVERY launch asserts that the ldy - B rows behind each summand, the whole spare summand and the
spare rows of out_uz / out_uhat / out_se still hold their fill, and that no entry inside the S x B x ncol block does.

Every (d, mode, case) of the fused sweeps runs, at the ragged batches of _ragged(d):

(a) the table against the DEVICE's own summands.  Summand i's sharded plain launch (rank 0 of a world of 2 owns that summand's units and nothing
    else) returns its unclipped float32 (u, z) through the same walker, in the same order of operations.  Entry [i, root, c] of the world = 1 table,
    in both SUM forms: exactly 0 where the launch's is (the sign of zero apart), not finite where it is not, and otherwise
    |difference| <= k 2^-24 |launch's value| with the z sweep's allowances, K_LEVEL = 4 for a level entry and for u's terminal entry, K_TERMINAL = 6
    for z's terminal entries.  Largest batch of each case; quadrature n = 5 (3224 summands) on DEEP_QUAD's one root.
(b) the table against the float64 oracle (PicardOracle.root_summands(with_z=True), one walk per case, cached) under
    tests/test_gpu_picard_summands.py's _check_table with its (ATOL, RTOL) per mode: every case with a finite z (quadrature n <= 3, every full-history
    level) at the largest batch.  Quadrature n = 4 is consulted at one d and one root, n = 5 has its NaN pattern from tests/golden.
(c) out_uz and, in ACCUMULATE, out_uhat equal the plain launch's bit for bit; the SUM = 1 table equals column 0 of the SUM = 2 table bit for bit.
(d) a root's entries keep their bits under every prefix batch, under ldy = B + 3 against ldy = 0 and, in ACCUMULATE, under a site_stride past the
    batch with NaN in every padding row.
(e) the ranks' tables add up (one case per d).  Worlds 2 and 3 with owner = NULL (unit % world splits a path's addends): every entry written, and
    the float32 sum of the ranks' tables within (world - 1) 2^-24 sum_r |partial_r| of the float64 sum of the same partials (one rounding per
    addition); where z is finite the summed table also meets check (b)'s bound.  World 2 with every summand whole on one rank: the other rank holds
    exact zeros there and the owner's rows equal the world = 1 table bit for bit.
(f) the closing kernel against float64 on ITS OWN input: se64 per column from the device's world = 1 table by se_stats / se_stats_z, and
    |se - se64| <= max(sqrt(Var + B_var) - se64, se64 - sqrt(max(Var - B_var, 0))) with the fused sweeps' B_var (the roundings of SeTerm<true>) and
    B_Y = 0 -- the input is the table itself; both ncol, ldy = 0 and ldy = B + 3.  se is exactly 0 where se64 is and not finite where se64 is not.
    Guard: the median se64 / bound over the finite columns is at least 10 -- on the device's table, and from the oracle's summands alone in
    test_the_closing_kernels_bound_is_far_below_the_standard_errors (no GPU).

Beside the sweep: all 100 instantiations (2 variants x 5 levels x TABLE_EQ_MODES x SUM) at one d per G, roots on both sides of the read-back switch,
the root counter wrap and a NaN row.

Measured on an MI355X (profiles/picard_summands_sweep.json, written when SCASML_SUMMANDS_SWEEP_JSON names a file): EVERY entry of check (a) is
bit-equal to its own launch's (share 1.0, largest ratio 0.0) in all 76 records -- the sweep, the 100 instantiations, near T, across the root counter
wrap and on quadrature n = 5's 3224 summands.  The allowance stays the asserted bound: the build keeps the compiler from contracting a product into
a sum (-ffp-contract=off), and a build that did not could round `u += y` and `ym += y` differently.  Check (f) reaches at most 0.228 of its bound
(full history n = 1, ACCUMULATE; 0.075 .. 0.21 elsewhere in the sweep, 0.074 .. 0.18 near T), with the bound at 6e-7 .. 4.5e-5 of se; the guard's
smallest median se64 / bound is 2.8e5 (quadrature n = 4, MLP mode), from the oracle alone 2.9e5.

What the module found.  picard_sum_kernel<quadrature, ACCUMULATE, 5, cubic equation> returned +NaN (0x7FC00000) in every z of a NaN root where the
plain, SE and SEZ kernels return -NaN (0xFFC00000): check (c), at every d of the table, in this one instance of the 100.  The sign of a NaN that an
operation produces or passes on is the compiler's choice, so no two kernels can promise each other's NaN bits; the tree kernels now store a NaN of
out_uz as the one pattern 0x7FC00000 (one_nan in csrc/picard_tree.hpp).
The sharded plain launch does not state a level summand's z for the full history at t = T (it returns 0 inf + z): those entries are held to an
exact 0 instead (test_summands_on_both_sides_of_the_read_back_switch).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_picard_stderr import MLP_TOL, SCASML_TOL, _groups
from test_gpu_picard_summands import _check_table
from test_gpu_picard_sweep import D_SWEEP, FLAG_D, G_ENDS, IDLE, NEAR_T_D, SIGMA, _G, _ids, _near_t_points, _points, _quad5, _ragged, _rpw
from test_gpu_stderr_sweep import (ACC, CASES, DEEP_QUAD, EPS, MLP, NAN_BITS, TABLE_EQ_MODES, TABLE_MAX_SUMMANDS, TOL, _Case, _same, _SeTree,
                                   _sweep_points, _sweep_tree, _table_par, se_stats)
from test_gpu_stderr_uz_sweep import K_LEVEL, K_TERMINAL, _z_is_nan_case, se_stats_z

gpu = pytest.mark.gpu

FILL_BITS = 0x7FC5F00D                    # a quiet NaN whose payload no operation of the kernels produces (the padding rows' NaN is NAN_BITS)
LDY_PAD = 3                               # ldy = B + 3: rows behind every summand that no launch may touch
SUMS = (1, 2)                             # SUM = 1: the summands of u (ncol = 1); 2: of (u, z) (ncol = 1 + d)
STRIDE_D = D_SWEEP                        # every ACCUMULATE case of the sweep also runs with site_stride > B
RANK_WORLDS = (2, 3)


def _rank_case(d):
    """Check (e)'s one case per d: the modes alternate along D_SWEEP and the two cases of a d every third d (ten different plans, two of them the
    ACCUMULATE quadrature (4, 4) whose every entry is NaN)."""
    i = D_SWEEP.index(d)
    mode = (MLP, ACC)[i % 2]
    return (mode,) + CASES[mode][d][(i // 3) % 2]


def _table_entries():
    return [(v, n, eq, mode) for eq, mode in TABLE_EQ_MODES for v in ("quad", "fh") for n in range(1, 6)]


def _counts(variant, n, par):
    return [N for N, _ in _groups(variant, n, par)[0]]


def test_the_summands_sweep_reaches_every_width_level_and_mode():
    assert set(CASES[MLP]) == set(CASES[ACC]) == set(D_SWEEP)
    for g, (lo, hi) in G_ENDS.items():                         # both ends of every G
        assert lo in D_SWEEP and hi in D_SWEEP and _G(lo) == _G(hi) == g
    for g, (lo, hi) in IDLE.items():                           # an idle-lane d for every G >= 16
        assert g >= 16 and any(lo <= d <= hi for d in D_SWEEP), g
    assert set(IDLE) == {g for g in G_ENDS if g >= 16}
    # put() stores a root's (u, z) row at out_y + local * (d + 1) without alignment: all four residues, and d mod 4 = 1 -- the last live lane stores
    # one float and the next root's u sits right behind it -- at three or more widths
    assert {d % 4 for d in D_SWEEP} == {0, 1, 2, 3}
    assert len({_G(d) for d in D_SWEEP if d % 4 == 1}) >= 3
    # every level of both variants in both modes, in the sweep itself but quadrature n = 5 (DEEP_QUAD in MLP mode, the table in ACCUMULATE)
    for mode in (MLP, ACC):
        reached = {(v, n) for cases in CASES[mode].values() for v, n, _ in cases}
        assert reached == {("quad", n) for n in range(1, 5)} | {("fh", n) for n in range(1, 6)}, mode
        for g in G_ENDS:
            ns = [n for d in D_SWEEP if _G(d) == g for _, n, _ in CASES[mode][d]]
            assert min(ns) <= 2 and max(ns) >= 3, (mode, g, ns)
    assert DEEP_QUAD[1] == ("quad", 5, 5) and DEEP_QUAD[0] in D_SWEEP and ("quad", 5, 0, ACC) in _table_entries()
    # check (a) launches once per summand: every sweep case stays under TABLE_MAX_SUMMANDS, quadrature n = 5 does not
    assert all(sum(_counts(*c)) <= TABLE_MAX_SUMMANDS for mode in (MLP, ACC) for cases in CASES[mode].values() for c in cases)
    assert sum(_counts(*DEEP_QUAD[1])) == 3224 > TABLE_MAX_SUMMANDS
    # ldy > B in every case of the sweep, site_stride > B in every ACCUMULATE case: both at every G
    assert LDY_PAD > 0 and {_G(d) for d in D_SWEEP} == {_G(d) for d in STRIDE_D} == set(G_ENDS)
    # check (e) meets both modes, both variants and every G
    picks = [_rank_case(d) for d in D_SWEEP]
    assert {p[0] for p in picks} == {MLP, ACC} and {p[1] for p in picks} == {"quad", "fh"} and all(p[1:] in CASES[p[0]][d] for p, d in zip(picks, D_SWEEP))
    assert {_G(d) for d, p in zip(D_SWEEP, picks)} == set(G_ENDS) == {_G(d) for d, p in zip(D_SWEEP, picks) if not _z_is_nan_case(*p[1:])}     # check (b) on a sum
    # the table: 2 variants x 5 levels x 5 (equation, mode) pairs x 2 SUM forms = the 100 instantiations of the four translation units, at one d per G
    assert len({e + (s,) for e in _table_entries() for s in SUMS}) == 100
    assert sorted(_G(d) for d in FLAG_D) == [4, 8, 16, 32, 64] and set(NEAR_T_D) <= set(D_SWEEP)
    for v in ("quad", "fh"):
        for n in range(1, 6):
            assert all(N >= 2 for N in _counts(v, n, _table_par(v, n)))
    # check (b)'s tolerances are those of tests/test_gpu_picard_summands.py
    assert TOL[MLP] == MLP_TOL and TOL[ACC] == SCASML_TOL
    assert FILL_BITS != NAN_BITS and np.isnan(np.array([FILL_BITS], dtype=np.uint32).view(np.float32)[0])


# ------------------------------------------------------------------------------------------------------------- launches
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _differ(a, b):
    """Where two float32 arrays of one shape differ in their bits: the first few (index, bits, bits), for an assertion's message."""
    a, b = _bits(a), _bits(b)
    return [(tuple(int(k) for k in i), "%08x" % a[tuple(i)], "%08x" % b[tuple(i)]) for i in np.argwhere(a != b)[:4]]


def _filled(shape):
    import torch
    return torch.full(shape, FILL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


class _Got:
    """One summand launch: out_uz (B, 1 + d), out_uhat (B,) or None, the table (S, B, ncol) float32, and the device buffer it sits in."""

    def __init__(self, uz, uhat, table, buf, ldy, ncol):
        self.uz, self.uhat, self.table, self.buf, self.ldy, self.ncol = uz, uhat, table, buf, ldy, ncol


class _SumCase(_Case):
    """_Case with the launch of scasml_picard_tree_summands, the closing kernel and the sharded plain launches' whole rows."""

    def __init__(self, *args, **kw):
        from scasml_gp_amd import _lib
        super().__init__(*args, **kw)
        self.counts = _counts(self.t.variant, self.n, self.par)
        self.S = int(_lib.load().scasml_plan_root_summands(C.byref(self.plan), None, None))
        assert self.S == sum(self.counts)

    def _rng(self, rank=0, world=1, owner=None):
        return self.t.rng(root0=self.root0, rank=rank, world=world, owner=owner)

    def plain(self, rank=0, world=1, owner=None):
        """scasml_picard_tree under the same sharding -> (out_uz, out_uhat or None)."""
        import torch
        out = torch.full((self.B, self.t.d + 1), -3.0, dtype=torch.float32, device="cuda")
        uh = torch.full((self.B,), -3.0, dtype=torch.float32, device="cuda") if self.t.mode == ACC else None
        self._call(False, self._rng(rank, world, owner), out, uh, None)
        torch.cuda.synchronize()
        return out.cpu().numpy(), None if uh is None else uh.cpu().numpy()

    def run_sum(self, form, ldy=0, rank=0, world=1, owner=None):
        """One launch of scasml_picard_tree_summands, with the guards of the module docstring asserted.  -> _Got."""
        import torch
        from scasml_gp_amd import _lib
        lib, t, B, S = _lib.load(), self.t, self.B, self.S
        ncol = 1 if form == 1 else t.d + 1
        rows = ldy or B
        what = (t.mode, t.variant, self.n, self.par, t.d, "B", B, "ldy", ldy, "ncol", ncol, "stride", self.stride, "world", world, rank)
        y = _filled((S + 1, rows, ncol))
        out = torch.full((B + 1, t.d + 1), -3.0, dtype=torch.float32, device="cuda")
        uh = torch.full((B + 1,), -3.0, dtype=torch.float32, device="cuda") if t.mode == ACC else None
        mode = _lib.MODE_ACCUMULATE if t.mode == ACC else _lib.MODE_MLP
        _lib.check(lib.scasml_picard_tree_summands(C.byref(t.prob), C.byref(self.plan), mode, _lib.ptr(self.x), B, self.stride, self._rng(rank, world, owner),
                                                   _lib.ptr(self.pts), _lib.ptr(self.vd), _lib.ptr(out), _lib.ptr(uh), _lib.ptr(y), ncol, ldy,
                                                   _lib.stream_ptr()), "picard_tree_summands")
        torch.cuda.synchronize()
        Y = y.cpu().numpy()
        b = Y.view(np.uint32)
        assert np.all(b[S] == FILL_BITS), (what, "the spare summand behind the table was written")
        assert np.all(b[:S, B:] == FILL_BITS), (what, "rows behind a summand's B roots were written", np.argwhere(b[:S, B:] != FILL_BITS)[:4].tolist())
        left = np.argwhere(b[:S, :B] == FILL_BITS)
        assert left.size == 0, (what, "entries (summand, root, column) left unwritten", left[:6].tolist())
        o = out.cpu().numpy()
        assert np.all(o[B:] == -3.0), (what, "out_uz was written past its B rows")
        u = None
        if uh is not None:
            u = uh.cpu().numpy()
            assert u[B] == -3.0, (what, "out_uhat was written past its B entries")
            u = u[:B]
        return _Got(o[:B], u, np.ascontiguousarray(Y[:S, :B]), y, ldy, ncol)

    def close(self, got):
        """scasml_picard_summands_stderr on the device buffer of a launch -> out_se (B, ncol) float32; the floats past B * ncol keep their fill."""
        import torch
        from scasml_gp_amd import _lib
        B, ncol = self.B, got.ncol
        se = _filled((B * ncol + 7,))
        _lib.check(_lib.load().scasml_picard_summands_stderr(C.byref(self.plan), _lib.ptr(got.buf), B, got.ldy, ncol, _lib.ptr(se), _lib.stream_ptr()),
                   "picard_summands_stderr")
        torch.cuda.synchronize()
        s = se.cpu().numpy()
        assert np.all(s.view(np.uint32)[B * ncol:] == FILL_BITS), ("out_se was written past its B * ncol floats", self.t.d, B, ncol, got.ldy)
        return s[:B * ncol].reshape(B, ncol)

    def summands_uz(self):
        """The device's own summands, all 1 + d columns: _Case.summands' launches, whose z columns that method drops.  -> (S, B, 1 + d) float32."""
        import torch
        groups, units = _groups(self.t.variant, self.n, self.par)
        rows = [mine for _, summ in groups for mine in summ]
        assert len(rows) == self.S
        own = np.ones((len(rows), units), dtype=np.uint8)
        for i, mine in enumerate(rows):
            own[i, mine] = 0
        owner = torch.from_numpy(own).cuda()
        out = torch.full((len(rows), self.B, self.t.d + 1), -3.0, dtype=torch.float32, device="cuda")
        for i in range(len(rows)):
            self._call(False, self.rng(owner=owner[i].data_ptr()), out[i], None, None)
        torch.cuda.synchronize()
        return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- the checks
MEASURED = {}                  # "(variant) n=(n) (mode or edge)" -> a: largest check (a) ratio; equal: smallest share of bit-equal entries;
                               # f: largest check (f) ratio; guard: smallest median se64 / bound (f)
_ORACLE = {}                   # (mode, d, variant, n, par) -> the oracle's summands at the largest batch, (S, B, 1 + d) float64; shared, never modified


def _record(key, **kw):
    m = MEASURED.setdefault("%s n=%d %s" % key, {})
    for k, v in kw.items():
        m[k] = min(m.get(k, float("inf")), float(v)) if k in ("equal", "guard") else max(m.get(k, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    """SCASML_SUMMANDS_SWEEP_JSON=path: write what the checks measured (profiles/picard_summands_sweep.json is such a file)."""
    yield
    path = os.environ.get("SCASML_SUMMANDS_SWEEP_JSON")
    if path and MEASURED:
        doc = dict(k_terminal=K_TERMINAL, k_level=K_LEVEL, ldy_pad=LDY_PAD, checks={k: MEASURED[k] for k in sorted(MEASURED)})
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


def _oracle_table(mode, d, variant, n, par):
    key = (mode, d, variant, n, par)
    if key not in _ORACLE:
        assert not _z_is_nan_case(variant, n, par), "the oracle walks these trees in 7 s and more: consulted at one d and one root"
        _ORACLE[key] = _walk(_sweep_tree(d, variant, mode), n, par, _sweep_points(d))
    return _ORACLE[key]


def _walk(t, n, par, xt, root0=0):
    from oracle.mlp import PicardOracle
    Y = PicardOracle(t.oeq, t.variant, gp=t.sur, seed=t.seed, stream=t.stream).root_summands(n, par, xt, root0=root0, with_z=True)
    table = np.concatenate(Y, axis=0)
    table.setflags(write=False)
    return table


def _split(table, counts):
    """(S, B, ncol) -> [Y_g, Y_0, ...] float64 (N_j, B, ncol)."""
    table = np.asarray(table, dtype=np.float64)
    at = np.concatenate([[0], np.cumsum(counts)])
    assert at[-1] == table.shape[0]
    return [table[at[j]:at[j + 1]] for j in range(len(counts))]


def check_a(table, ref, counts, what, key=None, skip=None):
    """table (S, B, ncol) float32 of the summand kernel against ref (S, B, 1 + d) float32 of the sharded plain launches.  skip: entries (a mask of
    ref's shape) at which the launch does not state the summand; the caller holds them to something stronger."""
    ref = ref[:, :, :table.shape[2]]
    if skip is not None:
        table, ref = np.where(skip[:, :, :table.shape[2]], np.float32(0), table), np.where(skip[:, :, :table.shape[2]], np.float32(0), ref)
    assert table.shape == ref.shape and table.dtype == ref.dtype == np.float32, (what, table.shape, ref.shape)
    k = np.full(ref.shape, K_LEVEL)
    k[:counts[0], :, 1:] = K_TERMINAL
    t64, r64 = table.astype(np.float64), ref.astype(np.float64)
    fin = np.isfinite(r64)
    assert not np.any(np.isfinite(t64[~fin])), (what, "a finite entry where the summand's own launch is not finite", np.argwhere(np.isfinite(t64) & ~fin)[:4].tolist())
    assert np.all(np.isfinite(t64[fin])), (what, "an entry that is not finite where the summand's own launch is", np.argwhere(~np.isfinite(t64) & fin)[:4].tolist())
    zero = fin & (r64 == 0)
    assert np.all(t64[zero] == 0.0), (what, "an entry that is not 0 where the summand's own launch is", np.argwhere(zero & (t64 != 0))[:4].tolist())
    same = (_bits(table) == _bits(ref)) | (zero & (t64 == 0)) | (~fin & np.isnan(t64) & np.isnan(r64))
    ok = fin & ~zero
    ratio = np.zeros(ref.shape)
    with np.errstate(invalid="ignore"):                    # inf - inf outside `ok`
        ratio[ok] = np.abs(t64 - r64)[ok] / (k[ok] * EPS * np.abs(r64[ok]))
    print("check (a) %s: %d x %d x %d, %.4f bit-equal, max |diff| / (k 2^-24 |Y|) %.4f" % ((what,) + ref.shape + (same.mean(), ratio.max())))
    if key:
        _record(key, a=ratio.max(), equal=same.mean())
    assert np.all(ratio <= 1.0), (what, ratio.max(), np.argwhere(ratio > 1.0)[:6].tolist())


def check_b(table, want, mode, what):
    """The (u, z) table against the oracle's summands for the same roots, under _check_table's bound."""
    _check_table(table, want, TOL[mode], what)


def bound_f(st):
    with np.errstate(invalid="ignore", over="ignore"):
        var, se, bv = st["var"], st["se"], st["b_var"]
        return np.maximum(np.sqrt(var + bv) - se, se - np.sqrt(np.maximum(var - bv, 0.0)))


def _stats(table, counts):
    Ys = _split(table, counts)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return se_stats_z(Ys) if table.shape[2] > 1 else se_stats(Ys)


def check_f(se, table, counts, what, guard=True, key=None):
    """se (B, ncol) float32 of the closing kernel against float64 arithmetic on the table it was given."""
    st = _stats(table, counts)
    se, se64, bound = se.astype(np.float64), st["se"], bound_f(st)
    assert se.shape == se64.shape, (what, se.shape, se64.shape)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(se64)
    assert not np.any(np.isfinite(se[~fin])), (what, "a finite se where float64 on the same table has none")
    assert np.all(np.isfinite(se[fin])), (what, "se is not finite where float64 on the same table is")
    zero = fin & (se64 == 0)
    assert np.all(se[zero] == 0.0), (what, "se64 = 0 but the kernel's se is not")
    ok = fin & ~zero
    if not ok.any():
        return
    dev, b, ref = np.abs(se - se64)[ok], bound[ok], se64[ok]
    g = float(np.median(ref / b))
    print("check (f) %s: max |se - se64| %.3e, max / bound %.4f, bound / se %.2e..%.2e, median se / bound %.0f" % (what, dev.max(), (dev / b).max(), (b / ref).min(),
                                                                                                                (b / ref).max(), g))
    if key:
        _record(key, f=(dev / b).max())
    if guard:
        if key:
            _record(key, guard=g)
        assert g >= 10.0, (what, "guard: the median se64 is %.1f x its bound" % g)
    assert np.all(dev <= b), (what, dev.max(), (dev / b).max(), np.argwhere(ok & (np.abs(se - se64) > bound))[:4].tolist())


def check_c(got, plain, what):
    """got: {SUM form: _Got} of one case; plain: (out_uz, out_uhat or None) of scasml_picard_tree with the same arguments."""
    for form, g in got.items():
        assert _same(g.uz, plain[0]), (what, form, "out_uz differs from the plain launch", _differ(g.uz, plain[0]))
        if plain[1] is not None:
            assert _same(g.uhat, plain[1]), (what, form, "out_uhat differs from the plain launch", _differ(g.uhat, plain[1]))
    if 1 in got and 2 in got:
        assert _same(got[1].table, got[2].table[:, :, :1]), (what, "the SUM = 1 table differs from column 0 of the SUM = 2 table",
                                                             _differ(got[1].table, got[2].table[:, :, :1]))


def _both(c, what, ldy=0):
    """Both SUM forms of one case, checked (c).  -> {1: _Got, 2: _Got}."""
    got = {form: c.run_sum(form, ldy=ldy) for form in SUMS}
    check_c(got, c.plain(), what)
    return got


def _a_and_c(c, what, key=None, ldy=0, skip=None):
    """Checks (a) and (c) of one case in both SUM forms.  skip(ref) -> check_a's mask.  -> ({form: _Got}, the device's own summands)."""
    got = _both(c, what, ldy=ldy)
    ref = c.summands_uz()
    for form in SUMS:
        check_a(got[form].table, ref, c.counts, what + ("SUM", form), key=key, skip=None if skip is None else skip(ref))
    return got, ref


@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_summands_at_every_width_level_and_mode(d):
    """Checks (a), (b), (c), (d) and (f) of the module docstring at ragged batches; the roots of every batch are a prefix of the largest one."""
    Bs = _ragged(d)
    xt = _sweep_points(d)
    nan = np.frombuffer(np.uint32(NAN_BITS).tobytes(), dtype=np.float32)[0]
    for mode in (MLP, ACC):
        for variant, n, par in CASES[mode][d]:
            key, what = (variant, n, mode), (mode, variant, n, par, d)
            t = _sweep_tree(d, variant, mode)
            full = None
            for B in reversed(Bs):
                c = _SumCase(t, n, par, xt[:B])
                wide = _both(c, what + (B, "ldy = B + 3"), ldy=B + LDY_PAD)
                got = _both(c, what + (B,))
                for form in SUMS:                                                                      # (d): ldy
                    assert _same(wide[form].table, got[form].table), (what, B, form, "a root's entries depend on ldy")
                if full is None:
                    full = got
                    ref = c.summands_uz()
                    for form in SUMS:
                        check_a(got[form].table, ref, c.counts, what + (B, "SUM", form), key=key)
                    if not _z_is_nan_case(variant, n, par):
                        check_b(got[2].table, _oracle_table(mode, d, variant, n, par), mode, what + (B,))
                    for form in SUMS:
                        for g in (got[form], wide[form]):
                            check_f(c.close(g), g.table, c.counts, what + (B, "ncol", g.ncol, "ldy", g.ldy), key=key)
                    if mode == ACC:             # (d): a site stride past the batch, NaN in every padding row
                        assert d in STRIDE_D
                        S = (B + 31) // 32 * 32 + 32
                        p = _SumCase(t, n, par, xt[:B], stride=S, pad=nan)
                        padded = _both(p, what + (B, "site_stride", S), ldy=B + LDY_PAD)
                        for form in SUMS:
                            assert _same(padded[form].table, got[form].table) and _same(padded[form].uz, got[form].uz), (what, "site_stride", S, form)
                            assert _same(padded[form].uhat, got[form].uhat), (what, "site_stride", S, form)
                else:
                    for form in SUMS:                                                                  # (d): prefix batches
                        assert _same(got[form].table, full[form].table[:, :B]), (what, B, form, "a root's entries depend on the batch")


@gpu
def test_quadrature_level_four_table_against_the_oracle_on_one_root():
    """Check (b)'s expectation for quadrature n = 4 at one d and one root: MLP mode (4, 4) at d = 13 has a finite u and no finite z in the oracle
    too (the q = 5 rule's nodes are not increasing: SURVEY.md Appendix B)."""
    d, (variant, n, par) = 13, ("quad", 4, 4)
    assert (variant, n, par) in CASES[MLP][d]
    xt = _sweep_points(d)[:1]
    t = _sweep_tree(d, variant, MLP)
    want = _walk(t, n, par, xt)
    assert np.all(np.isfinite(want[:, :, 0])) and not np.all(np.isfinite(want[:, :, 1:]))
    c = _SumCase(t, n, par, xt)
    got, _ = _a_and_c(c, ("quad (4, 4), one root",))
    check_b(got[2].table, want, MLP, "quad (4, 4), one root")


@gpu
def test_quadrature_level_five_on_one_root():
    """Checks (a), (c), (f) and the guards on tests/golden/oracle_quad5_d13.npz's root: 3224 summands, one launch each.  The root's u is NaN in the
    fixture: the column of u's summands holds a NaN, and the standard errors are not finite."""
    d, (variant, n, par) = DEEP_QUAD
    c = _SumCase(_SeTree(0, d, variant, MLP), n, par, _quad5()["x_t"])
    got, _ = _a_and_c(c, ("quad n=5",), key=(variant, n, MLP), ldy=c.B + LDY_PAD)
    with np.errstate(invalid="ignore"):
        total = got[2].table.astype(np.float64).sum(axis=0)
    assert np.array_equal(np.isnan(total), np.isnan(_quad5()["uz"]))
    for form in SUMS:
        check_f(c.close(got[form]), got[form].table, c.counts, ("quad n=5", form), guard=False)


def test_the_closing_kernels_bound_is_far_below_the_standard_errors():
    """Check (f)'s guard from the oracle alone (no GPU): with se64 and the bound formed from the oracle's summands of a sweep case, the median
    se64 / bound over the finite columns is at least 10 -- for every (variant, n, mode) with a finite z, at its first d of the sweep."""
    for mode in (MLP, ACC):
        seen = set()
        for d in D_SWEEP:
            for variant, n, par in CASES[mode][d]:
                if (variant, n) in seen or _z_is_nan_case(variant, n, par):
                    continue
                seen.add((variant, n))
                st = _stats(_oracle_table(mode, d, variant, n, par), _counts(variant, n, par))
                se, b = st["se"], bound_f(st)
                ok = np.isfinite(se) & (se > 0)
                g = float(np.median(se[ok] / b[ok]))
                print("guard (f) %s %s n=%d d=%d: median se64 / bound %.0f" % (mode, variant, n, d, g))
                assert ok.all() and g >= 10.0, (mode, variant, n, d, g)
        assert seen == {("quad", 1), ("quad", 2), ("quad", 3)} | {("fh", n) for n in range(1, 6)}, mode


# ------------------------------------------------------------------------------------------------------------- the ranks' tables
@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_rank_tables_add_up(d):
    """Check (e) at one case per d, the largest ragged batch, ldy = B + 3."""
    import torch
    mode, variant, n, par = _rank_case(d)
    what = (mode, variant, n, par, d)
    B = _ragged(d)[-1]
    t = _sweep_tree(d, variant, mode)
    c = _SumCase(t, n, par, _sweep_points(d)[:B])
    one = c.run_sum(2).table
    for world in RANK_WORLDS:                        # owner = NULL: unit % world
        parts = []
        for r in range(world):
            g = c.run_sum(2, ldy=B + LDY_PAD, rank=r, world=world)          # asserts that every entry is written
            plain = c.plain(rank=r, world=world)
            assert _same(g.uz, plain[0]) and (plain[1] is None or _same(g.uhat, plain[1])), (what, world, r, "the partial (u, z) differs from the plain launch")
            parts.append(g.table)
        with np.errstate(invalid="ignore", over="ignore"):
            acc = parts[0].copy()
            for p in parts[1:]:
                acc = (acc + p).astype(np.float32)
            exact = sum(p.astype(np.float64) for p in parts)
            room = (world - 1) * EPS * sum(np.abs(p.astype(np.float64)) for p in parts)
        fin = np.isfinite(exact)
        assert np.array_equal(np.isfinite(acc), fin) and np.array_equal(fin, np.isfinite(one)), (what, world, "the summed table is finite exactly where the one-rank table is")
        assert np.all(np.abs(acc.astype(np.float64) - exact)[fin] <= room[fin]), (what, world)
        if not _z_is_nan_case(variant, n, par):
            check_b(acc, _oracle_table(mode, d, variant, n, par), mode, what + ("world %d" % world,))
    # every summand whole on one rank
    groups, units = _groups(variant, n, par)
    per = [len(mine) for _, summ in groups for mine in summ]
    assert sum(per) == units and len(per) == c.S
    rank_of = np.arange(c.S) % 2
    owner = torch.from_numpy(np.repeat(rank_of, per).astype(np.uint8)).cuda()
    for r in range(2):
        tab = c.run_sum(2, ldy=B + LDY_PAD, rank=r, world=2, owner=owner.data_ptr()).table
        assert np.all(tab[rank_of != r] == 0.0), (what, r, "a rank that owns nothing of a summand holds something there")
        assert _same(tab[rank_of == r], one[rank_of == r]), (what, r, "a summand whole on one rank differs from the one-rank table")
        tab_u = c.run_sum(1, rank=r, world=2, owner=owner.data_ptr()).table
        assert _same(tab_u, tab[:, :, :1]), (what, r, "the SUM = 1 table differs from column 0 of the SUM = 2 table")


# ------------------------------------------------------------------------------------------------------------- the whole instantiation table
@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_every_summand_instantiation_against_its_own_summands(d):
    """Each of the 100 picard_sum_kernel instances (both variants, n = 1..5, equations 0 and 1 in MLP mode and ACCUMULATE, equation 2 in MLP mode,
    SUM = 1 and 2) at one d per G, B = roots-per-wave + 1, ldy = B + 3: check (c) and the guards; check (a) where the plan has at most
    TABLE_MAX_SUMMANDS summands (quadrature n = 5 apart: test_quadrature_level_five_on_one_root)."""
    B = _rpw(d) + 1
    xt = _points(d, B, seed=1000 + d)
    for variant, n, eq_id, mode in _table_entries():
        par = _table_par(variant, n)
        what = ("table", eq_id, mode, variant, n, par, d)
        t = _SeTree(eq_id, d, variant, mode)
        # quadrature n = 5 walks 113 745 sites per root: two roots, and in ACCUMULATE (whose surrogate values come from the CPU) one
        rows = xt if not (variant == "quad" and n == 5) else xt[:1 if mode == ACC else 2]
        c = _SumCase(t, n, par, rows)
        if c.S <= TABLE_MAX_SUMMANDS:
            _a_and_c(c, what, key=(variant, n, "%s equation %d, table" % (mode, eq_id)), ldy=c.B + LDY_PAD)
        else:
            _both(c, what, ldy=c.B + LDY_PAD)


# ------------------------------------------------------------------------------------------------------------- edges
@gpu
@pytest.mark.parametrize("d", NEAR_T_D, ids=_ids(NEAR_T_D))
def test_summands_on_both_sides_of_the_read_back_switch(d):
    """Roots at T - t = 0, one ulp, 1e-5, 1e-4, just below and above (kReadbackMinVol / sigma)^2 and 1e-2, both modes (amp = 0.3 in ACCUMULATE):
    checks (a), (c) and (f).  At t = T every terminal entry of u is the same float (every sample is the root itself) and every level entry, of u
    and of z, exactly 0: every path's weight is T - t, the steps 1 / (0 + 1e-6) of the z addends are finite, and the full history's children at
    t = T, whose z divides by T - t = 0, are clipped before f sees them.  The full history's own launch of a level summand does not state its z at
    t = T: a plain launch returns sz zs + (the paths' z) with zs = 1 / (mg 0) = inf and sz = 0 where the rank owns no terminal sample, NaN whatever the
    path added.  Check (a) leaves those entries (a level summand's z columns of the root at t = T, full history) to the exact 0 asserted here."""
    xt = _near_t_points(d, seed=500 + d)
    taus = np.float64(0.5) - xt[:, d].astype(np.float64)
    assert taus[0] == 0 and np.all(SIGMA * np.sqrt(taus[:5]) < 1e-2) and np.all(SIGMA * np.sqrt(taus[5:]) > 1e-2)
    for mode in (MLP, ACC):
        for variant, n, par in (("quad", 2, 3), ("quad", 3, 3), ("fh", 2, 3), ("fh", 3, 2)):
            what = (mode, variant, n, "near T", d)
            c = _SumCase(_SeTree(0, d, variant, mode, amp=0.3), n, par, xt)
            mg = c.counts[0]

            def at_T(ref):
                skip = np.zeros(ref.shape, dtype=bool)
                if variant == "fh":
                    assert not np.any(np.isfinite(ref[mg:, 0, 1:])), (what, "the full history's own launches at t = T")
                    skip[mg:, 0, 1:] = True
                return skip
            got, _ = _a_and_c(c, what, key=(variant, n, mode + " near T"), ldy=c.B + LDY_PAD, skip=at_T)
            tab = got[2].table
            assert np.all(_bits(tab[:mg, 0, 0]) == _bits(tab[0, 0, 0])) and np.isfinite(tab[0, 0, 0]), (what, "terminal entries of u at t = T", tab[:mg, 0, 0])
            assert np.all(tab[mg:, 0, 0] == 0.0), (what, "level entries of u at t = T", tab[mg:, 0, 0])
            assert np.all(tab[mg:, 0, :] == 0.0), (what, "level entries of z at t = T", tab[mg:, 0, :])
            for form in SUMS:
                se = c.close(got[form])
                check_f(se, got[form].table, c.counts, what + ("ncol", got[form].ncol), guard=False, key=(variant, n, mode + " near T"))
                assert se[0, 0] == 0.0, (what, "se_u at t = T", se[0, 0])


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_summands_root_counter_wraps(d):
    """root0 = 2^32 - 3, B = 8: checks (a) and (c) across the wrap; local root i >= 3 is root i - 3 of a launch that starts at 0."""
    root0, B = (1 << 32) - 3, 8
    xt = _points(d, B, seed=800 + d)
    for mode in (MLP, ACC):
        for variant, n, par in (("quad", 2, 3), ("fh", 3, 2)):
            t = _SeTree(0, d, variant, mode)
            c = _SumCase(t, n, par, xt, root0=root0)
            got, _ = _a_and_c(c, (mode, variant, "wrap", d), key=(variant, n, mode + " root counter wrap"), ldy=B + LDY_PAD)
            low = _both(_SumCase(t, n, par, xt[3:]), (mode, variant, "wrapped roots", d))
            for form in SUMS:
                assert _same(got[form].table[:, 3:], low[form].table) and _same(got[form].uz[3:], low[form].uz), (mode, variant, form, "wrapped roots")


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_a_nan_row_is_nan_in_its_own_entries_and_disturbs_no_other_root(d):
    """MLP mode, one coordinate of one row in the middle of a wave is NaN: every terminal entry of that root is NaN, its other entries are what their
    own launches say (check (a): the l = 0 paths of MLP mode add f(0, 0) = 0 whatever the point is), no other root holds a NaN and every other root
    keeps the bits of the launch without it."""
    B = 4 * _rpw(d) + 1
    xt = _points(d, B, seed=1100 + d)
    bad = xt.copy()
    r = _rpw(d) // 2 if _rpw(d) > 1 else 1            # G = 64: one root per wave, the second wave's
    bad[r, d // 2] = np.nan
    others = np.arange(B) != r
    for variant, n, par in (("quad", 3, 3), ("fh", 4, 2)):
        t = _SeTree(0, d, variant, MLP)
        ok = _SumCase(t, n, par, xt)
        clean = _both(ok, (variant, "clean", d), ldy=B + LDY_PAD)
        c = _SumCase(t, n, par, bad)
        got, _ = _a_and_c(c, (variant, "NaN row", d), ldy=B + LDY_PAD)
        for form in SUMS:
            tab = got[form].table
            assert np.all(np.isnan(tab[:c.counts[0], r, :])), (variant, form, "terminal entries of the NaN root")
            assert np.all(np.isnan(tab[:, r, :]) | (tab[:, r, :] == 0.0)), (variant, form, "an entry of the NaN root that is neither NaN nor an exact 0")
            assert np.all(np.isfinite(tab[:, others, :])), (variant, form, "a NaN outside the NaN root")
            assert _same(tab[:, others, :], clean[form].table[:, others, :]) and _same(got[form].uz[others], clean[form].uz[others]), (variant, form)
            se = c.close(got[form])
            assert np.all(np.isnan(se[r])) and np.all(np.isfinite(se[others])), (variant, form, se[r])
            assert _same(se[others], ok.close(clean[form])[others]), (variant, form, "se of the other roots")
