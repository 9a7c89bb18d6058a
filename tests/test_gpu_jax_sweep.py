"""The Picard tree kernel on the reference's own random stream -- picard_tree_kernel<VAR, MODE, N, EQ, JAX = true>, csrc/picard_tree_jax.hip
(levels 1..3) and csrc/picard_tree_jax_deep.hip (levels 4, 5) -- at every lane-group width, level and mode, called through ctypes.

tests/test_gpu_picard_sweep.py takes the same walk through every width on the Philox stream; what SCASML_RNG_JAX_STREAM changes is where a
normal comes from: Walker::normals_jax reads jax.random.normal(float16) by counter, at (row * width + m) * d + 4 gl + c under the key of the
call's slot, where row is the root's row in the reference's flattened batch (root0 + local at the root call, row * mc + m one call down, 64
bits wide).  The stride of that index is d, not the padded row length, so for odd d a row's first element changes alignment from row to
row and the lane that holds the last live dims is partly masked.  The sweep (D_SWEEP of the Philox sweep: both ends of every G, idle
lanes, every d mod 4) checks, against oracle/mlp.py with jax_stream=True on the same keys (a fresh oracle per case: the initial key state):

* SCASML_MODE_MLP, both variants, levels 1..5, ragged batches, equations 0 and 1; equation 2 and a missing key table are refused;
* GENERATE + ACCUMULATE around the closed-form surrogate, site stride > B with NaN padding, and the emitted rows against the points the
  oracle hands its surrogate;
* the normals themselves, recovered from GENERATE's rows and compared with oracle/jax_random.py at the index above: equal, so that an
  addressing error is named instead of showing up as an O(1) difference downstream;
* COMPAT_F16 on top, root0 (chunks of a batch bitwise, and a draw index past 2^32), and sample sharding with a dealt owner table.

Bounds: the normals are exact float16 values on both sides and the arithmetic is the Philox kernel's, so they are the Philox sweep's --
ATOL, RTOL in MLP mode (tests/test_gpu_mlp.py), ATOL_RB, RTOL_RB with _atol_rb where points are read back (tests/test_gpu_configs.py),
_close16 under the float16 casts (tests/test_gpu_compat.py).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_picard_sweep import (ATOL, ATOL_RB, D_SWEEP, FLAG_D, G_ENDS, IDLE, RTOL, RTOL_RB, _atol_rb, _close, _close16, _F4, _G, _ids, _is16,
                                   _kp, _points, _Q3, _ragged, _rpw, _Surrogate, _Tree)

gpu = pytest.mark.gpu

# per d: the (variant, n, par) of MLP mode and of GENERATE + ACCUMULATE, dealt round the sweep as MLP_CASES / ACC_CASES are (shifted, so that
# a d does not meet the level it meets on the Philox stream).  The oracle's cost is the tree's (test_gpu_picard_sweep.py): the deeper
# levels sit on small d.  Quadrature n = 5 (DEEP_QUAD) is NaN in every component whatever the stream: MLP mode and ACCUMULATE are only
# executed there, GENERATE's rows are checked through the normals recovered from them (DEEP_NORMALS).
JAX_MLP_CASES = {d: [("quad",) + _Q3[(i + 2) % 3], ("fh",) + _F4[(i + 1) % 4]] for i, d in enumerate(D_SWEEP)}
JAX_MLP_CASES[6].append(("quad", 4, 4))
JAX_MLP_CASES[13].append(("fh", 5, 2))
JAX_MLP_CASES[139].append(("fh", 4, 2))
JAX_ACC_CASES = {d: [("quad",) + _Q3[i % 3], ("fh",) + _F4[(i + 3) % 4]] for i, d in enumerate(D_SWEEP)}
JAX_ACC_CASES[12].append(("quad", 4, 4))
JAX_ACC_CASES[29].append(("fh", 5, 2))
JAX_ACC_CASES[125].append(("fh", 4, 2))
DEEP_QUAD = (13, ("quad", 5, 5))
EQ1_CASES = (("quad", 2, 2), ("fh", 2, 3))          # equation 1 in MLP mode, at every d
# the translation unit a level is compiled in
UNIT_OF_LEVEL = {1: "picard_tree_jax.hip", 2: "picard_tree_jax.hip", 3: "picard_tree_jax.hip", 4: "picard_tree_jax_deep.hip", 5: "picard_tree_jax_deep.hip"}


def test_the_sweep_reaches_every_width_and_every_instantiation():
    """The lists above against the library's own point stride: both ends of every G, an idle-lane d of each G >= 16, all residues of d mod 4
    (odd d among the flag cases too), every (variant, level) of both translation units in MLP mode and in GENERATE + ACCUMULATE, levels 3
    and 4 (either side of the split between the two files) in both variants and modes, and equation 1."""
    from scasml_gp_amd import _lib
    lib = _lib.load()
    stride = lambda d: int(lib.scasml_point_stride(d))
    G = lambda d: 1 << max(0, (stride(d) // 4 - 1).bit_length())
    assert all(_kp(d) == stride(d) and _G(d) == G(d) for d in range(1, _lib.MAX_DIM + 1))
    for g, (lo, hi) in G_ENDS.items():
        assert G(lo) == G(hi) == g and (lo == 1 or G(lo - 1) == g // 2) and (hi == _lib.MAX_DIM or G(hi + 1) == 2 * g)
        for cases in (JAX_MLP_CASES, JAX_ACC_CASES):
            assert lo in cases and hi in cases, g
    for g, (lo, hi) in IDLE.items():
        assert G(lo) == g and stride(lo) // 4 < g and {stride(d) for d in range(lo, hi + 1)} == {stride(lo)}
        for cases in (JAX_MLP_CASES, JAX_ACC_CASES):
            assert any(lo <= d <= hi for d in cases), g
        assert any(lo <= d <= hi for d in FLAG_D), g
    assert set(JAX_MLP_CASES) == set(JAX_ACC_CASES) == set(D_SWEEP)
    assert {d % 4 for d in JAX_MLP_CASES} == {d % 4 for d in JAX_ACC_CASES} == {0, 1, 2, 3}
    assert sorted(G(d) for d in FLAG_D) == [4, 8, 16, 32, 64] and {1, 3} & {d % 4 for d in FLAG_D} and any(d % 2 for d in FLAG_D)
    every = {(v, n) for v in ("quad", "fh") for n in range(1, _lib.MAX_LEVEL + 1)}
    for cases in (JAX_MLP_CASES, JAX_ACC_CASES):
        got = {(v, n) for c in cases.values() for v, n, _ in c} | {DEEP_QUAD[1][:2]}
        assert got == every
        assert {UNIT_OF_LEVEL[n] for _, n in got} == set(UNIT_OF_LEVEL.values())
        for v in ("quad", "fh"):
            assert (v, 3) in got and (v, 4) in got
        assert all(n <= par for c in cases.values() for v, n, par in c if v == "quad")
    # (quad, 5) is reached by execution only in MLP mode and ACCUMULATE (all NaN); its GENERATE rows are checked through DEEP_NORMALS
    assert DEEP_QUAD[0] in D_SWEEP and DEEP_QUAD[1][1] == _lib.MAX_LEVEL and (DEEP_QUAD[0],) + DEEP_QUAD[1] == DEEP_NORMALS[0][:4]
    assert {(v, n) for _, v, n, _, _ in DEEP_NORMALS} == {(v, n) for v in ("quad", "fh") for n in (4, 5)}
    assert set(FLAG_D) <= set(NORMALS_D) and any(d % 4 == 1 and G(d) >= 8 for d in NORMALS_D)
    assert {v for v, _, _ in EQ1_CASES} == {"quad", "fh"} and _lib.EQ_CUBIC_REACTION_DIFFUSION == 1
    assert all(1 in _ragged(d) and 4 * _rpw(d) + 1 in _ragged(d) for d in D_SWEEP)


# ------------------------------------------------------------------------------------------------------------- MLP mode
@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_mlp_mode_on_the_reference_stream_at_every_width_and_level(d):
    """Without COMPAT_F16: float32 arithmetic on exact float16 normals against float64 arithmetic on the same normals -- the Philox sweep's
    bound, NaN exactly where the oracle has NaN.  Each launch compares with a prefix of the one oracle batch."""
    Bs = _ragged(d)
    xt = _points(d, Bs[-1], seed=1100 + d)
    for variant, n, par in JAX_MLP_CASES[d]:
        t = _Tree(0, d, variant)
        want = t.oracle(n, par, xt, jax_stream=True)
        for B in Bs:
            _close(t.mlp(n, par, xt[:B], t.rng(jax=(n, par))), want[:B], ATOL, RTOL, (variant, n, par, B))


@gpu
def test_quadrature_level_five_is_executed_on_the_reference_stream():
    """Quadrature n = rho = 5 (the deepest quadrature instantiations of picard_tree_jax_deep.hip) on one root, MLP mode and ACCUMULATE: EXECUTED,
    not checked against values.  Every component of every root is NaN at this level whatever the random stream -- a level >= 4 call meets
    q = 5, whose tabulated nodes are not increasing (tests/golden/oracle_quad5_d13.npz is all NaN for the same reason)
    -- so all that can be asserted of `out` is that NaN is what arrives.  No wrong key slot, row or stride can fail this test; what is
    finite at this level, the rows GENERATE emits, is checked by test_normals_of_inner_calls_at_the_deep_levels."""
    d, (variant, n, par) = DEEP_QUAD
    xt = _points(d, 1, seed=1150)
    t = _Tree(0, d, variant)
    assert np.isnan(t.mlp(n, par, xt, t.rng(jax=(n, par)))).all()
    t = _Tree(0, d, variant, surrogate=True)
    got, uh, P, vals = t.scasml(n, par, xt, t.rng(jax=(n, par)))
    assert np.isnan(got).all() and np.array_equal(P[-1, :, :d + 1], xt.astype(np.float32)) and np.isfinite(uh).all()


@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_equation_one_on_the_reference_stream_and_the_refusals(d):
    """Equation 1 in MLP mode; equation 2 (f of |z|^2: Philox only) is refused in every mode with the flag set, and a flag without its key
    table is refused; the output buffers keep their sentinel."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    B = _rpw(d) + 1
    xt = _points(d, B, seed=1200 + d)
    for variant, n, par in EQ1_CASES:
        t = _Tree(1, d, variant)
        _close(t.mlp(n, par, xt, t.rng(jax=(n, par))), t.oracle(n, par, xt, jax_stream=True), ATOL, RTOL, (1, variant))
    t = _Tree(0, d, "quad", surrogate=True)
    plan = t.plan(2, 2)
    ppr = int(lib.scasml_points_per_root(C.byref(plan)))
    x = torch.from_numpy(xt).cuda()
    pts = torch.full((ppr * B, t.kp), 5.0, device="cuda")
    vals = torch.zeros((ppr * B, 4), device="cuda")
    out = torch.full((B, d + 1), 5.0, device="cuda")
    eq2 = _lib.Problem(t.prob.d, _lib.EQ_QUADRATIC_GRADIENT_REACTION_DIFFUSION, t.prob.T, t.prob.mu, t.prob.sigma, t.prob.clip)
    rng = t.rng(jax=(2, 2))
    for mode, kw in ((_lib.MODE_MLP, dict(out=out)), (_lib.MODE_GENERATE, dict(pts=pts)), (_lib.MODE_ACCUMULATE, dict(pts=pts, vals=vals, out=out))):
        assert t.launch(mode, plan, x, B, 0, rng, prob=eq2, **kw) == -2
        assert b"Philox stream only" in lib.scasml_last_error()
        nokeys = _lib.Rng(t.seed, t.stream, 0, 0, 1, _lib.RNG_JAX_STREAM, 0, None, None)
        assert t.launch(mode, plan, x, B, 0, nokeys, **kw) == -1
        assert b"jax_keys" in lib.scasml_last_error()
    assert bool((pts == 5.0).all()) and bool((out == 5.0).all())


# ------------------------------------------------------------------------------------------------------------- GENERATE + ACCUMULATE
class _Recorder(_Surrogate):
    """_Surrogate that keeps every batch of points the oracle asks u_hat at (terminal points in _g, nodes in _f)."""

    def __init__(self, d, amp=1e-3):
        super().__init__(d, amp)
        self.seen = None

    def predict(self, P):
        if self.seen is not None:
            self.seen.append(np.array(P, dtype=np.float64))
        return super().predict(P)


# an emitted coordinate is x plus at most 15 increments mu dt + sigma sqrt(dt) N of magnitude <= 1 -- quadrature n <= 3: three levels of
# q <= 5 steps; full history at any level n <= 5: one increment per level -- each a float32 fma on an O(1) running sum (half an ulp of 2:
# 1.2e-7) with sqrt_fast and the float32 tables adding about as much again.  (Quadrature n = 4 is NaN: its rows are not compared.)
ROW_ATOL = 15 * 2 * 1.2e-7 + 1e-6


def _rows_match_the_oracles_points(rows, seen, what):
    """rows (sites, d + 1): one root's emitted rows, the root row excluded; seen (calls, d + 1): the points the oracle evaluated its
    surrogate at for that root.  Each set within ROW_ATOL of the other, matched through a projection on a fixed direction."""
    w = np.cos(1.3 * np.arange(rows.shape[1]) + 0.4)
    for a, b, name in ((rows, seen, "emitted row is not a point of the oracle"), (seen, rows, "oracle point was not emitted")):
        pb = b @ w
        order = np.argsort(pb)
        pos = np.searchsorted(pb[order], a @ w)
        best = np.full(a.shape[0], np.inf)
        for off in (-3, -2, -1, 0, 1, 2):
            cand = b[order[np.clip(pos + off, 0, b.shape[0] - 1)]]
            best = np.minimum(best, np.abs(cand - a).max(axis=1))
        assert best.max() <= ROW_ATOL, (what, name, int(np.argmax(best)), best.max())


@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_generate_accumulate_on_the_reference_stream_around_a_closed_form_surrogate(d):
    """Every level, ragged batches, a site stride larger than B whose padding rows hold NaN in `points` (before GENERATE) and in `gp_vals`:
    the result against the oracle, the padding untouched, and the emitted rows of the first and the last root against the points the
    oracle evaluates its surrogate at."""
    Bs = _ragged(d)
    xt = _points(d, Bs[-1], seed=1300 + d)
    nan = np.float32(np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), dtype=np.float32)[0])
    for variant, n, par in JAX_ACC_CASES[d]:
        t = _Tree(0, d, variant, surrogate=True)
        t.sur = _Recorder(d)
        t.sur.seen = []
        want = t.oracle(n, par, xt, jax_stream=True)
        seen, t.sur.seen = np.stack(t.sur.seen), None
        for B in Bs:
            S = B + 3
            got, uh, P, vals = t.scasml(n, par, xt[:B], t.rng(jax=(n, par)), stride=S, pad=nan)
            _close(got, want[:B], _atol_rb(xt[:B], variant), RTOL_RB, (variant, n, par, B))
            assert np.all(P[:, B:].view(np.uint32) == np.uint32(0x7FC0BEEF)), (variant, n, par, B)
            assert np.array_equal(uh, vals[-1, :B, 0]) and np.array_equal(P[-1, :B, :d + 1], xt[:B].astype(np.float32))
            if np.isfinite(want).all():
                assert np.all(P[:, :B, d + 1:] == 0) and np.all(np.isfinite(P[:, :B]))
                for b in sorted({0, B - 1}):
                    _rows_match_the_oracles_points(P[:-1, b, :d + 1].astype(np.float64), np.unique(seen[:, b], axis=0), (variant, n, par, B, b))


# ------------------------------------------------------------------------------------------------------------- the normals themselves
def _normal_values():
    """The 1024 values jax.random.normal(float16) can take (oracle/jax_random.py normal_f16_at, by its ten random bits), sorted."""
    from oracle import jax_random as jr
    F16 = np.float16
    lo = np.nextafter(F16(-1.0), F16(0.0))
    u = ((np.arange(1024, dtype=np.uint16) | np.uint16(0x3C00)).view(F16) - F16(1.0)).astype(F16)
    u = np.maximum(lo, ((u * F16(F16(1.0) - lo)).astype(F16) + lo).astype(F16))
    return np.unique((F16(np.sqrt(2.0)) * jr.erf_inv32(u).astype(F16)).astype(F16).astype(np.float64))


def _snap(v, grid):
    i = np.clip(np.searchsorted(grid, v), 1, len(grid) - 1)
    near = np.where(np.abs(grid[i - 1] - v) <= np.abs(grid[i] - v), grid[i - 1], grid[i])
    return near, np.abs(near - v)


# one d per G and, beside FLAG_D's residues 2, 0, 3, 2, 3, two d with d mod 4 = 1, where a row of the draw starts at every alignment in turn
NORMALS_D = sorted(FLAG_D + [13, 61])
# the deep translation unit's GENERATE instantiations: (d, variant, n, par, roots)
DEEP_NORMALS = [(13, "quad", 5, 5, 1), (6, "quad", 4, 4, 3), (29, "fh", 4, 2, 3), (13, "fh", 5, 2, 3)]
# A normal is solved from X' = X + mu h + sigma sqrt(h) N with h >= MIN_H: X' carries two float32 roundings of a |coordinate| < 4
# (2.4e-7 each) and sqrt_fast, the product and the float32 h about 4e-7 |N| more, so the recovered N is off by at most
# 4.8e-7 / (0.25 sqrt(0.01)) + 4e-7 * 4 = 2.1e-5.  SNAP_TOL leaves a factor of five and stays under half the smallest spacing of the
# 1024 values (asserted > 5e-4), so the snap is unambiguous.
MIN_H, SNAP_TOL = 0.01, 1e-4


def _calls(plan, rows):
    """Every call of the tree that draws terminal samples, in site order: (level, base site, origin site, row of each root in the reference's
    flattened batch of that call, (q, mc) of the node that made the call or None) -- the site layout of oracle/mlp.py and the row rule of
    MLP.py:231, 253 (the children of sample m of a batch of rows r are rows r * mc + m)."""
    def rec(L, base, origin, r, parent):
        yield L, base, origin, r, parent
        o = int(plan.mg[L])
        for l in range(L):
            tm = plan.term[L][l]
            q, mc, s_l, s_lm = int(tm.q), int(tm.mc), int(tm.sites_l), int(tm.sites_lm1)
            for m in range(mc):
                for k in range(q):
                    node = base + o
                    o += 1
                    kid = r * np.uint64(mc) + np.uint64(m)
                    if l >= 1:
                        yield from rec(l, base + o, node, kid, (q, mc))
                    o += s_l
                    if l >= 2:
                        yield from rec(l - 1, base + o, node, kid, (q, mc))
                    o += s_lm
        assert o == int(plan.sites[L])
    return rec(int(plan.n), 0, int(plan.sites[plan.n]), rows, None)


def _generate(t, n, par, xt, root0):
    import torch
    from scasml_gp_amd import _lib
    plan = t.plan(n, par)
    B = xt.shape[0]
    ppr = int(_lib.load().scasml_points_per_root(C.byref(plan)))
    pts = torch.zeros((ppr * B, t.kp), device="cuda")
    _lib.check(t.launch(_lib.MODE_GENERATE, plan, torch.from_numpy(xt).cuda(), B, 0, t.rng(root0=root0, jax=(n, par)), pts=pts), "generate")
    words = t.jax_keys(n, par).cpu().numpy().view(np.uint32).reshape(-1, 2).astype(np.uint64)
    return plan, pts.cpu().numpy().reshape(ppr, B, t.kp).astype(np.float64), words


def _check_terminal_normals(t, plan, P, words, calls, grid, what):
    """The terminal samples X_T = X + mu tau + sigma sqrt(tau) N of each call, solved for N, snapped, against the terminal key at
    (row * mg + m) * d + i.  Roots whose origin is not finite (quadrature n >= 4) or closer to T than MIN_H are left out.  -> normals checked, per level of the call."""
    from oracle import jax_random as jr
    d, mu, sigma = t.d, float(t.prob.mu), float(t.prob.sigma)
    col = np.arange(d, dtype=np.uint64)[None, :]
    checked = {}
    for L, base, origin, r, _ in calls:
        mg = int(plan.mg[L])
        X, tau = P[origin, :, :d], float(t.prob.T) - P[origin, :, d]
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(P[origin]).all(axis=1) & (tau >= MIN_H)
        if not ok.any():
            continue
        XT = P[base:base + mg][:, ok, :d]                                 # (sample, root, dim)
        N = (XT - X[ok][None] - mu * tau[ok][None, :, None]) / (sigma * np.sqrt(tau[ok]))[None, :, None]
        near, dist = _snap(N, grid)
        index = (r[ok][None, :] * np.uint64(mg) + np.arange(mg, dtype=np.uint64)[:, None])[:, :, None] * np.uint64(d) + col[None]
        want = jr.normal_f16_at(words[0], index).astype(np.float64)
        assert dist.max() < SNAP_TOL and np.array_equal(near, want), (what, "call", L, base, dist.max(), int((near != want).sum()))
        checked[L] = checked.get(L, 0) + near.size
    return checked


@gpu
@pytest.mark.parametrize("d", NORMALS_D, ids=_ids(NORMALS_D))
def test_normals_recovered_from_generate_are_the_reference_draws(d):
    """The terminal samples of EVERY call of the tree -- the root call (row = root0 + local) and the level-1 calls below its nodes (row * mc + m
    one call down, where the quadrature plan has q != mc) -- and the first step X = x + mu dt + sigma sqrt(dt) xi of every level-0 path
    of the root call (quadrature: node k = 0 under path sub-key 0; full history: the one key again), each solved for its normal and snapped
    to the nearest of the 1024 possible values: equal to oracle/jax_random.py at (row * width + m) * d + i.  Roots with T - t >= 0.1."""
    from oracle import jax_random as jr
    grid = _normal_values()
    assert len(grid) > 900 and np.diff(grid).min() > 5e-4
    B, root0 = 2 * _rpw(d) + 1, 1000003
    xt = _points(d, B, seed=1400 + d)
    xt[:, d] = np.minimum(xt[:, d], np.float32(0.4))
    x64 = xt[:, :d].astype(np.float64)
    rows_ = np.uint64(root0) + np.arange(B, dtype=np.uint64)
    col = np.arange(d, dtype=np.uint64)[None, :]
    for variant, n, par in (("quad", 2, 2), ("fh", 2, 3)):
        t = _Tree(0, d, variant)
        plan, P, words = _generate(t, n, par, xt, root0)
        calls = list(_calls(plan, rows_))
        inner = [c for c in calls if c[4] is not None]
        assert calls[0][1:3] == (0, P.shape[0] - 1) and inner and (variant == "fh" or all(q != mc for *_, (q, mc) in inner))
        assert _check_terminal_normals(t, plan, P, words, calls[:1], grid, variant) == {n: int(plan.mg[n]) * B * d}
        assert sum(_check_terminal_normals(t, plan, P, words, inner, grid, variant).values()) >= len(inner) * B * d // 4
        mu, sigma = float(t.prob.mu), float(t.prob.sigma)
        mg, tm = int(plan.mg[n]), plan.term[n][0]
        q, mc = int(tm.q), int(tm.mc)
        checked = 0
        for m in range(mc):                                              # level-0 paths: sites mg + m q + k (their children are level-0 calls)
            site = mg + m * q
            dt = P[site, :, d] - xt[:, d].astype(np.float64)
            ok = dt >= MIN_H                                             # (full history: dt = U tau, any size)
            xi = (P[site, :, :d] - x64 - mu * dt[:, None]) / (sigma * np.sqrt(np.maximum(dt, 1e-30)))[:, None]
            near, dist = _snap(xi, grid)
            want = jr.normal_f16_at(words[1 if variant == "quad" else 0], (rows_ * np.uint64(mc) + np.uint64(m))[:, None] * np.uint64(d) + col).astype(np.float64)
            assert dist[ok].max(initial=0) < SNAP_TOL and np.array_equal(near[ok], want[ok]), (variant, "path", m, int((near[ok] != want[ok]).sum()))
            checked += int(ok.sum())
        assert checked >= mc * B // 4


@gpu
@pytest.mark.parametrize("d,variant,n,par,B", DEEP_NORMALS, ids=["%s%d-d%d" % (c[1], c[2], c[0]) for c in DEEP_NORMALS])
def test_normals_of_inner_calls_at_the_deep_levels(d, variant, n, par, B):
    """GENERATE of picard_tree_jax_deep.hip (levels 4 and 5): the terminal samples of every call of the tree, rows carried down up to four
    calls.  At quadrature n >= 4 the points after a path's first negative step are NaN; the rows before it, and every call made from
    them, are finite and are what this level can be checked on: calls of every level 1..n must be among those checked."""
    grid = _normal_values()
    xt = _points(d, B, seed=1450 + d)
    xt[:, d] = np.minimum(xt[:, d], np.float32(0.3))
    root0 = 70001
    t = _Tree(0, d, variant)
    plan, P, words = _generate(t, n, par, xt, root0)
    calls = list(_calls(plan, np.uint64(root0) + np.arange(B, dtype=np.uint64)))
    checked = _check_terminal_normals(t, plan, P, words, calls, grid, (variant, n))
    assert set(checked) == set(range(1, n + 1)) and checked[n] == int(plan.mg[n]) * B * d, checked


# ------------------------------------------------------------------------------------------------------------- flags at every width
@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_compat_f16_on_the_reference_stream(d):
    """The solver-level float16 casts on top (what reference_mode sets): tests/test_gpu_compat.py's bound; outputs are float16 values except
    full-history ACCUMULATE, which skips the final cast (ScaSML_full_history.py:199)."""
    from scasml_gp_amd import _lib
    B = max(_rpw(d) + 1, 33)
    xt = _points(d, B, seed=1500 + d)
    for surrogate in (False, True):
        for variant, n, par in (("quad", 3, 3), ("fh", 3, 2)):
            t = _Tree(0, d, variant, surrogate=surrogate, amp=0.05 if surrogate else 1e-3)      # (amp: test_compat_flags_at_every_width)
            run = (lambda rng: t.scasml(n, par, xt, rng)[0]) if surrogate else (lambda rng: t.mlp(n, par, xt, rng))
            plain = run(t.rng(jax=(n, par)))
            f16 = run(t.rng(jax=(n, par), flags=_lib.RNG_COMPAT_F16))
            assert _is16(f16) == (not (surrogate and variant == "fh")), (surrogate, variant)
            assert not np.array_equal(f16, plain)
            _close16(f16, t.oracle(n, par, xt, jax_stream=True, compat_f16=True), (surrogate, variant, "f16"))


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_root0_on_the_reference_stream(d):
    """Rows r .. r + k launched with root0 = r are bit for bit those rows of a root0 = 0 launch (what PicardEngine.solve relies on when it
    cuts a batch into chunks), in MLP mode and in GENERATE + ACCUMULATE; and a root0 that puts every draw index past 2^32 against the oracle."""
    B = 2 * _rpw(d) + 3
    xt = _points(d, B, seed=1600 + d)
    cuts = ((1, _rpw(d)), (_rpw(d) + 1, B - _rpw(d) - 1), (B - 1, 1))
    root0 = (1 << 31) + 12345
    for surrogate in (False, True):
        for variant, n, par in (("quad", 2, 2), ("fh", 3, 2)):
            t = _Tree(0, d, variant, surrogate=surrogate)
            run = (lambda x, rng: t.scasml(n, par, x, rng)[0]) if surrogate else (lambda x, rng: t.mlp(n, par, x, rng))
            whole = run(xt, t.rng(jax=(n, par)))
            for r, k in cuts:
                part = run(xt[r:r + k], t.rng(root0=r, jax=(n, par)))
                assert np.array_equal(part.view(np.uint64), whole[r:r + k].view(np.uint64)), (surrogate, variant, r, k)
            assert root0 * int(t.plan(n, par).mg[n]) * d > 1 << 32
            want = t.oracle(n, par, xt, root0=root0, jax_stream=True)
            assert np.isfinite(want).all(axis=1).mean() >= 0.9
            far = run(xt, t.rng(root0=root0, jax=(n, par)))
            assert not np.array_equal(far, whole)
            _close(far, want, _atol_rb(xt, variant) if surrogate else ATOL, RTOL_RB if surrogate else RTOL, (surrogate, variant, "past 2^32"))


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_dealt_sample_sharding_on_the_reference_stream(d):
    """world = 3 with the owner table of scasml_plan_deal_units: a draw is addressed by its index in the reference's flattened batch, whoever
    owns the sample, so each rank's partial sums equal the oracle's and their clipped sum the unsharded solve -- at the Philox sweep's bounds,
    and (sum against whole) at the bound tests/test_gpu_jax_stream.py holds at d = 20."""
    import torch
    B = _rpw(d) + 1
    xt = _points(d, B, seed=1700 + d)
    for surrogate in (False, True):
        for variant, n, par in (("quad", 3, 3), ("fh", 3, 2)):
            t = _Tree(0, d, variant, surrogate=surrogate)
            host, dev, _ = t.eng.unit_owners(n, par, 3)
            assert len(set(host.tolist())) == 3
            tol = (_atol_rb(xt, variant), RTOL_RB) if surrogate else (ATOL, RTOL)
            total = 0
            for r in range(3):
                rng = t.rng(rank=r, world=3, owner=dev.data_ptr(), jax=(n, par))
                got = t.scasml(n, par, xt, rng)[0] if surrogate else t.mlp(n, par, xt, rng)
                _close(got, t.oracle(n, par, xt, rank=r, world=3, owner=host, jax_stream=True), *tol, what=(surrogate, variant, r))
                total = total + got
            whole = t.scasml(n, par, xt, t.rng(jax=(n, par)))[0] if surrogate else t.mlp(n, par, xt, t.rng(jax=(n, par)))
            summed = t.eng.finalize_partials(torch.from_numpy(total.astype(np.float32)).cuda()).cpu().numpy().astype(np.float64)
            assert np.abs(summed - whole).max() <= 2.0 ** -10 * np.abs(whole).max()              # tests/test_gpu_jax_stream.py, d = 20
            _close(summed, whole, *tol, what=(surrogate, variant, "sum"))
