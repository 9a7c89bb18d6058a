"""The Picard tree kernel (scasml_picard_tree, csrc/picard_tree.hpp) at every lane-group width, level and mode, called through ctypes.

A root owns G = ceil_pow2(kp / 4) lanes, kp = scasml_point_stride(d): G is 4, 8, 16, 32 or 64 and a wave holds 16 .. 1 roots.  G is a
runtime value -- one binary serves every width -- so what a width changes is the lane mapping, the masks (mask, tmask, row_lane) and the
length of the xor-shuffle sum over dims.  Where kp / 4 < G the top lanes of a group idle (d = 29..44, 61..76, 125..140).  The sweep takes
both ends of every G, an idle-lane d of each G >= 16 and all four residues of d mod 4 (which decide the float4 lane that holds t in an
emitted row), and checks, against oracle/mlp.py on the same Philox stream:

* SCASML_MODE_MLP, both variants, levels 1..5, ragged batches (1, roots-per-wave +- 1, a partial workgroup), equations 0, 1 and 2;
* GENERATE + ACCUMULATE around a closed-form surrogate (_Surrogate) instead of the GP evaluation, so that no float32 / float16
  surrogate error stands between the tree and the oracle: levels 1..4 (quadrature) and 1..5 (full history); roots on both sides of
  the read-back switch (kReadbackMinVol) at world 1 and 2; padding rows of a site stride > B that hold NaN; the emitted rows themselves;
* sample sharding with a dealt owner table, COMPAT_CRN, COMPAT_F16 and a root counter that wraps, at one d per G.

Bounds are the ones tests/test_gpu_mlp.py (MLP mode) and tests/test_gpu_configs.py (points read back) hold; where points are read back, a
root within 1e-2 of T adds the float32 floor of g - u_hat divided by T - t (_atol_rb), negligible further from T.  The float16 rounding helpers
(scasml_round16, scasml_round16_diag, scasml_clip_round16) are compared bit for bit with NumPy's casts at the end of the file.
"""
import ctypes as C
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu

ATOL, RTOL = 2e-5, 1e-4          # MLP mode (tests/test_gpu_mlp.py)
ATOL_RB, RTOL_RB = 5e-5, 2e-4    # wherever points are read back (tests/test_gpu_configs.py)

# both ends of every G (4: 1..12, 8: 13..28, 16: 29..60, 32: 61..124, 64: 125..252), an idle-lane d of each G >= 16 (29, 43; 61, 70;
# 125, 139) and every residue of d mod 4.  test_the_sweep_reaches_every_lane_group_width checks this list against the library.
D_SWEEP = [1, 6, 12, 13, 28, 29, 43, 60, 61, 70, 124, 125, 139, 252]
G_ENDS = {4: (1, 12), 8: (13, 28), 16: (29, 60), 32: (61, 124), 64: (125, 252)}
IDLE = {16: (29, 44), 32: (61, 76), 64: (125, 140)}           # kp / 4 < G, the most idle lanes of each G: 4, 12, 28
FLAG_D = [6, 28, 43, 70, 139]                                  # one d per G for the flag cases

# per d: the (variant, n, par) of MLP mode and of GENERATE + ACCUMULATE.  The oracle walks a tree once for a whole batch, so its cost is
# the tree's: about 0.5 s at quadrature n = 3, 7 s at n = 4, 30 to 90 s at n = 5 (one root), 1.5 s at full history n = 5 (measured on CPUs).
_Q3 = [(1, 2), (2, 2), (3, 3)]
_F4 = [(1, 3), (2, 3), (3, 2), (4, 2)]
MLP_CASES = {d: [("quad",) + _Q3[i % 3], ("fh",) + _F4[i % 4]] for i, d in enumerate(D_SWEEP)}
MLP_CASES[29].append(("quad", 4, 4))
MLP_CASES[125].append(("fh", 5, 2))
MLP_CASES[6].append(("fh", 5, 2))
DEEP_QUAD = (13, ("quad", 5, 5))        # one root, against tests/golden/oracle_quad5_d13.npz: the oracle walks this tree in a minute or more
ACC_CASES = {d: [("quad",) + _Q3[(i + 1) % 3], ("fh",) + _F4[(i + 2) % 4]] for i, d in enumerate(D_SWEEP)}
ACC_CASES[28].append(("quad", 4, 4))
ACC_CASES[60].append(("fh", 5, 2))
# T - t of the roots around the read-back switch: sigma sqrt(T - t) >= kReadbackMinVol = 1e-2 reads the stored X_T back, below it replays
SIGMA = 0.25
TAU_SWITCH = (1e-2 / SIGMA) ** 2
NEAR_T = [0.0, None, 1e-5, 1e-4, TAU_SWITCH * (1 - 1e-3), TAU_SWITCH * (1 + 1e-3), 1e-2]      # None: one float32 ulp below T
NEAR_T_D = [13, 70]


def _kp(d):
    return -(-(d + 4) // 16) * 16


def _G(d):
    g = 1
    while g < _kp(d) // 4:
        g *= 2
    return g


def _rpw(d):
    return 64 // _G(d)


def _ragged(d):
    """B = 1, roots-per-wave -+ 1 and 4 roots-per-wave + 1 (a workgroup of four waves, then one more root)."""
    r = _rpw(d)
    return sorted({b for b in (1, r - 1, r + 1, 4 * r + 1) if b > 0})


def _ids(ds):
    return ["G%02d-d%d" % (_G(d), d) for d in ds]


def test_the_sweep_reaches_every_lane_group_width():
    """The sweep against the library's own point stride: both ends of every G, an idle-lane d for G >= 16, all residues of d mod 4, and
    every level of both variants in MLP mode and in GENERATE + ACCUMULATE."""
    from scasml_gp_amd import _lib
    lib = _lib.load()
    stride = lambda d: int(lib.scasml_point_stride(d))
    G = lambda d: 1 << max(0, (stride(d) // 4 - 1).bit_length())
    assert all(_kp(d) == stride(d) and _G(d) == G(d) for d in range(1, _lib.MAX_DIM + 1))
    assert sorted({G(d) for d in range(1, _lib.MAX_DIM + 1)}) == [4, 8, 16, 32, 64]
    for g, (lo, hi) in G_ENDS.items():
        assert G(lo) == G(hi) == g and (lo == 1 or G(lo - 1) == g // 2) and (hi == _lib.MAX_DIM or G(hi + 1) == 2 * g)
        assert lo in D_SWEEP and hi in D_SWEEP, g
    for g, (lo, hi) in IDLE.items():
        assert {stride(d) for d in range(lo, hi + 1)} == {stride(lo)} and G(lo) == g and stride(lo) < stride(hi + 1)
        assert g - stride(lo) // 4 == {16: 4, 32: 12, 64: 28}[g]
        assert any(lo <= d <= hi for d in D_SWEEP), g
    assert {d % 4 for d in D_SWEEP} == {0, 1, 2, 3}
    assert sorted(G(d) for d in FLAG_D) == [4, 8, 16, 32, 64] and set(NEAR_T_D) <= set(D_SWEEP)
    mlp = {(v, n) for cases in MLP_CASES.values() for v, n, _ in cases} | {DEEP_QUAD[1][:2]}
    acc = {(v, n) for cases in ACC_CASES.values() for v, n, _ in cases}
    assert mlp == {(v, n) for v in ("quad", "fh") for n in range(1, 6)}
    assert acc == {("quad", n) for n in range(1, 5)} | {("fh", n) for n in range(1, 6)}
    assert set(MLP_CASES) == set(ACC_CASES) == set(D_SWEEP)
    assert all(n <= par for cases in list(MLP_CASES.values()) + list(ACC_CASES.values()) for v, n, par in cases if v == "quad")
    # ragged batches: a partial wave at every G below 64, and always a partly filled second workgroup
    assert all(1 in _ragged(d) and 4 * _rpw(d) + 1 in _ragged(d) for d in D_SWEEP)
    assert NEAR_T[4] < TAU_SWITCH < NEAR_T[5]


# ------------------------------------------------------------------------------------------------------------- helpers
class _Surrogate:
    """A smooth closed-form stand-in for the GP, the interface PicardOracle(gp=...) calls:
    u_hat = g + amp sin(a.x + b t) with g = 1 - 1/(1 + exp(t + sum x)) the terminal condition, so that g - u_hat stays of order amp
    (1e-3: z inside the 0.1 clip down to T - t of order 1e-2); eps = 1e-3 cos(c.x + e t).  Every coordinate and t carries its own weight,
    so a value taken from a misplaced column shows."""
    compat = None            # what PicardEngine.unit_owners asks of a surrogate: the documented operators' site costs

    def __init__(self, d, amp=1e-3):
        self.amp = amp
        i = np.arange(d, dtype=np.float64)
        self.a, self.b = 0.4 + 0.9 * np.cos(1.7 * i + 0.3), 1.3
        self.c, self.e = 0.6 - 1.1 * np.sin(0.9 * i + 0.2), -0.7

    @staticmethod
    def _split(P):
        P = np.asarray(P, dtype=np.float64)
        return P[:, :-1], P[:, -1]

    def predict(self, P):
        x, t = self._split(P)
        return (1 - 1 / (1 + np.exp(t + x.sum(1))) + self.amp * np.sin(x @ self.a + self.b * t))[:, None]

    def compute_gradient(self, P):
        x, t = self._split(P)
        L = 1 - 1 / (1 + np.exp(t + x.sum(1)))
        dL, c = L * (1 - L), self.amp * np.cos(x @ self.a + self.b * t)
        return np.concatenate([dL[:, None] + c[:, None] * self.a[None, :], (dL + c * self.b)[:, None]], axis=1)

    def compute_PDE_loss(self, P):
        x, t = self._split(P)
        return 1e-3 * np.cos(x @ self.c + self.e * t)[:, None]

    def values(self, P):
        """gp_vals rows (u_hat, sum_i d_i u_hat, eps_PDE, d_t u_hat), float64 cast to float32 once."""
        g = self.compute_gradient(P)
        return np.stack([self.predict(P)[:, 0], g[:, :-1].sum(1), self.compute_PDE_loss(P)[:, 0], g[:, -1]], axis=1).astype(np.float32)


_PRODUCT_EQ = {0: "Grad_Dependent_Nonlinear", 1: "Cubic_Reaction_Diffusion", 2: "Quadratic_Gradient_Reaction_Diffusion"}
_ORACLE_EQ = {0: "GradDependentNonlinear", 1: "CubicReactionDiffusion", 2: "QuadraticGradientReactionDiffusion"}


class _Tree:
    """One (equation, d, variant) of the kernel: the structs the solvers build (PicardEngine.plan / .problem), the launches, the oracle."""

    def __init__(self, eq_id, d, variant, surrogate=False, seed=7, stream=3, amp=1e-3):
        from oracle import equation as oe
        from scasml_gp_amd.equations import equations as pe
        from scasml_gp_amd.solvers._picard import PicardEngine
        self.d, self.variant, self.seed, self.stream = d, variant, seed, stream
        self.eq = getattr(pe, _PRODUCT_EQ[eq_id])(d + 1).geometry()          # as the solver classes do: T
        self.oeq = getattr(oe, _ORACLE_EQ[eq_id])(d + 1)
        self.sur = _Surrogate(d, amp) if surrogate else None
        # ScaSML's plan (stale_delta_t=False, clip = uncertainty) when a surrogate is in play, MLP's otherwise
        self.eng = PicardEngine(self.eq, variant, gp=self.sur, seed=seed)
        self.prob = self.eng.problem()
        self.kp = _kp(d)
        self._keys = {}
        assert self.prob.sigma == SIGMA and self.prob.clip == np.float32(0.1 if surrogate else 1.0)

    def plan(self, n, par):
        return self.eng.plan(n, par)

    def rng(self, root0=0, rank=0, world=1, flags=0, owner=None, jax=None):
        """jax = (n, par): the reference's own stream (RNG_JAX_STREAM) for that plan, from the initial key state."""
        from scasml_gp_amd import _lib
        keys = None
        if jax is not None:
            flags |= _lib.RNG_JAX_STREAM
            keys = self.jax_keys(*jax).data_ptr()
        return _lib.Rng(self.seed, self.stream, root0, rank, world, flags, 0, owner, keys)

    def jax_keys(self, n, par):
        """Device key words [terminal key | path sub-keys] of a solve that starts at PRNGKey(0), as PicardEngine._jax_keys builds them; kept
        alive here for as long as the launches that read them."""
        import torch
        from scasml_gp_amd import threefry
        if (n, par) not in self._keys:
            plan = self.plan(n, par)
            q = [[int(plan.term[level][l].q) for l in range(level)] for level in range(plan.n + 1)]
            words, _ = threefry.solver_key_words(q, plan.n, (0, 0), quadrature=self.variant == "quad")
            self._keys[(n, par)] = torch.from_numpy(words.view(np.int32).reshape(-1).copy()).cuda()
        return self._keys[(n, par)]

    def launch(self, mode, plan, x, B, stride, rng, pts=None, vals=None, out=None, uhat=None, prob=None):
        import torch
        from scasml_gp_amd import _lib
        lib = _lib.load()
        rc = lib.scasml_picard_tree(C.byref(prob or self.prob), C.byref(plan), mode, _lib.ptr(x), B, stride, rng, _lib.ptr(pts), _lib.ptr(vals),
                                    _lib.ptr(out), _lib.ptr(uhat), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def mlp(self, n, par, xt, rng):
        import torch
        from scasml_gp_amd import _lib
        x = torch.from_numpy(np.ascontiguousarray(xt, dtype=np.float32)).cuda()
        out = torch.full((x.shape[0], self.d + 1), -3.0, dtype=torch.float32, device="cuda")
        _lib.check(self.launch(_lib.MODE_MLP, self.plan(n, par), x, x.shape[0], 0, rng, out=out), "picard_tree(mlp)")
        return out.cpu().numpy().astype(np.float64)

    def scasml(self, n, par, xt, rng, stride=0, pad=0.0):
        """GENERATE; gp_vals from the surrogate in float64 at the emitted rows, cast to float32; ACCUMULATE.  Padding rows of `points`
        (before GENERATE) and of `gp_vals` hold ``pad``.  -> (out_uz, out_uhat, points (ppr, stride, kp), gp_vals (ppr, stride, 4))."""
        import torch
        from scasml_gp_amd import _lib
        lib = _lib.load()
        plan = self.plan(n, par)
        B, d = xt.shape[0], self.d
        S = stride or B
        ppr = int(lib.scasml_points_per_root(C.byref(plan)))
        x = torch.from_numpy(np.ascontiguousarray(xt, dtype=np.float32)).cuda()
        pts = torch.from_numpy(np.full((ppr * S, self.kp), pad, dtype=np.float32)).cuda()
        _lib.check(self.launch(_lib.MODE_GENERATE, plan, x, B, stride, rng, pts=pts), "picard_tree(generate)")
        P = pts.cpu().numpy().reshape(ppr, S, self.kp)
        vals = np.full((ppr, S, 4), pad, dtype=np.float32)
        vals[:, :B] = self.sur.values(P[:, :B, :d + 1].reshape(-1, d + 1)).reshape(ppr, B, 4)
        vd = torch.from_numpy(vals.reshape(-1, 4)).cuda()
        out = torch.full((B, d + 1), -3.0, dtype=torch.float32, device="cuda")
        uh = torch.full((B,), -3.0, dtype=torch.float32, device="cuda")
        _lib.check(self.launch(_lib.MODE_ACCUMULATE, plan, x, B, stride, rng, pts=pts, vals=vd, out=out, uhat=uh), "picard_tree(accumulate)")
        return out.cpu().numpy().astype(np.float64), uh.cpu().numpy(), pts.cpu().numpy().reshape(ppr, S, self.kp), vals

    def oracle(self, n, par, xt, **kw):
        from oracle.mlp import PicardOracle
        flags = {k: kw.pop(k) for k in ("compat_crn", "compat_f16", "jax_stream") if k in kw}     # a fresh oracle: the initial key state
        return PicardOracle(self.oeq, self.variant, gp=self.sur, seed=self.seed, stream=self.stream, **flags).uz_solve(n, par, xt, **kw)


def _points(d, B, seed):
    from oracle.equation import sample_points
    dom, bdy = sample_points(np.random.default_rng(seed), d, B - B // 4, B // 4)
    return np.concatenate([dom, bdy])


def _close(got, want, atol, rtol, what):
    """got within atol + rtol |want|.  NaN where the oracle has NaN and nowhere else: quadrature n >= 4 meets q = 5, whose tabulated nodes are
    not increasing (oracle/tables.py), and a negative step's square root makes the whole root NaN, as in the reference."""
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.all(np.isfinite(got[~nan])), what
    got, want = np.where(nan, 0, got), np.where(nan, 0, want)
    err = np.abs(got - want)
    bad = err > np.reshape(atol, (-1,) + (1,) * (want.ndim - 1)) + rtol * np.abs(want) if np.ndim(atol) else err > atol + rtol * np.abs(want)
    assert not bad.any(), "%s: %d of %d elements beyond %s + %g |v|, worst %.3e at %s" % (
        what, int(bad.sum()), bad.size, atol, rtol, err.max(), np.unravel_index(np.argmax(err - rtol * np.abs(want)), err.shape))


def _atol_rb(xt, variant):
    """ATOL_RB plus, per root, 2^-22 / (T - t + eps): where points are read back, g and u_hat are float32 values of O(1) numbers (half an
    ulp each), and the z estimator divides their difference by T - t + eps (eps = 1e-6 for quadrature, MLP.py:201; none for full history,
    MLP_full_history.py:122).  1e-6 at T - t = 0.25, 2.4e-5 at 1e-2, 2.4e-3 at 1e-4."""
    tau = np.float64(0.5) - np.asarray(xt, dtype=np.float32)[:, -1].astype(np.float64)
    return ATOL_RB + 2.0 ** -22 / (tau + (1e-6 if variant == "quad" else 0.0))


def _is16(v):
    return np.array_equal(v.astype(np.float16).astype(v.dtype), v)


def _close16(got, want, what):
    """tests/test_gpu_compat.py's bound under the float16 casts: a cast decided on a float32 value here and a float64 value in the oracle
    can land one float16 ulp apart on rare elements."""
    diff = np.abs(got - want)
    ulp = 2.0 ** -10 * np.maximum(np.abs(want), 2.0 ** -14)
    assert (diff > ulp + 1e-6).mean() <= 0.03, (what, (diff > ulp + 1e-6).mean())
    assert np.abs(got[:, 0] - want[:, 0]).max() <= 6e-4 and diff.max() <= 2e-2, (what, diff.max())


# ------------------------------------------------------------------------------------------------------------- MLP mode
@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_mlp_mode_matches_the_oracle_at_every_width_and_level(d):
    """Every level of both variants against the oracle at ragged batches: B = 1, a wave short of or one past full, a partial workgroup.
    The roots are 0 .. B-1 of the one oracle batch, so each launch compares with a prefix of it."""
    Bs = _ragged(d)
    xt = _points(d, Bs[-1], seed=100 + d)
    for variant, n, par in MLP_CASES[d]:
        t = _Tree(0, d, variant)
        want = t.oracle(n, par, xt)
        for B in Bs:
            _close(t.mlp(n, par, xt[:B], t.rng()), want[:B], ATOL, RTOL, (variant, n, par, B))


def _quad5():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_quad5_d13.npz"))


@pytest.mark.slow
def test_oracle_reproduces_the_quadrature_level_five_fixture():
    """tests/golden/oracle_quad5_d13.npz (tests/golden/make_golden.py) is the oracle's own result: 113 745 tree sites, more than the GPU
    file's time allows to walk in NumPy each run."""
    d, (variant, n, par) = DEEP_QUAD
    g = _quad5()
    from oracle.equation import GradDependentNonlinear
    from oracle.mlp import PicardOracle
    assert g["x_t"].shape == (1, d + 1)
    got = PicardOracle(GradDependentNonlinear(d + 1), variant, seed=7, stream=3).uz_solve(n, par, g["x_t"])
    assert np.allclose(got, g["uz"], rtol=0, atol=1e-12, equal_nan=True)


@gpu
def test_mlp_mode_quadrature_level_five_on_one_root():
    d, (variant, n, par) = DEEP_QUAD
    t = _Tree(0, d, variant)
    assert (t.seed, t.stream) == (7, 3)
    g = _quad5()
    _close(t.mlp(n, par, g["x_t"], t.rng()), g["uz"], ATOL, RTOL, "quad n=5")


@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_mlp_mode_other_equations_and_their_refusals(d):
    """Equations 1 and 2 (f of |z|^2: one more xor-shuffle sum per evaluation of f) in MLP mode; GENERATE and ACCUMULATE refuse equation 2
    and leave their buffers alone."""
    import torch
    from scasml_gp_amd import _lib
    B = _rpw(d) + 1
    xt = _points(d, B, seed=200 + d)
    for eq_id in (1, 2):
        for variant, n, par in (("quad", 2, 2), ("fh", 2, 3)):
            t = _Tree(eq_id, d, variant)
            _close(t.mlp(n, par, xt, t.rng()), t.oracle(n, par, xt), ATOL, RTOL, (eq_id, variant))
    t = _Tree(0, d, "quad", surrogate=True)
    plan = t.plan(2, 2)
    prob = _lib.Problem(t.prob.d, _lib.EQ_QUADRATIC_GRADIENT_REACTION_DIFFUSION, t.prob.T, t.prob.mu, t.prob.sigma, t.prob.clip)
    ppr = int(_lib.load().scasml_points_per_root(C.byref(plan)))
    x = torch.from_numpy(xt).cuda()
    pts = torch.full((ppr * B, t.kp), 5.0, device="cuda")
    vals = torch.zeros((ppr * B, 4), device="cuda")
    out = torch.full((B, d + 1), 5.0, device="cuda")
    assert t.launch(_lib.MODE_GENERATE, plan, x, B, 0, t.rng(), pts=pts, prob=prob) != 0
    assert t.launch(_lib.MODE_ACCUMULATE, plan, x, B, 0, t.rng(), pts=pts, vals=vals, out=out, prob=prob) != 0
    assert bool((pts == 5.0).all()) and bool((out == 5.0).all())


# ------------------------------------------------------------------------------------------------------------- GENERATE + ACCUMULATE
def _check_rows(t, plan, xt, P, world=1):
    """The emitted rows: the root row at site ppr-1 is x_t bit for bit, terminal rows carry t = T exactly, columns d+1 .. kp-1 are zero."""
    from scasml_gp_amd import _lib, tables
    d, B = t.d, xt.shape[0]
    rows = P[:, :B]
    assert np.array_equal(rows[-1, :, :d + 1], xt.astype(np.float32))
    term = tables.stage_list(plan, _lib.STAGE_TERMINALS, 0)
    if world == 1:
        assert np.all(rows[:, :, d + 1:] == 0) and np.all(np.isfinite(rows))
        assert np.all(rows[term, :, d] == np.float32(t.prob.T))
        assert np.all(rows[:, :, d] >= xt[None, :, d]) and np.all(rows[:, :, d] <= np.float32(t.prob.T))


@gpu
@pytest.mark.parametrize("d", D_SWEEP, ids=_ids(D_SWEEP))
def test_generate_accumulate_match_the_oracle_around_a_closed_form_surrogate(d):
    """The tree alone, with no GP-kernel error in the way: every level, ragged batches, and the emitted rows."""
    Bs = _ragged(d)
    xt = _points(d, Bs[-1], seed=300 + d)
    for variant, n, par in ACC_CASES[d]:
        t = _Tree(0, d, variant, surrogate=True)
        want = t.oracle(n, par, xt)
        for B in Bs:
            got, uh, P, vals = t.scasml(n, par, xt[:B], t.rng())
            _close(got, want[:B], _atol_rb(xt[:B], variant), RTOL_RB, (variant, n, par, B))
            assert np.array_equal(uh, vals[-1, :B, 0])                       # u_hat of the root row (ScaSML.py:303)
            assert np.allclose(uh, t.sur.predict(xt[:B])[:, 0], rtol=0, atol=1e-6)
            if np.isfinite(want).all():                      # (quadrature n = 4: NaN states, whose padding columns are 0 * NaN)
                _check_rows(t, t.plan(n, par), xt[:B], P)


@gpu
@pytest.mark.parametrize("d", D_SWEEP[::3], ids=_ids(D_SWEEP[::3]))
def test_padding_rows_are_neither_written_nor_read(d):
    """site_stride = B rounded up to 32, plus 32: NaN in every padding row of `points` and `gp_vals` changes no output bit, and GENERATE
    leaves the padding of `points` as it found it."""
    B = 4 * _rpw(d) + 1
    xt = _points(d, B, seed=400 + d)
    S = (B + 31) // 32 * 32 + 32
    nan = np.float32(np.frombuffer(np.uint32(0x7FC0BEEF).tobytes(), dtype=np.float32)[0])
    for variant, n, par in (("quad", 2, 2), ("fh", 3, 2)):
        t = _Tree(0, d, variant, surrogate=True)
        base = t.scasml(n, par, xt, t.rng())
        zero = t.scasml(n, par, xt, t.rng(), stride=S, pad=0.0)
        poisoned = t.scasml(n, par, xt, t.rng(), stride=S, pad=nan)
        for a, b in ((base, zero), (zero, poisoned)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert np.array_equal(a[2][:, :B].view(np.uint32), b[2][:, :B].view(np.uint32))
        assert np.all(poisoned[2][:, B:].view(np.uint32) == np.uint32(0x7FC0BEEF))
        assert np.all(zero[2][:, B:] == 0)


def _near_t_points(d, seed):
    T = np.float32(0.5)
    xt = _points(d, len(NEAR_T), seed)
    for i, tau in enumerate(NEAR_T):
        xt[i, d] = np.nextafter(T, np.float32(0)) if tau is None else np.float32(0.5 - tau)
    return xt


@gpu
@pytest.mark.parametrize("d", NEAR_T_D, ids=_ids(NEAR_T_D))
def test_accumulate_on_both_sides_of_the_read_back_switch(d):
    """Roots at T - t = 0, one float32 ulp, 1e-5, 1e-4, just below and above (kReadbackMinVol / sigma)^2 and 1e-2.  At world 1 the terminal
    rows come through the prefetch queue; at world 2 through the direct reads, and the partial sums are compared before any clip (the
    z of a root this close to T is far outside it, where a clip would hide a read-back error), around a surrogate whose g - u_hat is O(0.3):
    a read-back error is proportional to it.

    Bound: 5e-5 + 2e-4 |v| plus, per root, the float32 floor of g - u_hat divided by T - t (_atol_rb)."""
    xt = _near_t_points(d, seed=500 + d)
    taus = np.float64(0.5) - xt[:, d].astype(np.float64)
    assert taus[0] == 0 and 0 < taus[1] < 1e-7
    assert np.all(SIGMA * np.sqrt(taus[:5]) < 1e-2) and np.all(SIGMA * np.sqrt(taus[5:]) > 1e-2)
    for variant, n, par in (("quad", 2, 2), ("quad", 3, 3), ("fh", 2, 3)):
        keep = slice(None) if variant == "quad" else slice(1, None)      # full history: 1 / (T - t), no epsilon -- not at T itself
        rows = xt[keep]
        atol = _atol_rb(rows, variant)
        t = _Tree(0, d, variant, surrogate=True)
        _close(t.scasml(n, par, rows, t.rng())[0], t.oracle(n, par, rows), atol, RTOL_RB, (variant, n, "world 1"))
        t = _Tree(0, d, variant, surrogate=True, amp=0.3)
        for r in range(2):
            got = t.scasml(n, par, rows, t.rng(rank=r, world=2))[0]
            _close(got, t.oracle(n, par, rows, rank=r, world=2), atol, RTOL_RB, (variant, n, "world 2 rank %d" % r))
            assert np.abs(got[:, 1:]).max() > 100.0                            # un-clipped: a clip would have hidden a read-back error


# ------------------------------------------------------------------------------------------------------------- flags at every width
@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_dealt_sample_sharding_at_every_width(d):
    """world = 3 with the owner table of scasml_plan_deal_units: each rank's partial sums against the oracle's, and their clipped sum
    against the unsharded solve -- MLP mode and ACCUMULATE."""
    import torch
    B = _rpw(d) + 1
    xt = _points(d, B, seed=600 + d)
    for surrogate in (False, True):
        for variant, n, par in (("quad", 3, 3), ("fh", 3, 2)):
            t = _Tree(0, d, variant, surrogate=surrogate)
            host, dev, _ = t.eng.unit_owners(n, par, 3)
            assert len(set(host.tolist())) == 3
            tol = (_atol_rb(xt, variant), RTOL_RB) if surrogate else (ATOL, RTOL)
            total = 0
            for r in range(3):
                rng = t.rng(rank=r, world=3, owner=dev.data_ptr())
                got = t.scasml(n, par, xt, rng)[0] if surrogate else t.mlp(n, par, xt, rng)
                _close(got, t.oracle(n, par, xt, rank=r, world=3, owner=host), *tol, what=(surrogate, variant, r))
                total = total + got
            whole = t.scasml(n, par, xt, t.rng())[0] if surrogate else t.mlp(n, par, xt, t.rng())
            summed = torch.from_numpy(total.astype(np.float32)).cuda()
            _close(t.eng.finalize_partials(summed).cpu().numpy().astype(np.float64), whole, *tol, what=(surrogate, variant, "sum"))


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_compat_flags_at_every_width(d):
    """COMPAT_CRN (terminal draws keyed by the k = 0 position) at the plain bounds; COMPAT_F16 (the solver-level float16 casts) at the
    bound of tests/test_gpu_compat.py -- full-history ACCUMULATE skips the final cast (ScaSML_full_history.py:199), the others end in it."""
    from scasml_gp_amd import _lib
    B = max(_rpw(d) + 1, 33)           # the float16 bound is a fraction of elements: a few roots would make it a coin toss
    xt = _points(d, B, seed=700 + d)
    for surrogate in (False, True):
        for variant, n, par in (("quad", 3, 3), ("fh", 3, 2)):
            t = _Tree(0, d, variant, surrogate=surrogate)
            run = (lambda rng: t.scasml(n, par, xt, rng)[0]) if surrogate else (lambda rng: t.mlp(n, par, xt, rng))
            tol = (_atol_rb(xt, variant), RTOL_RB) if surrogate else (ATOL, RTOL)
            plain = run(t.rng())
            crn = run(t.rng(flags=_lib.RNG_COMPAT_CRN))
            # (full-history MLP of equation 0: the level-0 draws CRN moves feed f(0, 0) = 0 only)
            assert np.array_equal(crn, plain) == (variant == "fh" and not surrogate)
            _close(crn, t.oracle(n, par, xt, compat_crn=True), *tol, what=(surrogate, variant, "crn"))
            if surrogate:
                # g - u_hat of order 5e-2, not 1e-3: a float16 cast of a difference that small would be decided by the float32 rounding of
                # its two O(1) terms on a few percent of the sites, each flip moving every z of its root
                t = _Tree(0, d, variant, surrogate=True, amp=0.05)
                plain = run(t.rng())
            f16 = run(t.rng(flags=_lib.RNG_COMPAT_F16))
            assert _is16(f16) == (not (surrogate and variant == "fh")), (surrogate, variant)
            assert not np.array_equal(f16, plain)
            _close16(f16, t.oracle(n, par, xt, compat_f16=True), (surrogate, variant, "f16"))


@gpu
@pytest.mark.parametrize("d", FLAG_D, ids=_ids(FLAG_D))
def test_root_counter_wraps_at_every_width(d):
    """root0 = 2^32 - 5 and a batch past the end of the 32-bit counter: roots 2^32 - 5 .. 2^32 - 1, then 0, 1, ... (the oracle masks them
    to 32 bits), in MLP mode and in GENERATE + ACCUMULATE."""
    root0 = (1 << 32) - 5
    B = max(_rpw(d) + 1, 9)
    xt = _points(d, B, seed=800 + d)
    for surrogate in (False, True):
        for variant, n, par in (("quad", 2, 2), ("fh", 3, 2)):
            t = _Tree(0, d, variant, surrogate=surrogate)
            want = t.oracle(n, par, xt, root0=root0)
            if surrogate:
                _close(t.scasml(n, par, xt, t.rng(root0=root0))[0], want, _atol_rb(xt, variant), RTOL_RB, (variant, "wrap"))
            else:
                got = t.mlp(n, par, xt, t.rng(root0=root0))
                _close(got, want, ATOL, RTOL, (variant, "wrap"))
                # the wrapped roots are roots 0, 1, ... of a batch that starts at 0
                _close(t.mlp(n, par, xt[5:], t.rng()), got[5:], 1e-7, 0, (variant, "wrapped rows"))


# ------------------------------------------------------------------------------------------------------------- float16 rounding helpers
def _round16_inputs():
    """float64: every float16 value, every midpoint between neighbours and one float64 ulp either side, the overflow edge, the
    underflow-to-zero edge and the specials."""
    h = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16)
    h = h[np.isfinite(h)]
    v = np.unique(h.astype(np.float64))                                  # -0 and +0 collapse here; both are added below
    mid = (v[:-1] + v[1:]) / 2
    edge = np.array([65504.0, 65519.0, 65519.99999999999, np.nextafter(65520.0, 0), 65520.0, np.nextafter(65520.0, np.inf), 65536.0, 1e300,
                     2.0 ** -25, np.nextafter(2.0 ** -25, 0), np.nextafter(2.0 ** -25, 1), 2.0 ** -24, 2.0 ** -26, 3 * 2.0 ** -26,
                     np.nextafter(3 * 2.0 ** -26, 0), 5e-324, 2.0 ** -14, 2.0 ** -15 * 3])
    edge = np.concatenate([edge, -edge])
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan])
    return np.concatenate([h.astype(np.float64), mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf), edge, special])


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, want, x):
    """bit for bit (the sign of zero included), a NaN of any payload matching a NaN"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = _bits(got)[~nan] != _bits(want)[~nan]
    assert not bad.any(), "%d differ, first %r -> %r (want %r)" % (int(bad.sum()), x[~nan][bad][0], got[~nan][bad][0], want[~nan][bad][0])


@gpu
def test_round16_is_numpys_float16_cast_bit_for_bit():
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    x = _round16_inputs()
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).astype(np.float64)
    v = torch.from_numpy(x.copy()).cuda()
    _lib.check(lib.scasml_round16(_lib.ptr(v), v.numel(), _lib.stream_ptr()), "round16")
    _same_bits(v.cpu().numpy(), want, x)


@gpu
def test_round16_diag_rounds_the_diagonal_and_nothing_else():
    """A[i][i] = float16(A[i][i] + nugget) with lda > M: the diagonal against NumPy, every other element (the padding columns included)
    untouched, bit for bit.  (The rounding itself is scasml_round16's, swept above.)"""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    x = _round16_inputs()
    M, lda = 700, 709
    A = np.random.default_rng(0).standard_normal((M, lda)) * 1e3
    A.view(np.uint64)[3, :] = np.random.default_rng(1).integers(0, 1 << 63, lda, dtype=np.uint64)      # arbitrary bits, NaNs included
    picks = np.concatenate([x[-42:], np.random.default_rng(2).choice(x, 2 * M - 42, replace=False)])    # edges, specials, a sample
    off = ~np.eye(M, lda, dtype=bool)
    for diag in (picks[:M], picks[M:]):
        for nugget in (0.0, 0.5):
            B = A.copy()
            B[np.arange(M), np.arange(M)] = diag
            dev = torch.from_numpy(B.copy()).cuda()
            _lib.check(lib.scasml_round16_diag(_lib.ptr(dev), M, lda, nugget, _lib.stream_ptr()), "round16_diag")
            got = dev.cpu().numpy()
            assert np.array_equal(got.view(np.uint64)[off], B.view(np.uint64)[off])
            with np.errstate(over="ignore", invalid="ignore"):
                want = (diag + nugget).astype(np.float16).astype(np.float64)
            _same_bits(np.diagonal(got).copy(), want, diag + nugget)


@gpu
def test_clip_round16_is_numpys_clip_then_float16_cast():
    """scasml_clip_round16 on float32: clip keeps NaN (jnp.clip); round16 = 0 clips only."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    x64 = _round16_inputs()
    with np.errstate(over="ignore"):                                     # 65536 and up: inf in float16, some already in float32
        x = np.unique(np.concatenate([x64.astype(np.float32), np.nextafter(x64.astype(np.float32), np.float32(np.inf)),
                                      np.nextafter(x64.astype(np.float32), np.float32(-np.inf))]))
    x = np.concatenate([x, np.array([-0.0, np.nan], dtype=np.float32)])
    for clip in (np.float32(np.inf), np.float32(0.1), np.float32(65519.0), np.float32(1e-7)):
        for round16 in (0, 1):
            v = torch.from_numpy(x.copy()).cuda()
            _lib.check(lib.scasml_clip_round16(_lib.ptr(v), v.numel(), float(clip), round16, _lib.stream_ptr()), "clip_round16")
            with np.errstate(over="ignore", invalid="ignore"):
                want = np.where(x < -clip, -clip, np.where(x > clip, clip, x)).astype(np.float32)
                if round16:
                    want = want.astype(np.float16).astype(np.float32)
            got = v.cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(x)), (clip, round16)
            m = ~np.isnan(x)
            assert np.array_equal(got[m].view(np.uint32), want[m].view(np.uint32)), (clip, round16)
