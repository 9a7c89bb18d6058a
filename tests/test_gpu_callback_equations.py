"""Equations outside the registry: MLP and MLP_full_history on torch f and g through the staged Picard tree (csrc/picard_staged.hip,
solvers/_picard.py PicardEngine._solve_staged).  Checked against the float64 oracle on the same Philox stream, against the fused kernels on
twins of the registered equations, and for the callback contract of the Equation docstring.  Tolerance as for ScaSML: the stage kernels
read the tree points back as ACCUMULATE does -> |diff| <= 5e-5 + 2e-4 |value|."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ATOL, RTOL = 5e-5, 2e-4


def _points(d, B, seed):
    from oracle.equation import sample_points
    dom, bdy = sample_points(np.random.default_rng(seed), d, B - B // 4, B // 4)
    return np.concatenate([dom, bdy])


def _close(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    err = np.abs(got[m] - want[m])
    assert np.all(err <= ATOL + RTOL * np.abs(want[m])), err.max()


def _weights(d):
    return 0.5 + np.arange(d) / max(d - 1, 1)          # a_i in [0.5, 1.5]: f sees z component by component


def _wavy(d, rowwise=False):
    """An equation outside the registry: f uses x_t (a coordinate and the time) and z component-wise, g is not a function of sum x.
    rowwise: f and g without reductions over a row, so that their bits cannot depend on how many rows a call holds."""
    import torch
    from scasml_gp_amd.equations.equations import Equation

    class Wavy(Equation):
        eq_id = None
        torch_callbacks = True

        def __init__(self, n_input):
            super().__init__(n_input)
            self.norm_estimation = 1.0
            self.uncertainty = 0.1
            self.a = torch.tensor(_weights(n_input - 1), dtype=torch.float32, device="cuda")

        def geometry(self, t0=0, T=0.5):
            self.t0, self.T = t0, T

        def mu(self, x_t=0):
            return 0.1

        def sigma(self, x_t=0):
            return 0.25

        def f(self, x_t, u, z):
            if rowwise:
                return -u * torch.sin(x_t[:, :1] + x_t[:, -1:]) + z[:, :1] * z[:, 1:2]
            return -u * torch.sin(x_t[:, :1] + x_t[:, -1:]) + (self.a * z * z).mean(dim=1, keepdim=True)

        def g(self, x_t):
            if rowwise:
                return torch.cos(x_t[:, :1]) * torch.cos(x_t[:, 1:2])
            return torch.cos(x_t[:, :-1]).mean(dim=1, keepdim=True)
    return Wavy(d + 1)


class _WavyNP:
    """The float64 NumPy twin of _wavy for oracle.mlp.PicardOracle."""
    eq_id = None

    def __init__(self, n_input):
        self.n_input, self.d = n_input, n_input - 1
        self.t0, self.T = 0.0, 0.5
        self.norm_estimation, self.uncertainty = 1.0, 0.1
        self.a = _weights(self.d)

    def mu(self):
        return 0.1

    def sigma(self):
        return 0.25

    def f(self, x_t, u, z):
        return -u * np.sin(x_t[:, :1] + x_t[:, -1:]) + np.mean(self.a * z * z, axis=1, keepdims=True)

    def g(self, x_t):
        return np.mean(np.cos(x_t[:, :-1]), axis=1, keepdims=True)


def _solver(eq, variant, seed):
    from scasml_gp_amd.solvers.MLP import MLP
    from scasml_gp_amd.solvers.MLP_full_history import MLP_full_history
    return MLP(eq, seed=seed) if variant == "quad" else MLP_full_history(eq, seed=seed)


def _solve(solver, variant, n, par, xt):
    return solver.uz_solve(n, par, xt) if variant == "quad" else solver.uz_solve(n, None, xt, par)


@pytest.mark.parametrize("variant,d,n,par,B", [("quad", 20, 1, 1, 64), ("quad", 20, 2, 2, 257), ("quad", 7, 2, 2, 33), ("quad", 100, 3, 3, 16),
                                               ("quad", 8, 4, 4, 4), ("fh", 20, 2, 3, 129), ("fh", 100, 3, 3, 8), ("fh", 12, 5, 2, 3)])
def test_staged_solve_matches_the_oracle(variant, d, n, par, B):
    from oracle.mlp import PicardOracle
    xt = _points(d, B, 30 + d)
    got = _solve(_solver(_wavy(d), variant, 4), variant, n, par, xt)
    want = PicardOracle(_WavyNP(d + 1), variant, seed=4, stream=0).uz_solve(n, par, xt)
    if variant == "quad" and par == 1:
        assert np.isnan(want).any()                   # rho = 1: the NaN quadrature weight of q = 2
    _close(got, want)


@pytest.mark.parametrize("variant", ["quad", "fh"])
def test_rows_at_terminal_time(variant):
    from oracle.mlp import PicardOracle
    xt = _points(20, 24, 7)
    xt[::3, -1] = 0.5                                 # t = T: the horizon is zero, the terminal normals are replayed, not read back
    xt[1::3, -1] = 0.4999
    got = _solve(_solver(_wavy(20), variant, 9), variant, 2, 2, xt)
    want = PicardOracle(_WavyNP(21), variant, seed=9, stream=0).uz_solve(2, 2, xt)
    _close(got, want)


def _twins():
    import torch
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear, Quadratic_Gradient_Reaction_Diffusion

    def g(self, x_t):
        return 1 - 1 / (1 + torch.exp(x_t[:, -1:] + x_t[:, :-1].sum(dim=1, keepdim=True)))

    class GDN(Grad_Dependent_Nonlinear):
        eq_id = None
        torch_callbacks = True

        def f(self, x_t, u, z):
            return self.sigma() * u * z.sum(dim=1, keepdim=True)
    GDN.g = g

    class QGRD(Quadratic_Gradient_Reaction_Diffusion):
        eq_id = None
        torch_callbacks = True

        def f(self, x_t, u, z):
            s, d = self.sigma(), self.n_input - 1
            w = u * (1 - u)
            return -w * (1 + (s * s * d / 2) * (1 - 2 * u)) + ((z * z).sum(dim=1, keepdim=True) - s * s * d * w * w)
    QGRD.g = g
    return [(GDN, Grad_Dependent_Nonlinear), (QGRD, Quadratic_Gradient_Reaction_Diffusion)]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("variant,d,n,par,B", [("quad", 20, 2, 2, 65), ("quad", 10, 3, 3, 9), ("fh", 20, 2, 3, 33), ("fh", 10, 3, 2, 9)])
def test_twins_of_registered_equations_match_the_fused_kernels(which, variant, d, n, par, B):
    twin, registered = _twins()[which]
    xt = _points(d, B, 50 + d)
    got = _solve(_solver(twin(d + 1), variant, 5), variant, n, par, xt)
    want = _solve(_solver(registered(d + 1), variant, 5), variant, n, par, xt)
    _close(got, want)


class _Spy:
    """Wraps f and g of an equation: records what they receive."""

    def __init__(self, eq):
        self.eq, self.calls = eq, []
        self.f0, self.g0 = eq.f, eq.g
        eq.f, eq.g = self.f, self.g

    def f(self, x_t, u, z):
        self.calls.append(("f", x_t, u, z))
        return self.f0(x_t, u, z)

    def g(self, x_t):
        self.calls.append(("g", x_t))
        return self.g0(x_t)


@pytest.mark.parametrize("variant,n,par", [("quad", 3, 3), ("fh", 2, 2)])
def test_callback_contract_and_call_counts(variant, n, par):
    import torch
    d, B = 9, 21
    eq = _wavy(d)
    spy = _Spy(eq)
    solver = _solver(eq, variant, 1)
    xt = _points(d, B, 3)
    out = _solve(solver, variant, n, par, xt)
    assert isinstance(out, np.ndarray) and out.shape == (B, d + 1) and out.dtype == np.float32
    assert [c[0] for c in spy.calls] == ["g"] + ["f"] * n          # one chunk: g once, f exactly n times
    for c in spy.calls:
        for tsr in c[1:]:
            assert isinstance(tsr, torch.Tensor) and tsr.is_cuda and tsr.dtype == torch.float32 and tsr.is_contiguous()
        R = c[1].shape[0]
        assert R % B == 0 and c[1].shape == (R, d + 1)
        if c[0] == "g":
            assert torch.all(c[1][:, -1] == 0.5)                    # the time column of a terminal sample is T
        else:
            assert c[2].shape == (R, 1) and c[3].shape == (R, d)
    # torch in -> torch out, on the device
    got = _solve(solver, variant, n, par, torch.from_numpy(xt).cuda())
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (B, d + 1)
    # n = 0 and B = 0 call nothing
    spy.calls.clear()
    assert np.array_equal(_solve(solver, variant, 0, par, xt), np.zeros((B, d + 1), dtype=np.float32))
    assert _solve(solver, variant, n, par, xt[:0]).shape == (0, d + 1)
    assert spy.calls == []


@pytest.mark.parametrize("bad", ["shape", "dtype", "host", "numpy"])
def test_wrong_callback_results_are_refused(bad):
    import torch
    eq = _wavy(6)
    g0 = eq.g
    eq.g = {"shape": lambda x: g0(x).reshape(1, -1), "dtype": lambda x: g0(x).double(), "host": lambda x: g0(x).cpu(),
            "numpy": lambda x: g0(x).cpu().numpy()}[bad]
    with pytest.raises(ValueError, match="g must return"):
        _solver(eq, "quad", 0).uz_solve(2, 2, _points(6, 8, 1))
    eq = _wavy(6)
    eq.f = lambda x_t, u, z: torch.zeros((x_t.shape[0], 2), device=x_t.device)
    with pytest.raises(ValueError, match="f must return"):
        _solver(eq, "fh", 0).uz_solve(2, None, _points(6, 8, 1), 2)


def test_determinism_chunking_and_call_stream(monkeypatch):
    from oracle.mlp import PicardOracle
    from scasml_gp_amd.solvers import _picard
    d, n, rho, B = 7, 2, 2, 97
    xt = _points(d, B, 8)
    a = _solver(_wavy(d), "quad", 6)
    first = a.uz_solve(n, rho, xt)
    assert np.array_equal(first, _solver(_wavy(d), "quad", 6).uz_solve(n, rho, xt))     # same seed, same stream: bit-identical
    # explicit stream ids replay work and leave the call counter alone
    r1, _, _ = a._engine.solve(n, rho, xt, stream_id=5)
    r2, _, _ = a._engine.solve(n, rho, xt, stream_id=5)
    assert np.array_equal(r1.cpu().numpy(), r2.cpu().numpy())
    assert np.array_equal(a._engine.solve(n, rho, xt, stream_id=0)[0].cpu().numpy(), first)
    # the second uz_solve of a solver draws from stream 1
    second = a.uz_solve(n, rho, xt)
    _close(second, PicardOracle(_WavyNP(d + 1), "quad", seed=6, stream=1).uz_solve(n, rho, xt))
    # a budget too small for one root per chunk: 97 chunks, the same bits as one (f and g without reductions over a row: a torch
    # reduction may add in another order when the batch is smaller)
    one = _solver(_wavy(d, rowwise=True), "quad", 6).uz_solve(n, rho, xt)
    eq = _wavy(d, rowwise=True)
    spy = _Spy(eq)
    monkeypatch.setattr(_picard, "STAGED_BUFFER_BYTES", 1)
    chunked = _solver(eq, "quad", 6).uz_solve(n, rho, xt)
    assert sum(c[0] == "g" for c in spy.calls) == B >= 3
    assert np.array_equal(chunked, one)


def test_refusals():
    import torch
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP
    from scasml_gp_amd.solvers.MLP import MLP
    from scasml_gp_amd.solvers.MLP_full_history import MLP_full_history
    from scasml_gp_amd.solvers.ScaSML import ScaSML
    from scasml_gp_amd.solvers.ScaSML_full_history import ScaSML_full_history
    eq = _wavy(10)
    gp = GP(eq)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for cls in (ScaSML, ScaSML_full_history):
        with pytest.raises(NotImplementedError, match="f_parts"):
            cls(eq, gp)
    assert torch.cuda.memory_allocated() == before                       # refused before anything was allocated or launched
    x = torch.zeros((4, 11), device="cuda")
    with pytest.raises(NotImplementedError):
        gp.GPsolver(x, x)
    for kw in ({"compat_rng": "jax"}, {"compat_f16": True}, {"compat_crn": True}, {"reference_mode": True}):
        for cls in (MLP, MLP_full_history):
            with pytest.raises(NotImplementedError, match="Philox"):
                cls(eq, **kw)
    with pytest.raises(NotImplementedError, match="sharded"):
        MLP(eq)._engine.solve(2, 2, _points(10, 4, 0), rank=0, world=2)
    for what in ("mu", "sigma"):
        bad = _wavy(10)
        setattr(bad, what, lambda x_t=0: np.array([0.1, 0.2]))
        with pytest.raises(ValueError, match=what):
            MLP(bad)

    class NoCallbacks(Grad_Dependent_Nonlinear):                         # eq_id None without torch_callbacks: refused as before
        eq_id = None
    with pytest.raises(NotImplementedError, match="eq_id unset"):
        MLP(NoCallbacks(11))


def test_stage_kernel_validates_its_arguments():
    import ctypes as C
    import torch
    from scasml_gp_amd import _lib, tables
    lib = _lib.load()
    plan = tables.build_plan("quad", 2, 2, 0.5, True)
    prob = _lib.Problem(10, 0, 0.5, 0.0, 0.25, 1.0)
    ent = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    buf = torch.zeros(64, device="cuda")
    p = _lib.ptr(buf)
    rng = _lib.Rng(0, 0, 0, 0, 1, 0, 0)
    s = _lib.stream_ptr()
    for stage in (0, 3):
        assert lib.scasml_picard_stage(C.byref(prob), C.byref(plan), stage, _lib.ptr(ent), 1, 4, 0, rng, p, p, p, p, s) == -1
    assert b"stage" in lib.scasml_last_error()
    deep = tables.build_plan("quad", 2, 2, 0.5, True)
    deep.n = _lib.MAX_LEVEL + 1
    assert lib.scasml_picard_stage(C.byref(prob), C.byref(deep), 1, _lib.ptr(ent), 1, 4, 0, rng, p, p, p, p, s) == -2
    for flags in (_lib.RNG_COMPAT_CRN, _lib.RNG_COMPAT_F16, _lib.RNG_JAX_STREAM):
        bad = _lib.Rng(0, 0, 0, 0, 1, flags, 0)
        assert lib.scasml_picard_stage(C.byref(prob), C.byref(plan), 1, _lib.ptr(ent), 1, 4, 0, bad, p, p, p, p, s) == -2
    sharded = _lib.Rng(0, 0, 0, 0, 2, 0, 0)
    assert lib.scasml_picard_stage(C.byref(prob), C.byref(plan), 1, _lib.ptr(ent), 1, 4, 0, sharded, p, p, p, p, s) == -2
    assert lib.scasml_picard_stage(C.byref(prob), C.byref(plan), 2, _lib.ptr(ent), 1, 4, 0, rng, p, p, p, None, s) == -1   # S = n needs out
    assert lib.scasml_picard_stage(C.byref(prob), C.byref(plan), 1, _lib.ptr(ent), 1, 4, 2, rng, p, p, p, p, s) == -1      # stride < B
