"""Standard errors for equations outside the registry: MLP and MLP_full_history with torch f and g return the Monte-Carlo standard errors of u
and of every z_i through their ``return_stderr`` arguments, from the last stage of the staged Picard tree (scasml_picard_stage_stderr,
PicardEngine._solve_staged).  The equation is the torch twin of _Steep (tests/test_gpu_stage_stderr_sweep.py); its sums over the dims are taken
column by column with elementwise operations, so that a row's bits cannot depend on how many rows a callback receives (a torch reduction may
add in another order when the batch is smaller) and a chunked solve can be compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_callback_equations import _points, _solver, _wavy
from test_gpu_picard_sweep import ATOL_RB, RTOL_RB
from test_gpu_stage_stderr_sweep import _Steep, bound_a
from test_gpu_stderr_uz_sweep import se_stats_z

pytestmark = pytest.mark.gpu

SHAPES = [(20, 33), (100, 9)]
PLANS = [("quad", 2, 3), ("fh", 2, 3)]


def _steep(d):
    """The torch twin of _Steep on the Equation subclass of _wavy: f = -u sin(x_0 + t) + mean(a_i z_i^2), g = cos(2 sum x_i)."""
    import torch
    eq = _wavy(d)
    eq.staged_stderr = True              # the equation asks for the staged estimate (Equation docstring)

    def columns(v):
        s = v[:, 0:1]
        for i in range(1, v.shape[1]):
            s = s + v[:, i:i + 1]
        return s

    eq.f = lambda x_t, u, z: -u * torch.sin(x_t[:, :1] + x_t[:, -1:]) + columns(eq.a * z * z) / float(d)
    eq.g = lambda x_t: torch.cos(2.0 * columns(x_t[:, :-1]))
    return eq


def _uz(solver, variant, n, par, xt, **kw):
    return solver.uz_solve(n, par, xt, **kw) if variant == "quad" else solver.uz_solve(n, None, xt, par, **kw)


def _u(solver, variant, n, par, xt, **kw):
    return solver.u_solve(n, par, xt, **kw) if variant == "quad" else solver.u_solve(n, None, xt, par, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("variant,n,par", PLANS)
@pytest.mark.parametrize("d,B", SHAPES)
def test_classes_return_standard_errors_for_callback_equations(d, B, variant, n, par, monkeypatch):
    import torch
    from oracle.mlp import PicardOracle
    from scasml_gp_amd import _lib
    from scasml_gp_amd.solvers import _picard
    xt = _points(d, B, 40 + d)
    solver = _solver(_steep(d), variant, 4)
    eng = solver._engine

    def at_call_zero(fn, *a, **kw):
        eng.calls = 0
        counted = solver.evaluation_counter
        r = fn(solver, variant, n, par, *a, **kw)
        assert eng.calls == 1 and solver.evaluation_counter - counted == eng.evaluation_increment(n, par)    # as a plain call moves them
        return r

    plain = at_call_zero(_uz, xt)
    uz, se = at_call_zero(_uz, xt, return_stderr="uz")
    assert isinstance(uz, np.ndarray) and isinstance(se, np.ndarray) and uz.shape == se.shape == (B, d + 1) and se.dtype == np.float32
    assert np.array_equal(_bits(uz), _bits(plain)), "return_stderr changed (u, z)"
    assert np.all(np.isfinite(se)) and np.all(se > 0)
    uz1, se1 = at_call_zero(_uz, xt, return_stderr=True)
    assert se1.shape == (B, 1) and np.array_equal(_bits(se1), _bits(se[:, 0:1])) and np.array_equal(_bits(uz1), _bits(plain))
    u, se_u = at_call_zero(_u, xt, return_stderr=True)
    assert u.shape == se_u.shape == (B, 1) and np.array_equal(_bits(u), _bits(plain[:, 0:1])) and np.array_equal(_bits(se_u), _bits(se1))
    # a CUDA tensor in, CUDA tensors out
    tu, ts = at_call_zero(_uz, torch.from_numpy(xt).cuda(), return_stderr="uz")
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == (B, d + 1) for t in (tu, ts))
    assert np.array_equal(_bits(ts.cpu().numpy()), _bits(se)) and np.array_equal(_bits(tu.cpu().numpy()), _bits(uz))
    # against the oracle's summands with the float64 twin: the bound of check (a) of tests/test_gpu_stage_stderr_sweep.py
    st = se_stats_z(PicardOracle(_Steep(d + 1), variant, seed=4, stream=0).root_summands(n, par, xt, with_z=True))
    dev, bound = np.abs(se.astype(np.float64) - st["se"]), bound_a(st, ATOL_RB, RTOL_RB)
    print("%s d=%d: max |se - oracle| / bound %.4f, smallest se / bound %.1f" % (variant, d, (dev / bound).max(), (st["se"] / bound).min()))
    assert np.all(np.isfinite(st["se"])) and np.all(dev <= bound), (dev / bound).max()
    # three chunks: the bits of the one-shot solve
    lib = _lib.load()
    plan = eng.plan(n, par)
    ppr, kp = int(lib.scasml_points_per_root(C.byref(plan))), int(lib.scasml_point_stride(d))
    per_root = 4 * (2 * ppr * kp + 2 * ppr + eng.stage_lists(n, par)["widest"] * (2 * d + 3))
    monkeypatch.setattr(_picard, "STAGED_BUFFER_BYTES", per_root * (B // 3))
    launches = []
    stage = eng._stage
    monkeypatch.setattr(eng, "_stage", lambda S, *a, **kw: (launches.append((S, kw.get("se") is not None)), stage(S, *a, **kw))[1])
    uz3, se3 = at_call_zero(_uz, xt, return_stderr="uz")
    assert [x for x in launches if x[0] == n] == [(n, True)] * 3 and not any(flag for S, flag in launches if S < n)
    assert np.array_equal(_bits(uz3), _bits(uz)) and np.array_equal(_bits(se3), _bits(se))


@pytest.mark.parametrize("variant", ["quad", "fh"])
def test_refusals_zeros_and_empty_batches(variant):
    d, B = 20, 5
    xt = _points(d, B, 3)
    solver = _solver(_steep(d), variant, 1)
    calls, counted = solver._engine.calls, solver.evaluation_counter
    for how in (True, "uz"):                       # a term of one sample: refused before anything moves
        with pytest.raises(ValueError, match=r"term \[2\]\[1\] has 1 sample path" if variant == "quad" else "no estimable variance"):
            _uz(solver, variant, 2, 2 if variant == "quad" else 1, xt, return_stderr=how)
    assert solver._engine.calls == calls and solver.evaluation_counter == counted
    par = 3
    uz, se = _uz(solver, variant, 0, par, xt, return_stderr="uz")
    assert np.array_equal(uz, np.zeros((B, d + 1), dtype=np.float32)) and np.array_equal(se, np.zeros((B, d + 1), dtype=np.float32))
    uz, se = _uz(solver, variant, 0, par, xt, return_stderr=True)
    assert np.array_equal(se, np.zeros((B, 1), dtype=np.float32))
    uz, se = _uz(solver, variant, 2, par, xt[:0], return_stderr="uz")
    assert uz.shape == se.shape == (0, d + 1)
    uz, se = _uz(solver, variant, 2, par, xt[:0], return_stderr=True)
    assert uz.shape == (0, d + 1) and se.shape == (0, 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        solver._engine.solve(2, par, xt, rank=0, world=2, stderr="uz")


@pytest.mark.parametrize("variant", ["quad", "fh"])
def test_an_equation_that_does_not_ask_keeps_its_refusal(variant):
    """staged_stderr is the equation's own request: without it return_stderr raises NotImplementedError naming the attribute, as such
    equations were always refused, and moves no counter; plain solves are the same with and without it, bit for bit."""
    d, B = 20, 5
    xt = _points(d, B, 3)
    eq = _steep(d)
    eq.staged_stderr = False
    solver = _solver(eq, variant, 1)
    for how in (True, "uz"):
        with pytest.raises(NotImplementedError, match="staged_stderr = True"):
            _uz(solver, variant, 2, 3, xt, return_stderr=how)
        with pytest.raises(NotImplementedError, match="staged_stderr = True"):
            _u(solver, variant, 2, 3, xt, return_stderr=True)
    assert solver._engine.calls == 0 and solver.evaluation_counter == 0
    plain = _uz(solver, variant, 2, 3, xt)
    asking = _solver(_steep(d), variant, 1)
    assert np.array_equal(_bits(_uz(asking, variant, 2, 3, xt)), _bits(plain))
    asking._engine.calls = 0
    assert np.array_equal(_bits(_uz(asking, variant, 2, 3, xt, return_stderr="uz")[0]), _bits(plain))
