"""The reference's own runs of MLP.u_solve, replayed digit for digit (oracle/replay.py on oracle/jax_random.py).

The reference cannot run here (no JAX), ships no golden vectors, and draws its normals from JAX's threefry -- but its logs print what its runs
computed, to sixteen digits.  With the random stream, the key schedule and the dtype of every operation restated, the replay must print the
same numbers; one float16 normal drawn or rounded differently among the ~300 000 of a solve moves the last digits."""
import json
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LOGGED = json.load(open(os.path.join(HERE, "golden", "reference_logged.json")))["quadrature"]
DIMS = [20, 40, 60, 80]


def _line(d, prefix):
    for l in LOGGED[str(d)]["simple_uniform"]["head"]:
        if l.startswith(prefix):
            return l
    raise KeyError(prefix)


def _numbers(line):
    return [float(v) for v in re.findall(r"(?<=[:>] )-?\d+\.?\d*(?:e[-+]?\d+)?", line)]


def test_the_normal_stream_is_counter_based_and_standard():
    from oracle import jax_random as jr
    key = jr.split(jr.prng_key(0), 1)[0]
    a = jr.normal_f16(key, (50, 7, 20))
    assert a.dtype == np.float16 and bool(np.isfinite(a).all())
    assert abs(float(a.astype(np.float64).mean())) < 0.02 and abs(float(a.astype(np.float64).std()) - 1.0) < 0.02
    idx = np.array([0, 19, 20, 6999, 3141])                           # random access = the array draw at those row-major positions
    assert np.array_equal(jr.normal_f16_at(key, idx), a.reshape(-1)[idx])
    assert np.array_equal(jr.normal_f16(key, (7000,)), a.reshape(-1))  # the shape does not enter: only the row-major index does
    # float16 uniform grid: 1024 values, symmetric support (-1, 1) exclusive, so no infinite normals
    assert float(np.abs(a).max()) < 4.0


@pytest.mark.parametrize("d", DIMS)
def test_simple_uniform_mlp_numbers_all_printed_digits(d):
    """results/Grad_Dependent_Nonlinear/<d>d/SimpleUniform/SimpleUniform.log: a fresh MLP, n = rho = 2, on the harness's 1000 + 200 test points
    (np.random.seed(1234): the training draw, then this one; tests/SimpleUniform.py:73-86, 134-136)."""
    from oracle.equation import GradDependentNonlinear, deepxde_points, logistic_wave_f16
    from oracle.replay import ReplayMLP
    state = np.random.get_state()
    np.random.seed(1234)
    deepxde_points(d, 1000, 200)
    xt = np.concatenate(deepxde_points(d, 1000, 200))
    np.random.set_state(state)
    exact = logistic_wave_f16(xt).astype(np.float64)
    solver = ReplayMLP(GradDependentNonlinear(d + 1))
    sol = solver.u_solve(2, 2, xt).astype(np.float64)
    assert solver.splits == 15                                         # 3 (l = 0) + 3 x (1 + 3) (l = 1 and its level-1 children)
    err = np.abs(sol - exact)
    rel = float(np.linalg.norm(err) / np.linalg.norm(exact))
    assert rel == _numbers(_line(d, "MLP rel L2"))[-1]                  # e.g. 0.1603708391443781 at d = 20: every digit
    lo, hi, mean, std = _numbers(_line(d, "MLP L1"))[:4]
    assert float(err.min()) == lo and float(err.max()) == hi
    assert abs(float(err.mean()) - mean) <= 1e-15 and abs(float(err.std()) - std) <= 1e-15
    sq = err ** 2
    lo2, hi2, mean2, std2 = _numbers(_line(d, "MLP L2"))[:4]
    assert float(sq.max()) == pytest.approx(hi2, rel=1e-12) and float(sq.mean()) == pytest.approx(mean2, rel=1e-12)


@pytest.mark.parametrize("d", DIMS)
def test_repeated_experiment_mlp_statistics_to_the_printed_digits(d):
    """results/**/RepeatedExperiment.log: ten test sets (np.random.seed(42 + i)) through ONE solver object, whose key state carries over from
    call to call (MLP.py:220); relative L2 with the harness's float16 norm of the exact solution (RepeatedExperiment.py:71, 125-127:
    ``np.linalg.norm`` of a float16 array)."""
    from oracle.equation import GradDependentNonlinear, deepxde_points, logistic_wave_f16
    from oracle.replay import ReplayMLP
    solver = ReplayMLP(GradDependentNonlinear(d + 1))
    rel, l1, l2 = [], [], []
    state = np.random.get_state()
    for i in range(10):
        np.random.seed(42 + i)
        xt = np.concatenate(deepxde_points(d, 1000, 200))
        exact16 = logistic_wave_f16(xt).ravel()
        err = np.abs(solver.u_solve(2, 2, xt).astype(np.float64).ravel() - exact16)
        rel.append(np.linalg.norm(err) / np.linalg.norm(exact16))
        l1.append(err.mean())
        l2.append((err ** 2).mean())
    np.random.set_state(state)
    want = LOGGED[str(d)]["repeated"]
    for got, key in ((rel, "rel_l2"), (l1, "l1"), (l2, "l2")):
        got = np.asarray(got, dtype=np.float64)
        w = want[key]["MLP"]
        for value, name in ((got.mean(), "mean"), (got.std(ddof=1), "std"), (got.min(), "min"), (got.max(), "max")):
            assert value == pytest.approx(w[name], rel=2e-6), (key, name, value, w[name])      # seven printed digits


FH = json.load(open(os.path.join(HERE, "golden", "reference_logged.json")))["full_history"]


@pytest.mark.parametrize("d", DIMS)
def test_full_history_mlp_numbers_all_printed_digits(d):
    """results_full_history/Grad_Dependent_Nonlinear/<d>d/SimpleUniform/SimpleUniform.log: MLP_full_history, n = 2, M = 3.  Every draw of that
    solver comes from one key (MLP_full_history.py:92-93, 99, 133, 138), so the uniform time of a sample and its normals are functions of
    overlapping threefry outputs -- which is why a restatement on independent draws (oracle/mlp.py on Philox, and the HIP path) lands at 0.150
    where the log says 0.184 at d = 20 (profiles/HISTORY.md, round-4 sections 2 and 9): with the reference's stream the numbers are the log's, digit for digit."""
    from oracle.equation import GradDependentNonlinear, deepxde_points, logistic_wave_f16
    from oracle.replay import ReplayMLPFullHistory
    state = np.random.get_state()
    np.random.seed(1234)
    deepxde_points(d, 1000, 200)
    xt = np.concatenate(deepxde_points(d, 1000, 200))
    np.random.set_state(state)
    exact = logistic_wave_f16(xt).astype(np.float64)
    err = np.abs(ReplayMLPFullHistory(GradDependentNonlinear(d + 1)).u_solve(2, 3, xt).astype(np.float64) - exact)
    head = FH[str(d)]["simple_uniform"]["head"]
    rel = [l for l in head if l.startswith("MLP rel L2")][0]
    l1 = [l for l in head if l.startswith("MLP L1")][0]
    assert float(np.linalg.norm(err) / np.linalg.norm(exact)) == _numbers(rel)[-1]
    lo, hi, mean, std = _numbers(l1)[:4]
    assert float(err.min()) == lo and float(err.max()) == hi
    assert abs(float(err.mean()) - mean) <= 1e-15 and abs(float(err.std()) - std) <= 1e-15


def test_full_history_repeated_experiment_statistics_at_d20():
    from oracle.equation import GradDependentNonlinear, deepxde_points, logistic_wave_f16
    from oracle.replay import ReplayMLPFullHistory
    d = 20
    solver = ReplayMLPFullHistory(GradDependentNonlinear(d + 1))
    rel = []
    state = np.random.get_state()
    for i in range(10):
        np.random.seed(42 + i)
        xt = np.concatenate(deepxde_points(d, 1000, 200))
        exact16 = logistic_wave_f16(xt).ravel()
        err = np.abs(solver.u_solve(2, 3, xt).astype(np.float64).ravel() - exact16)
        rel.append(np.linalg.norm(err) / np.linalg.norm(exact16))
    np.random.set_state(state)
    w = FH[str(d)]["repeated"]["rel_l2"]["MLP"]
    rel = np.asarray(rel)
    for value, name in ((rel.mean(), "mean"), (rel.std(ddof=1), "std"), (rel.min(), "min"), (rel.max(), "max")):
        assert value == pytest.approx(w[name], rel=2e-6), (name, value, w[name])


def test_the_philox_oracle_fed_the_reference_normals_follows_the_replay():
    """oracle/mlp.py (float64, path by path: what the HIP path is checked against) with ``jax_stream=True`` reads the reference's normals by
    counter instead of Philox's.  Its recursion, its sample-to-row bookkeeping and its key schedule are then exercised against the replay,
    which walks the reference's batch-vectorised order: u agrees on every one of the 1200 points to two float16 ulps -- what is left is the
    float16 ARITHMETIC of the root call, which only the replay follows -- and the error metric to 3e-4."""
    from oracle.equation import GradDependentNonlinear, deepxde_points, logistic_wave_f16
    from oracle.mlp import PicardOracle
    from oracle.replay import ReplayMLP
    d = 20
    eq = GradDependentNonlinear(d + 1)
    state = np.random.get_state()
    np.random.seed(1234)
    deepxde_points(d, 1000, 200)
    xt = np.concatenate(deepxde_points(d, 1000, 200))
    np.random.set_state(state)
    exact = logistic_wave_f16(xt).astype(np.float64)
    want = ReplayMLP(eq).uz_solve(2, 2, xt).astype(np.float64)
    ora = PicardOracle(eq, "quad", jax_stream=True, compat_f16=True)
    got = ora.uz_solve(2, 2, xt.astype(np.float32))
    assert ora.jax_splits == 15
    du = np.abs(got[:, 0] - want[:, 0])
    assert du.max() <= 2 * 2.0 ** -11 and (du == 0).mean() > 0.4
    rel_got = np.linalg.norm(got[:, 0:1] - exact) / np.linalg.norm(exact)
    rel_want = np.linalg.norm(want[:, 0:1] - exact) / np.linalg.norm(exact)
    assert rel_want == _numbers(_line(d, "MLP rel L2"))[-1] and abs(rel_got - rel_want) <= 3e-4 * rel_want
    # a second call continues the solver's key state, as the harness's solver object does
    ora.uz_solve(2, 2, xt[:8].astype(np.float32))
    assert ora.jax_splits == 30


def test_the_philox_oracle_full_history_fed_the_reference_stream_follows_the_replay():
    """The same for the full-history variant: uniform times and normals of every call from the one key (MLP_full_history.py:92-93, 133, 138).
    On Philox draws this oracle gives 0.150 at d = 20; on the reference's stream 0.18997 -- the log's 0.1899677 to 2e-5, the rest being the
    reference's float16 arithmetic, which here runs through the whole recursion and which only the replay follows."""
    from oracle.equation import GradDependentNonlinear, deepxde_points, logistic_wave_f16
    from oracle.mlp import PicardOracle
    from oracle.replay import ReplayMLPFullHistory
    d = 20
    eq = GradDependentNonlinear(d + 1)
    state = np.random.get_state()
    np.random.seed(1234)
    deepxde_points(d, 1000, 200)
    xt = np.concatenate(deepxde_points(d, 1000, 200))
    np.random.set_state(state)
    exact = logistic_wave_f16(xt).astype(np.float64)
    want = ReplayMLPFullHistory(eq).uz_solve(2, 3, xt).astype(np.float64)
    got = PicardOracle(eq, "fh", jax_stream=True, compat_f16=True).uz_solve(2, 3, xt.astype(np.float32))
    du = np.abs(got[:, 0] - want[:, 0])
    assert du.max() <= 3 * 2.0 ** -11 and np.median(du) == 0.0
    rel = np.linalg.norm(got[:, 0:1] - exact) / np.linalg.norm(exact)
    rel_replay = np.linalg.norm(want[:, 0:1] - exact) / np.linalg.norm(exact)
    assert abs(rel - rel_replay) <= 1e-4 * rel_replay
    philox = PicardOracle(eq, "fh", compat_crn=True, compat_f16=True).uz_solve(2, 3, xt.astype(np.float32))
    assert np.linalg.norm(philox[:, 0:1] - exact) / np.linalg.norm(exact) < 0.16          # independent draws: a different (better) estimator


def test_scasml_oracle_on_the_reference_normals_lands_on_the_logged_numbers_at_d20():
    """ScaSML (solvers/ScaSML.py:149-304) = the same recursion on the defect of the surrogate.  oracle/mlp.py with the as-coded surrogate
    (oracle/gp_compat.py, fitted on the reference's training set with its Hutchinson indices) and the reference's normals gives the
    ScaSML numbers of 20d/SimpleUniform/SimpleUniform.log to 0.5 % -- against 3.5 % for one standard deviation over test sets, and
    1 % with Philox normals.  (Not to the digit: where the reference hands the surrogate float16 rows -- the root call's terminal points
    and the test points themselves -- its kernels differentiate through float16 arithmetic, which gp_compat.py does not follow.)
    About a minute."""
    from oracle.equation import GradDependentNonlinear, deepxde_points, logistic_wave_f16
    from oracle.gp_compat import OracleGPCompat
    from oracle.mlp import PicardOracle
    from scasml_gp_amd.threefry import reference_laplacian_idx
    d = 20
    eq = GradDependentNonlinear(d + 1)
    state = np.random.get_state()
    np.random.seed(1234)
    dom, bdy = deepxde_points(d, 1000, 200)
    xt = np.concatenate(deepxde_points(d, 1000, 200))
    np.random.set_state(state)
    gp = OracleGPCompat(eq, reference_laplacian_idx(d, "partitionable"))
    gp.GPsolver(dom.astype(np.float64), bdy.astype(np.float64), GN_steps=20)
    exact = logistic_wave_f16(xt).astype(np.float64)
    sol = PicardOracle(eq, "quad", gp=gp, jax_stream=True, compat_f16=True).u_solve(2, 2, xt.astype(np.float32))
    err = np.abs(sol - exact)                                                         # u_solve: float16 + float16 (ScaSML.py:300-304), compat_f16 rounds it
    rel = float(np.linalg.norm(err) / np.linalg.norm(exact))
    want = _numbers(_line(d, "ScaSML rel L2"))[-1]                                    # 0.07009992384811603
    assert abs(rel - want) <= 5e-3 * want, (rel, want)
    lo, hi, mean, std = _numbers(_line(d, "ScaSML L1"))[:4]
    assert abs(float(err.mean()) - mean) <= 6e-3 * mean and abs(float(err.max()) - hi) <= 4 * 2.0 ** -11


@pytest.mark.parametrize("variant,n,par", [("quad", 2, 2), ("quad", 3, 3), ("fh", 2, 3), ("fh", 3, 2)])
def test_reference_stream_rows_start_at_root0(variant, n, par):
    """A root's draws are addressed by its row in the reference's flattened batch, root0 + local in 64 bits (what picard_tree_kernel does
    and PicardEngine.solve relies on when it cuts a batch into chunks with root0 + b0): uz_solve(xt[r:r+k], root0=r) is rows r..r+k of
    uz_solve(xt), bit for bit -- also where (root0 + i) * width * d is past 2^32 -- and the key state advances as without root0."""
    from oracle.equation import GradDependentNonlinear, sample_points
    from oracle.mlp import PicardOracle
    d, B = 7, 12
    eq = GradDependentNonlinear(d + 1)
    xt = np.concatenate(sample_points(np.random.default_rng(3), d, B - 3, 3)).astype(np.float32)
    fresh = lambda: PicardOracle(eq, variant, jax_stream=True)
    whole = fresh()
    want = whole.uz_solve(n, par, xt)
    assert np.isfinite(want).all()
    for r, k in ((0, B), (1, 4), (5, 7), (11, 1)):
        part = fresh()
        assert np.array_equal(part.uz_solve(n, par, xt[r:r + k], root0=r), want[r:r + k]), (r, k)
        assert part.jax_splits == whole.jax_splits                      # (0 for full history: everything comes from the one key)
    # past 2^32: the terminal draw of the first root alone is at index root0 * mg * d
    big = (1 << 32) - 6
    assert big * 1 * d > 1 << 32 and big + B > 1 << 32                  # the row itself passes 2^32 too: it does not wrap
    far = fresh().uz_solve(n, par, xt, root0=big)
    assert not np.array_equal(far, want)
    for r, k in ((2, 5), (6, 6)):                                       # (6, 6): rows 2^32 .. 2^32 + 5
        assert np.array_equal(fresh().uz_solve(n, par, xt[r:r + k], root0=big + r), far[r:r + k]), (r, k)
    # a second call of one oracle continues the key state, with or without root0
    a, b = fresh(), fresh()
    a.uz_solve(n, par, xt)
    b.uz_solve(n, par, xt[:1], root0=9)
    assert a.jax_splits == b.jax_splits
    assert np.array_equal(a.uz_solve(n, par, xt[3:6], root0=3), b.uz_solve(n, par, xt, root0=0)[3:6])
