"""PicardOracle.root_summands(..., with_z=True): what every sample of the root call adds to (u, z_1 .. z_d), recorded in ONE walk of the tree.

The yardstick is the method of tests/test_gpu_picard_stderr_uz.py (_oracle_se_uz): one walk per summand, with that summand's units owned by
rank 0 of a world of 2, whose result IS the summand's unclipped addition to (u, z).  The one-walk arrays must equal it exactly -- the same
float64 expressions on the same operands -- and their column 0 must be the with_z=False arrays, which must not have moved by a bit.  No GPU.
"""
import numpy as np
import pytest

from test_gpu_picard_stderr import _groups
from test_gpu_picard_sweep import _points
from test_gpu_stderr_sweep import _SweepSurrogate

D, B = 6, 3


def _oracle(variant, surrogate):
    from oracle.equation import GradDependentNonlinear
    from oracle.mlp import PicardOracle
    return PicardOracle(GradDependentNonlinear(D + 1), variant, gp=_SweepSurrogate(D) if surrogate else None, seed=7, stream=3)


@pytest.mark.parametrize("variant,n,par,surrogate", [("quad", 2, 3, False), ("fh", 3, 2, False), ("quad", 2, 3, True), ("fh", 2, 3, True)],
                         ids=["quad-2-3-mlp", "fh-3-2-mlp", "quad-2-3-surrogate", "fh-2-3-surrogate"])
def test_one_walk_z_summands_equal_the_one_summand_owner_method(variant, n, par, surrogate):
    xt = _points(D, B, 77)
    ora = _oracle(variant, surrogate)
    before = ora.uz_solve(n, par, xt)
    plain = ora.root_summands(n, par, xt)
    Ys = ora.root_summands(n, par, xt, with_z=True)
    assert ora._rec is None and ora._rec_z is False and np.array_equal(ora.uz_solve(n, par, xt), before)
    groups, units = _groups(variant, n, par)
    assert [Y.shape for Y in Ys] == [(N, B, 1 + D) for N, _ in groups] and all(Y.dtype == np.float64 for Y in Ys)
    assert [Y.shape for Y in plain] == [(N, B) for N, _ in groups]
    # the default result has not moved, and column 0 is it
    again = _oracle(variant, surrogate).root_summands(n, par, xt)
    for Y, P, A in zip(Ys, plain, again):
        assert np.array_equal(Y[:, :, 0], P) and np.array_equal(P, A)
    worst = 0.0
    for j, (Y, (N, summands)) in enumerate(zip(Ys, groups)):
        # the l = 0 term of MLP mode is f(0, 0) = 0 times a weight; every other term moves every component of every root
        assert np.all(Y == 0) if (j == 1 and not surrogate) else np.all(np.any(Y != 0, axis=0)), j
        for i, mine in enumerate(summands):
            owner = np.ones(units, dtype=np.uint8)
            owner[mine] = 0
            want = ora.uz_solve(n, par, xt, rank=0, world=2, owner=owner)
            assert np.all(np.isfinite(want))
            assert np.array_equal(Y[i][:, 1:], want[:, 1:]), (N, i, np.abs(Y[i] - want).max())
            worst = max(worst, float(np.abs(Y[i][:, 0] - want[:, 0]).max()))
    assert worst == 0.0, worst
    # the summands add up to the unclipped (u, z) of a two-rank solve summed over its ranks (the same addends in another order)
    uz = sum(ora.uz_solve(n, par, xt, rank=r, world=2) for r in range(2))
    total = sum(Y.sum(axis=0) for Y in Ys)
    assert np.abs(total - uz).max() <= 1e-13 * max(1.0, np.abs(uz).max())


def test_z_summands_follow_a_wrapped_root_counter_and_refuse_the_parity_modes():
    from oracle.equation import GradDependentNonlinear
    from oracle.mlp import PicardOracle
    xt = _points(D, B, 77)
    ora = _oracle("quad", False)
    Yw = ora.root_summands(2, 3, xt, root0=(1 << 32) - 1, with_z=True)
    Y0 = ora.root_summands(2, 3, xt[1:], with_z=True)
    assert all(np.array_equal(a[:, 1:], b) for a, b in zip(Yw, Y0))
    for kw in (dict(compat_crn=True), dict(compat_f16=True), dict(jax_stream=True)):
        with pytest.raises(ValueError):
            PicardOracle(GradDependentNonlinear(D + 1), "quad", seed=1, **kw).root_summands(2, 3, xt, with_z=True)
