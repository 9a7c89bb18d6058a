"""Check (b) of tests/test_gpu_stderr_uz_sweep.py without a GPU: a float32 emulation of SeTerm4 (csrc/picard_tree.hpp: add, and close_into with
its `scale` argument) on the oracle's z summands stays inside the bound that the sweep derives, and the bound is not vacuous.

The emulation is given what the kernel accumulates: for the terminal term the UNSCALED P_m = g nrm_m in float32, closed with fl(zs zs); for a
level's term the float32 summands, closed with 1.  The yardstick is given what the sweep's sharded launches return: fl(P_m zs) and the same level
summands, all in float32, with se64 formed from them in float64.  So the two sides differ by exactly what the derivation accounts for under B_var
and by the one rounding of fl(P_m zs) under B_Y, and by nothing else: the emulation must stay inside B_var + the share 1 / 6 of the terminal
term's B_Y, which is sharper than the sweep's whole bound.  One root of every batch lies at T - t = 1e-5, where every sample of g nearly
coincides, the terminal scale is 1e5 / mg (quadrature: 1 / (mg (1e-5 + 1e-6))) and the deviations dv carry few significant bits."""
import numpy as np
import pytest

from test_gpu_picard_sweep import _points
from test_gpu_stderr_sweep import EPS, _SweepSurrogate
from test_gpu_stderr_uz_sweep import K_TERMINAL, emulate_float32_z, se_stats_z

D, B, NEAR = 6, 16, 0


def _summands(variant, n, par, surrogate):
    """-> (P (mg, B, d) float32, zs (B,) float32, [level summands (N, B, d) float32]) from the oracle's one walk."""
    from oracle.equation import GradDependentNonlinear
    from oracle.mlp import PicardOracle
    f32 = np.float32
    xt = _points(D, B, 78)
    xt[NEAR, -1] = f32(0.5 - 1e-5)
    ora = PicardOracle(GradDependentNonlinear(D + 1), variant, gp=_SweepSurrogate(D) if surrogate else None, seed=7, stream=3)
    Ys = ora.root_summands(n, par, xt, with_z=True)
    mg = Ys[0].shape[0]
    tau = np.float64(0.5) - xt[:, -1].astype(np.float64)
    scale = mg * (tau + (1e-6 if variant == "quad" else 0.0))                       # the oracle's terminal summand is G N / scale
    P = (Ys[0][:, :, 1:] * scale[None, :, None]).astype(f32)
    zs = (f32(1.0 / mg) * (f32(1) / (tau + (1e-6 if variant == "quad" else 0.0)).astype(f32))).astype(f32)   # inv_mg * rcp(tau + eps), in float32
    return P, zs, [Y[:, :, 1:].astype(f32) for Y in Ys[1:]]


@pytest.mark.parametrize("surrogate", [False, True], ids=["mlp", "surrogate"])
@pytest.mark.parametrize("variant,n,par", [("quad", 2, 3), ("quad", 3, 3), ("fh", 2, 3), ("fh", 3, 2), ("fh", 4, 2)])
def test_a_float32_emulation_of_the_z_accumulation_stays_inside_the_derived_bound(variant, n, par, surrogate):
    P, zs, levels = _summands(variant, n, par, surrogate)
    device = [(P * zs[None, :, None]).astype(np.float32)] + levels                  # the sharded launch's summands: fl(P_m zs)
    assert all(Y.dtype == np.float32 for Y in device)
    st = se_stats_z([Y.astype(np.float64) for Y in device])
    var32 = emulate_float32_z([P] + levels, zs[:, None])
    assert var32.dtype == np.float32 and var32.shape == (B, D)
    se32 = np.sqrt(np.maximum(var32, np.float32(0))).astype(np.float64)              # the kernel's final store: sqrtf
    var, se = st["var"], st["se"]
    assert np.all(var > 0) and np.all(np.isfinite(var))
    # what the emulation can use of the bound: B_var and the rounding of fl(P_m zs), 1 of the terminal term's K_TERMINAL
    N = P.shape[0]
    y_g = EPS * np.sqrt(N / (N - 1.0) * (device[0].astype(np.float64) ** 2).sum(axis=0))
    b = st["b_var_z"]
    sharp = np.maximum(np.sqrt(var + b) - se, se - np.sqrt(np.maximum(var - b, 0.0))) + y_g
    err = np.abs(se32 - se)
    far = np.arange(B) != NEAR
    print("%s n=%d: |se32 - se64| / sharp bound %.3f (near T %.3f), bound / se %.1e..%.1e (near T %.1e..%.1e)" % (
        variant, n, (err / sharp)[far].max(), (err / sharp)[NEAR].max(), (st["bound_z"] / se)[far].min(), (st["bound_z"] / se)[far].max(),
        (st["bound_z"] / se)[NEAR].min(), (st["bound_z"] / se)[NEAR].max()))
    assert np.all(sharp <= st["bound_z"]) and np.all(y_g * K_TERMINAL <= st["bound_z"] + 1e-300)
    assert np.all(err <= sharp), (err / sharp).max()
    # not vacuous: the whole bound of check (b) is below 1e-4 of se_z, a hundredth of what check (a) allows, within 1e-5 of T too
    assert np.all(st["bound_z"] <= 1e-4 * se)


def test_close_into_scales_the_terminal_term_by_the_square_of_its_scale():
    """The emulation itself: two summands per term, by hand.  The variance of the SUM P_0 + P_1 is 2 ((P_0 - mean)^2 + (P_1 - mean)^2) = (P_1 - P_0)^2, times zs^2;
    a level's term has scale 1."""
    f32 = np.float32
    P = np.array([[1.0], [3.0]], dtype=f32)
    L = np.array([[0.5], [0.25]], dtype=f32)
    zs = np.array([0.5], dtype=f32)
    assert emulate_float32_z([P], zs)[0] == f32(4.0 * 0.25)
    assert emulate_float32_z([P, L], zs)[0] == f32(4.0 * 0.25 + 0.0625)
    assert emulate_float32_z([P, L], f32(2) * zs)[0] == f32(4.0 + 0.0625)
