"""Host side of the Picard standard errors (scasml_picard_tree_stderr): the header and the binding declare the entry, the ABI version stays 7,
PicardEngine.stderr_supported answers from the plan without a GPU, and the kernels of the new translation units (csrc/picard_tree_stderr.hip,
csrc/picard_tree_stderr_deep.hip) stay inside the register, scratch and loop figures of the plain instances of csrc/picard_tree.hip.

The baseline is what tools/kernel_regs.py prints for picard_tree.hip (profiles/picard_stderr_regs.txt): for n <= 4 every plain MLP and ACCUMULATE
instance has 0 bytes of scratch except the quadrature MLP kernels of n = 4 (36 bytes: the stack slot of six spilled SGPRs), and
none touches scratch inside a loop.  The quadrature instances of n = 5 spill already (3568 bytes): their figures are recorded, not bounded.
Needs hipcc ($HIPCC or /opt/rocm)."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE_MLP, MODE_ACCUMULATE = 0, 2


def _plain_scratch(var, mode, n, eq):
    """Scratch bytes of picard_tree_kernel<var, mode, n, eq> without the flag, n <= 4 (profiles/picard_stderr_regs.txt)."""
    return 36 if (var == 0 and mode == MODE_MLP and n == 4) else 0


def test_header_declares_the_entry_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", text)
    m = re.search(r"int scasml_picard_tree_stderr\(([^;]*)\);", text)
    assert m, "include/scasml_hip.h does not declare scasml_picard_tree_stderr"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["prob_h", "plan_h", "mode", "x_t", "B", "site_stride", "rng", "points", "gp_vals", "out_uz",
                                                         "out_uhat", "out_se", "stream"]
    assert "float *out_se" in args


def test_binding_declares_the_entry_as_the_plain_one_plus_out_se():
    import ctypes as C
    from scasml_gp_amd import _lib
    assert _lib.ABI_VERSION == 7
    res, args = _lib.SIGNATURES["scasml_picard_tree_stderr"]
    plain_res, plain_args = _lib.SIGNATURES["scasml_picard_tree"]
    assert res is plain_res and args == plain_args[:-1] + [C.c_void_p] + plain_args[-1:]


def test_sources_of_the_build_hold_the_new_translation_units():
    from scasml_gp_amd import _build
    for name in ("picard_tree_stderr.hip", "picard_tree_stderr_deep.hip"):
        assert name in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, name))


def _engine(variant):
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.solvers._picard import PicardEngine
    eq = Grad_Dependent_Nonlinear(21)
    eq.geometry()                                        # sets T, as the solver classes do before they build their engine
    return PicardEngine(eq, variant)


@pytest.mark.parametrize("n,rho,ok", [(0, 3, True), (1, 3, True), (2, 3, True), (3, 3, True), (2, 4, True), (4, 4, True), (5, 5, True),
                                      (1, 2, False), (2, 2, False), (1, 1, False)])
def test_stderr_supported_quadrature_plans_without_a_gpu(n, rho, ok):
    got, why = _engine("quad").stderr_supported(n, rho)
    assert got is ok
    assert why == "" if ok else "no estimable variance" in why


def test_stderr_supported_names_the_one_sample_term():
    # n = rho = 2: Mf = (1, 2), so the TOP term l = 1 has one sample path; n = 1 at rho = 2: term l = 0
    assert "term [2][1]" in _engine("quad").stderr_supported(2, 2)[1]
    assert "term [1][0]" in _engine("quad").stderr_supported(1, 2)[1]


@pytest.mark.parametrize("n,M,ok", [(0, 1, True), (1, 2, True), (2, 3, True), (4, 3, True), (5, 2, True), (1, 1, False), (3, 1, False)])
def test_stderr_supported_full_history_plans_without_a_gpu(n, M, ok):
    got, why = _engine("fh").stderr_supported(n, M)
    assert got is ok and (why == "") is ok


def _kernel_regs(source, tmp):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), source], capture_output=True, text=True, check=True,
                          env=dict(os.environ, KERNEL_REGS_OUT=os.path.join(tmp, source.replace(".hip", ".s")))).stdout


def test_standard_error_instances_stay_inside_the_plain_scratch_and_loop_figures():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=2) as ex:
        out = "".join(ex.map(lambda src: _kernel_regs(src, tmp), ["picard_tree_stderr.hip", "picard_tree_stderr_deep.hip"]))
    seen = {}
    for line in out.splitlines():
        m = re.search(r"picard_tree_kernel<(\d+), (\d+), (\d+), (\d+), false, true>.*scratch\s+(\d+)\s+vgpr\s+(\d+)", line)
        if not m:
            assert "picard_tree_kernel" not in line, "an instance without the flag in a standard-error translation unit: " + line
            continue
        var, mode, n, eq, scratch, vgpr = (int(g) for g in m.groups())
        seen[(var, mode, n, eq)] = (scratch, vgpr, "!!" in line)
        if n <= 4:
            assert scratch <= _plain_scratch(var, mode, n, eq), line
            assert "!!" not in line, "scratch traffic inside a loop where the plain instance has none: " + line
        assert vgpr <= 512, line
    # VAR 0/1 x {MLP, ACCUMULATE} x N = 1..5 x equations 0 and 1, and equation 2 (f of |z|^2) in MLP only
    want = [(var, mode, n, eq) for var in (0, 1) for mode in (MODE_MLP, MODE_ACCUMULATE) for n in range(1, 6) for eq in (0, 1)]
    want += [(var, MODE_MLP, n, 2) for var in (0, 1) for n in range(1, 6)]
    assert sorted(seen) == sorted(want)
    # the full-history instances of n = 5 do not spill without the flag (0 bytes) and must not with it
    assert all(seen[(1, mode, 5, eq)][0] == 0 and not seen[(1, mode, 5, eq)][2] for mode in (MODE_MLP, MODE_ACCUMULATE) for eq in (0, 1))
    for key in sorted(k for k in seen if k[0] == 0 and k[2] == 5):
        print("quadrature n = 5 (spills without the flag too): <%d, %d, 5, %d> scratch %d vgpr %d" % (key[0], key[1], key[3], seen[key][0], seen[key][1]))


# ---- the oracle's one-walk summands (PicardOracle.root_summands) and the rounding bound of tests/test_gpu_stderr_sweep.py ----------------
def _summand_oracle(variant, surrogate, d=6, seed=7, stream=3):
    from oracle.equation import GradDependentNonlinear
    from oracle.mlp import PicardOracle
    from test_gpu_picard_sweep import _Surrogate
    return PicardOracle(GradDependentNonlinear(d + 1), variant, gp=_Surrogate(d) if surrogate else None, seed=seed, stream=stream)


@pytest.mark.parametrize("surrogate", [False, True], ids=["mlp", "surrogate"])
@pytest.mark.parametrize("variant,n,par", [("quad", 2, 3), ("quad", 3, 3), ("fh", 2, 3), ("fh", 3, 2)])
def test_root_summands_are_the_owner_mask_summands_from_one_walk(variant, n, par, surrogate):
    """Summand by summand against uz_solve(..., world=2, owner=...) with one summand's units marked (one walk per summand), to 1e-15; the
    summands add up to the unclipped u of a two-rank solve summed over its ranks; uz_solve itself is undisturbed by the recording."""
    import numpy as np
    from test_gpu_picard_stderr import _groups
    from test_gpu_picard_sweep import _points
    d, B = 6, 3
    xt = _points(d, B, 77)
    ora = _summand_oracle(variant, surrogate)
    before = ora.uz_solve(n, par, xt)
    Ys = ora.root_summands(n, par, xt)
    assert ora._rec is None and np.array_equal(ora.uz_solve(n, par, xt), before, equal_nan=True)
    groups, units = _groups(variant, n, par)
    assert [Y.shape for Y in Ys] == [(N, B) for N, _ in groups] and all(Y.dtype == np.float64 for Y in Ys)
    for Y, (N, summands) in zip(Ys, groups):
        for i, mine in enumerate(summands):
            owner = np.ones(units, dtype=np.uint8)
            owner[mine] = 0
            want = ora.uz_solve(n, par, xt, rank=0, world=2, owner=owner)[:, 0]
            assert np.abs(Y[i] - want).max() <= 1e-15, (N, i, np.abs(Y[i] - want).max())
    u = sum(ora.uz_solve(n, par, xt, rank=r, world=2)[:, 0] for r in range(2))
    total = sum(Y.sum(axis=0) for Y in Ys)
    assert np.abs(total - u).max() <= 1e-14 * max(1.0, np.abs(u).max())     # the same addends in another order
    # a wrapped root counter reaches the summands as it reaches uz_solve
    Yw = ora.root_summands(n, par, xt, root0=(1 << 32) - 1)
    assert np.abs(Yw[0][:, 1:] - ora.root_summands(n, par, xt[1:])[0]).max() == 0.0


def test_root_summands_refuses_the_parity_modes():
    import numpy as np
    from oracle.equation import GradDependentNonlinear
    from oracle.mlp import PicardOracle
    xt = np.zeros((1, 7))
    for kw in (dict(compat_crn=True), dict(compat_f16=True), dict(jax_stream=True)):
        with pytest.raises(ValueError):
            PicardOracle(GradDependentNonlinear(7), "quad", seed=1, **kw).root_summands(2, 3, xt)


@pytest.mark.parametrize("surrogate", [False, True], ids=["mlp", "surrogate"])
@pytest.mark.parametrize("variant,n,par", [("quad", 3, 3), ("fh", 3, 2), ("fh", 4, 2)])
def test_a_float32_emulation_of_the_accumulation_stays_inside_the_derived_bound(variant, n, par, surrogate):
    """B_var of tests/test_gpu_stderr_sweep.py (check (b)) against a float32 emulation of SeTerm on the oracle's summands rounded to float32:
    the emulation stays inside the bound (it is not too tight) and the bound is a few 1e-6 of Var (it is not vacuous)."""
    import numpy as np
    from test_gpu_picard_sweep import _points
    from test_gpu_stderr_sweep import emulate_float32, se_stats
    xt = _points(6, 16, 78)
    Ys = [Y.astype(np.float32).astype(np.float64) for Y in _summand_oracle(variant, surrogate).root_summands(n, par, xt)]
    st = se_stats(Ys)
    err = np.abs(emulate_float32(Ys).astype(np.float64) - st["var"])
    print("%s n=%d: |Var32 - Var64| / Var %.1e..%.1e, B_var / Var %.1e..%.1e" % (variant, n, (err / st["var"]).min(), (err / st["var"]).max(),
                                                                                (st["b_var"] / st["var"]).min(), (st["b_var"] / st["var"]).max()))
    assert np.all(st["var"] > 0) and np.all(err <= st["b_var"])
    assert np.all(st["b_var"] <= 1e-4 * st["var"])
    # and of se: the whole bound of check (b) is below 1e-4 of se, a hundredth of what check (a) allows
    assert np.all(st["bound_b"] <= 1e-4 * st["se"])
