"""Host side of the staged tree's standard errors (scasml_picard_stage_stderr): the header and the binding declare the entry, the ABI version
stays 7, every refusal of the entry fails alone with its message (none needs a GPU: a refused call launches nothing), the standard-error
instances of picard_stage_kernel hold no scratch while the plain ones keep the register figures they had before the template gained its flag
(profiles/picard_stage_stderr_regs.txt), and the bound of check (b) of tests/test_gpu_stage_stderr_sweep.py holds for a float32 emulation of the
accumulators on this equation's magnitudes.  The register test needs hipcc ($HIPCC or /opt/rocm)."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_gpu_picard_sweep import _G, _points, _ragged
from test_gpu_stage_stderr_sweep import ROOT0, SE_CASES, SEED, STREAM, _Steep
from test_gpu_stderr_uz_sweep import emulate_float32_z, se_stats_z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -2
# picard_stage_kernel<VAR> before the flag: VAR -> (vgpr, sgpr, scratch bytes), as the compiler reports them (profiles/picard_stage_stderr_regs.txt)
PLAIN_BEFORE = {0: (61, 56, 0), 1: (58, 70, 0)}


def test_header_declares_the_entry_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "scasml_hip.h")).read()
    assert re.search(r"#define SCASML_ABI_VERSION 7\b", text)
    m = re.search(r"int scasml_picard_stage_stderr\(([^;]*)\);", text)
    assert m, "include/scasml_hip.h does not declare scasml_picard_stage_stderr"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["prob_h", "plan_h", "stage", "entries", "n_entries", "B", "site_stride", "rng", "points", "values",
                                                         "out_uz", "out_se_uz", "stream"]
    assert "float *out_se_uz" in args and "float *out_uz" in args
    # the argument list of scasml_picard_stage with `uz` dropped and the new output after out_uz
    plain = re.search(r"int scasml_picard_stage\(([^;]*)\);", text)
    want = [a.strip() for a in " ".join(plain.group(1).split()).split(",")]
    want.remove("float *uz")
    want.insert(want.index("float *out_uz") + 1, "float *out_se_uz")
    assert args == want


def test_binding_declares_the_entry_with_the_arity_of_the_header():
    from scasml_gp_amd import _lib
    assert _lib.ABI_VERSION == 7
    res, args = _lib.SIGNATURES["scasml_picard_stage_stderr"]
    plain_res, plain_args = _lib.SIGNATURES["scasml_picard_stage"]
    assert res is plain_res and len(args) == 13 and args == plain_args          # one pointer fewer (uz), one more (out_se_uz)
    assert _lib.load().scasml_abi_version() == 7


# ------------------------------------------------------------------------------------------------------------- refusals
def _call(**kw):
    """scasml_picard_stage_stderr on quadrature n = 2, rho = 3 at d = 10, B = 4, with every argument in order unless ``kw`` replaces it.  Host
    memory stands in for the device buffers: a refused call reads none of them.  -> (return code, message)."""
    from scasml_gp_amd import _lib, tables
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    a = dict(prob=_lib.Problem(10, 0, 0.5, 0.0, 0.25, 1.0), plan=tables.build_plan("quad", 2, 3, 0.5, True), stage=2, entries=p, n_entries=1, B=4,
             site_stride=0, rng=_lib.Rng(0, 0, 0, 0, 1, 0, 0), points=p, values=p, out_uz=p, out_se_uz=p)
    a.update(kw)
    ref = lambda v: None if v is None else C.byref(v)
    rc = lib.scasml_picard_stage_stderr(ref(a["prob"]), ref(a["plan"]), a["stage"], a["entries"], a["n_entries"], a["B"], a["site_stride"], a["rng"],
                                        a["points"], a["values"], a["out_uz"], a["out_se_uz"], None)
    assert np.all(buf == 0)
    return rc, lib.scasml_last_error().decode()


def _plan(variant="quad", n=2, par=3, fields=()):
    from scasml_gp_amd import tables
    plan = tables.build_plan(variant, n, par, 0.5, True)
    for k, v in dict(fields).items():
        setattr(plan, k, v)
    return plan


def _refusals():
    from scasml_gp_amd import _lib
    prob = lambda d: _lib.Problem(d, 0, 0.5, 0.0, 0.25, 1.0)
    one_terminal = _plan()
    one_terminal.mg[2] = 1
    no_node = _plan()
    no_node.term[1][0].q = 0
    return [
        # those of scasml_picard_stage, in its order
        (dict(prob=None), ERR_ARG, "null argument"),
        (dict(plan=None), ERR_ARG, "null argument"),
        (dict(B=-1), ERR_ARG, "negative batch"),
        (dict(site_stride=3), ERR_ARG, "site_stride 3 is smaller than the batch 4"),
        (dict(prob=prob(0)), ERR_UNSUPPORTED, "d=0 outside 1.."),
        (dict(prob=prob(_lib.MAX_DIM + 1)), ERR_UNSUPPORTED, "d=%d outside 1.." % (_lib.MAX_DIM + 1)),
        (dict(plan=_plan(fields=dict(variant=2))), ERR_ARG, "variant 2"),
        (dict(plan=_plan(fields=dict(n=_lib.MAX_LEVEL + 1))), ERR_UNSUPPORTED, "level n=%d outside 1..%d" % (_lib.MAX_LEVEL + 1, _lib.MAX_LEVEL)),
        (dict(stage=0), ERR_ARG, "stage 0 outside 1..2"),
        (dict(stage=3), ERR_ARG, "stage 3 outside 1..2"),
        (dict(rng=_lib.Rng(0, 0, 0, 0, 1, _lib.RNG_COMPAT_CRN, 0)), ERR_UNSUPPORTED, "the staged path runs on the Philox stream only"),
        (dict(rng=_lib.Rng(0, 0, 0, 0, 2, 0, 0)), ERR_UNSUPPORTED, "sample sharding (world 2) is not supported"),
        (dict(n_entries=0), ERR_ARG, "no subtree entries"),
        (dict(entries=None), ERR_ARG, "no subtree entries"),
        (dict(plan=no_node), ERR_ARG, "bad term [1][0]"),
        (dict(points=None), ERR_ARG, "points and values are required"),
        (dict(values=None), ERR_ARG, "points and values are required"),
        # its own
        (dict(stage=1), ERR_ARG, "only the root call has an estimate"),
        (dict(out_uz=None), ERR_ARG, "out_uz is null"),
        (dict(out_se_uz=None), ERR_ARG, "out_se_uz is null"),
        (dict(plan=one_terminal), ERR_UNSUPPORTED, "the terminal term of level 2 has 1 sample: no estimable variance"),
        (dict(plan=_plan(par=2)), ERR_UNSUPPORTED, "term [2][1] has 1 sample path: no estimable variance"),
        (dict(plan=_plan("fh", 2, 1)), ERR_UNSUPPORTED, "no estimable variance"),
        (dict(site_stride=1 << 28), ERR_UNSUPPORTED, "too large for 32-bit row offsets"),
    ]


def test_every_refusal_fails_alone_with_its_message():
    assert _plan().mg[2] >= 2 and all(_plan().term[2][l].mc >= 2 for l in range(2))
    for kw, code, text in _refusals():
        rc, msg = _call(**kw)
        assert rc == code and msg.startswith("picard_stage_stderr: ") and text in msg, (sorted(kw), rc, msg)


def test_the_one_sample_refusals_are_worded_as_the_tree_entry_words_them():
    """scasml_picard_tree_stderr on the same plans (refused before x_t is read): the same text after the entry's prefix."""
    from scasml_gp_amd import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    one_terminal = _plan()
    one_terminal.mg[2] = 1
    for plan in (one_terminal, _plan(par=2)):
        prob = _lib.Problem(10, 0, 0.5, 0.0, 0.25, 1.0)
        assert lib.scasml_picard_tree_stderr(C.byref(prob), C.byref(plan), _lib.MODE_MLP, p, 4, 0, _lib.Rng(0, 0, 0, 0, 1, 0, 0), None, None, p, None, p,
                                             None) == ERR_UNSUPPORTED
        tree = lib.scasml_last_error().decode()
        rc, msg = _call(plan=plan)
        assert rc == ERR_UNSUPPORTED and tree.startswith("picard_tree_stderr: ")
        assert msg[len("picard_stage_stderr: "):] == tree[len("picard_tree_stderr: "):]


def test_an_empty_batch_does_nothing_whatever_the_pointers():
    assert _call(B=0)[0] == 0
    assert _call(B=0, points=None, values=None, out_uz=None, out_se_uz=None, site_stride=8)[0] == 0


def test_the_engine_applies_the_one_sample_rule_to_callback_equations_without_a_gpu():
    """stderr_supported is the rule of every solve; PicardEngine.solve raises its ValueError for a callback equation too (on the GPU:
    tests/test_gpu_callback_stderr.py)."""
    from scasml_gp_amd.solvers._picard import PicardEngine

    class Callbacks:
        eq_id, torch_callbacks, n_input, T = None, True, 7, 0.5
        mu = sigma = staticmethod(lambda x_t=0: 0.25)
    eng = PicardEngine(Callbacks(), "quad")
    assert eng.callbacks and eng.stderr_supported(2, 2)[0] is False and "term [2][1]" in eng.stderr_supported(2, 2)[1]
    assert eng.stderr_supported(2, 3) == (True, "")


# ------------------------------------------------------------------------------------------------------------- registers
def test_se_instances_hold_no_scratch_and_the_plain_instances_keep_their_figures():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    with tempfile.TemporaryDirectory() as tmp:
        isa = os.path.join(tmp, "picard_staged.s")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "picard_staged.hip"], capture_output=True, text=True, check=True,
                             env=dict(os.environ, KERNEL_REGS_OUT=isa)).stdout
        text = open(isa).read()
    sgpr = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)", text):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        sgpr[name.split("(")[0]] = (int(m.group(2)), int(m.group(3)))
    seen = {}
    for line in out.splitlines():
        m = re.search(r"(picard_stage_kernel<(\d+), (true|false)>).*scratch\s+(\d+)\s+vgpr\s+(\d+)\s+lds\s+\d+\s+spill\s+(\d+)", line)
        assert m, "a kernel of another template in picard_staged.hip: " + line
        assert "!!" not in line, line
        full = [k for k in sgpr if k.endswith(m.group(1))]
        assert len(full) == 1, (m.group(1), sorted(sgpr))
        seen[(int(m.group(2)), m.group(3) == "true")] = (int(m.group(5)), sgpr[full[0]][0], int(m.group(4)), int(m.group(6)), sgpr[full[0]][1])
    assert sorted(seen) == [(0, False), (0, True), (1, False), (1, True)]
    for (var, se), (vgpr, sg, scratch, spill, sspill) in sorted(seen.items()):
        print("picard_stage_kernel<%d, %s> vgpr %d sgpr %d scratch %d spill %d sgpr spill %d" % (var, str(se).lower(), vgpr, sg, scratch, spill, sspill))
        if se:
            assert scratch == 0 and spill == 0 and sspill == 0, (var, seen[(var, se)])
        else:
            assert (vgpr, sg, scratch) == PLAIN_BEFORE[var] and spill == 0 and sspill == 0, (var, seen[(var, se)])


# ------------------------------------------------------------------------------------------------------------- the bound of check (b)
@pytest.mark.parametrize("d,case", [(6, 1), (43, 1), (139, 0)], ids=["G04-d6", "G16-d43", "G64-d139"])
def test_a_float32_emulation_of_the_accumulators_stays_inside_the_bound_of_check_b(d, case):
    """tests/test_picard_stderr_uz_emulation.py's comparison on _Steep's oracle summands of three sweep cases, all 1 + d columns: the emulation
    is given what the kernel accumulates (the unscaled g_m and P_m = g_m nrm_m, closed with inv_mg^2 and zs^2; the level summands, closed with 1),
    the yardstick what the masked launches of check (b) return (fl(g_m inv_mg), fl(P_m zs) and the same level summands)."""
    from oracle.mlp import PicardOracle
    f32, f64 = np.float32, np.float64
    variant, n, par = SE_CASES[d][case]
    assert sorted({_G(6), _G(43), _G(139)}) == [4, 16, 64]
    xt = _points(d, _ragged(d)[-1], seed=3100 + d)
    Ys = PicardOracle(_Steep(d + 1), variant, seed=SEED, stream=STREAM).root_summands(n, par, xt, root0=ROOT0, with_z=True)
    mg = Ys[0].shape[0]
    tau = f64(0.5) - xt[:, -1].astype(f32).astype(f64)
    eps = 1e-6 if variant == "quad" else 0.0
    scale = np.concatenate([np.full((len(tau), 1), float(mg)), np.repeat((mg * (tau + eps))[:, None], d, axis=1)], axis=1)      # (B, 1 + d)
    P = (Ys[0] * scale[None]).astype(f32)                                                # g_m, then g_m nrm_m
    zs = (f32(1.0 / mg) * (f32(1) / (tau + eps).astype(f32))).astype(f32)
    close = np.concatenate([np.full((len(tau), 1), f32(1.0 / mg)), np.repeat(zs[:, None], d, axis=1)], axis=1).astype(f32)
    levels = [Y.astype(f32) for Y in Ys[1:]]
    device = [(P * close[None]).astype(f32)] + levels
    st = se_stats_z([Y.astype(f64) for Y in device])
    var32 = emulate_float32_z([P] + levels, close)
    assert var32.dtype == f32 and var32.shape == (len(tau), d + 1)
    se32 = np.sqrt(np.maximum(var32, f32(0))).astype(f64)
    err = np.abs(se32 - st["se"])
    print("%s n=%d d=%d: |se32 - se64| / bound_z at most %.3f, bound_z / se %.1e..%.1e" % (variant, n, d, (err / st["bound_z"]).max(),
                                                                                          (st["bound_z"] / st["se"]).min(), (st["bound_z"] / st["se"]).max()))
    assert np.all(st["var"] > 0) and np.all(np.isfinite(st["var"]))
    assert np.all(err <= st["bound_z"]), (err / st["bound_z"]).max()
    assert np.all(st["bound_z"] <= 1e-4 * st["se"])                                      # not vacuous: a hundredth of what check (a) allows
