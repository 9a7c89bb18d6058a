"""Registers of the kernels that store the root call's summands (picard_sum_kernel, csrc/picard_tree.hpp) from the code objects' metadata, in
the manner of tests/test_picard_registers.py: levels 1..3 of picard_tree_summands.hip (u) and picard_tree_summands_uz.hip (u, z), every
variant, mode and equation they hold.

A summand kernel keeps one address where the SE / SEZ kernels keep a term's three accumulators and the running variance, so in the same build
  * none holds more VGPRs than the SE instance (u) or the SEZ instance (u, z) of the same (variant, mode, level, equation), and
  * the equation-0 kernels have no scratch and no spilled VGPRs.
The counts are recorded in profiles/picard_summands_regs.txt.  Needs hipcc ($HIPCC or /opt/rocm).

As measured (profiles/picard_summands_regs.txt): the u kernels sit 0 .. 14 VGPRs below the SE kernels, the (u, z) kernels 7 .. 46 below the
SEZ kernels; no kernel spills, none has scratch.  What this caught: with the parity flags of scasml_rng read at run time, as the other kernels
read them, picard_sum_kernel<0, 0, 3, 0, *> (quadrature, MLP mode, n = 3) reported the 36-byte stack slot of spilled SGPRs that the level-4 MLP
kernels have -- any store inside its sample loops brought it.  The summand kernels run under flags = 0 only, so Walker::crn() / f16() are
compile-time false in them, and the slot is gone.
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

UNITS = {"picard_tree_summands.hip": r"picard_sum_kernel<(\d), (\d), (\d), (\d), 1>",
         "picard_tree_summands_uz.hip": r"picard_sum_kernel<(\d), (\d), (\d), (\d), 2>",
         "picard_tree_stderr.hip": r"picard_tree_kernel<(\d), (\d), (\d), (\d), false, true>",
         "picard_tree_stderr_uz.hip": r"picard_se_uz_kernel<(\d), (\d), (\d), (\d)>"}
TAIL = r".*scratch\s+(\d+)\s+vgpr\s+(\d+)\s+lds\s+\d+\s+spill\s+(\d+)"


def _report():
    """{unit: {(variant, mode, level, equation): (scratch, vgpr, spill, line)}} of the four translation units, compiled side by side."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        procs = {tu: subprocess.Popen([sys.executable, os.path.join(root, "tools", "kernel_regs.py"), tu], stdout=subprocess.PIPE, text=True,
                                      env=dict(os.environ, KERNEL_REGS_OUT=os.path.join(tmp, tu.replace(".hip", ".s")))) for tu in UNITS}
        outs = {tu: p.communicate()[0] for tu, p in procs.items()}
        assert all(p.returncode == 0 for p in procs.values())
    seen = {}
    for tu, pat in UNITS.items():
        seen[tu] = {}
        for line in outs[tu].splitlines():
            m = re.search(pat + TAIL, line)
            if m:
                seen[tu][tuple(int(v) for v in m.groups()[:4])] = (int(m.group(5)), int(m.group(6)), int(m.group(7)), line)
    return seen


def test_summand_kernels_hold_no_more_registers_than_the_fused_estimates_and_no_scratch():
    seen = _report()
    # levels 1..3, both variants, MLP (0) and ACCUMULATE (2): equations 0, 1 and, surrogate-free only, 2
    want = sorted((v, mode, n, eq) for v in (0, 1) for mode in (0, 2) for n in (1, 2, 3) for eq in ((0, 1, 2) if mode == 0 else (0, 1)))
    failures = []
    for sums, fused in (("picard_tree_summands.hip", "picard_tree_stderr.hip"), ("picard_tree_summands_uz.hip", "picard_tree_stderr_uz.hip")):
        assert sorted(seen[sums]) == want and sorted(seen[fused]) == want, (sums, sorted(seen[sums]))
        for key in want:
            scratch, vgpr, spill, line = seen[sums][key]
            print(line, "  (fused: %d VGPRs)" % seen[fused][key][1])
            if vgpr > seen[fused][key][1]:
                failures.append("%s: the fused kernel holds %d VGPRs" % (line, seen[fused][key][1]))
            if spill != 0 or "!!" in line:
                failures.append("%s: spills" % line)
            if key[3] == 0 and scratch != 0:
                failures.append("%s: scratch" % line)
    assert not failures, "\n".join(failures)
