"""Registers of the Picard tree kernels (csrc/picard_tree.hpp) from the code object's metadata, as tests/test_kpack_registers.py reads the evaluation
kernel's: the equation-0 GENERATE, ACCUMULATE and MLP kernels of levels 1..3, both variants, plain and with standard errors.

The sum over dims in registers (group_sum: DPP and one swizzle instead of a loop of ds_bpermute) and ACCUMULATE's level-0 nodes without their
"+" addend must not cost registers: no kernel may hold more VGPRs than the commit before them did (PARENT below, read off that commit's code
objects with the same tool), none may pass 128 (four waves per SIMD; ACCUMULATE n = 3 sat at 112), and none of these levels has scratch (the
stack slot of six spilled SGPRs that rocprof reports as 36 bytes belongs to the level-4 MLP and GENERATE kernels).  Needs hipcc ($HIPCC or /opt/rocm).

What this caught: with the o = 32 step as the first case of group_sum's switch the MLP-mode kernels of quadrature n = 2 held 82 (the parent 81) and,
with standard errors, 94 (93); with that step in front of the switch they are at 80 and 92, but ACCUMULATE with standard errors goes from 94 to 101.
group_sum puts the step where each mode loses nothing (profiles/r09_picard_dim_sum_ab.txt, "Registers").
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

MLP, GEN, ACC = 0, 1, 2
# (variant, mode, SE) -> VGPRs at levels 1, 2, 3 on the parent commit
PARENT = {(0, MLP, False): (46, 81, 107), (1, MLP, False): (62, 80, 103),
          (0, GEN, False): (48, 54, 68), (1, GEN, False): (48, 50, 57),
          (0, ACC, False): (63, 90, 112), (1, ACC, False): (66, 90, 113),
          (0, MLP, True): (54, 93, 122), (1, MLP, True): (70, 92, 119),
          (0, ACC, True): (63, 94, 128), (1, ACC, True): (76, 103, 129)}


def test_tree_kernels_hold_no_more_registers_than_before_and_no_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:               # the two translation units side by side, each its own ISA file
        procs = [subprocess.Popen([sys.executable, os.path.join(root, "tools", "kernel_regs.py"), tu], stdout=subprocess.PIPE, text=True,
                                  env=dict(os.environ, KERNEL_REGS_OUT=os.path.join(tmp, tu.replace(".hip", ".s"))))
                 for tu in ("picard_tree.hip", "picard_tree_stderr.hip")]
        outs = [p.communicate()[0] for p in procs]
        assert all(p.returncode == 0 for p in procs)
    seen = {}
    for line in "\n".join(outs).splitlines():
        m = re.search(r"picard_tree_kernel<(\d), (\d), (\d), 0, false, (\w+)>.*scratch\s+(\d+)\s+vgpr\s+(\d+)\s+lds\s+\d+\s+spill\s+(\d+)", line)
        if not m or int(m.group(3)) > 3:
            continue
        var, mode, n, se = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == "true"
        scratch, vgpr, spill = int(m.group(5)), int(m.group(6)), int(m.group(7))
        seen[(var, mode, se, n)] = vgpr
        assert "!!" not in line and scratch == 0 and spill == 0, line
        assert vgpr <= min(PARENT[(var, mode, se)][n - 1], 128), "%s: the parent commit held %d" % (line, PARENT[(var, mode, se)][n - 1])
    assert sorted(seen) == sorted(k + (n,) for k in PARENT for n in (1, 2, 3))
    assert seen[(0, ACC, False, 3)] <= 112                   # the headline's ACCUMULATE
