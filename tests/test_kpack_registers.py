"""Registers of the tail-packed entry point of the as-coded evaluation (csrc/gp_eval_compat_mfma.hip, gp_eval_compat_mfma_tail_kernel), from the
code object's metadata: what tests/test_abi_and_host.py pins for the long-tail entry point, for the one the headline runs.

The launch table sets __launch_bounds__(256, BPC) from the long-tail register estimate for both column maps, and the packed map only frees
registers (the four of the last low-plane fragment), yet the allocation of these kernels moves with every change of the prologue: every as-coded
instance must still fit its bound WITHOUT scratch (KS = 7, the headline's, sits at the 128 of four workgroups per CU), and no instance may touch
scratch inside a loop: a reload there would also drain the LDS-DMA prefetch behind its counted vmcnt.  Needs hipcc ($HIPCC or /opt/rocm).
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest


def test_tail_packed_instances_hold_their_launch_bounds_without_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:               # its own ISA file: tests/test_abi_and_host.py compiles the same source
        out = subprocess.run([sys.executable, os.path.join(root, "tools", "kernel_regs.py"), "gp_eval_compat_mfma.hip"], capture_output=True, text=True,
                             check=True, env=dict(os.environ, KERNEL_REGS_OUT=os.path.join(tmp, "gp_eval_compat_mfma.s"))).stdout
    seen = {}
    for line in out.splitlines():
        m = re.search(r"gp_eval_compat_mfma_tail_kernel<(\d+), (\d+), (\w+), (\d+)>.*scratch\s+(\d+)\s+vgpr\s+(\d+)", line)
        if not m:
            continue
        ks, bpc, r16, planes, scratch, vgpr = int(m.group(1)), int(m.group(2)), m.group(3) == "true", int(m.group(4)), int(m.group(5)), int(m.group(6))
        seen[(ks, r16, planes)] = (bpc, vgpr)
        assert "!!" not in line, "scratch traffic inside a loop: " + line
        assert vgpr <= 512 // bpc, line                      # 512 VGPRs per SIMD lane, one 256-thread workgroup = one wave per SIMD
        assert scratch == 0 if r16 else scratch <= 32, line  # as tests/test_abi_and_host.py holds the long-tail entry point
    # KS = 1..16 x {as coded, geometry with 2 planes}; with one plane packing saves no MFMA and the long-tail kernel reads either map
    assert sorted(seen) == sorted((ks, r16, 2) for ks in range(1, 17) for r16 in (False, True))
    assert seen[(7, True, 2)][0] == 4 and seen[(7, True, 2)][1] <= 128       # the headline instance: four workgroups per CU
    assert all(bpc == 4 for (ks, r16, planes), (bpc, _) in seen.items() if r16 and ks <= 7)
