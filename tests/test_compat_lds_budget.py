"""Registers and LDS of every instance of the matrix-core evaluation of the as-coded surrogate (csrc/gp_eval_compat_mfma.hip), from the code
object's metadata as tools/kernel_regs.py reads it.  The kernels' LDS is one static array, so the metadata states it: the ring of three stage slots
and, as coded, the 8 KiB in which the four waves park their Q fragments (compat_lds_floats).

* LDS bytes x workgroups per CU (the BPC of __launch_bounds__(256, BPC)) stay within the CU's 160 KiB, the bytes are the ones the source states,
  and no instance runs fewer workgroups per CU than it did before the parked region existed (table below, KS = 1 .. 16);
* no instance has a spilled dword or touches scratch inside a loop (a reload there would also drain the LDS-DMA prefetch behind its counted vmcnt).

Needs hipcc ($HIPCC or /opt/rocm).
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

KIB = 1024
# workgroups per CU before the Q fragments moved to LDS (ring only: 3 (KS + 2) KiB), min(register estimate, LDS), KS = 1 .. 16
BPC_BEFORE = {
    (True, 2): [4, 4, 4, 4, 4, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2],        # as coded
    (False, 2): [4, 4, 4, 4, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2],       # geometry mode, two point planes
    (False, 1): [4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 3, 3, 3, 3, 3, 2],       # geometry mode, one
}


@pytest.fixture(scope="module")
def instances():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc at %s" % hipcc)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:               # its own ISA file: other test modules compile the same source
        out = subprocess.run([sys.executable, os.path.join(root, "tools", "kernel_regs.py"), "gp_eval_compat_mfma.hip"], capture_output=True, text=True,
                             check=True, env=dict(os.environ, KERNEL_REGS_OUT=os.path.join(tmp, "gp_eval_compat_mfma.s"))).stdout
    found = []
    for line in out.splitlines():
        m = re.search(r"gp_eval_compat_mfma(_tail)?_kernel<(\d+), (\d+), (\w+), (\d+)>.*scratch\s+(\d+)\s+vgpr\s+(\d+)\s+lds\s+(\d+)\s+spill\s+(\d+)", line)
        if m:
            found.append(dict(tail=bool(m.group(1)), ks=int(m.group(2)), bpc=int(m.group(3)), r16=m.group(4) == "true", planes=int(m.group(5)),
                              scratch=int(m.group(6)), vgpr=int(m.group(7)), lds=int(m.group(8)), spill=int(m.group(9)), line=line))
    # KS = 1 .. 16 x {as coded, geometry with two planes} x {long-tail, tail-packed entry point} and the one-plane geometry kernel
    want = sorted((ks, r16, 2, tail) for ks in range(1, 17) for r16 in (False, True) for tail in (False, True)) + \
        sorted((ks, False, 1, False) for ks in range(1, 17))
    assert sorted((i["ks"], i["r16"], i["planes"], i["tail"]) for i in found) == sorted(want)
    return found


def test_lds_times_workgroups_per_cu_fits_and_no_instance_lost_a_workgroup(instances):
    for i in instances:
        ring = 3 * (i["ks"] + 2) * KIB
        assert i["lds"] == ring + (8 * KIB if i["r16"] else 0), i["line"]          # as coded: + 4 waves x 2 fragments x 64 lanes x 16 B
        assert i["lds"] * i["bpc"] <= 160 * KIB, i["line"]
        assert i["bpc"] >= BPC_BEFORE[(i["r16"], i["planes"])][i["ks"] - 1], i["line"]
        assert i["vgpr"] <= 512 // i["bpc"], i["line"]
    headline = [i for i in instances if i["r16"] and i["ks"] == 7]
    assert len(headline) == 2 and all(i["lds"] == 35 * KIB and i["bpc"] == 4 for i in headline)


def test_no_as_coded_instance_spills_or_touches_scratch(instances):
    for i in instances:
        if i["r16"]:
            assert i["spill"] == 0 and i["scratch"] == 0 and "!!" not in i["line"], i["line"]


def test_no_geometry_instance_touches_scratch_inside_a_loop(instances):
    for i in instances:
        if not i["r16"]:
            assert "!!" not in i["line"], "scratch traffic inside a loop: " + i["line"]


def test_no_geometry_instance_spills(instances):
    """The one-plane instances run four (three from KS = 10) workgroups per CU and spilled a few dwords outside loops (KS = 8, 9, 15 before the
    Q fragments moved; KS = 6, 9, 15 after): values formed in front of the prologue and read in a form's sweep or at the store.  The sweep now
    forms them again where they are read (compat_mfma_sweep, late_lane)."""
    spilled = {(i["ks"], i["planes"]): (i["spill"], i["scratch"]) for i in instances if not i["r16"] and (i["spill"] or i["scratch"])}
    assert not spilled, spilled
