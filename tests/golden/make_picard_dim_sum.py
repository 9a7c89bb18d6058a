#!/usr/bin/env python
"""Writes tests/golden/picard_dim_sum_parent.npz: what scasml_picard_tree and scasml_picard_tree_stderr return on an MI355X for the cases of
tests/test_gpu_picard_dim_sum.py (which holds the cases, the inputs and the launches; this file only runs them and saves the results).

The fixture that is committed was recorded with the library of the commit BEFORE the sum over dims moved into registers, ACCUMULATE's level-0
"+" addend was dropped and GENERATE's mapping shrank to the live quads -- build that commit, then

    SCASML_HIP_LIB=<that commit's libscasml_hip.so> python tests/golden/make_picard_dim_sum.py [OUT.npz]

Recording it again with a later library only restates what that library does.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_gpu_picard_dim_sum as cases  # noqa: E402

if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
    out = cases.record(path)
    print("wrote %s: %d arrays of %d cases, %d bytes" % (path, len(out), len(cases.CASES), os.path.getsize(path)))
