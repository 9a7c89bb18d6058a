"""scasml_plan_root_summands (include/scasml_hip.h): the number of summands of the root call and where every term's lie, against the unit
grouping the header states for scasml_plan_deal_units -- a terminal sample is one unit and one summand; sample path m of level l is one
summand made of its q (l = 0) or 2 q (l > 0) addends.  Host only: no GPU."""
import ctypes as C

import numpy as np
import pytest

from scasml_gp_amd import _lib, tables


def _summands(plan):
    lib = _lib.load()
    n = plan.n
    first, count = np.full(n + 2, -7, dtype=np.int32), np.full(n + 1, -7, dtype=np.int32)
    S = lib.scasml_plan_root_summands(C.byref(plan), first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p))
    assert S == lib.scasml_plan_root_summands(C.byref(plan), None, None)                       # either pointer may be NULL
    only_first = np.full(n + 2, -7, dtype=np.int32)
    assert S == lib.scasml_plan_root_summands(C.byref(plan), only_first.ctypes.data_as(C.c_void_p), None) and np.array_equal(only_first, first)
    return S, first, count


@pytest.mark.parametrize("variant,n,par,want", [("quad", 3, 3, [27, 5, 3, 2]), ("fh", 4, 3, [81, 81, 27, 9, 3]), ("quad", 2, 4, None), ("quad", 4, 4, None),
                                                ("quad", 1, 3, None), ("fh", 2, 2, None), ("fh", 5, 2, None), ("quad", 5, 5, None)])
def test_root_summands_follow_the_unit_grouping_of_the_header(variant, n, par, want):
    plan = tables.build_plan(variant, n, par, 0.5, True)
    S, first, count = _summands(plan)
    expect = [int(plan.mg[n])] + [int(plan.term[n][l].mc) for l in range(n)]
    if want is not None:
        assert expect == want
    assert S == sum(expect) and list(count) == expect
    assert list(first) == [0] + list(np.cumsum(expect))                                         # first[n + 1] = S
    # every unit of scasml_plan_deal_units belongs to exactly one summand, in order: 1 per terminal sample, q (l = 0) or 2 q per path
    from scasml_gp_amd.parallel import sample_units
    per = [1] + [int(plan.term[n][l].q) * (2 if l else 1) for l in range(n)]
    assert sum(c * p for c, p in zip(expect, per)) == sample_units(plan)


def test_quadrature_n3_rho3_has_37_summands_and_level_zero_none():
    assert _summands(tables.build_plan("quad", 3, 3, 0.5, True))[0] == 27 + 5 + 3 + 2 == 37
    assert _summands(tables.build_plan("fh", 4, 3, 0.5, True))[0] == 81 + 81 + 27 + 9 + 3
    lib = _lib.load()
    plan0 = tables.build_plan("quad", 0, 3, 0.5, True)
    first = np.full(2, -7, dtype=np.int32)
    assert lib.scasml_plan_root_summands(C.byref(plan0), first.ctypes.data_as(C.c_void_p), None) == 0 and list(first) == [-7, -7]
    assert lib.scasml_plan_root_summands(None, None, None) < 0 and b"plan_root_summands" in lib.scasml_last_error()
    bad = tables.build_plan("quad", 2, 3, 0.5, True)
    bad.n = _lib.MAX_LEVEL + 1
    assert lib.scasml_plan_root_summands(C.byref(bad), None, None) < 0
