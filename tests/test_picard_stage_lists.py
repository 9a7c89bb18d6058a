"""The schedule of a staged Picard solve (scasml_plan_stage_list) against a brute-force walk of the tree, written here after the site
layout of oracle/mlp.py: a level-L call at base site b draws its terminal samples at b .. b + mg - 1, then, per level l < L, sample path m
and node k, the node's site followed by its "+" child (a level-l call) and, for l > 0, its "-" child (a level-(l-1) call).  No GPU."""
import numpy as np
import pytest

from oracle.mlp import site_count
from oracle.tables import approx_parameters

PLANS = [("quad", 1, 1), ("quad", 2, 2), ("quad", 3, 3), ("quad", 4, 4), ("quad", 5, 5), ("fh", 3, 3), ("fh", 5, 2)]


def _walk(variant, n, par):
    """-> (terminal sites, nodes [(site, level l, + child base, - child base or None)], calls [(level, base, origin)])."""
    tab = approx_parameters(par, 0.5) if variant == "quad" else None
    terms, nodes, calls = [], [], []

    def shape(L, l):
        if variant == "quad":
            Mf, Mg, Q, _, _ = tab
            return int(Q[par - 1, L - l - 1]), int(Mf[par - 1, L - l - 1])
        return 1, par ** (L - l)

    def mg(L):
        return int(tab[1][par - 1, L]) if variant == "quad" else par ** L

    def rec(L, base, origin):
        if L == 0:
            return
        calls.append((L, base, origin))
        terms.extend(range(base, base + mg(L)))
        o = mg(L)
        for l in range(L):
            q, mc = shape(L, l)
            s_l = site_count(variant, l, par, tab)
            s_lm = site_count(variant, l - 1, par, tab) if l else 0
            for _ in range(mc):
                for _ in range(q):
                    node = base + o
                    nodes.append((node, l, node + 1, node + 1 + s_l if l else None))
                    rec(l, node + 1, node)
                    if l:
                        rec(l - 1, node + 1 + s_l, node)
                    o += 1 + s_l + s_lm
        assert o == site_count(variant, L, par, tab)

    total = site_count(variant, n, par, tab)
    rec(n, 0, total)
    return total, terms, nodes, calls


@pytest.mark.parametrize("variant,n,par", PLANS)
def test_stage_lists_match_the_recursion(variant, n, par):
    from scasml_gp_amd import tables
    plan = tables.build_plan(variant, n, par, 0.5, stale_delta_t=True)
    total, terms, nodes, calls = _walk(variant, n, par)
    assert total == plan.sites[n]
    lists = tables.stage_lists(plan)

    # every site of [0, sites[n]) is exactly one terminal sample or one node
    node_sites = [s for s, _, _, _ in nodes]
    assert np.array_equal(np.sort(lists["terminals"]), np.array(terms))
    assert np.array_equal(np.sort(np.concatenate([lists["terminals"], np.array(node_sites, dtype=np.int32)])), np.arange(total))

    # the level-S subtrees: as many as the recursion's uz<S> calls, with their bases and origins; the root call last, at the root row
    for S in range(1, n + 1):
        want = sorted((b, o) for L, b, o in calls if L == S)
        got = sorted(map(tuple, lists["subtrees"][S].tolist()))
        assert got == want
    assert lists["subtrees"][n].tolist() == [[0, total]]

    # f after stage S: "+" of every node of a level-S term, "-" of every node of a level-(S+1) term, each with its child's base
    seen = {}
    for S in range(n):
        want = sorted([(s, cp, 0) for s, l, cp, _ in nodes if l == S] + [(s, cm, 1) for s, l, _, cm in nodes if l == S + 1])
        got = sorted(map(tuple, lists["f_after"][S].tolist()))
        assert got == want
        for s, _, slot in got:
            seen[(s, slot)] = seen.get((s, slot), 0) + 1
    # each node once with "+" and, if l > 0, once with "-"
    for s, l, _, _ in nodes:
        assert seen.pop((s, 0)) == 1
        if l:
            assert seen.pop((s, 1)) == 1
    assert not seen

    # after stage S >= 1 every child is a level-S subtree of that stage's list, and its origin is the node that calls f on it
    for S in range(1, n):
        origin_of = dict(map(tuple, lists["subtrees"][S].tolist()))
        for s, cb, _ in lists["f_after"][S].tolist():
            assert origin_of[cb] == s


def test_stage_list_arguments_are_checked():
    import ctypes as C
    from scasml_gp_amd import _lib, tables
    lib = _lib.load()
    plan = tables.build_plan("quad", 2, 2, 0.5, stale_delta_t=True)
    for kind, stage in [(_lib.STAGE_SUBTREES, 0), (_lib.STAGE_SUBTREES, 3), (_lib.STAGE_F_AFTER, 2), (_lib.STAGE_F_AFTER, -1),
                        (_lib.STAGE_TERMINALS, 1), (7, 0)]:
        assert lib.scasml_plan_stage_list(C.byref(plan), kind, stage, None, 0) == -1
    n = lib.scasml_plan_stage_list(C.byref(plan), _lib.STAGE_TERMINALS, 0, None, 0)
    small = np.zeros(n - 1, dtype=np.int32)
    assert lib.scasml_plan_stage_list(C.byref(plan), _lib.STAGE_TERMINALS, 0, small.ctypes.data_as(C.c_void_p), n - 1) == -1
    assert b"capacity" in lib.scasml_last_error()
    zero = tables.build_plan("quad", 0, 2, 0.5, stale_delta_t=True)
    assert lib.scasml_plan_stage_list(C.byref(zero), _lib.STAGE_TERMINALS, 0, None, 0) == -1
