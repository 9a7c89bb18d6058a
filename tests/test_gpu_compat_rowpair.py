"""The as-coded evaluation's epilogue rounds its lone entries two accumulator rows at a time (csrc/gp_eval_compat_mfma.hip, compat_epilogue) and
reads its Q fragments from a wave-private LDS region.  What that must not change, and what would show a half that entered the wrong row's sum:

* every output row meets the float64 statement (oracle/gp_compat.py) within the bounds tests/test_gpu_compat_mfma.py holds the rounded form to;
* what a site consumes (u_hat; div too for kind 4) has the full form's bits in whichever form its workgroup ran;
* u_hat, div and dt are, bit for bit, what the library of the commit BEFORE the pairing returned on an MI355X for the same seeded inputs
  (tests/golden/compat_rowpair_parent.npz): their entries are pinned or were paired within a row already, and v_cvt_pk_f16_f32 rounds a float32
  value as v_cvt_f16_f32 does.  `lap` is held to the float64 statement only: its lone entries e6, h3 and the boundary h1 were products rounded
  once while they were alone and are float32 values first now (one float16 ulp of one term in about one entry in 8000);
* negative control: one collocation row's cL made large moves `lap` at kind-0 sites and u_hat at every site, and the outputs still meet the float64
  statement of the changed model -- a half added with the neighbouring row's coefficient would miss it by about the size of the term itself.

Shapes: d = 5, 12, 28, 100, 108, 250 (KS = 1, 1, 2, 7 tail-packed, 7 long-tail, 16) against 40 + 20 collocation points (two tiles: a full domain
tile and a domain tile that is mostly boundary and padding rows) and against 40 + 30 (a third tile: boundary rows and padding only, the tile kind
that 60 points do not reach); 5 sites of 32 rows with kinds 0, 1, 3, 4, 0, and the same points with no kinds.  With 32-row sites the first
workgroup spans kinds 0, 1, 3, 4 and runs the full form, so the u-only and (u, div) forms are entered through site lists as well.

The fixture is written by this file:   SCASML_HIP_LIB=<the parent commit's libscasml_hip.so> python tests/test_gpu_compat_rowpair.py OUT.npz
"""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

for _p in (os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))):      # run as a script too
    if _p not in sys.path:
        sys.path.insert(0, _p)
from test_gpu_compat_mfma import _magnitudes, _raw, _setup, _test_points

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compat_rowpair_parent.npz")
ND = 40
KINDS = [0, 1, 3, 4, 0]
ROWS = 32
DIMS = [5, 12, 28, 100, 108, 250]
CASES = [(d, nb) for d in DIMS for nb in (20, 30)]
# site lists that make a workgroup of one form: full, u only (kinds 1, 3), u and div (kind 4)
LISTS = {0: [0, 4], 1: [1, 2], 2: [3]}


def _idx(d):
    return [0, 1, 2, 3, 4] if d == 5 else [d - 1, 0, d // 2, 3, d // 3 + 1]


def _site_list(gp, X, round16, order):
    """(out4, lap) of scasml_gp_eval_compat_site_list over the sites in `order`; rows of other sites keep -7."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    pts = gp._points_device(X)[0]
    out4 = torch.full((pts.shape[0], 4), -7.0, dtype=torch.float32, device="cuda")
    lap = torch.full((pts.shape[0],), -7.0, dtype=torch.float32, device="cuda")
    kd = torch.from_numpy(np.asarray(KINDS, dtype=np.uint8)).cuda()
    od = torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda()
    _lib.check(lib.scasml_gp_eval_compat_site_list(
        gp.d, 1.0 / float(gp.sigma) ** 2, float(gp.equation.sigma()), float(gp.equation.mu()), int(gp.equation.eq_id), _lib.ptr(gp._compat_model),
        gp.N_domain, gp.N_boundary, gp.laplacian_idx.ctypes.data_as(C.c_void_p), round16, 0.0, _lib.ptr(pts), pts.shape[0], ROWS,
        _lib.ptr(kd), _lib.ptr(od), len(order), _lib.ptr(out4), _lib.ptr(lap), _lib.stream_ptr()), "gp_eval_compat_site_list")
    return out4.cpu().numpy().astype(np.float64), lap.cpu().numpy().astype(np.float64)


def _reference(ogp, X):
    """The float64 statement with rounded entries and unrounded outputs, and the per-point bounds of tests/test_gpu_compat_mfma.py."""
    ogp.round_out = False
    mag = _magnitudes(ogp, X)
    dt, div, lp = ogp.pde_parts(X)
    # a flipped rounding decision moves one term by 2^-11 of itself: a few of the largest per point
    flip = {op: 4 * 2.0 ** -11 * (np.abs(ogp._features(op, X)) * np.abs(ogp.right_vector)[:, 0][None, :]).max(1) for op in mag}
    val = {"I": ogp.predict(X)[:, 0], "dt": dt[:, 0], "div": div[:, 0], "lap": lp[:, 0]}
    return val, {op: 2e-5 * mag[op] + flip[op] for op in mag}


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def _case(d, nb, with_reference=True):
    """Inputs, the float64 statement and the device outputs of one case, computed once and shared (never modified) by the tests below."""
    gp, ogp, _ = _setup(d, _idx(d), ND, nb, seed=31 + d)
    X = _test_points(d, ROWS * len(KINDS), seed=57 + d)
    c = {"gp": gp, "ogp": ogp, "X": X,
         "digest": _digest(X, ogp.x_t_domain, ogp.x_t_boundary, ogp.right_vector)}
    c["full"], c["lap_full"] = _raw(gp, X, round16=1)
    c["part"], c["lap_part"] = _raw(gp, X, round16=1, kinds=KINDS, rows_per_site=ROWS)
    c["listed"] = {form: _site_list(gp, X, 1, order) for form, order in LISTS.items()}
    if with_reference:
        c["val"], c["tol"] = _reference(ogp, X)
    return c


def _site(s):
    return slice(s * ROWS, (s + 1) * ROWS)


def _assert_meets_statement(out4, lap, val, tol, rows, what, ops=("I", "dt", "div", "lap")):
    got = {"I": out4[:, 0], "div": out4[:, 1], "dt": out4[:, 3], "lap": lap}
    for op in ops:
        err = np.abs(got[op][rows] - val[op][rows])
        assert np.all(err <= tol[op][rows]), (what, op, float((err / tol[op][rows]).max()))


@pytest.mark.parametrize("d,nb", CASES)
def test_every_output_row_meets_the_float64_statement(d, nb):
    c = _case(d, nb)
    every = slice(0, ROWS * len(KINDS))
    _assert_meets_statement(c["full"], c["lap_full"], c["val"], c["tol"], every, "no kinds")
    for s, k in enumerate(KINDS):
        # a site's row holds what its kind asks for; the workgroup may have run a richer form
        ops = {0: ("I", "dt", "div", "lap"), 1: ("I",), 3: ("I",), 4: ("I", "div")}[k]
        _assert_meets_statement(c["part"], c["lap_part"], c["val"], c["tol"], _site(s), ("kinds", s, k), ops)
    for form, order in LISTS.items():
        out4, lap = c["listed"][form]
        for s in order:
            ops = {0: ("I", "dt", "div", "lap"), 1: ("I",), 2: ("I", "div")}[form]
            _assert_meets_statement(out4, lap, c["val"], c["tol"], _site(s), ("list", form, s), ops)


@pytest.mark.parametrize("d,nb", CASES)
def test_what_a_site_consumes_has_the_full_forms_bits_in_every_form(d, nb):
    c = _case(d, nb)
    full = c["full"]
    for s, k in enumerate(KINDS):
        assert np.array_equal(c["part"][_site(s), 0], full[_site(s), 0]), (s, k)                 # u_hat: kinds 1, 3, 4 (and 0)
        if k in (0, 4):
            assert np.array_equal(c["part"][_site(s), 1], full[_site(s), 1]), (s, k)             # div: kind 4 (and 0)
        if k == 0:
            assert np.array_equal(c["part"][_site(s)], full[_site(s)]) and np.array_equal(c["lap_part"][_site(s)], c["lap_full"][_site(s)])
    for form, order in LISTS.items():                                                            # workgroups that RUN the lesser forms
        out4, lap = c["listed"][form]
        for s in range(len(KINDS)):
            if s not in order:
                assert (out4[_site(s)] == -7.0).all()
                continue
            assert np.array_equal(out4[_site(s), 0], full[_site(s), 0]), (form, s)
            if form in (0, 2):
                assert np.array_equal(out4[_site(s), 1], full[_site(s), 1]), (form, s)
            if form == 0:
                assert np.array_equal(out4[_site(s)], full[_site(s)]) and np.array_equal(lap[_site(s)], c["lap_full"][_site(s)])


@pytest.mark.parametrize("d,nb", CASES)
def test_u_div_and_dt_keep_the_bits_of_the_library_before_the_pairing(d, nb):
    c = _case(d, nb)
    with np.load(GOLDEN) as z:
        key = "d%d_nb%d_" % (d, nb)
        assert str(z[key + "digest"]) == c["digest"], "the seeded inputs are not the recorded ones"
        for name in ("full", "part"):
            want = z[key + name].astype(np.float64)
            for col, what in ((0, "u"), (1, "div"), (3, "dt")):
                assert np.array_equal(c[name][:, col], want[:, col]), (name, what)
        # reported, not asserted: how far lap moved (a float16 ulp of single terms, rarely)
        dl = np.abs(c["lap_full"] - z[key + "lap_full"].astype(np.float64))
        print("d=%d nb=%d: lap differs in %d of %d rows, max |delta| %.3g (bound min %.3g)" % (d, nb, int((dl > 0).sum()), dl.size, dl.max(),
                                                                                            float(c["tol"]["lap"].min())))


@pytest.mark.parametrize("d,nb", CASES)
def test_one_rows_cL_moves_lap_and_u_and_stays_in_its_own_rows_sum(d, nb):
    """Row 5 of the first domain tile (an odd accumulator row's neighbour is row 4) gets a cL fifty times the others'."""
    from scasml_gp_amd.equations.equations import Grad_Dependent_Nonlinear
    from scasml_gp_amd.models.GP import GP_Grad_Dependent_Nonlinear
    import copy
    c = _case(d, nb)
    ogp = copy.copy(c["ogp"])
    rv = c["ogp"].right_vector[:, 0].copy()
    rv[ND + nb + 5] = 2.5                                                   # cL of domain row 5: the others are ~ N(0, 0.05)
    ogp.right_vector = rv[:, None]
    gp = GP_Grad_Dependent_Nonlinear(Grad_Dependent_Nonlinear(d + 1), compat="reference", laplacian_idx=_idx(d))
    gp.load_right_vector(ogp.x_t_domain.astype(np.float32), ogp.x_t_boundary.astype(np.float32), rv)
    X = c["X"]
    val, tol = _reference(ogp, X)
    full, lap_full = _raw(gp, X, round16=1)
    part, lap_part = _raw(gp, X, round16=1, kinds=KINDS, rows_per_site=ROWS)
    # the control has teeth by the float64 statement alone: the changed term is far beyond both bounds at most points of every site ...
    far = {op: np.abs(val[op] - c["val"][op]) > 4 * (tol[op] + c["tol"][op]) for op in ("I", "lap")}
    for s, k in enumerate(KINDS):
        assert far["I"][_site(s)].mean() > 0.9 and far["lap"][_site(s)].mean() > 0.9, (s, k)
        # ... and there the device outputs moved: u_hat at every site, lap where it is computed
        assert np.all(part[_site(s), 0][far["I"][_site(s)]] != c["part"][_site(s), 0][far["I"][_site(s)]]), (s, k)
        if k == 0:
            assert np.all(lap_part[_site(s)][far["lap"][_site(s)]] != c["lap_part"][_site(s)][far["lap"][_site(s)]]), s
    every = slice(0, ROWS * len(KINDS))
    _assert_meets_statement(full, lap_full, val, tol, every, "no kinds")
    for s, k in enumerate(KINDS):
        ops = {0: ("I", "dt", "div", "lap"), 1: ("I",), 3: ("I",), 4: ("I", "div")}[k]
        _assert_meets_statement(part, lap_part, val, tol, _site(s), ("kinds", s, k), ops)
    for form, order in LISTS.items():
        out4, lap = _site_list(gp, X, 1, order)
        for s in order:
            ops = {0: ("I", "dt", "div", "lap"), 1: ("I",), 2: ("I", "div")}[form]
            _assert_meets_statement(out4, lap, val, tol, _site(s), ("list", form, s), ops)


if __name__ == "__main__":      # record the fixture (module docstring)
    rec = {}
    for d_, nb_ in CASES:
        c_ = _case(d_, nb_, with_reference=False)
        key_ = "d%d_nb%d_" % (d_, nb_)
        rec[key_ + "digest"] = np.asarray(c_["digest"])
        rec[key_ + "full"] = c_["full"].astype(np.float32)
        rec[key_ + "part"] = c_["part"].astype(np.float32)
        rec[key_ + "lap_full"] = c_["lap_full"].astype(np.float32)
    np.savez_compressed(sys.argv[1], **rec)
    print("wrote", sys.argv[1], len(rec), "arrays")
