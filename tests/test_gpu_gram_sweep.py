"""The Gram layer at every chunk and tile edge against a direct-difference float64 reference.

Entry points (ctypes, include/scasml_hip.h): scasml_gp_gram and scasml_gp_gram_rows (FP64-MFMA pair tiles, csrc/gp_train.hip),
scasml_gp_gram_compat, scasml_gp_gram_compat_rows and scasml_gp_cross_rows (one thread per pair, csrc/gp_compat.hip).  What the kernels
switch on, and what the shape lists below are built round (test_the_sweep_covers_every_chunk_tile_and_block_edge checks them):

* NB = 32 (gp_train.hip:17): the MFMA tiles stream the K = d + 1 coordinates through LDS NB at a time, zero-padding the last chunk.
* TBX = 32 * NT, NT = 2 (gp_gram_mfma_kernel, gp_gram_rows_kernel; kGramTile of csrc/gp_gram_tile.hpp): 64 x 64 collocation pairs per workgroup, a 64-point tile edge.
* 16 x 16 thread blocks (dim3(16, 16) in scasml_gp_gram_compat / _compat_rows / _cross_rows): a 16-point block edge.

The reference (DirectGP, DirectGPCompat) is oracle/gp.py and oracle/gp_compat.py with the pair geometry taken from exact differences
r = x - y (float32 inputs: every r_k is exact in float64) instead of the norm expansion |x|^2 + |y|^2 - 2 x.y, which is also how the MFMA
Gram forms r^2 and so shares its cancellation.  The polynomial tables (``block``) are the oracle's own.

Per-entry bounds, u = 2^-53, D = d + 1, E_ij = kappa_ij * (sum of |terms| of the entry's polynomial in rho^2, r_t, r_i and
S_1 = sum_{k<d} |r_k|, which stands for S because a sum of d differences is accurate relative to S_1, not to |S|):

* MFMA Gram:  |K - K_ref| <= c u (1 + a D (|x_i|^2 + |y_j|^2)) E_ij.  The x.y accumulation over D products has an absolute error
  <= D u sum_k |x_k y_k| <= D u (|x|^2 + |y|^2) / 2 (Cauchy-Schwarz); |x|^2, |y|^2 are accurate to D u of themselves; so r^2 and rho^2 carry
  an absolute error of order D u (|x|^2 + |y|^2).  kappa = exp(-a r^2 / 2) then moves by a/2 times that, relative, and each polynomial
  moves by its derivative in rho^2 times it; term by term that derivative is at most a E / kappa (e.g. 2 a^4 rho^2 <= a (a^4 rho^4 +
  a^2 d^2) for the Lap-Lap block, by AM-GM).  The remaining roundings (products, the subtraction of constants, exp itself) are a few u of E.
  The reference's own error (D u of r^2, again moved by a/2) is smaller: r^2 <= 2 (|x|^2 + |y|^2).
* Direct-difference kernels (as-coded Gram with round16 = 0, cross rows): |K - K_ref| <= c u D (1 + a r^2) E_ij with r^2 of the entry's
  geometry: both sides sum D exact squares (D u of r^2, a/2 r^2 D u of kappa), the differences are exact, and S is D u of S_1.

c is the smallest power of two that passed on an MI355X: 1 for both (the largest ratio |K - K_ref| / (bound / c) is printed; it was 0.77 for
the MFMA Gram, at d = 2, and 0.43 for the direct kernels).  Where kappa underflows
the entries are 0 on both sides; a floor of 1e-300 keeps a subnormal kappa from asking for more than its absolute spacing.
"""
import ctypes as C

import numpy as np
import pytest

from oracle.equation import GradDependentNonlinear, sample_points
from oracle.gp import OracleGP
from oracle.gp_compat import OracleGPCompat, f16, shift

gpu = pytest.mark.gpu

U = 2.0 ** -53
FLOOR = 1e-300
NB = 32                      # K chunk of the FP64-MFMA pair tiles (csrc/gp_train.hip:17)
TILE = 32 * 2                # TBX = 32 * NT, NT = 2: collocation points per tile side (gp_gram_mfma_kernel)
BLOCK = 16                   # dim3(16, 16) blocks of the per-pair kernels (csrc/gp_compat.hip: scasml_gp_gram_compat and the row / cross entry points)
MAX_DIM = 252                # SCASML_MAX_DIM
C_MFMA = 1                   # bound constants (module docstring): the largest ratios measured were 0.77 (MFMA Gram) and 0.43 (direct kernels)
C_DIRECT = 1
SENTINEL = -7.25
CHUNK = 1 << 22              # float64 elements of one (rows, m, D) difference block of the reference
ROWS = OracleGP._ROWS        # [u(dom), u(bdy), Lap(dom), dt(dom), div(dom)]

# ---------------------------------------------------------------------------------------------------------------- shape lists
# documented Gram: d + 1 = 0, 1, 31 mod 32 and 1, 2, 8 K-chunks
D_DOC = [1, 2, 3, 4, 30, 31, 32, 33, 63, 64, 65, 100, 127, 128, 250, 252]
# (n_dom, n_bdy): N = 64k - 1, 64k, 64k + 1; the domain / boundary split inside a tile and on a tile edge; no boundary points
COLLOC_DOC = [(1, 0), (64, 0), (63, 1), (40, 24), (64, 1), (100, 28), (70, 59), (129, 0), (90, 37)]
CLOUDS = ("plain", "shifted", "close")
# every d at two collocation shapes (consecutive in the list, so each shape meets at least three d), the cloud dealt round
DOC_CASES = [(d, COLLOC_DOC[(2 * i + k) % len(COLLOC_DOC)], CLOUDS[(2 * i + k) % len(CLOUDS)]) for i, d in enumerate(D_DOC) for k in range(2)]
ROWS_COLLOC = (70, 59)       # the rows sweep: one N at every d

# as-coded Gram: N = 15, 0, 1 mod 16, with and without boundary points
D_COMPAT = [5, 6, 20, 31, 32, 33, 100, 128, 250, 252]
COLLOC_COMPAT = [(15, 0), (40, 24), (33, 0), (50, 13), (64, 1), (31, 0)]
COMPAT_CASES = [(d, COLLOC_COMPAT[(2 * i + k) % len(COLLOC_COMPAT)]) for i, d in enumerate(D_COMPAT) for k in range(2)]
ROUND16_MODES = (0, 1, 5, 13)

# cross rows
D_CROSS = [5, 31, 100, 252]
COLLOC_CROSS = (30, 17)      # N = 47: not a multiple of 16
N_INF = (0, 1, 15, 17)


def _hutch(d):
    """Five distinct Hutchinson indices with 0 and d - 1 (index d - 1 of the shifted vector is the time coordinate)."""
    if d == 5:
        return [4, 2, 0, 3, 1]
    mid = np.random.default_rng(d).choice(np.arange(1, d - 1), 3, replace=False)
    return [d - 1, int(mid[0]), 0, int(mid[1]), int(mid[2])]


def _row_ranges(nd, nb):
    """(row0, nrows, ncols): starts inside a 64-row tile, several tiles, every operator boundary straddled, ranges ending at M, ncols at
    1, N - 1, N, N + 1 and M."""
    N, M = nd + nb, 4 * nd + nb
    ranges = [(37, 100, M), (nd - 5, 20, N + 1), (N - 3, 10, N), (N + nd - 2, nd + 4, N - 1), (N + 2 * nd - 7, M - (N + 2 * nd - 7), M),
              (0, M, M), (M - 1, 1, 1), (M - 70, 70, M)]
    clipped = []
    for row0, nrows, ncols in ranges:                  # small M: the same ranges, cut to the matrix
        row0 = min(max(row0, 0), M - 1)
        clipped.append((row0, min(nrows, M - row0), min(max(ncols, 1), M)))
    return clipped


# ---------------------------------------------------------------------------------------------------------------- reference
class _G:
    pass


_GEOM = {}


def _geometry(X, Y, d, which="al", cols=None):
    """Pair geometry from exact differences: r = X' - Y (which = "xs"), X - Y' ("ys") or X - Y ("al"); r^2, rho^2 (spatial), S, S_1 = sum |r_k|
    (k < d), r_t / r_D (component d) and the components ``cols``.  Chunked over rows; kept per (X, Y, which) while those arrays live."""
    key = (id(X), id(Y), which, None if cols is None else tuple(cols))
    hit = _GEOM.get(key)
    if hit is not None and hit[0] is X and hit[1] is Y:
        return hit[2]
    Xg, Yg = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    if which == "xs":
        Xg = shift(Xg)
    elif which == "ys":
        Yg = shift(Yg)
    n, m = len(Xg), len(Yg)
    g = _G()
    g.rho2, g.S, g.S1, g.rt = (np.empty((n, m)) for _ in range(4))
    g.ri = np.empty((n, m, len(cols))) if cols is not None else None
    step = max(1, CHUNK // max(1, m * (d + 1)))
    for i0 in range(0, n, step):
        r = Xg[i0:i0 + step, None, :] - Yg[None, :, :]
        g.rho2[i0:i0 + step] = (r[:, :, :d] * r[:, :, :d]).sum(2)
        g.S[i0:i0 + step] = r[:, :, :d].sum(2)
        g.S1[i0:i0 + step] = np.abs(r[:, :, :d]).sum(2)
        g.rt[i0:i0 + step] = r[:, :, d]
        if cols is not None:
            g.ri[i0:i0 + step] = r[:, :, cols]
    g.r2 = g.rho2 + g.rt * g.rt
    if len(_GEOM) > 32:
        _GEOM.clear()
    _GEOM[key] = (X, Y, g)
    return g


class DirectGP(OracleGP):
    """oracle/gp.py with the pair geometry from exact differences."""

    def _pairs(self, X, Y):
        g = _geometry(X, Y, self.d)
        return np.exp(-self.a * g.r2 / 2.0), g.rho2, g.S, g.rt


class DirectGPCompat(OracleGPCompat):
    """oracle/gp_compat.py with every geometry (al, ys, xs and the Laplacian-free blocks' pairs) from exact differences."""

    def _pairs(self, X, Y):
        g = _geometry(X, Y, self.d)
        return np.exp(-self.a * g.r2 / 2.0), g.rho2, g.S, g.rt

    def _geom(self, X, Y, which):
        cols = self.idx if which != "al" else self.idx + 1
        g = _geometry(X, Y, self.d, which, cols)
        return np.exp(-self.a * g.r2 / 2.0), g.S, g.rt, g.ri


def _mag_doc(ox, oy, a, d, g):
    """E / kappa of a documented entry: the sum of |terms| of its polynomial (oracle/gp.py block), S replaced by S_1."""
    rho2, S1, rt = g.rho2, g.S1, np.abs(g.rt)
    lap = a * a * rho2 + a * d
    key = frozenset((ox, oy)) if ox != oy else ox
    table = {"I": 1.0, "lap": a ** 4 * rho2 ** 2 + (2 * d + 4) * a ** 3 * rho2 + (d * d + 2 * d) * a * a,
             "dt": a + a * a * rt * rt, "div": a * d + a * a * S1 * S1,
             frozenset(("I", "lap")): lap, frozenset(("I", "dt")): a * rt, frozenset(("I", "div")): a * S1,
             frozenset(("dt", "div")): a * a * rt * S1, frozenset(("dt", "lap")): a * rt * lap,
             frozenset(("div", "lap")): a * S1 * lap + 2 * a * a * S1}
    return np.broadcast_to(table[key], g.r2.shape)


def _mag_compat(ox, oy, ref, X, Y):
    """(E, r^2 of the entry's geometry) of an as-coded entry (oracle/gp_compat.py block)."""
    a, d = ref.a, ref.d
    h = d / float(ref.MC)
    if "lap" not in (ox, oy):
        g = _geometry(X, Y, d)
        return _mag_doc(ox, oy, a, d, g) * np.exp(-a * g.r2 / 2), g.r2
    which = "al" if ox == oy else ("ys" if oy == "lap" else "xs")
    g = _geometry(X, Y, d, which, ref.idx if which != "al" else ref.idx + 1)
    ri, rD, S1 = g.ri, np.abs(g.rt), g.S1
    sg = (a * a * ri * ri + a).sum(2)
    mix = (2 * a * a * np.abs(ri) + (a * a * S1)[:, :, None] + a ** 3 * S1[:, :, None] * ri * ri).sum(2)
    other = oy if ox == "lap" else ox
    if ox == oy:
        P = h * h * (sg * sg + (2 * a * a + 4 * a ** 3 * ri * ri).sum(2))
    elif other == "I":
        P = h * sg
    elif other == "dt":
        P = a * rD * h * sg
    else:
        P = h * mix
    return P * np.exp(-a * g.r2 / 2), g.r2


def _assemble(f, dom, bdy):
    pts = {"dom": dom, "bdy": bdy}
    return np.block([[f(ox, oy, pts[px], pts[py]) for (oy, py) in ROWS] for (ox, px) in ROWS])


# ---------------------------------------------------------------------------------------------------------------- points
def _cloud(d, nd, nb, kind, seed, as_f16=False):
    """sample_points; "shifted": the same cloud centred at 3 in every coordinate (|x|^2 ~ 9 D against r^2 ~ D / 6: the norm expansion cancels
    ~50 D-fold); "close": exact duplicates (within the domain and across domain / boundary) and points one float32 ulp apart (one coordinate,
    and every coordinate) -- r^2 = 0 or ~1e-15, where the expansion can come out negative and the kernels clamp it."""
    dom, bdy = sample_points(np.random.default_rng(seed), d, nd, nb)
    if kind == "shifted":
        dom, bdy = (dom.astype(np.float64) + 3.0).astype(np.float32), (bdy.astype(np.float64) + 3.0).astype(np.float32)
    if as_f16:
        dom, bdy = dom.astype(np.float16).astype(np.float32), bdy.astype(np.float16).astype(np.float32)
    if kind == "close":
        up = lambda v: np.nextafter(v, np.float32(np.inf)) if not as_f16 else np.float32(np.nextafter(np.float16(v), np.float16(np.inf)))
        P = np.concatenate([dom, bdy])
        N = len(P)
        if N >= 2:
            P[1] = P[0]
        if N >= 3:
            P[2] = P[0]
            P[2, d // 2] = up(P[0, d // 2])
        if N >= 4:
            P[3] = [up(v) for v in P[0]]
        if nb >= 1 and N >= 6:
            P[nd] = P[5 if nd > 5 else 0]
        if N >= 64:
            P[63] = P[64 % N]                            # a pair across the 64-point tile edge
        dom, bdy = P[:nd], P[nd:]
    return np.ascontiguousarray(dom, dtype=np.float32), np.ascontiguousarray(bdy, dtype=np.float32)


def _a(d):
    return DirectGP(GradDependentNonlinear(d + 1)).a


# ---------------------------------------------------------------------------------------------------------------- device calls
def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _guarded(M_rows, M_cols, call, ld=None, fill=np.nan):
    """Run `call(ptr)` on an (M_rows x ld) float64 buffer filled with `fill` and followed by 64 sentinel doubles; the padding columns beyond
    M_cols hold the sentinel too.  Returns the (M_rows, M_cols) result; asserts the padding and the tail are untouched."""
    import torch
    from scasml_gp_amd import _lib
    ld = M_cols if ld is None else ld
    buf = torch.full((M_rows * ld + 64,), fill, dtype=torch.float64, device="cuda")
    view = buf[:M_rows * ld].view(M_rows, ld) if M_rows * ld else None
    if view is not None and ld > M_cols:
        view[:, M_cols:] = SENTINEL
    buf[M_rows * ld:] = SENTINEL
    call(_lib.ptr(buf))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[M_rows * ld:] == SENTINEL), "wrote past the end of the buffer"
    out = host[:M_rows * ld].reshape(M_rows, ld)
    assert np.all(out[:, M_cols:] == SENTINEL), "wrote into the padding beyond the requested columns"
    return out[:, :M_cols]


def _gram(d, a, dom, bdy, idx=None, round16=0):
    from scasml_gp_amd import _lib
    lib = _lib.load()
    nd, nb = len(dom), len(bdy)
    M = 4 * nd + nb
    xd, xb = _dev(dom), (_dev(bdy) if nb else None)
    if idx is None:
        call = lambda p: _lib.check(lib.scasml_gp_gram(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, p, _lib.stream_ptr()), "gp_gram")
    else:
        ih = np.asarray(idx, dtype=np.int32)
        call = lambda p: _lib.check(lib.scasml_gp_gram_compat(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, ih.ctypes.data_as(C.c_void_p), round16, p,
                                                              _lib.stream_ptr()), "gp_gram_compat")
    K = _guarded(M, M, call)
    assert not np.isnan(K).any(), "entries left unwritten: %d" % int(np.isnan(K).sum())
    return K


def _gram_rows(d, a, dom, bdy, row0, nrows, ncols, idx=None, round16=0):
    from scasml_gp_amd import _lib
    lib = _lib.load()
    nd, nb = len(dom), len(bdy)
    xd, xb = _dev(dom), (_dev(bdy) if nb else None)
    ld = ncols + 7
    if idx is None:
        call = lambda p: _lib.check(lib.scasml_gp_gram_rows(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, row0, nrows, ncols, p, ld, _lib.stream_ptr()),
                                    "gp_gram_rows")
    else:
        ih = np.asarray(idx, dtype=np.int32)
        call = lambda p: _lib.check(lib.scasml_gp_gram_compat_rows(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, ih.ctypes.data_as(C.c_void_p), round16,
                                                                   row0, nrows, ncols, p, ld, _lib.stream_ptr()), "gp_gram_compat_rows")
    return _guarded(nrows, ncols, call, ld=ld)


def _check_rows(d, a, dom, bdy, K, idx=None, round16=0):
    """Every row range: the rows of the full Gram, bit for bit, and nothing beyond; nrows = 0 / ncols = 0 write nothing."""
    nd, nb = len(dom), len(bdy)
    for row0, nrows, ncols in _row_ranges(nd, nb):
        got = _gram_rows(d, a, dom, bdy, row0, nrows, ncols, idx, round16)
        assert np.array_equal(got, K[row0:row0 + nrows, :ncols]), (row0, nrows, ncols, int((got != K[row0:row0 + nrows, :ncols]).sum()))
    for row0, nrows, ncols in ((5, 0, 10), (5, 10, 0)):
        got = _gram_rows(d, a, dom, bdy, row0, nrows, ncols, idx, round16)
        assert got.size == 0


def _ratio(err, bound):
    return float(np.max(err / bound)) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- CPU: the lists
def test_the_sweep_covers_every_chunk_tile_and_block_edge():
    """The shape lists reach what the kernels switch on: d + 1 = 0, 1, 31 mod NB at 1, 2 and 8 chunks, up to SCASML_MAX_DIM; N = 0, 1, 63 mod
    the 64-point tile and 0, 1, 15 mod the 16 x 16 blocks; no boundary points at every entry point; Hutchinson sets with 0 and d - 1."""
    from scasml_gp_amd import _lib
    assert MAX_DIM == _lib.MAX_DIM and max(D_DOC) == max(D_COMPAT) == max(D_CROSS) == MAX_DIM
    assert {(d + 1) % NB for d in D_DOC} >= {0, 1, NB - 1}
    assert {-(-(d + 1) // NB) for d in D_DOC} >= {1, 2, 8}
    doc_N = {nd + nb for _, (nd, nb), _ in DOC_CASES}
    assert {n % TILE for n in doc_N} >= {0, 1, TILE - 1}
    assert any(nd % TILE == 0 and nb > 0 for nd, nb in COLLOC_DOC) and any(0 < nd % TILE and nb > 0 for nd, nb in COLLOC_DOC)
    # every d at two or more collocation shapes, every shape at three or more d, every cloud at every kernel edge it matters for
    for d in D_DOC:
        assert len({c for dd, c, _ in DOC_CASES if dd == d}) >= 2
    for c in COLLOC_DOC:
        assert len({d for d, cc, _ in DOC_CASES if cc == c}) >= 3, c
    for kind in CLOUDS:
        assert {(d + 1) % NB for d, _, k in DOC_CASES if k == kind} >= {0, 1}, kind
    compat_N = {nd + nb for _, (nd, nb) in COMPAT_CASES}
    assert {n % BLOCK for n in compat_N} >= {0, 1, BLOCK - 1}
    assert sum(COLLOC_CROSS) % BLOCK != 0 and {n % BLOCK for n in N_INF} >= {0, 1, BLOCK - 1}
    assert any(nb == 0 for _, (nd, nb), _ in DOC_CASES) and any(nb == 0 for _, (nd, nb) in COMPAT_CASES)
    for d in set(D_COMPAT) | set(D_CROSS):
        idx = _hutch(d)
        assert len(set(idx)) == 5 and 0 in idx and d - 1 in idx and max(idx) < d
    # the row ranges start inside a tile, straddle every operator boundary and end at M
    nd, nb = ROWS_COLLOC
    N, M = nd + nb, 4 * nd + nb
    ranges = _row_ranges(nd, nb)
    assert any(r0 % TILE and n > TILE for r0, n, _ in ranges)
    for edge in (nd, N, N + nd, N + 2 * nd):
        assert any(r0 < edge < r0 + n for r0, n, _ in ranges), edge
    assert any(r0 + n == M for r0, n, _ in ranges) and {c for _, _, c in ranges} >= {1, N - 1, N, N + 1, M}


def test_direct_reference_agrees_with_the_oracles_expansion():
    """The direct-difference reference is the oracle up to the norm expansion's cancellation (CPU): it changes no table."""
    d, nd, nb = 7, 20, 6
    dom, bdy = _cloud(d, nd, nb, "plain", 1)
    D64, B64 = dom.astype(np.float64), bdy.astype(np.float64)
    eq = GradDependentNonlinear(d + 1)
    K, Ko = DirectGP(eq).kernel_phi_phi(D64, B64), OracleGP(eq).kernel_phi_phi(D64, B64)
    assert np.abs(K - Ko).max() <= 1e-12 * np.abs(Ko).max()
    idx = _hutch(d)
    Kc = DirectGPCompat(eq, idx, round16=False).kernel_phi_phi(D64, B64)
    Kco = OracleGPCompat(eq, idx, round16=False).kernel_phi_phi(D64, B64)
    assert np.abs(Kc - Kco).max() <= 1e-12 * np.abs(Kco).max()


# ---------------------------------------------------------------------------------------------------------------- documented Gram
def _doc_bound(ref, dom, bdy):
    a, d = ref.a, ref.d
    D = d + 1
    P = np.concatenate([dom, bdy]).astype(np.float64)
    n2 = (P * P).sum(1)
    n2 = {"dom": n2[:len(dom)], "bdy": n2[len(dom):]}
    X, Y = ref.x_t_domain, ref.x_t_boundary

    def blk(ox, oy, A, B):
        g = _geometry(A, B, d)
        na, nb_ = n2["dom" if A is X else "bdy"], n2["dom" if B is X else "bdy"]
        return (1 + a * D * (na[:, None] + nb_[None, :])) * _mag_doc(ox, oy, a, d, g) * np.exp(-a * g.r2 / 2)

    return U * _assemble(blk, X, Y) + FLOOR


@gpu
@pytest.mark.parametrize("d,colloc,kind", DOC_CASES, ids=["d%d-n%d+%d-%s" % (d, c[0], c[1], k) for d, c, k in DOC_CASES])
def test_documented_gram_within_the_per_entry_bound(d, colloc, kind):
    nd, nb = colloc
    dom, bdy = _cloud(d, nd, nb, kind, seed=d * 31 + nd)
    ref = DirectGP(GradDependentNonlinear(d + 1))
    a = ref.a
    K = _gram(d, a, dom, bdy)                                  # NaN-filled: every entry written, nothing past M x M
    want = ref.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64))
    bound = _doc_bound(ref, dom, bdy)
    err = np.abs(K - want)
    ratio = _ratio(err, bound)
    print("documented Gram d=%d N=%d+%d %s: max err / (u (1 + a D |x|^2..) E) = %.3g" % (d, nd, nb, kind, ratio))
    assert ratio <= C_MFMA, ratio
    # x.y and y.x come out of the matrix cores bit for bit equal (every case of this sweep on an MI355X), and the rest of an entry is
    # odd or even in the pair's order exactly: the Gram is symmetric bitwise
    assert np.array_equal(K, K.T), _ratio(np.abs(K - K.T), bound + bound.T)


@gpu
@pytest.mark.parametrize("d", D_DOC)
def test_documented_gram_rows_are_the_full_grams_rows(d):
    nd, nb = ROWS_COLLOC
    dom, bdy = _cloud(d, nd, nb, "plain", seed=d + 500)
    a = _a(d)
    K = _gram(d, a, dom, bdy)
    _check_rows(d, a, dom, bdy, K)


# ---------------------------------------------------------------------------------------------------------------- as-coded Gram
def _direct_bound(ref, dom, bdy):
    """c-free bound u D (1 + a r^2) E of the as-coded entries, r^2 of each entry's geometry."""
    a, D = ref.a, ref.d + 1

    def blk(ox, oy, A, B):
        E, r2 = _mag_compat(ox, oy, ref, A, B)
        return D * (1 + a * r2) * E

    return U * _assemble(blk, ref.x_t_domain, ref.x_t_boundary) + FLOOR


@gpu
@pytest.mark.parametrize("d,colloc", COMPAT_CASES, ids=["d%d-n%d+%d" % (d, c[0], c[1]) for d, c in COMPAT_CASES])
def test_as_coded_gram_unrounded_and_rounded(d, colloc):
    """round16 = 0 against the direct reference per entry; round16 = 1 is round16 = 0 rounded to float16, bit for bit."""
    nd, nb = colloc
    idx = _hutch(d)
    kind = "close" if d % 2 else "plain"
    dom, bdy = _cloud(d, nd, nb, kind, seed=d * 7 + nd)
    ref = DirectGPCompat(GradDependentNonlinear(d + 1), idx, round16=False)
    a = ref.a
    K0 = _gram(d, a, dom, bdy, idx, 0)
    want = ref.kernel_phi_phi(dom.astype(np.float64), bdy.astype(np.float64))
    ratio = _ratio(np.abs(K0 - want), _direct_bound(ref, dom, bdy))
    print("as-coded Gram d=%d N=%d+%d %s, round16 = 0: max err / (u D (1 + a r^2) E) = %.3g" % (d, nd, nb, kind, ratio))
    assert ratio <= C_DIRECT, ratio
    K1 = _gram(d, a, dom, bdy, idx, 1)
    assert np.array_equal(K1, f16(K0))
    # the two orders of a pair take the same differences, negated: symmetric bit for bit
    assert np.array_equal(K0, K0.T) and np.array_equal(K1, K1.T)


@gpu
@pytest.mark.parametrize("d,colloc", COMPAT_CASES, ids=["d%d-n%d+%d" % (d, c[0], c[1]) for d, c in COMPAT_CASES])
def test_as_coded_gram_float16_op_sequence_and_rows(d, colloc):
    """round16 = 5 and 13 on float16 rows against the oracle's float16 op sequence (f16_graph = 2, 3): at most a handful of entries
    differ, by at most one float16 ulp (tests/test_gpu_f16_graph.py); the rows entry point gives the full Gram's rows in all four modes."""
    nd, nb = colloc
    idx = _hutch(d)
    dom, bdy = _cloud(d, nd, nb, "plain", seed=d * 11 + nd, as_f16=True)
    a = _a(d)
    D64, B64 = dom.astype(np.float64), bdy.astype(np.float64)
    K = {m: _gram(d, a, dom, bdy, idx, m) for m in ROUND16_MODES}
    for mode, level in ((5, 2), (13, 3)):
        want = DirectGPCompat(GradDependentNonlinear(d + 1), idx, f16_graph=level).kernel_phi_phi(D64, B64)
        got = K[mode]
        assert np.array_equal(f16(got), got)
        differs = got != want
        print("as-coded Gram d=%d N=%d+%d round16 = %d: %d of %d entries differ from the float16 op sequence" % (d, nd, nb, mode, int(differs.sum()),
                                                                                                              differs.size))
        assert differs.sum() <= 4, int(differs.sum())
        assert np.all(np.abs(got - want)[differs] <= 2.0 ** -10 * np.abs(want)[differs] + 2.0 ** -24)
    for mode in ROUND16_MODES:
        _check_rows(d, a, dom, bdy, K[mode], idx, mode)


# ---------------------------------------------------------------------------------------------------------------- cross rows
def _cross_points(d, n, seed):
    """n rows: float16-exact, arbitrary float32, and (from the fourth on, every fourth) far away, where kappa underflows to 0."""
    X = sample_points(np.random.default_rng(seed), d, n, 0)[0].astype(np.float64)
    X[::2] = f16(X[::2])
    X[3::4] += 100.1
    return X.astype(np.float32)


def _cross(d, a, dom, bdy, idx, round16, surrogate, op, X):
    """scasml_gp_cross_rows from rows of a wider array (ld_inf = d + 6, the extra columns NaN) into ld = M + 3 (op 4: n * M * D doubles)."""
    import torch
    from scasml_gp_amd import _lib
    lib = _lib.load()
    nd, nb = len(dom), len(bdy)
    M, D = 4 * nd + nb, d + 1
    n = len(X)
    wide = np.full((max(n, 1), D + 5), np.nan, dtype=np.float32)
    wide[:n, :D] = X
    xi = torch.from_numpy(wide).cuda()
    xd, xb = _dev(dom), (_dev(bdy) if nb else None)
    ih = np.asarray(idx, dtype=np.int32)
    ld = M + 3
    call = lambda p: _lib.check(lib.scasml_gp_cross_rows(d, a, _lib.ptr(xd), nd, _lib.ptr(xb), nb, ih.ctypes.data_as(C.c_void_p), round16, surrogate, op,
                                                         _lib.ptr(xi), n, D + 5, p, ld, _lib.stream_ptr()), "gp_cross_rows")
    if op == 4:
        out = _guarded(n, M * D, call).reshape(n, M, D)
    else:
        out = _guarded(n, M, call, ld=ld)
    assert not np.isnan(out).any()
    return out


def _feature_grad(X, dom, bdy, a, d, idx):
    """d/dx_k of the op-0 row [kappa(dom), kappa(bdy), lap_y kappa, dt_y kappa, div_y kappa] (models/GP.py:296-324), by float64 autograd through
    the direct-difference statement; idx None: the documented Laplacian, else the as-coded one (5-index Hutchinson, y shifted)."""
    import torch
    Yd, Yb = torch.from_numpy(dom.astype(np.float64)), torch.from_numpy(bdy.astype(np.float64))
    Ys = torch.roll(Yd, -1, 1)
    h = d / 5.0

    def row(x):
        r = x[None, :] - Yd
        kap = torch.exp(-0.5 * a * (r * r).sum(1))
        rb = x[None, :] - Yb
        kb = torch.exp(-0.5 * a * (rb * rb).sum(1))
        if idx is None:
            lap = (a * a * (r[:, :d] * r[:, :d]).sum(1) - a * d) * kap
        else:
            r1 = x[None, :] - Ys
            lap = h * (a * a * r1[:, idx] * r1[:, idx] - a).sum(1) * torch.exp(-0.5 * a * (r1 * r1).sum(1))
        return torch.cat([kap, kb, lap, a * r[:, d] * kap, a * r[:, :d].sum(1) * kap])

    return torch.func.vmap(torch.func.jacrev(row))(torch.from_numpy(X.astype(np.float64))).numpy()


def _feature_grad_bound(X, dom, bdy, a, d, idx):
    """u D (1 + a r^2) G: G the sum of |terms| of each derivative (gp_cross_grad_rows_kernel's closed forms), r^2 of its geometry."""
    D = d + 1
    X64 = X.astype(np.float64)
    out = []
    for Y, full in ((dom, True), (bdy, False)):
        Y64 = Y.astype(np.float64)
        r = X64[:, None, :] - Y64[None, :, :]
        r2 = (r * r).sum(2)
        k0 = np.exp(-0.5 * a * r2)
        w = (D * (1 + a * r2) * k0)[:, :, None]
        cols = [w * a * np.abs(r)]
        if full:
            rho2 = (r[:, :, :d] ** 2).sum(2)
            S1 = np.abs(r[:, :, :d]).sum(2)
            rt = np.abs(r[:, :, d])
            if idx is None:
                G = 2 * a * a * np.abs(r) + (a * np.abs(r) * (a * a * rho2 + a * d)[:, :, None])
                G[:, :, d] = (a * np.abs(r[:, :, d]) * (a * a * rho2 + a * d))
                cols.append(w * G)
            else:
                r1 = X64[:, None, :] - shift(Y64)[None, :, :]
                r2s = (r1 * r1).sum(2)
                sg = (a * a * r1[:, :, idx] ** 2 + a).sum(2)
                G = (d / 5.0) * np.exp(-0.5 * a * r2s)[:, :, None] * np.abs(r1) * (2 * a * a + a * sg[:, :, None])
                cols.append((D * (1 + a * r2s))[:, :, None] * G)
            dt = a * a * rt[:, :, None] * np.abs(r)
            dt[:, :, d] += a
            dv = a * a * S1[:, :, None] * np.abs(r)
            dv[:, :, :d] += a
            cols += [w * dt, w * dv]
        out.append(cols)
    (k_d, lap, dt, dv), (k_b,) = out
    return U * np.concatenate([k_d, k_b, lap, dt, dv], axis=1) + FLOOR


@gpu
@pytest.mark.parametrize("d", D_CROSS)
def test_cross_rows_ops_0_to_3_both_surrogates(d):
    nd, nb = COLLOC_CROSS
    idx = _hutch(d)
    dom, bdy = _cloud(d, nd, nb, "plain", seed=d + 900, as_f16=True)
    D64, B64 = dom.astype(np.float64), bdy.astype(np.float64)
    eq = GradDependentNonlinear(d + 1)
    comp, doc = DirectGPCompat(eq, idx, round16=False), DirectGP(eq)
    a = doc.a
    for n in N_INF:
        X = _cross_points(d, n, seed=d + n)
        X64 = X.astype(np.float64)
        is16 = np.all(X64 == f16(X64), axis=1)
        for ox in ("I", "lap", "dt", "div"):
            op = ("I", "lap", "dt", "div").index(ox)
            for surrogate, ref in ((0, comp), (1, doc)):
                got = _cross(d, a, dom, bdy, idx, 0, surrogate, op, X)
                if n == 0:
                    continue
                want = np.concatenate([ref.block(ox, oy, X64, {"dom": D64, "bdy": B64}[py]) for oy, py in ROWS], axis=1)
                if surrogate == 0:
                    bound = np.concatenate([(d + 1) * (1 + a * r2) * E for E, r2 in
                                            (_mag_compat(ox, oy, comp, X64, {"dom": D64, "bdy": B64}[py]) for oy, py in ROWS)], axis=1)
                else:
                    bound = np.concatenate([(d + 1) * (1 + a * g.r2) * _mag_doc(ox, oy, a, d, g) * np.exp(-a * g.r2 / 2) for g, oy in
                                            ((_geometry(X64, {"dom": D64, "bdy": B64}[py], d), oy) for oy, py in ROWS)], axis=1)
                ratio = _ratio(np.abs(got - want), U * bound + FLOOR)
                print("cross rows d=%d n=%d op %s surrogate %d: max err / (u D (1 + a r^2) E) = %.3g" % (d, n, ox, surrogate, ratio))
                assert ratio <= C_DIRECT, (ox, surrogate, ratio)
                assert np.all(got[3::4] == 0.0)                              # far rows: kappa underflows, entries are 0 (not NaN)
                if surrogate == 1:
                    continue
                g1 = _cross(d, a, dom, bdy, idx, 1, 0, op, X)
                assert np.array_equal(g1, f16(got))
                g5 = _cross(d, a, dom, bdy, idx, 5, 0, op, X)
                assert np.array_equal(g5[~is16], g1[~is16])                   # rows that are not float16 values: one rounding per entry
                w5 = np.concatenate([DirectGPCompat(eq, idx, f16_graph=2).block(ox, oy, X64[is16], {"dom": D64, "bdy": B64}[py]) for oy, py in ROWS],
                                    axis=1)
                differs = g5[is16] != w5
                print("  round16 = 5: %d of %d float16-row entries differ from the float16 op sequence" % (int(differs.sum()), differs.size))
                assert differs.sum() <= 4
                assert np.all(np.abs(g5[is16] - w5)[differs] <= 2.0 ** -10 * np.abs(w5)[differs] + 2.0 ** -24)


@gpu
@pytest.mark.parametrize("d", D_CROSS)
def test_cross_gradient_rows_entry_by_entry(d):
    nd, nb = COLLOC_CROSS
    idx = _hutch(d)
    dom, bdy = _cloud(d, nd, nb, "plain", seed=d + 950, as_f16=True)
    a = _a(d)
    for n in N_INF:
        X = _cross_points(d, n, seed=d + n + 1)
        for surrogate in (0, 1):
            si = idx if surrogate == 0 else None
            got = _cross(d, a, dom, bdy, idx, 0, surrogate, 4, X)
            if n == 0:
                continue
            want = _feature_grad(X, dom, bdy, a, d, si)
            ratio = _ratio(np.abs(got - want), _feature_grad_bound(X, dom, bdy, a, d, si))
            print("gradient rows d=%d n=%d surrogate %d: max err / (u D (1 + a r^2) G) = %.3g" % (d, n, surrogate, ratio))
            assert ratio <= C_DIRECT, (surrogate, ratio)
            assert np.all(got[3::4] == 0.0)
            if surrogate == 0:
                assert np.array_equal(_cross(d, a, dom, bdy, idx, 1, 0, 4, X), f16(got))
