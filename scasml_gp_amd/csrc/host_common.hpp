// Host-only helpers of libscasml_hip.so that need no HIP header: the thread-local error string and fail(), the argument checks the Picard entry
// points share, and the tile order of the FP64 update kernels.
// plan_host.cpp (plain C++, also built with -fsanitize=address,undefined by tests/test_host_sanitizers.py) includes only this.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "scasml_hip.h"

namespace scasml {

char *error_buffer();  // thread-local, 512 bytes (plan_host.cpp)

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

// The checks scasml_picard_tree and scasml_picard_stage both open with, in this order (what follows them differs: the tree answers an empty
// batch next, the stage only after it has looked at everything else).  `who` prefixes the message.
inline int check_batch(const char *who, const void *prob, const void *plan, int64_t B, int64_t site_stride) {
    if (!prob || !plan) return fail(SCASML_ERR_ARG, "%s: null argument", who);
    if (B < 0) return fail(SCASML_ERR_ARG, "%s: negative batch", who);
    if (site_stride != 0 && site_stride < B) return fail(SCASML_ERR_ARG, "%s: site_stride %lld is smaller than the batch %lld", who, (long long)site_stride, (long long)B);
    return 0;
}

// The first term [np][l] of a plan's levels 1 .. n that no walk can take (a path of no or too many nodes, no sample); false: every term is fine.
// plan.n must already be known to lie in 0 .. SCASML_MAX_LEVEL.
inline bool first_bad_term(const scasml_plan &plan, int &np, int &l) {
    for (np = 1; np <= plan.n; ++np)
        for (l = 0; l < np; ++l) {
            const scasml_term &t = plan.term[np][l];
            if (t.q < 1 || t.q > SCASML_MAX_Q || t.mc < 1) return true;
        }
    return false;
}

// The feature rows [row0, row0 + nrows) of a Gram matrix cut at the operator boundaries of the feature order [u(dom), u(bdy), Lap(dom), dt(dom),
// div(dom)]: fn(ox, i_lo, n_i, row_offset) for every piece in rising row order -- operator ox (0 = I, 1 = Lap, 2 = dt, 3 = div) at the points
// [i_lo, i_lo + n_i), its first row row_offset rows after row0.  fn returns 0 to go on; any other value ends the walk and is returned.
template <class Fn>
inline int for_each_operator_segment(int32_t n_dom, int32_t n_bdy, int64_t row0, int64_t nrows, Fn fn) {
    const int64_t N = (int64_t)n_dom + n_bdy, r_end = row0 + nrows;
    for (int64_t r = row0; r < r_end;) {
        const int ox = r < N ? 0 : 1 + (int)((r - N) / n_dom);
        const int64_t first = ox == 0 ? 0 : N + (int64_t)(ox - 1) * n_dom, past = ox == 0 ? N : first + n_dom;   // this operator's block of rows
        const int64_t stop = past < r_end ? past : r_end;
        if (const int rc = fn(ox, (int)(r - first), (int)(stop - r), r - row0)) return rc;
        r = stop;
    }
    return 0;
}

// host + device where the HIP compiler sees it (the kernels' tile order), plain host code in plan_host.cpp (scasml_tile_order: the CPU tests)
#if defined(__HIPCC__)
#define SCASML_HD __host__ __device__
#else
#define SCASML_HD
#endif

// Tile order of the 128 x 128 kernels (WS = 4: one workgroup per CU).  Workgroups b and b + 8 of a launch are observed to share an XCD and
// its 4 MB L2 (MI355X_MICROARCH.md, Workgroup dispatch: round-robin placement; used for speed only, any placement gives the same result),
// and an XCD runs 32 of them at a time.  With a row-major 2-D grid the 32 tiles an XCD holds at one moment lie in ONE tile row, eight
// columns apart: one shared row panel and 32 column panels of their own -- the update read 3.1 x the bytes it wrote
// (profiles/r06_cholesky_counters_70k.txt: 274 KB of operands per tile against 256 KB of C traffic), and at 15.8 flop per fabric byte the
// FP64 matrix cores cannot be fed.  The 1-D grid here deals an XCD SUPER-TILES of 8 x 4 tiles: 8 row panels + 4 column panels (3 MB at
// K = 256, streamed 32 columns at a time by workgroups that start together) feed 32 tiles.  Triangular launches (tj <= ti, nti == ntj)
// enumerate the super-tiles of the lower triangle only: super-row sr holds super-columns 0 .. 2 sr + 1.
constexpr int kSuperRows = 8, kSuperCols = 4, kSuperTiles = kSuperRows * kSuperCols, kXcds = 8;
SCASML_HD inline int64_t super_tile_count(int64_t nti, int64_t ntj, bool tri) {
    const int64_t nsr = (nti + kSuperRows - 1) / kSuperRows, nsc = (ntj + kSuperCols - 1) / kSuperCols;
    return tri ? nsr * nsr + nsr : nsr * nsc;
}
SCASML_HD inline unsigned super_tile_grid(int64_t nti, int64_t ntj, bool tri) {
    const int64_t n = super_tile_count(nti, ntj, tri);
    return (unsigned)((n + kXcds - 1) / kXcds * kXcds * kSuperTiles);
}
// false: this workgroup has no tile (beyond the last super-tile; the caller still tests its tile against the matrix)
SCASML_HD inline bool super_tile_of_block(int64_t b, int64_t nti, int64_t ntj, bool tri, int64_t &ti, int64_t &tj) {
    const int64_t x = b % kXcds, q = b / kXcds;
    const int64_t S = (q / kSuperTiles) * kXcds + x, w = q % kSuperTiles;
    const int64_t nsr = (nti + kSuperRows - 1) / kSuperRows, nsc = (ntj + kSuperCols - 1) / kSuperCols;
    int64_t sr, sc;
    if (tri) {
        if (S >= nsr * nsr + nsr) return false;
        sr = (int64_t)((sqrt(4.0 * (double)S + 1.0) - 1.0) * 0.5);   // largest sr with sr^2 + sr <= S
        while (sr * sr + sr > S) --sr;
        while ((sr + 1) * (sr + 1) + (sr + 1) <= S) ++sr;
        sc = S - (sr * sr + sr);
    } else {
        if (S >= nsr * nsc) return false;
        sr = S / nsc;
        sc = S % nsc;
    }
    ti = sr * kSuperRows + w / kSuperCols;
    tj = sc * kSuperCols + w % kSuperCols;
    return ti < nti && tj < ntj;
}

}  // namespace scasml
