// The one statement of a collocation pair's 16 entries of K and of K_a = dK/da (DESIGN.md sections 4.3 and 4.10), read by every visit of the Gram
// pair tile (gp_gram_tile.hpp).  An entry of K is P(ox, oy) kappa with kappa = exp(-a r^2 / 2) and P the operator polynomials of Appendix C, so
// the entry of K_a is (P_a - r^2 P / 2) kappa with P_a = dP/da at fixed geometry; ops: 0 = I, 1 = Lap, 2 = dt, 3 = div.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace scasml {

enum GramTable { kGramK, kGramKa };

// k[ox][oy] <- the pair's 16 entries of table T from its geometry: r2 = |x - y|^2 with the time coordinate (clamped at 0 by the caller),
// rt = t_x - t_y, S = sum x - sum y over the spatial coordinates, fd = d.  Entries a caller does not use cost nothing once its loops are unrolled.
// The build does not contract: every product and sum below is rounded as written, and K and its rows, K_a and its rows agree bit for bit.
template <GramTable T>
__device__ __forceinline__ void gram_pair(double a, double fd, double r2, double rt, double S, double (&k)[4][4]) {
    double rho2 = fma(-rt, rt, r2);
    rho2 = rho2 < 0.0 ? 0.0 : rho2;
    const double kap = exp(-0.5 * a * r2);
    const double lap = a * a * rho2 - a * fd;
    const double aS = a * S, art = a * rt, mix = aS * lap - 2.0 * a * aS;
    const double c3 = 2.0 * fd + 4.0, c2 = fd * fd + 2.0 * fd;
    const double ll = a * a * a * a * rho2 * rho2 - c3 * a * a * a * rho2 + c2 * a * a;
    const double P[4][4] = {
        {1.0, lap, art, aS},
        {lap, ll, art * lap, mix},
        {-art, -art * lap, a - art * art, -art * aS},
        {-aS, -mix, -art * aS, a * fd - aS * aS}};
    if (T == kGramK) {
#pragma unroll
        for (int ox = 0; ox < 4; ++ox)
#pragma unroll
            for (int oy = 0; oy < 4; ++oy) k[ox][oy] = P[ox][oy] * kap;
        return;
    }
    const double lap_a = 2.0 * a * rho2 - fd;
    const double mix_a = S * lap + aS * lap_a - 4.0 * aS, tl_a = rt * lap + art * lap_a;
    const double ll_a = 4.0 * a * a * a * rho2 * rho2 - 3.0 * c3 * a * a * rho2 + 2.0 * c2 * a;
    const double Pa[4][4] = {
        {0.0, lap_a, rt, S},
        {lap_a, ll_a, tl_a, mix_a},
        {-rt, -tl_a, 1.0 - 2.0 * art * rt, -2.0 * art * S},
        {-S, -mix_a, -2.0 * art * S, fd - 2.0 * aS * S}};
    const double h = 0.5 * r2;
#pragma unroll
    for (int ox = 0; ox < 4; ++ox)
#pragma unroll
        for (int oy = 0; oy < 4; ++oy) k[ox][oy] = (Pa[ox][oy] - h * P[ox][oy]) * kap;
}

}  // namespace scasml
