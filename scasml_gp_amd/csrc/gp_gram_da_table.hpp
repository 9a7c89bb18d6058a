// The one statement of K_a = dK/da per collocation pair, shared by gp_evidence.hip (which contracts it) and gp_loo.hip
// (which writes rows of it).  An entry of K is P(ox, oy) kappa with kappa = exp(-a r^2 / 2), so the entry of K_a is (P_a - r^2 P / 2) kappa with
// P_a = dP/da at fixed geometry; ops: 0 = I, 1 = Lap, 2 = dt, 3 = div (the operator polynomials P of gp_gram_mfma_kernel, gp_train.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace scasml {

// ka[ox][oy] <- the pair's 16 entries of K_a from its geometry: r2 = |x - y|^2 with the time coordinate (clamped at 0 by the caller),
// rt = t_x - t_y, S = sum x - sum y over the spatial coordinates, fd = d.  Entries a caller does not use cost nothing once its loops are unrolled.
__device__ __forceinline__ void gram_da_pair(double a, double fd, double r2, double rt, double S, double (&ka)[4][4]) {
    double rho2 = fma(-rt, rt, r2);
    rho2 = rho2 < 0.0 ? 0.0 : rho2;
    const double kap = exp(-0.5 * a * r2);
    const double lap = a * a * rho2 - a * fd, lap_a = 2.0 * a * rho2 - fd;
    const double aS = a * S, art = a * rt, mix = aS * lap - 2.0 * a * aS;
    const double mix_a = S * lap + aS * lap_a - 4.0 * aS, tl_a = rt * lap + art * lap_a;
    const double c3 = 2.0 * fd + 4.0, c2 = fd * fd + 2.0 * fd;
    const double ll = a * a * a * a * rho2 * rho2 - c3 * a * a * a * rho2 + c2 * a * a;
    const double ll_a = 4.0 * a * a * a * rho2 * rho2 - 3.0 * c3 * a * a * rho2 + 2.0 * c2 * a;
    const double P[4][4] = {
        {1.0, lap, art, aS},
        {lap, ll, art * lap, mix},
        {-art, -art * lap, a - art * art, -art * aS},
        {-aS, -mix, -art * aS, a * fd - aS * aS}};
    const double Pa[4][4] = {
        {0.0, lap_a, rt, S},
        {lap_a, ll_a, tl_a, mix_a},
        {-rt, -tl_a, 1.0 - 2.0 * art * rt, -2.0 * art * S},
        {-S, -mix_a, -2.0 * art * S, fd - 2.0 * aS * S}};
    const double h = 0.5 * r2;
#pragma unroll
    for (int ox = 0; ox < 4; ++ox)
#pragma unroll
        for (int oy = 0; oy < 4; ++oy) ka[ox][oy] = (Pa[ox][oy] - h * P[ox][oy]) * kap;
}

}  // namespace scasml
