// Staged Picard tree: the ACCUMULATE walk of picard_tree.hpp one subtree level at a time, with f and g read from a per-site
// values buffer instead of evaluated -- the path of equations outside the registry, whose f and g are batched torch functions the
// driver calls between the stages (solvers/_picard.py).
//
// Stage S takes every level-S subtree (base site, origin site) of the tree, GENERATE's points and, per site, g (terminal samples)
// or f+ / f- (nodes), and writes the subtree's clipped (u, z) to the site-major uz buffer at its base site (S = n: to out_uz).
// Mapping as in SCASML_MODE_MLP: G = ceil_pow2(kp / 4) lanes per (subtree, root) work item, a float4 of dims per lane; the grid
// is flat over (entry, root group) so that a wave's subtree, hence its site base, is wave-uniform.  No sum over dims is taken
// (f and g come from memory), so the group needs no shuffle.  The level is a runtime loop over plan.term[S][l]: one
// instantiation per variant.
//
// SE (scasml_picard_stage_stderr, the root call S = plan.n only): the same walk also estimates the Monte-Carlo standard errors of u and
// of every z_i with the accumulators of picard_tree.hpp (SeTerm, SeTerm4), summand by summand as Walker's TOP frame does in
// SCASML_MODE_MLP, and stores them as picard_se_uz_kernel does.  u and z are accumulated by the statements of the plain instances.

#include "picard_tree.hpp"

namespace scasml {

struct StageArgs {
    scasml_plan plan;
    const float *points;
    const float2 *vals;
    const int2 *entries;
    float *uz;
    float *out;
    int64_t B, Bs, ppr, n_entries, groups;   // groups: root groups (64 / G roots each) per entry
    uint32_t k0, k1, stream, root0;
    int32_t S, d, G, logG, kp;
    float T, mu, sigma, clip;
    float *out_se;   // SE only: B rows of 1 + d, the standard errors of (u, z_1 .. z_d).  Last: the plain instances' arguments stay where they were
};

template <int VAR, bool SE = false>
__global__ __launch_bounds__(256) void picard_stage_kernel(const StageArgs a) {
    normal_table_to_lds();   // every thread, before any return
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= a.n_entries * a.groups) return;
    const int64_t e = wave / a.groups;
    const int2 ent = a.entries[e];                                  // wave-uniform
    const int S = a.S;
    const int64_t base = ent.x, origin = ent.y;
    if (base < 0 || origin < 0 || origin >= a.ppr || base + a.plan.sites[S] > a.ppr - 1) return;   // not a subtree of this tree

    int64_t local = (wave - e * a.groups) * (64 >> a.logG) + (lane >> a.logG);
    const bool valid = local < a.B;
    if (!valid) local = a.B - 1;                                    // idle lanes shadow the last root; their stores are masked
    const uint32_t gl = (uint32_t)(lane & (a.G - 1));
    const uint32_t root = a.root0 + (uint32_t)local;
    const int dim0 = 4 * (int)gl;
    const bool row_lane = dim0 < a.kp;
    const float4 mask = live_mask(dim0, a.d);
    // site-major rows: the site's block starts at a wave-uniform 64-bit base, the lane adds a 32-bit offset (site_stride * kp < 2^32)
    const int64_t block = a.Bs * a.kp;
    const uint32_t off4 = (uint32_t)((local * a.kp + (row_lane ? dim0 : 0)) >> 2);
    auto load = [&](int64_t site) { return reinterpret_cast<const float4 *>(a.points + site * block)[off4]; };
    auto val = [&](int64_t site) { return (a.vals + site * a.Bs)[local]; };
    auto sel = [&](float4 v) {   // the lane's live dims of v, zero elsewhere (no 0 * inf)
        return make_float4(mask.x != 0.0f ? v.x : 0.0f, mask.y != 0.0f ? v.y : 0.0f, mask.z != 0.0f ? v.z : 0.0f, mask.w != 0.0f ? v.w : 0.0f);
    };

    // the origin: the parent node's stored point (X_k, t_k), or the root row
    const float4 x = sel(load(origin));
    const float t = a.points[origin * block + local * a.kp + a.d];
    const float tau = fmaxf(a.T - t, 0.0f);
    const int mg = a.plan.mg[S];
    float su = 0.0f;
    float4 sz = f4(0.0f);
    [[maybe_unused]] float var_u = 0.0f;                            // SE: the variance estimates of u and of this lane's four dims of z, summed over the terms
    [[maybe_unused]] float4 var_z = f4(0.0f);
    SeTerm<SE> st;
    SeTerm4<SE> zt;
    if constexpr (SE) {
        st.begin();
        zt.begin();
    }
    for (int m = 0; m < mg; ++m) {                                  // MLP.py:175-202
        const int64_t site = base + m;
        // The terminal normals are replayed, never recovered from the stored X_T as ACCUMULATE does above kReadbackMinVol: a
        // recovered normal is off by ~3e-8 / vol, and the z estimator multiplies that by g / (T - t).  ACCUMULATE's g is the
        // surrogate's defect (small); here g is the whole terminal value, O(1), and a full-history child drawn close to T (vol just
        // above the threshold) put 2e-4 into z at d = 100.  Replayed, the normals are GENERATE's own bits.
        const float4 nrm = mul4(normal4(gl, (uint32_t)site, root, a.stream, a.k0, a.k1), mask);
        const float g = val(site).x;
        su += g;
        if constexpr (SE) st.add(g, m == 0);
        sz = fma4(g, nrm, sz);
        if constexpr (SE) zt.add(f4_scale(nrm, g), m == 0);        // P_m = g nrm: what the line above adds
    }
    const float inv_mg = rcp_fast((float)mg);
    if constexpr (SE) var_u += st.close(mg) * (inv_mg * inv_mg);    // the summands are g / mg
    float u = su * inv_mg;
    const float zs = inv_mg * rcp_fast(VAR == 0 ? tau + 1e-6f : tau);   // MLP.py:201 / MLP_full_history.py:122
    if constexpr (SE) zt.close_into(var_z, mg, zs * zs);            // the summands are P_m zs (at the full history's T - t = 0: inf P_m, never finite)
    float4 z = sel(f4_scale(sz, zs));
    int64_t o = mg;
    const float inv_sigma = 1.0f / a.sigma;
    for (int l = 0; l < S; ++l) {
        const scasml_term &tm = a.plan.term[S][l];
        const int q = tm.q, mc = tm.mc;
        const int64_t skip = (int64_t)tm.sites_l + tm.sites_lm1;
        const float inv_mc = rcp_fast((float)mc);
        if constexpr (SE) {
            st.begin();
            zt.begin();
        }
        for (int m = 0; m < mc; ++m) {
            [[maybe_unused]] float ym = 0.0f;                              // SE: what sample path m adds to u
            [[maybe_unused]] float4 zm = f4(0.0f);                         // and to z
            for (int k = 0; k < q; ++k) {
                const int64_t site = base + o;
                o += 1 + skip;
                float wk, dplus, dminus;
                float4 wvec;
                if constexpr (VAR == 0) {
                    // X_k read back; W_k = (X_k - x - mu c_k) / sigma, as ACCUMULATE recovers it
                    const float ck = tau * tm.cfrac[k];
                    wvec = mul4(fma4(inv_sigma, add4(load(site), -a.mu * ck), f4_scale(x, -inv_sigma)), mask);
                    wk = tau * tm.wfrac[k];
                    dplus = rcp_fast(fmaf(tau, tm.dplus[k], 1e-6f));      // MLP.py:249 (stale delta_t)
                    dminus = rcp_fast(fmaf(tau, tm.cfrac[k], 1e-6f));     // MLP.py:270
                } else {                                                   // MLP_full_history.py:133-159: replayed
                    const float D = uniform_tau((uint32_t)site, root, a.stream, a.k0, a.k1) * tau;
                    wvec = mul4(normal4(gl, (uint32_t)site, root, a.stream, a.k0, a.k1), mask);
                    wk = tau;
                    dplus = dminus = __builtin_amdgcn_rsqf(D + 1e-6f);
                }
                const float2 fv = val(site);
                float y = fv.x * (wk * inv_mc);
                u += y;                                                    // MLP.py:248
                if constexpr (SE) ym += y;
                z = fma4(y * dplus, wvec, z);                              // MLP.py:249
                if constexpr (SE) zm = fma4(y * dplus, wvec, zm);
                if (l > 0) {
                    y = fv.y * (wk * inv_mc);
                    u -= y;                                                // MLP.py:269
                    if constexpr (SE) ym -= y;
                    z = fma4(-y * dminus, wvec, z);                        // MLP.py:271
                    if constexpr (SE) zm = fma4(-y * dminus, wvec, zm);
                }
            }
            if constexpr (SE) {
                st.add(ym, m == 0);
                zt.add(zm, m == 0);
            }
        }
        if constexpr (SE) {
            var_u += st.close(mc);
            zt.close_into(var_z, mc, 1.0f);
        }
    }
    u = clip1(u, a.clip);                                                  // MLP.py:272-274, NaN kept
    z = clip4(z, a.clip);
    if (!valid) return;
    if (!SE && S < a.plan.n) {                                             // (SE: the entry point admits the root call only)
        if (!row_lane) return;
        // (z_1 .. z_d, u, 0 ...): a point row's layout with u in the time column
        const float4 r = make_float4(mask.x != 0.0f ? z.x : (dim0 + 0 == a.d ? u : 0.0f), mask.y != 0.0f ? z.y : (dim0 + 1 == a.d ? u : 0.0f),
                                     mask.z != 0.0f ? z.z : (dim0 + 2 == a.d ? u : 0.0f), mask.w != 0.0f ? z.w : (dim0 + 3 == a.d ? u : 0.0f));
        reinterpret_cast<float4 *>(a.uz + base * block)[off4] = r;
    } else {
        float *out = a.out + local * (a.d + 1);
        if (gl == 0) out[0] = u;
        store_z(out, dim0, a.d, z);
        if constexpr (SE) {
            // as picard_se_uz_kernel: Var <= 0 (rounding) gives 0, a NaN Var stays NaN; padding dims (which may hold 0 * inf) are not stored
            float *se = a.out_se + local * (a.d + 1);
            if (gl == 0) se[0] = var_u <= 0.0f ? 0.0f : sqrtf(var_u);
            store_z(se, dim0, a.d, make_float4(var_z.x <= 0.0f ? 0.0f : sqrtf(var_z.x), var_z.y <= 0.0f ? 0.0f : sqrtf(var_z.y),
                                               var_z.z <= 0.0f ? 0.0f : sqrtf(var_z.z), var_z.w <= 0.0f ? 0.0f : sqrtf(var_z.w)));
        }
    }
}

}  // namespace scasml

using namespace scasml;

// scasml_picard_stage and scasml_picard_stage_stderr (se: the latter; `who` prefixes the messages): one validation, one launch geometry
static int stage_run(const char *who, bool se, const scasml_problem *prob, const scasml_plan *plan, int32_t stage, const int32_t *entries, int64_t n_entries,
                     int64_t B, int64_t site_stride, scasml_rng rng, const float *points, const float *values, float *uz, float *out_uz, float *out_se,
                     void *stream) {
    if (const int rc = check_batch(who, prob, plan, B, site_stride)) return rc;
    if (prob->d < 1 || prob->d > SCASML_MAX_DIM) return fail(SCASML_ERR_UNSUPPORTED, "%s: d=%d outside 1..%d", who, prob->d, SCASML_MAX_DIM);
    if (plan->variant != 0 && plan->variant != 1) return fail(SCASML_ERR_ARG, "%s: variant %d", who, plan->variant);
    if (plan->n < 1 || plan->n > SCASML_MAX_LEVEL) return fail(SCASML_ERR_UNSUPPORTED, "%s: level n=%d outside 1..%d", who, plan->n, SCASML_MAX_LEVEL);
    if (stage < 1 || stage > plan->n) return fail(SCASML_ERR_ARG, "%s: stage %d outside 1..%d", who, stage, plan->n);
    if (rng.flags != 0) return fail(SCASML_ERR_UNSUPPORTED, "%s: rng.flags 0x%x: the staged path runs on the Philox stream only", who, rng.flags);
    if (rng.world != 1 || rng.rank != 0) return fail(SCASML_ERR_UNSUPPORTED, "%s: sample sharding (world %d) is not supported", who, rng.world);
    if (n_entries < 1 || !entries) return fail(SCASML_ERR_ARG, "%s: no subtree entries", who);
    int np, l;
    if (first_bad_term(*plan, np, l)) return fail(SCASML_ERR_ARG, "%s: bad term [%d][%d]", who, np, l);
    if (B == 0) return 0;
    if (!points || !values) return fail(SCASML_ERR_ARG, "%s: points and values are required", who);
    if (!se) {
        if (stage < plan->n ? !uz : !out_uz) return fail(SCASML_ERR_ARG, "%s: stage %d of %d needs %s", who, stage, plan->n, stage < plan->n ? "uz" : "out_uz");
    } else {    // what has no estimate is refused, never answered with a partial number (as scasml_picard_tree_stderr)
        if (stage != plan->n) return fail(SCASML_ERR_ARG, "%s: stage %d of %d: only the root call has an estimate", who, stage, plan->n);
        if (!out_uz || !out_se) return fail(SCASML_ERR_ARG, "%s: %s is null", who, out_uz ? "out_se_uz" : "out_uz");
        if (plan->mg[plan->n] < 2)
            return fail(SCASML_ERR_UNSUPPORTED, "%s: the terminal term of level %d has %d sample: no estimable variance", who, plan->n, plan->mg[plan->n]);
        for (int t = 0; t < plan->n; ++t)
            if (plan->term[plan->n][t].mc < 2)
                return fail(SCASML_ERR_UNSUPPORTED, "%s: term [%d][%d] has %d sample path: no estimable variance", who, plan->n, t, plan->term[plan->n][t].mc);
    }
    StageArgs a;
    const int rpw = fill_common_args(a, prob, plan, rng, B, site_stride);
    a.points = points;
    a.vals = reinterpret_cast<const float2 *>(values);
    a.entries = reinterpret_cast<const int2 *>(entries);
    a.uz = uz;
    a.out = out_uz;
    a.out_se = se ? out_se : nullptr;
    a.n_entries = n_entries;
    a.S = stage;
    if (a.Bs * a.kp >= ((int64_t)1 << 32)) return fail(SCASML_ERR_UNSUPPORTED, "%s: site_stride %lld too large for 32-bit row offsets", who, (long long)a.Bs);
    a.groups = (B + rpw - 1) / rpw;
    const int64_t blocks = (n_entries * a.groups + 3) / 4;
    if (blocks > 0x7FFFFFFF) return fail(SCASML_ERR_UNSUPPORTED, "%s: batch too large", who);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks);
    if (se) {
        if (plan->variant == 0) hipLaunchKernelGGL((picard_stage_kernel<0, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((picard_stage_kernel<1, true>), grid, dim3(256), 0, s, a);
        return check_launch("picard_stage_stderr launch");
    }
    if (plan->variant == 0) hipLaunchKernelGGL((picard_stage_kernel<0>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((picard_stage_kernel<1>), grid, dim3(256), 0, s, a);
    return check_launch("picard_stage launch");
}

extern "C" int scasml_picard_stage(const scasml_problem *prob, const scasml_plan *plan, int32_t stage, const int32_t *entries, int64_t n_entries,
                                   int64_t B, int64_t site_stride, scasml_rng rng, const float *points, const float *values, float *uz,
                                   float *out_uz, void *stream) {
    return stage_run("picard_stage", false, prob, plan, stage, entries, n_entries, B, site_stride, rng, points, values, uz, out_uz, nullptr, stream);
}

extern "C" int scasml_picard_stage_stderr(const scasml_problem *prob, const scasml_plan *plan, int32_t stage, const int32_t *entries, int64_t n_entries,
                                          int64_t B, int64_t site_stride, scasml_rng rng, const float *points, const float *values, float *out_uz,
                                          float *out_se_uz, void *stream) {
    return stage_run("picard_stage_stderr", true, prob, plan, stage, entries, n_entries, B, site_stride, rng, points, values, nullptr, out_uz, out_se_uz,
                     stream);
}
