// Ramp-fit plans (include/romanhip.h: rip_plan_create, rip_plan_destroy): the host tables and their device image.
// Host code only.
#include <string.h>

#include <cmath>
#include <memory>

#include "rip_host.h"

// weights of fit variant v (0: the full ramp, the caller's K; v > 0: the two-point weights of the ramp truncated to g groups,
// fitting.py:165-169)
static std::vector<float> variant_weights(const rip_plan_desc *d, int v, int g, int start) {
    std::vector<float> K(g, 0.0f);
    if (v == 0) {
        for (int i = 0; i < g; ++i) K[i] = d->K[i];
    } else {
        K[g - 1] = 1.0f / (d->tbar[g - 1] - d->tbar[start]);
        K[start] = -K[g - 1];
    }
    return K;
}

extern "C" {

// 1: a plan made from `d` excludes the first group and gives group 0 the weight zero (+-0) in the full-ramp weights and in every
// truncated variant's -- what the fused kernel's form that skips group 0 rests on (rip_plan_create records the same of the
// weights it uploads); 0 otherwise.  Host arithmetic only.
int rip_plan_desc_first_weight_zero(const rip_plan_desc *d) {
    if (!d || !d->exclude_first || d->ngrp < 3 || d->ngrp > RIP_MAX_GROUPS) return 0;
    const int G = d->ngrp, nvar = 1 + (G - 4 > 0 ? G - 4 : 0);
    for (int v = 0; v < nvar; ++v)
        if (variant_weights(d, v, v == 0 ? G : G - v, 1)[0] != 0.0f) return 0;
    return 1;
}

int rip_plan_create(rip_ctx *ctx, const rip_plan_desc *d, int *plan_id) {
    if (!d || !plan_id) return rip_fail(ctx, RIP_EINVAL, "plan: NULL argument");
    const int G = d->ngrp, start = d->exclude_first ? 1 : 0;
    if (G < 2 + start || G > RIP_MAX_GROUPS) return rip_fail(ctx, RIP_EINVAL, "plan: %d groups unsupported", G);
    const int nvar = 1 + (G - 3 - start > 0 ? G - 3 - start : 0);
    if (d->nvariants != nvar) return rip_fail(ctx, RIP_EINVAL, "plan: expected %d fit variants, got %d", nvar, d->nvariants);
    std::unique_ptr<RipPlan, PlanFree> p(new RipPlan());
    RipPlanHeader &h = p->h;
    memset(&h, 0, sizeof h);
    h.ngrp = G;
    h.start = start;
    h.nvariants = nvar;
    h.do_not_flag_first = d->do_not_flag_first;
    h.sa = d->sthresh_a;
    h.dsb = d->sthresh_b - d->sthresh_a;
    h.loglen = std::log(d->ithresh_b / d->ithresh_a);
    h.ia = (float)d->ithresh_a;
    h.ib = (float)d->ithresh_b;
    for (int i = 0; i < G; ++i) {
        h.tbar[i] = d->tbar[i];
        h.tau[i] = d->tau[i];
        h.nreads[i] = (float)d->nreads[i];
    }
    for (int v = 0; v < nvar; ++v) {
        const int g = (v == 0) ? G : G - v;  // G, G-1, ..., 3+start  (fitting.py:326)
        if (d->variant_g[v] != g)
            return rip_fail(ctx, RIP_EINVAL, "plan: variant %d covers %d groups, expected %d", v, d->variant_g[v], g);
        RipVariant rv;
        rv.g = g;
        rv.coef = d->variant_coef[v];
        rv.rfac = d->variant_rfac[v];
        rv.k_ofs = (int)p->kvals.size();
        const std::vector<float> K = variant_weights(d, v, g, start);
        p->kvals.insert(p->kvals.end(), K.begin(), K.end());
        rv.diff_ofs = (int)p->diffs.size();
        rv.ndiff = 0;
        for (int i = start; i < g - 1; ++i) {  // fitting.py:225-229
            const int dimax = (i == g - 2 || g - 1 - start == 2) ? 1 : 2;
            for (int di = 1; di <= dimax; ++di) {
                RipDiff df;
                df.i = i;
                df.j = i + di;
                df.dt = d->tbar[i + di] - d->tbar[i];
                const float inv = 1.0f / df.dt;
                // fast-path variance coefficients: var = A*read^2 + B*dvardt, sums in f64
                double A = 0.0, B = 0.0, Babs = 0.0;
                for (int a = 0; a < g; ++a) {
                    const double wa = ((a == df.j) ? (double)inv : (a == df.i) ? (double)(-inv) : 0.0) - (double)K[a];
                    A += wa * wa / (double)d->nreads[a];
                    B += wa * wa * (double)d->tau[a];
                    Babs += wa * wa * (double)d->tau[a];
                    for (int b = 0; b < a; ++b) {
                        const double wb = ((b == df.j) ? (double)inv : (b == df.i) ? (double)(-inv) : 0.0) - (double)K[b];
                        B += 2.0 * wa * wb * (double)d->tbar[b];
                        Babs += std::fabs(2.0 * wa * wb) * (double)d->tbar[b];
                    }
                }
                // the reference rounds each term of the variance in f32/f64 as it goes; with cancellation between
                // the terms of B the relative error of any evaluation order is amplified by Babs/B
                const double amp = (B > 0.0) ? Babs / B : 1.0;
                df.relerr = (float)(2.5e-7 * (1.0 + amp) + 5e-7);
                df.A = (float)A;
                df.B = (float)B;
                df.inv_dt = inv;
                p->diffs.push_back(df);
                rv.ndiff++;
            }
        }
        p->variants.push_back(rv);
    }
    // device image: header | variants | K | diffs (each section 16-byte aligned)
    auto al = [](size_t x) { return (x + 15) / 16 * 16; };
    const size_t o_var = al(sizeof(RipPlanHeader));
    const size_t o_k = o_var + al(p->variants.size() * sizeof(RipVariant));
    const size_t o_d = o_k + al(p->kvals.size() * sizeof(float));
    const size_t o_dense = o_d + al(p->diffs.size() * sizeof(RipDiff));
    p->bytes = o_dense + al(sizeof(RipDense));
    {  // dense view of variant 0 (the full ramp) for the register-resident fit
        RipDense &dn = p->dense;
        memset(&dn, 0, sizeof dn);
        for (int i = 0; i < G; ++i) dn.K2[i] = d->K[i];
        const RipVariant &v0 = p->variants[0];
        double amin = 1e301;
        for (int k = 0; k < v0.ndiff; ++k) {
            const RipDiff &df = p->diffs[v0.diff_ofs + k];
            const int i = df.i, di = df.j - df.i, ps = 2 * (i / 2) + (di - 1), e = i & 1;
            // the mask holds the differences of up to 16 groups, the most a fused form fits (highest bit 28: i = 14, di = 1); a
            // longer ramp (ps up to 63) keeps valid = 0, which is no form's mask (rip_full_valid_of is non-zero for every
            // count), so no shift by 32 or more is ever formed
            if (G <= 16) dn.valid |= 1u << (2 * ps + e);
            dn.kidx[2 * ps + e] = k;
            dn.pairs[ps].inv_dt[e] = df.inv_dt;
            dn.pairs[ps].A[e] = df.A;
            dn.pairs[ps].B[e] = df.B;
            // acceptance factors of the packed fast path (device_rampfit.h, fit_full_pk_a): r = relerr + 4.1e-7 covers
            // the variance approximation and the part of the difference's rounding that scales with the significance
            const double r = (double)df.relerr + 4.1e-7;
            if (r < 9.9e-3) {
                dn.pairs[ps].k1[e] = std::nextafter((float)((1.0 / (1.0 - r)) * (1.0 + 4e-7)), INFINITY);
            } else {  // never accepted: the exact path decides
                dn.pairs[ps].k1[e] = INFINITY;
            }
            amin = (df.B >= 0.0f) ? std::fmin(amin, (double)df.A) : 0.0;
        }
        dn.amin = (v0.ndiff > 0 && amin > 0.0 && amin < 1e300) ? (float)(amin * (1.0 - 1e-6)) : 0.0f;
        for (int ps = 0; ps < RIP_MAX_GROUPS; ++ps)
            for (int e = 0; e < 2; ++e) {
                const int bit = 2 * ps + e;
                const bool used = bit < 32 && ((dn.valid >> bit) & 1u);
                if (!used) dn.pairs[ps].A[e] = 1.0f;  // keeps the approximate variance positive for unused slots
                dn.pairs[ps].k2[e] = 2.0f - dn.pairs[ps].k1[e];  // the subtraction the kernels made per difference
            }
    }
    // group 0's weight in every variant: the one question, asked of the description the weights above were made from
    // (variant_weights serves both)
    p->k0_zero = rip_plan_desc_first_weight_zero(d) == 1;
    std::vector<char> img(p->bytes, 0);
    memcpy(img.data(), &h, sizeof h);
    memcpy(img.data() + o_var, p->variants.data(), p->variants.size() * sizeof(RipVariant));
    memcpy(img.data() + o_k, p->kvals.data(), p->kvals.size() * sizeof(float));
    if (!p->diffs.empty()) memcpy(img.data() + o_d, p->diffs.data(), p->diffs.size() * sizeof(RipDiff));
    memcpy(img.data() + o_dense, &p->dense, sizeof(RipDense));
    hipError_t e = hipMalloc(&p->dev, p->bytes);
    if (e == hipSuccess) e = hipMemcpy(p->dev, img.data(), p->bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return rip_fail(ctx, RIP_EHIP, "plan upload: %s", hipGetErrorString(e));
    p->d_variants = reinterpret_cast<const RipVariant *>((char *)p->dev + o_var);
    p->d_k = reinterpret_cast<const float *>((char *)p->dev + o_k);
    p->d_diffs = reinterpret_cast<const RipDiff *>((char *)p->dev + o_d);
    p->d_dense = reinterpret_cast<const RipDense *>((char *)p->dev + o_dense);
    int id = -1;
    for (size_t i = 0; i < ctx->plans.size(); ++i)
        if (!ctx->plans[i]) {
            id = (int)i;
            break;
        }
    if (id < 0) {
        ctx->plans.push_back(nullptr);
        id = (int)ctx->plans.size() - 1;
    }
    ctx->plans[id] = p.release();
    *plan_id = id;
    return RIP_OK;
}

int rip_plan_destroy(rip_ctx *ctx, int id) {
    if (id < 0 || id >= (int)ctx->plans.size() || !ctx->plans[id]) return rip_fail(ctx, RIP_EINVAL, "plan %d does not exist", id);
    RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PlanFree()(ctx->plans[id]);
    ctx->plans[id] = nullptr;
    return RIP_OK;
}

}  // extern "C"

RipPlan *get_plan(rip_ctx *ctx, int id) {
    if (id < 0 || id >= (int)ctx->plans.size() || !ctx->plans[id]) {
        rip_fail(ctx, RIP_EINVAL, "plan %d does not exist", id);
        return nullptr;
    }
    return ctx->plans[id];
}
