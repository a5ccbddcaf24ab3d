// C-ABI of libromanhip.so (include/romanhip.h): error text, workspaces, context and options, diagnostics and profiling.
// Host code only.  The device-resident CALDIR is in caldir.hip, the ramp-fit plans in plan.hip, the chain driver in
// calibrate.hip and the stage-level entry points in stage.hip; kernels live in the other translation units.
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "rip_host.h"

static std::string g_create_error;

int rip_fail(rip_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_create_error = buf;
    return code;
}

void *rip_ws(rip_ctx *ctx, RipWs slot, size_t bytes) {
    if (ctx->ws_bytes[slot] >= bytes && ctx->ws[slot]) return ctx->ws[slot];
    if (ctx->ws[slot]) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);   // (the overlapped pre-pass uses workspaces too)
        (void)hipFree(ctx->ws[slot]);
        ctx->ws[slot] = nullptr;
        ctx->ws_bytes[slot] = 0;
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        rip_fail(ctx, RIP_ENOMEM, "hipMalloc(%zu bytes, workspace %d): %s", bytes, slot, hipGetErrorString(e));
        return nullptr;
    }
    ctx->ws[slot] = p;
    ctx->ws_bytes[slot] = bytes;
    return p;
}

// ---- the options of a context: one row each.  rip_set_option / rip_get_option (_f64 for the f64 row), rip_reset_options (the
// values a new context starts with) and rip_option_info all read this table; include/romanhip.h documents the rows.
struct RipOption {
    const char *name;
    double def, lo, hi;      // accepted: lo <= value <= hi (never NaN), anything else is RIP_EINVAL ...
    bool clamp_lo;           // ... except that a value below lo is stored as lo
    int rip_ctx::*i;         // where the value lives: an int member,
    double rip_ctx::*f64;    // or the f64 one
};
static const double ANY_LO = INT_MIN, ANY_HI = INT_MAX;   // unchecked
static const RipOption k_options[] = {
    {"fused", 1, ANY_LO, ANY_HI, false, &rip_ctx::use_fused, nullptr},
    {"chain2", 1, ANY_LO, ANY_HI, false, &rip_ctx::use_chain2, nullptr},
    {"chain_quad", 1, ANY_LO, ANY_HI, false, &rip_ctx::chain_quad, nullptr},
    {"skip_first", 1, ANY_LO, ANY_HI, false, &rip_ctx::skip_first, nullptr},
    {"chain_reserve", 8, 0, ANY_HI, true, &rip_ctx::chain_reserve, nullptr},
    {"prepass_form", -1, -1, 1, false, &rip_ctx::prepass_form, nullptr},
    {"prepass_gate", 0, 0, 1000000, false, &rip_ctx::prepass_gate, nullptr},
    {"pink_form", -1, ANY_LO, ANY_HI, false, &rip_ctx::pink_form, nullptr},
    {"overlap", -1, -1, 1, false, &rip_ctx::overlap_mode, nullptr},
    {"chain_dbg", 0, ANY_LO, ANY_HI, false, &rip_ctx::chain_dbg, nullptr},
    {"guard_band", 1e-5, 0, INFINITY, false, nullptr, &rip_ctx::guard_band},
};

// the row of this name among the int or the f64 options; nullptr (error recorded): no such option there
static const RipOption *find_option(rip_ctx *ctx, const char *name, bool f64) {
    for (const RipOption &o : k_options)
        if (name && (o.f64 != nullptr) == f64 && strcmp(name, o.name) == 0) return &o;
    (void)rip_fail(ctx, RIP_EINVAL, "unknown option %s", name ? name : "(null)");
    return nullptr;
}

static void store_option(rip_ctx *ctx, const RipOption &o, double v) {
    if (o.f64)
        ctx->*o.f64 = v;
    else
        ctx->*o.i = (int)v;
}

static int set_option(rip_ctx *ctx, const char *name, bool f64, double value) {
    const RipOption *o = find_option(ctx, name, f64);
    if (!o) return RIP_EINVAL;
    if (o->clamp_lo && value < o->lo) value = o->lo;
    if (!(value >= o->lo && value <= o->hi)) return rip_fail(ctx, RIP_EINVAL, "%s must be in %g .. %g", o->name, o->lo, o->hi);
    store_option(ctx, *o, value);
    return RIP_OK;
}

extern "C" {

#ifdef RIP_TIMING_BUILD
int rip_version(void) { return RIP_VERSION + RIP_TIMING_BUILD_FLAG; }
#else
int rip_version(void) { return RIP_VERSION; }
#endif

const char *rip_last_error(const rip_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rip_ctx_create(int device_id, rip_ctx **out) {
    if (!out) return rip_fail(nullptr, RIP_EINVAL, "rip_ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return rip_fail(nullptr, RIP_EHIP, "no HIP device visible (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return rip_fail(nullptr, RIP_EINVAL, "device %d out of range [0,%d)", device_id, ndev);
    e = hipSetDevice(device_id);
    if (e != hipSuccess) return rip_fail(nullptr, RIP_EHIP, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) return rip_fail(nullptr, RIP_EHIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return rip_fail(nullptr, RIP_EHIP, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id,
                        prop.gcnArchName);
    rip_ctx *ctx = new rip_ctx();
    rip_reset_options(ctx);
    ctx->device = device_id;
    ctx->ncu = prop.multiProcessorCount;
    // (queue priorities -- main stream above the second -- and a raised wave priority of the fused kernel were both tried against
    // the 4 % the overlapped pre-pass costs the fused kernel it runs beside: no effect, profiles/r04_summary.md)
    // A gate that holds the pre-pass back until the fused grid is resident (option "prepass_gate", calibrate.hip) moves its start
    // from the kernel boundary to 9 us behind it and gains 0.3-0.6 % of the wall time, inside the benchmark's noise: off by default.
    // The traces show where the rest goes: the first histogram kernel (16 KB of LDS) finds no room until the fused workgroups
    // begin to leave, 600 us on, so two thirds of the pre-pass run in the fused kernel's tail either way (profiles/prepass_gate.txt)
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return rip_fail(nullptr, RIP_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess) ctx->stream2 = nullptr;
    if (hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking) != hipSuccess) ctx->stream3 = nullptr;
    ctx->can_overlap = ctx->stream2 != nullptr;
    for (int i = 0; i < 2 && ctx->stream2; ++i)
        if (hipEventCreateWithFlags(&ctx->ev_tab[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_done[i], hipEventDisableTiming) != hipSuccess) {
            ctx->can_overlap = false;
        }
    // the words of the pre-pass gate (calibrate.hip); without them, or without the clock that bounds its wait, no gate is queued
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_id) == hipSuccess && khz > 0) ctx->wall_khz = khz;
    if (hipMalloc((void **)&ctx->gate_words, RIP_GATE_WORDS * 4) != hipSuccess) ctx->gate_words = nullptr;
    if (ctx->gate_words && hipMemset(ctx->gate_words, 0, RIP_GATE_WORDS * 4) != hipSuccess) {
        (void)hipFree(ctx->gate_words);
        ctx->gate_words = nullptr;
    }
    *out = ctx;
    return RIP_OK;
}

void rip_ctx_destroy(rip_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    for (auto &c : ctx->cals) free_cal(c);
    for (auto *p : ctx->plans)
        if (p) PlanFree()(p);
    rip_pink_release(ctx);
    for (hipEvent_t e : {ctx->ev_tab[0], ctx->ev_tab[1], ctx->ev_done[0], ctx->ev_done[1], ctx->ev_in, ctx->ev_pre, ctx->ev_frames, ctx->ev_fill, ctx->ev_pink, ctx->ev_ahead})
        if (e) (void)hipEventDestroy(e);
    for (void *p : ctx->ws)   // every workspace slot, the Level-1 synthesis ones included
        if (p) (void)hipFree(p);
    for (void *p : ctx->batch_buf)
        if (p) (void)hipFree(p);
    if (ctx->chain_dbg_buf) (void)hipFree(ctx->chain_dbg_buf);
    if (ctx->prepass_stamps) (void)hipFree(ctx->prepass_stamps);
    if (ctx->gate_words) (void)hipFree(ctx->gate_words);
    if (ctx->refread_dev) (void)hipFree(ctx->refread_dev);
    if (ctx->refread_host) (void)hipHostFree(ctx->refread_host);
    if (ctx->stream3) {
        (void)hipStreamSynchronize(ctx->stream3);
        (void)hipStreamDestroy(ctx->stream3);
    }
    (void)hipStreamDestroy(ctx->stream);
    if (ctx->stream2) {
        (void)hipStreamSynchronize(ctx->stream2);
        (void)hipStreamDestroy(ctx->stream2);
    }
    delete ctx;
}

int rip_synchronize(rip_ctx *ctx) {
    if (ctx->stream2) RIP_HIP(ctx, hipStreamSynchronize(ctx->stream2));
    RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RIP_OK;
}

void *rip_stream(rip_ctx *ctx) { return (void *)ctx->stream; }

// page-locked host memory for the caller's arrays: copies from / to it run at PCIe rate and asynchronously
void *rip_host_alloc(rip_ctx *ctx, size_t bytes) {
    void *p = nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess || hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void)rip_fail(ctx, RIP_ENOMEM, "rip_host_alloc: %zu bytes of page-locked memory", bytes);
        return nullptr;
    }
    return p;
}
void rip_host_free(rip_ctx *ctx, void *p) {
    (void)ctx;
    if (p) (void)hipHostFree(p);
}

int rip_option_info(int index, const char **name, int *def, int *lo, int *hi) {
    if (index < 0 || index >= (int)(sizeof k_options / sizeof k_options[0])) return 0;
    const RipOption &o = k_options[index];
    const auto as_int = [](double v) { return v <= INT_MIN ? INT_MIN : v >= INT_MAX ? INT_MAX : (int)v; };
    if (name) *name = o.name;
    if (def) *def = as_int(o.def);
    if (lo) *lo = as_int(o.lo);
    if (hi) *hi = as_int(o.hi);
    return o.f64 ? 2 : 1;
}

int rip_reset_options(rip_ctx *ctx) {
    for (const RipOption &o : k_options) store_option(ctx, o, o.def);
    return RIP_OK;
}

int rip_set_option(rip_ctx *ctx, const char *name, int value) { return set_option(ctx, name, false, value); }
int rip_set_option_f64(rip_ctx *ctx, const char *name, double value) { return set_option(ctx, name, true, value); }

int rip_get_option(rip_ctx *ctx, const char *name, int *value) {
    const RipOption *o = find_option(ctx, name, false);
    if (o) *value = ctx->*o->i;
    return o ? RIP_OK : RIP_EINVAL;
}
int rip_get_option_f64(rip_ctx *ctx, const char *name, double *value) {
    const RipOption *o = find_option(ctx, name, true);
    if (o) *value = ctx->*o->f64;
    return o ? RIP_OK : RIP_EINVAL;
}

// diagnostic builds (-DCH_STAMP): per-phase cycle sums of the fused kernel, summed over waves; clears the buffer
int rip_chain_stamps(rip_ctx *ctx, double out[9]) {
    const size_t n = 4096 * 9;
    if (!ctx->chain_dbg_buf) {
        RIP_HIP(ctx, hipMalloc((void **)&ctx->chain_dbg_buf, n * 8));
        RIP_HIP(ctx, hipMemset(ctx->chain_dbg_buf, 0, n * 8));
        for (int i = 0; i < 9; ++i) out[i] = 0;
        return RIP_OK;
    }
    RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<unsigned long long> h(n);
    RIP_HIP(ctx, hipMemcpy(h.data(), ctx->chain_dbg_buf, n * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < 9; ++i) out[i] = 0;
    for (size_t k = 0; k < n; ++k) out[k % 9] += (double)h[k];
    RIP_HIP(ctx, hipMemset(ctx->chain_dbg_buf, 0, n * 8));
    return RIP_OK;
}

// same buffer, per wave of a workgroup of nw waves: out[w * 9 + i] (diagnostic builds; tools/gpu_checks/stamp_roles.py)
int rip_chain_stamps_n(rip_ctx *ctx, int nw, double *out) {
    const size_t n = 4096 * 9;
    for (int i = 0; i < nw * 9; ++i) out[i] = 0;
    if (!ctx->chain_dbg_buf || nw < 1) return RIP_OK;
    RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<unsigned long long> h(n);
    RIP_HIP(ctx, hipMemcpy(h.data(), ctx->chain_dbg_buf, n * 8, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k) out[((k / 9) % (size_t)nw) * 9 + k % 9] += (double)h[k];
    RIP_HIP(ctx, hipMemset(ctx->chain_dbg_buf, 0, n * 8));
    return RIP_OK;
}

// diagnostic (tools/gpu_checks/prepass_stamps.py): clock stamps of the single-launch pre-pass, 16 per workgroup; the first call
// switches them on (out may be NULL), later calls copy the last launch's stamps out (nwg workgroups)
int rip_prepass_stamps(rip_ctx *ctx, int nwg, unsigned long long *out) {
    const size_t bytes = (size_t)4096 * 16 * 8;
    if (!ctx->prepass_stamps) {
        RIP_HIP(ctx, hipMalloc(&ctx->prepass_stamps, bytes));
        RIP_HIP(ctx, hipMemset(ctx->prepass_stamps, 0, bytes));
    }
    if (out && nwg > 0 && nwg <= 4096) {
        RIP_HIP(ctx, rip_synchronize(ctx) ? hipErrorUnknown : hipSuccess);
        RIP_HIP(ctx, hipMemcpy(out, ctx->prepass_stamps, (size_t)nwg * 16 * 8, hipMemcpyDeviceToHost));
    }
    return RIP_OK;
}

int rip_last_chain_form(rip_ctx *ctx) { return ctx ? ctx->last_form : RIP_EINVAL; }
int rip_last_chain_first_group(rip_ctx *ctx) { return ctx ? (ctx->last_form == 2 ? ctx->last_first_group : 0) : RIP_EINVAL; }
int rip_last_chain_bias_stream(rip_ctx *ctx) { return ctx ? (ctx->last_form == 2 ? ctx->last_bias_stream : 0) : RIP_EINVAL; }
// the gate of the last rip_calibrate: 0 none queued, 1 released by the counter, 2 gave up at its bound; *giveups (may be NULL):
// the give-ups of every gate of this context so far.  Waits for both streams.
int rip_last_prepass_gate(rip_ctx *ctx, int *giveups) {
    if (!ctx) return RIP_EINVAL;
    if (giveups) *giveups = 0;
    if (!ctx->gate_words) return 0;
    if (const int rc = rip_synchronize(ctx)) return rc;
    uint32_t w[2] = {0, 0};
    RIP_HIP(ctx, hipMemcpy(w, ctx->gate_words + RIP_GATE_GIVEUPS, sizeof w, hipMemcpyDeviceToHost));
    if (giveups) *giveups = (int)w[0];
    return ctx->last_gate ? (int)w[1] : 0;
}
int rip_caldir_first_group_safe(rip_ctx *ctx, int slot) {
    if (!ctx) return RIP_EINVAL;
    if (slot < 0 || slot >= (int)ctx->cals.size() || !ctx->cals[slot].valid) return rip_fail(ctx, RIP_EINVAL, "caldir slot %d is empty", slot);
    return ctx->cals[slot].first_group_safe ? 1 : 0;
}
int rip_caldir_bias_state(rip_ctx *ctx, int slot) {
    if (!ctx) return RIP_EINVAL;
    if (slot < 0 || slot >= (int)ctx->cals.size() || !ctx->cals[slot].valid) return rip_fail(ctx, RIP_EINVAL, "caldir slot %d is empty", slot);
    const RipCal &c = ctx->cals[slot];
    return c.has_bias ? RIP_BIAS_PRESENT : (c.bias_dropped ? RIP_BIAS_DROPPED : RIP_BIAS_ABSENT);
}
int rip_last_chain_geometry(rip_ctx *ctx, int out[8]) {
    if (!ctx || !out) return RIP_EINVAL;
    for (int i = 0; i < 8; ++i) out[i] = ctx->last_form == 2 ? ctx->last_geo[i] : 0;
    return RIP_OK;
}

int rip_profile_enable(rip_ctx *ctx, int on) {
    ctx->prof = on != 0;
    return RIP_OK;
}

int rip_profile_read(rip_ctx *ctx, double out_ms[4], int *ncalls) {
    RIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 4; ++i) out_ms[i] = 0.0;
    if (ctx->stream2) RIP_HIP(ctx, hipStreamSynchronize(ctx->stream2));
    const size_t n = ctx->prof_events.size() / 6;  // per call: pre-pass begin/end, then 4 marks on the main stream
    for (size_t c = 0; c < n; ++c) {
        const hipEvent_t *e = &ctx->prof_events[c * 6];
        float ms = 0.f;
        RIP_HIP(ctx, hipEventElapsedTime(&ms, e[0], e[1]));
        out_ms[0] += ms;
        for (int i = 1; i < 4; ++i) {
            RIP_HIP(ctx, hipEventElapsedTime(&ms, e[1 + i], e[2 + i]));
            out_ms[i] += ms;
        }
    }
    for (hipEvent_t e : ctx->prof_events) (void)hipEventDestroy(e);
    ctx->prof_events.clear();
    if (ncalls) *ncalls = (int)n;
    return RIP_OK;
}

}  // extern "C"
