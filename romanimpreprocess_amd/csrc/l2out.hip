// The planes of the L2 tree, made on the device from the chain's results and the Level-1 cube (include/romanhip.h):
//   gen_cal_image.py:653-662   make_asdf(slope[act], err_read[act]**2, err_poisson[act]**2, dq = pdq[act])   -> rip_stage_l2_planes
//     (romanisim's make_asdf is not in the reference tree: err = sqrt(var_rnoise + var_poisson))
//   oututils.py:52-55          dq_border_ref_pix_{left,right,top,bottom} = edges of the pixel flags           -> rip_stage_l2_planes
//   typefix.py:38-56           err, var_poisson, var_rnoise as float16 under newer schemas                    -> rip_stage_l2_planes
//   oututils.py:46-49          border_ref_pix_{left,right,top,bottom} = f32 edges of the Level-1 cube         -> rip_stage_l2_refpix_strips
// The planes kernel is a stream: up to four full-frame reads, up to five active-region writes, no LDS.  Where nb and nx are
// multiples of 4 and every pointer in use sits on a 16-byte boundary (8 bytes for a float16 plane) -- the standard frame, nb = 4 --
// the first active pixel of every input and output row is 16-byte aligned and a lane takes four adjacent pixels of a row: 16-byte
// loads and stores, 8-byte stores for float16.  Everything else goes one pixel per lane.  Capped grid, grid-stride loop, 64-bit
// indices; a lane divides once and then steps (row, position in the row) by the grid's stride.
// Arithmetic: f32 products, an f32 sum, sqrtf (the correctly rounded form under this build's flags; __fsqrt_rn is not), and for
// float16 one v_cvt_f16_f32 in the default mode: round to nearest-even, subnormals kept.  stats.hip (rip_stats_l2_pack) holds a
// second statement of err = sqrt(err_read^2 + err_poisson^2) for the harness' packed stacks; the two agree bit for bit.
#include <cmath>

#include "rip_host.h"

// The vector body's stores are non-temporal: every plane is written once and next read by a copy engine or another kernel
// (profiles/l2_out.txt).  -DRIP_L2_PLAIN_STORES=1 builds the library without the hint: the variant
// tools/gpu_checks/l2_out_timing.py --variant times against this one.
#ifndef RIP_L2_PLAIN_STORES
#define RIP_L2_PLAIN_STORES 0
#endif

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr unsigned L2_BLOCK = 256, L2_MAX_BLOCKS = 2048;   // 8 blocks for each of the 256 compute units

struct L2Planes {   // device pointers; an output that is null is not made
    const uint32_t *slope;   // (the crop moves bits)
    const float *err_read, *err_poisson;
    const uint32_t *pixeldq;
    uint32_t *data, *dq;
    void *var_rnoise, *var_poisson, *err;
};

__device__ __forceinline__ uint32_t f16_bits(float x) {
    const _Float16 h = (_Float16)x;   // round to nearest-even
    return (uint32_t)__builtin_bit_cast(uint16_t, h);
}

template <int V>
__device__ __forceinline__ void load_words(const uint32_t *p, uint32_t (&w)[V]) {
    if constexpr (V == 4) {
        const u32x4 q = *reinterpret_cast<const u32x4 *>(p);
        w[0] = q[0], w[1] = q[1], w[2] = q[2], w[3] = q[3];
    } else {
        w[0] = *p;
    }
}

template <int V, bool NT>
__device__ __forceinline__ void store_words(uint32_t *p, const uint32_t (&w)[V]) {
    if constexpr (V == 4) {
        u32x4 q;
        q[0] = w[0], q[1] = w[1], q[2] = w[2], q[3] = w[3];
        if (NT)
            __builtin_nontemporal_store(q, reinterpret_cast<u32x4 *>(p));
        else
            *reinterpret_cast<u32x4 *>(p) = q;
    } else {
        *p = w[0];
    }
}

// V f32 values to plane `p` at element `at`, as they are or rounded to float16
template <int V, bool F16, bool NT>
__device__ __forceinline__ void store_values(void *p, size_t at, const float (&v)[V]) {
    if constexpr (!F16) {
        uint32_t w[V];
#pragma unroll
        for (int j = 0; j < V; ++j) w[j] = __float_as_uint(v[j]);
        store_words<V, NT>(reinterpret_cast<uint32_t *>(p) + at, w);
    } else if constexpr (V == 4) {
        u32x2 q;
        q[0] = f16_bits(v[0]) | (f16_bits(v[1]) << 16), q[1] = f16_bits(v[2]) | (f16_bits(v[3]) << 16);
        u32x2 *d = reinterpret_cast<u32x2 *>(reinterpret_cast<uint16_t *>(p) + at);
        if (NT)
            __builtin_nontemporal_store(q, d);
        else
            *d = q;
    } else {
        reinterpret_cast<uint16_t *>(p)[at] = (uint16_t)f16_bits(v[0]);
    }
}

// item i = V adjacent pixels of active row i / nq at position i % nq (nq = (nx - 2 nb) / V items a row); (step_r, step_q) = the
// grid's stride divided by nq, quotient and remainder
template <int V, bool F16, bool NT>
__global__ __launch_bounds__(L2_BLOCK) void l2_planes_kernel(L2Planes a, int nx, int nb, unsigned nq, size_t nitems, size_t step_r,
                                                             unsigned step_q) {
    const size_t gid = (size_t)blockIdx.x * L2_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * L2_BLOCK;
    if (gid >= nitems) return;
    size_t r = gid / nq;
    unsigned q = (unsigned)(gid - r * nq);
    const size_t nxa = (size_t)nq * V;
    const bool need_r = a.var_rnoise || a.err, need_p = a.var_poisson || a.err;
    for (size_t i = gid; i < nitems; i += stride) {
        const size_t in = (r + (size_t)nb) * (size_t)nx + (size_t)nb + (size_t)q * V, out = r * nxa + (size_t)q * V;
        uint32_t w[V];
        if (a.data) {
            load_words<V>(a.slope + in, w);
            store_words<V, NT>(a.data + out, w);
        }
        if (a.dq) {
            load_words<V>(a.pixeldq + in, w);
            store_words<V, NT>(a.dq + out, w);
        }
        float vr[V], vp[V], e[V];
        if (need_r) {
            load_words<V>(reinterpret_cast<const uint32_t *>(a.err_read) + in, w);
#pragma unroll
            for (int j = 0; j < V; ++j) vr[j] = __fmul_rn(__uint_as_float(w[j]), __uint_as_float(w[j]));
            if (a.var_rnoise) store_values<V, F16, NT>(a.var_rnoise, out, vr);
        }
        if (need_p) {
            load_words<V>(reinterpret_cast<const uint32_t *>(a.err_poisson) + in, w);
#pragma unroll
            for (int j = 0; j < V; ++j) vp[j] = __fmul_rn(__uint_as_float(w[j]), __uint_as_float(w[j]));
            if (a.var_poisson) store_values<V, F16, NT>(a.var_poisson, out, vp);
        }
        if (a.err) {
#pragma unroll
            for (int j = 0; j < V; ++j) e[j] = sqrtf(__fadd_rn(vr[j], vp[j]));
            store_values<V, F16, NT>(a.err, out, e);
        }
        r += step_r, q += step_q;
        if (q >= nq) q -= nq, ++r;
    }
}

// dst (np,h,w) = src[:, y0:y0+h, x0:x0+w] of an (np,ny,nx) array (plane = ny * nx), converted TI -> TO
template <typename TI, typename TO>
__global__ __launch_bounds__(L2_BLOCK) void l2_strip_kernel(const TI *__restrict__ src, size_t plane, int nx, int y0, int h, int x0,
                                                            int w, size_t n, TO *__restrict__ dst) {
    const size_t stride = (size_t)gridDim.x * L2_BLOCK;
    for (size_t i = (size_t)blockIdx.x * L2_BLOCK + threadIdx.x; i < n; i += stride) {
        const size_t t = i / (size_t)w, x = i - t * (size_t)w, g = t / (size_t)h, y = t - g * (size_t)h;
        dst[i] = (TO)src[g * plane + ((size_t)y0 + y) * (size_t)nx + (size_t)x0 + x];
    }
}

template <typename TI, typename TO>
int launch_strip(rip_ctx *ctx, const void *src, int np, int ny, int nx, int y0, int h, int x0, int w, void *dst) {
    const size_t n = (size_t)np * h * w;
    if (!dst || !n) return RIP_OK;
    size_t blocks = (n + L2_BLOCK - 1) / L2_BLOCK;
    if (blocks > L2_MAX_BLOCKS) blocks = L2_MAX_BLOCKS;
    hipLaunchKernelGGL((l2_strip_kernel<TI, TO>), dim3((unsigned)blocks), dim3(L2_BLOCK), 0, ctx->stream, (const TI *)src,
                       (size_t)ny * nx, nx, y0, h, x0, w, n, (TO *)dst);
    RIP_HIP(ctx, hipGetLastError());
    return RIP_OK;
}

// the four edges of an (np,ny,nx) array: left, right (np,ny,nb), top (the LAST nb rows), bottom (the first) (np,nb,nx)
template <typename TI, typename TO>
int launch_strips(rip_ctx *ctx, const void *src, int np, int ny, int nx, int nb, void *left, void *right, void *top, void *bottom) {
    int rc;
    if ((rc = launch_strip<TI, TO>(ctx, src, np, ny, nx, 0, ny, 0, nb, left))) return rc;
    if ((rc = launch_strip<TI, TO>(ctx, src, np, ny, nx, 0, ny, nx - nb, nb, right))) return rc;
    if ((rc = launch_strip<TI, TO>(ctx, src, np, ny, nx, ny - nb, nb, 0, nx, top))) return rc;
    return launch_strip<TI, TO>(ctx, src, np, ny, nx, 0, nb, 0, nx, bottom);
}

// device pointers
int launch_l2_planes(rip_ctx *ctx, const L2Planes &a, int ny, int nx, int nb, bool f16) {
    const int nya = ny - 2 * nb, nxa = nx - 2 * nb;
    if (a.data || a.dq || a.var_rnoise || a.var_poisson || a.err) {
        const uintptr_t va = f16 ? 8 : 16;
        const bool need_r = a.var_rnoise || a.err, need_p = a.var_poisson || a.err;
        const bool vec = nb % 4 == 0 && nx % 4 == 0 && (!a.data || (aligned(a.slope, 16) && aligned(a.data, 16))) &&
                         (!a.dq || (aligned(a.pixeldq, 16) && aligned(a.dq, 16))) && (!need_r || aligned(a.err_read, 16)) &&
                         (!need_p || aligned(a.err_poisson, 16)) && aligned(a.var_rnoise, va) && aligned(a.var_poisson, va) &&
                         aligned(a.err, va);
        const unsigned nq = (unsigned)(vec ? nxa / 4 : nxa);
        const size_t nitems = (size_t)nya * nq;
        size_t blocks = (nitems + L2_BLOCK - 1) / L2_BLOCK;
        if (blocks > L2_MAX_BLOCKS) blocks = L2_MAX_BLOCKS;
        const size_t stride = blocks * L2_BLOCK, step_r = stride / nq;
        const unsigned step_q = (unsigned)(stride - step_r * nq);
        const dim3 grid((unsigned)blocks), block(L2_BLOCK);
        constexpr bool nt = !RIP_L2_PLAIN_STORES;
        if (vec && f16)
            hipLaunchKernelGGL((l2_planes_kernel<4, true, nt>), grid, block, 0, ctx->stream, a, nx, nb, nq, nitems, step_r, step_q);
        else if (vec)
            hipLaunchKernelGGL((l2_planes_kernel<4, false, nt>), grid, block, 0, ctx->stream, a, nx, nb, nq, nitems, step_r, step_q);
        else if (f16)
            hipLaunchKernelGGL((l2_planes_kernel<1, true, false>), grid, block, 0, ctx->stream, a, nx, nb, nq, nitems, step_r, step_q);
        else
            hipLaunchKernelGGL((l2_planes_kernel<1, false, false>), grid, block, 0, ctx->stream, a, nx, nb, nq, nitems, step_r, step_q);
        RIP_HIP(ctx, hipGetLastError());
    }
    return RIP_OK;
}

struct Out {   // an output of an entry: the caller's pointer, its bytes, its element size, its name
    void *p;
    size_t bytes;
    uintptr_t elem;
    const char *name;
};

}   // namespace

extern "C" int rip_stage_l2_planes(rip_ctx *ctx, const float *slope, const float *err_read, const float *err_poisson,
                                   const uint32_t *pixeldq, int ny, int nx, int nb, int var_dtype, int location, float *data,
                                   uint32_t *dq, void *var_rnoise, void *var_poisson, void *err, uint32_t *dq_left,
                                   uint32_t *dq_right, uint32_t *dq_top, uint32_t *dq_bottom) {
    if (!slope || !err_read || !err_poisson || !pixeldq) return rip_fail(ctx, RIP_EINVAL, "l2_planes: a NULL input");
    if (ny < 1 || nx < 1) return rip_fail(ctx, RIP_EINVAL, "l2_planes: frame %d x %d", ny, nx);
    if (nb < 0) return rip_fail(ctx, RIP_EINVAL, "l2_planes: nb = %d", nb);
    if (2 * (long long)nb >= ny || 2 * (long long)nb >= nx)
        return rip_fail(ctx, RIP_EINVAL, "l2_planes: a border of %d leaves no active region in a %d x %d frame", nb, ny, nx);
    if (var_dtype != RIP_F32 && var_dtype != RIP_F16) return rip_fail(ctx, RIP_EINVAL, "l2_planes: var_dtype %d", var_dtype);
    if (const int rc = rip_check_location(ctx, "l2_planes", "location", location)) return rc;
    const bool f16 = var_dtype == RIP_F16;
    const size_t n = (size_t)ny * nx, na = (size_t)(ny - 2 * nb) * (size_t)(nx - 2 * nb), vw = f16 ? 2 : 4;
    const size_t side = (size_t)ny * nb * 4, edge = (size_t)nb * nx * 4;
    const Out outs[9] = {{data, na * 4, 4, "data"}, {dq, na * 4, 4, "dq"}, {var_rnoise, na * vw, vw, "var_rnoise"},
                         {var_poisson, na * vw, vw, "var_poisson"}, {err, na * vw, vw, "err"}, {dq_left, side, 4, "dq_left"},
                         {dq_right, side, 4, "dq_right"}, {dq_top, edge, 4, "dq_top"}, {dq_bottom, edge, 4, "dq_bottom"}};
    const void *ins[4] = {slope, err_read, err_poisson, pixeldq};
    for (const Out &o : outs) {
        for (const void *in : ins)
            if (ranges_meet(o.p, o.bytes, in, n * 4)) return rip_fail(ctx, RIP_EINVAL, "l2_planes: %s overlaps an input", o.name);
        if (location == RIP_DEVICE && o.p && !aligned(o.p, o.elem))
            return rip_fail(ctx, RIP_EINVAL, "l2_planes: the device pointer %s is not aligned to its %d-byte element", o.name, (int)o.elem);
    }
    if (location == RIP_DEVICE)
        for (const void *in : ins)
            if (!aligned(in, 4)) return rip_fail(ctx, RIP_EINVAL, "l2_planes: a device input pointer is not aligned to its 4-byte element");
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    if (location == RIP_DEVICE) ctx->stream_dirty = true;   // (the next overlapped rip_calibrate orders its pre-pass behind this work)
    DevArg<float> d_in[3];
    DevArg<uint32_t> d_pdq;
    DevArg<char> d[9];
    int rc;
    if ((rc = d_in[0].in(ctx, slope, n, location)) || (rc = d_in[1].in(ctx, err_read, n, location)) ||
        (rc = d_in[2].in(ctx, err_poisson, n, location)) || (rc = d_pdq.in(ctx, pixeldq, n, location)))
        return rc;
    for (int k = 0; k < 9; ++k)
        if ((rc = d[k].out(ctx, (char *)outs[k].p, outs[k].bytes, location))) return rc;
    const L2Planes a = {reinterpret_cast<const uint32_t *>(d_in[0].p), d_in[1].p, d_in[2].p, d_pdq.p, reinterpret_cast<uint32_t *>(d[0].p),
                        reinterpret_cast<uint32_t *>(d[1].p), d[2].p, d[3].p, d[4].p};
    if ((rc = launch_l2_planes(ctx, a, ny, nx, nb, f16))) return rc;
    if ((rc = launch_strips<uint32_t, uint32_t>(ctx, d_pdq.p, 1, ny, nx, nb, d[5].p, d[6].p, d[7].p, d[8].p))) return rc;
    for (int k = 0; k < 9; ++k)
        if ((rc = d[k].download())) return rc;
    return location == RIP_DEVICE ? RIP_OK : dev_sync(ctx);   // device pointers: queued, not waited for
}

extern "C" int rip_stage_l2_refpix_strips(rip_ctx *ctx, const void *cube, int cube_dtype, int ngrp, int ny, int nx, int nb,
                                          int location, float *left, float *right, float *top, float *bottom) {
    if (!cube) return rip_fail(ctx, RIP_EINVAL, "l2_refpix_strips: cube is NULL");
    if (ngrp < 1 || ny < 1 || nx < 1) return rip_fail(ctx, RIP_EINVAL, "l2_refpix_strips: cube %d x %d x %d", ngrp, ny, nx);
    if (nb < 0 || nb > ny || nb > nx) return rip_fail(ctx, RIP_EINVAL, "l2_refpix_strips: nb = %d in a %d x %d frame", nb, ny, nx);
    if (cube_dtype != RIP_U16 && cube_dtype != RIP_F32) return rip_fail(ctx, RIP_EINVAL, "l2_refpix_strips: cube_dtype %d", cube_dtype);
    if (const int rc = rip_check_location(ctx, "l2_refpix_strips", "location", location)) return rc;
    const bool u16 = cube_dtype == RIP_U16;
    const size_t cw = u16 ? 2 : 4, n = (size_t)ngrp * ny * nx;
    const size_t side = (size_t)ngrp * ny * nb * 4, edge = (size_t)ngrp * nb * nx * 4;
    const Out outs[4] = {{left, side, 4, "left"}, {right, side, 4, "right"}, {top, edge, 4, "top"}, {bottom, edge, 4, "bottom"}};
    for (const Out &o : outs) {
        if (ranges_meet(o.p, o.bytes, cube, n * cw)) return rip_fail(ctx, RIP_EINVAL, "l2_refpix_strips: %s overlaps the cube", o.name);
        if (location == RIP_DEVICE && o.p && !aligned(o.p, 4))
            return rip_fail(ctx, RIP_EINVAL, "l2_refpix_strips: the device pointer %s is not aligned to its 4-byte element", o.name);
    }
    if (location == RIP_DEVICE && !aligned(cube, cw))
        return rip_fail(ctx, RIP_EINVAL, "l2_refpix_strips: the device pointer cube is not aligned to its %d-byte element", (int)cw);
    RIP_HIP(ctx, hipSetDevice(ctx->device));
    if (location == RIP_DEVICE) ctx->stream_dirty = true;
    DevArg<char> d_cube, d[4];
    int rc;
    if ((rc = d_cube.in(ctx, (const char *)cube, n * cw, location))) return rc;
    for (int k = 0; k < 4; ++k)
        if ((rc = d[k].out(ctx, (char *)outs[k].p, outs[k].bytes, location))) return rc;
    if ((rc = u16 ? launch_strips<uint16_t, float>(ctx, d_cube.p, ngrp, ny, nx, nb, d[0].p, d[1].p, d[2].p, d[3].p)
                  : launch_strips<uint32_t, uint32_t>(ctx, d_cube.p, ngrp, ny, nx, nb, d[0].p, d[1].p, d[2].p, d[3].p)))
        return rc;
    for (int k = 0; k < 4; ++k)
        if ((rc = d[k].download())) return rc;
    return location == RIP_DEVICE ? RIP_OK : dev_sync(ctx);
}
