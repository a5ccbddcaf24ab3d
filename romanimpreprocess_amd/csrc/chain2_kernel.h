// The fused L1->L2 kernel (f32 gain; f32 or f64 ipc4d; 5 to 16 groups), wave-specialised: one launch per
// ramp does reference-pixel apply + bias + Legendre linearity + IPC deconvolution + ramp fit / jump detection / flag propagation
// + dark rate + error split + flat (gen_cal_image.py:533-629; stage arithmetic and reference lines as in linearity.hip, ipc.hip,
// rampfit.hip), every array read from HBM once.
//
// Geometry: the frame is cut into strips of 252 output columns (256-column windows: 2 + 2 halo columns for the two 3 x 3 IPC
// passes); a workgroup owns one strip and one row range and marches down its rows, keeping the rows the 3 x 3 stencils need in
// LDS rings.  The grid is exactly resident (the row ranges are equal, no tail).  A workgroup of 512 threads covers its 256
// columns with TWO ROLES of four waves each (one wave doing every phase needs > 200 registers: 2 waves/SIMD, issue bound):
//     ingest waves (tid < 256)   A: refpix/bias/linearity of row r+3 -> x ring      (raw loads of row r+4 issued between
//                                C: first IPC iterate of row r+2 -> O1 ring             its arithmetic blocks)
//     fit waves    (tid >= 256)  O2: second iterate of row r / gain (reads O1 rows r-1..r+1, x of its own column)
//                                F: ramp fit with jump detection and saturated refits of pixel (r, c)
//                                T: flag propagation, finish (dark rate, error split, flat), stores of pixel (r, c)
// so each role needs <= 128 VGPRs and a CU holds 2 workgroups = 16 waves = 4 waves/SIMD.  That is the 256-column form (f32 ipc4d
// with 6 / 8 groups, the bench path); 16 groups and f64 ipc4d, whose rings would leave one such workgroup per CU or none, run the
// NARROW forms (one wide workgroup per CU that drops rings; C2Form below).  Per step:
//     S1: ingest A(r+3)   | fit O2(r) and the first half of F(r)                         -- barrier --
//     S2: ingest C(r+2)   | fit: the rest of F(r) and T(r), the ring words of row r+1  -- barrier --
// Everything after O2 is register-only in a fit thread, so the half-step barrier could fall anywhere in it (C2Form: where it
// sits and why).  Rings (3 rows each): x = gain*phi; the first iterate O1 (C writes row r+2 into the slot of
// row r-1, which O2(r) finished reading before the barrier; doubles with f64 ipc4d); the per-pixel words that travel from the
// ingest thread of a column to its fit thread (merged flag word, packed groupdq bytes, gain); and the K ring (2 rows): the nine
// IPC coefficients of a pixel are loaded ONCE, by its ingest thread, and handed to its fit thread.  Saturated pixels are
// refitted from registers (trunc_layers), so no per-pixel ramp staging in LDS.
// The 256-column form is bound by the instructions it issues, not by its bytes, and has two LEAN pieces of its own (C2Form::nobias,
// C2Form::lt): an instantiation without any biascorr load or subtraction (BIAS = false) for calls without a bias stream, and the
// channel-line values m * y + c of a row from a small per-wave LDS table instead of two f64 operations per lane and group.
#pragma once
#include "chain_common.h"
#include "chain2_form.h"

// Diagnostic builds only (RIP_TIMING_BUILD: rip_version() then reports a timing build and the Python binding refuses the library
// unless told otherwise): -DC2_DBG switches phases off by ChainArgs::dbg (results invalid by construction), -DCH_STAMP records
// per-phase clock stamps.  Nothing else in this header changes what the kernel computes.
#if (defined(C2_DBG) || defined(CH_STAMP)) && !defined(RIP_TIMING_BUILD)
#error "C2_DBG / CH_STAMP are timing experiments: build them with -DRIP_TIMING_BUILD"
#endif
#ifdef CH_STAMP
#define C2_DRAIN()                                \
    if (a.dbg & 2048) {                           \
        __builtin_amdgcn_s_waitcnt(0);            \
    }
#else
#define C2_DRAIN()
#endif
#define C2_SYNC() __syncthreads()

// Returns x, opaque to the optimiser: used on loop-invariant per-lane offsets right before a global access so that
// the zero-extension stays next to the address add and instruction selection can use the
// `global_load v, v_off32, s[base:base+1]` form (with the offset hoisted out of the loop it falls back to a 64-bit
// vector add per access).  Emits no instruction.
__device__ __forceinline__ unsigned c2_opaque(unsigned x) {
    asm volatile("" : "+v"(x));
    return x;
}

// Buffer addressing for the global loads: descriptor (base, no stride, no bound) in four scalar registers, the
// loop-invariant column offset of the lane as the vector offset, plane + row as a 32-bit scalar offset -- one s_add per
// load where a 64-bit base costs two.  Every array addressed this way is smaller than 4 GiB.
// records: the bound the hardware's range check holds offsets against.  -1 everywhere but on the biascorr planes, whose
// descriptor has 0 records where the call has no bias stream (ChainArgs::bias_records): every load through it is dropped by the
// range check and returns 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t c2_rsrc(const void *p, int records = -1) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, records, 0x00020000);
}
template <int AUX = 0>
__device__ __forceinline__ float c2_ld_f32(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, AUX));
}
__device__ __forceinline__ double c2_ld_f64(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
template <int AUX = 0>
__device__ __forceinline__ uint32_t c2_ld_u32(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ uint32_t c2_ld_u16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ uint32_t c2_ld_u8(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(r, voff, soff, AUX);
}
// XCD-aware block order (the dispatcher deals consecutive block ids round the 8 XCDs, each with its own L2): block ids that
// share an XCD get CONSECUTIVE cells of the (row range, strip) grid, so that neighbouring strips -- whose 256-column windows at
// a 252-column pitch share cache lines and halo columns -- find each other's lines in their L2.  Bijective for any grid size;
// a speed choice only.
__device__ __forceinline__ int c2_xcd_block(int b, int n) {
    const int q = n >> 3, r = n & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// The kernel arguments re-read from the kernarg segment (scalar loads from the constant address space) through a
// pointer made opaque once per phase: the ~25 pointers and sizes of ChainArgs then live in scalar registers only
// from their first to their last use inside a phase, instead of all being loop invariants that the register
// allocator spills to VGPR lanes (v_readlane/v_writelane are vector-ALU instructions with scalar hazards).
struct C2KernArgs {  // the kernel's argument list as it lies in the kernarg segment
    ChainArgs a;
    const RipPlanHeader *h;
    const RipVariant *vars;
    const float *kvals;
    const RipDiff *diffs;
    double guard;
};
__device__ __forceinline__ const RIP_K C2KernArgs *c2_args(const RIP_K C2KernArgs *p) {
    asm volatile("" : "+s"(p));
    return p;
}

template <int N>
struct C2Int {
    static constexpr int value = N;
};

// forward IPC operator in f64 for NBB groups in lockstep (f64 ipc4d): v[b][k] = source value of term k of group b, terms in the
// reference's order (0 centre, 1 (y-1, x), 2 (y+1, x), 3 (y, x-1), 4 (y, x+1), 5 (y-1, x-1), 6 (y-1, x+1), 7 (y+1, x-1),
// 8 (y+1, x+1) as the rows / columns of the rings hold them); the NBB products of a term first, then the NBB accumulating adds --
// independent chains that hide the f64 latencies (one group at a time: 1.51 ms, batched: 1.34 ms for 8 groups, same box).
// Term order and edge rule of ipc_linearity.py:69-94.
template <bool ALL, int NBB, typename VT>
__device__ __forceinline__ void c2_ipc9_batch(const VT (&v)[NBB][9], const double (&kk)[9], unsigned valid, double (&acc)[NBB]) {
#pragma unroll
    for (int b = 0; b < NBB; ++b) acc[b] = (double)v[b][0] * kk[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        double p_[NBB];
#pragma unroll
        for (int b = 0; b < NBB; ++b) p_[b] = (double)v[b][k] * kk[k];
#pragma unroll
        for (int b = 0; b < NBB; ++b) acc[b] = (ALL || ((valid >> k) & 1u)) ? acc[b] + p_[b] : acc[b];
    }
}

// (float)(a[g] / (double)bf) for NG numerators and ONE divisor (the second iterate over the pixel's gain, f64 ipc4d), lanes with
// `use` only.  The compiler expands an f64 division into v_div_scale x 2, v_rcp_f64, two Newton steps on the reciprocal (four
// fma), q0 = a * y, r = fma(-b, q0, a), v_div_fmas (= fma(r, y, q0) when nothing was scaled), v_div_fixup (= its first operand for
// finite non-zero operands).  Everything up to y depends on the divisor alone, so it is computed once and each quotient costs a
// multiply and two fma: the same operations on the same operands as the expansion, hence the same bits, as long as v_div_scale
// scales nothing and v_div_fixup has nothing to fix -- which holds for 2^-60 < |b| < 2^60 and every quotient (rounded to f32)
// finite, non-zero and within 2^-59 .. 2^59 (then 2^-119 < |a| < 2^119: far from every scaling rule of the instruction).  One
// wave vote checks that; otherwise every lane takes the division operator.  G0: the first value divided (1 where group 0 is
// skipped: it is neither divided nor in the vote).
template <int NG, int NA, int G0 = 0>
__device__ __forceinline__ void c2_div64_shared(const double (&a)[NA], float bf, bool use, float (&qf)[NA]) {
    static_assert(NA >= NG && G0 >= 0 && G0 < NG, "the values G0 .. NG - 1 of NA are divided");
    const double b = (double)bf;
    double y = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    float asum = 0.0f, amin = 3.0e38f;   // NaN / Inf show in the sum, zeros and tiny values in the minimum
#pragma unroll
    for (int g = G0; g < NG; ++g) {
        const double q0 = a[g] * y;
        const double r = __builtin_fma(-b, q0, a[g]);
        qf[g] = (float)__builtin_fma(r, y, q0);
        asum = asum + fabsf(qf[g]);
        amin = fminf(amin, fabsf(qf[g]));
    }
    const bool ok = rcp_safe(bf) && asum < 5.7e17f && amin > 1.8e-18f;
    if (!__all(ok || !use)) {
#pragma unroll
        for (int g = G0; g < NG; ++g) qf[g] = (float)(a[g] / b);
    }
}

// operands of rip_legendre_series in registers: the coefficients of the prefetched row, the constants per degree
template <int NP>
struct C2Legendre {
    const float (&cfs)[NP], (&c1s)[NP], (&c2s)[NP], (&chfs)[NP];
    static constexpr __device__ int n() { return NP; }
    __device__ __forceinline__ float cf(int L) const { return cfs[L]; }
    __device__ __forceinline__ float c1(int L) const { return c1s[L]; }
    __device__ __forceinline__ float c2(int L) const { return c2s[L]; }
    __device__ __forceinline__ float chf(int L) const { return chfs[L]; }
};

template <int NP, int G, int START, typename KT, bool SKIP0 = false, bool BIAS = true>
__global__ __launch_bounds__((C2Form<G + (G & 1), sizeof(KT) == 8>::threads), (C2Form<G + (G & 1), sizeof(KT) == 8>::wps)) void chain2_kernel(
    ChainArgs a, const RipPlanHeader *__restrict__ h, const RipVariant *__restrict__ vars, const float *__restrict__ kvals,
    const RipDiff *__restrict__ diffs, double guard) {
    static_assert(G > 4 && G <= 16, "pairs of groups; the groupdq bytes travel packed four to a word");
    // SKIP0: the first half of pair 0 is DEAD (chain2_form.h, "SKIPPED FIRST GROUP"): the launcher takes this form only where
    // the fit gives group 0 the weight zero, tests no difference on it, and d[0] is known to be finite without computing it
    static_assert(!SKIP0 || START == 1, "group 0 can be skipped only where the fit excludes it");
    // odd G: GE = G + 1 register / ring slots, the last one DEAD (see the note above C2Form); g < G guards are compile-time
    constexpr int GE = G + (G & 1);
    using F = C2Form<GE, sizeof(KT) == 8>;
    // BIAS = false: no biascorr stream at all (the launcher takes it where ChainArgs::bias_records == 0; C2Form::nobias)
    static_assert(BIAS || F::nobias, "only the forms the table names have an instantiation without a bias stream");
    constexpr bool LT = F::lt;   // line values from the per-wave table instead of two f64 operations per lane and group
    constexpr int COLS = F::cols;
    constexpr int KRN = F::krn;
    // narrow forms: the fit role requests the coefficients the K ring does not carry itself (k >= KRN: none at f64 ipc4d x 6
    // groups, where the partial ring has room for all nine)
    constexpr bool KFIT = F::narrow > 0;
    constexpr int QW = (G + 3) / 4;  // words of packed group flags per pixel
    constexpr int GP = GE / 2;
    static_assert(QW == (GE + 3) / 4, "the padded count packs into the same flag words");
    // f64 ipc4d (KT = double; the reference's production writer stores f64): x = gain*phi stays f32, the Neumann iterates and
    // the division by the gain are f64 (numpy promotion, ipc_linearity.py:95-142), so the O1 ring holds doubles, one plane per
    // group
    constexpr bool K64 = sizeof(KT) == 8;
    constexpr int SA = F::stream_aux;   // cache policy of the once-read arrays
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int XR = 3;  // rows of the x ring
    f2 *X2 = reinterpret_cast<f2 *>(lds_raw + F::x_ofs);         // [GP][XR][COLS]
    f2 *O12 = reinterpret_cast<f2 *>(lds_raw + F::o1_ofs);       // [GP][3][COLS]
    double *O1d = reinterpret_cast<double *>(lds_raw + F::o1_ofs);   // f64 ipc4d: [G][3][COLS] instead
    // per-pixel words from the ingest thread of a column to its fit thread (slots as the x ring: the fit thread takes row r+1's at
    // the end of step r)
    uint32_t *DQ = reinterpret_cast<uint32_t *>(lds_raw + F::dq_ofs);   // [3][COLS] flag word
    uint32_t *QS = reinterpret_cast<uint32_t *>(lds_raw + F::qs_ofs);   // [3][QW][COLS] groupdq bytes, packed
    float *GN = reinterpret_cast<float *>(lds_raw + F::gn_ofs);         // [3][COLS] gain
    double *LN = reinterpret_cast<double *>(lds_raw + F::ln_ofs);       // [NLC][G][2]
    double *LTB = reinterpret_cast<double *>(lds_raw + F::lt_ofs);      // [COLS / 64][NLC][GE] (C2Form::lt): m * y + c of the row A ingests
    // K ring: the nine IPC coefficients of destination (row, col), loaded ONCE by the ingest thread of the column and handed to
    // its fit thread (two rows live: C of row y runs two steps before O2 of row y)
    constexpr int NLC = F::nlc;
    f2 *KR2 = reinterpret_cast<f2 *>(lds_raw + F::kr_ofs);              // f32 ipc4d: [2][4][COLS] pairs (k0,k1)..(k6,k7)
    float *KR1 = reinterpret_cast<float *>(KR2 + 2 * 4 * COLS);        //            [2][COLS] k8
    double *KRd = reinterpret_cast<double *>(lds_raw + F::kr_ofs);      // f64 ipc4d: [2][KRN][COLS]

    // ChainArgs is the first kernel argument: it sits at offset 0 of the kernarg segment
    const RIP_K C2KernArgs *kargs = (const RIP_K C2KernArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x;
    // every workgroup of the launch (the idle ones of the grid's tail too) counts itself in as it starts: the gate in front of the
    // next call's pre-pass waits until the whole grid has its slots (calibrate.hip).  Relaxed: nothing is published through it.
    if (a.wg_counter && tid == 0) __hip_atomic_fetch_add(a.wg_counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef C2_DBG
    const int dbg = a.dbg;  // timing experiments only (tools/gpu_checks/phase_timing.py): bits switch phases off
#else
    constexpr int dbg = 0;
#endif
    const bool fit_role = tid >= COLS;
    const int col = fit_role ? tid - COLS : tid;
    const int ny = a.ny, nx = a.nx, nb = a.nb;
    const int ay0 = nb, ay1 = ny - nb, ax0 = nb, ax1 = nx - nb;
    const unsigned npix = (unsigned)ny * (unsigned)nx;
    const unsigned pl4 = npix * 4u;
    const int nch = nx / RIP_CW;
    const uint32_t bad = DQ_NO_LIN_CORR | DQ_REFERENCE_PIXEL;

    float c1[NP], c2[NP], chf[NP];
#pragma unroll
    for (int L = 1; L < NP; ++L) {
        const RipLegendreK k = rip_legendre_k(L);
        c1[L] = k.c1, c2[L] = k.c2, chf[L] = k.chf;
    }

    const int nstrips = F::nstrips(nx);
    const int bid = c2_xcd_block((int)blockIdx.x, (int)gridDim.x);
    // (strip, row range) of this workgroup -- in QUAD mode (the last strip, when it has at most 64 live columns) of each of its
    // COLS / 64 wave columns (four at 256 columns, six at 384): 64-column windows (2 + 2 halo lanes each) of the same strip that
    // march down as many different row ranges, so that a strip 64 columns wide takes 64 / COLS of the workgroups of a full one
    // (launcher: chain2_geometry)
    const int nfull = a.geo_rows_q ? nstrips - 1 : nstrips;
    const bool quad = bid >= nfull * a.geo_nr;
    const int rows_wg = quad ? a.geo_rows_q : a.geo_rows;   // steps of every wave of the workgroup (barriers inside)
    const int strip = quad ? nfull : bid % nfull;
    const int wcol = quad ? (col & 63) : col;               // column inside the wave column's window
    const int wl = quad ? 64 : COLS;                     // ... and its width
    const int R0 = min(ny, quad ? ((bid - nfull * a.geo_nr) * (COLS / 64) + __builtin_amdgcn_readfirstlane(col >> 6)) * rows_wg
                                : (bid / nfull) * rows_wg);
    const int R1 = min(ny, R0 + rows_wg);
    if (bid >= nfull * a.geo_nr + a.geo_nq) return;
    const int c = strip * F::outw + wcol;
    const bool col_ok = (c >= 0 && c < nx);
    const bool col_act = (c >= ax0 && c < ax1);
    const int cc = col_ok ? c : 0;
    const int ch0 = (strip * F::outw) / RIP_CW;
    const int chr = cc / RIP_CW - ch0;
    for (int i = tid; i < NLC * G * 2; i += F::threads) {
        const int ch = i / (G * 2), g = (i / 2) % G, w = i & 1;
        LN[i] = (ch0 + ch < nch && !(SKIP0 && g == 0)) ? a.lines[(g * nch + ch0 + ch) * 2 + w] : 0.0;   // (SKIP0: group 0's lines may be unwritten)
    }
    __syncthreads();

    // Addressing: every global access is (wave-uniform 64-bit base: array + plane + row, scalar ALU) + (per-lane
    // 32-bit column offset, loop-invariant VGPR), i.e. the saddr form of global_load/store with no vector
    // address arithmetic per access.
    const unsigned cc4 = (unsigned)cc * 4u, cc2 = (unsigned)cc * 2u, cc1 = (unsigned)cc;
    unsigned cx4[3];  // byte offset of the clamped source column c - dx, index dx + 1
    unsigned colmask = 0;  // bit k: source column of term k is in the active box (and so is c)
    {
        bool okx[3];
#pragma unroll
        for (int dxi = 0; dxi < 3; ++dxi) {
            const int sx = c - (dxi - 1);
            okx[dxi] = sx >= ax0 && sx < ax1;
            cx4[dxi] = (unsigned)min(max(sx, 0), nx - 1) * 4u;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int dx = RIP_IPC_DX(k);
            if (okx[dx + 1]) colmask |= 1u << k;
        }
        if (!col_act) colmask = 0;
    }
    const unsigned lane_mask = fit_role ? ((wcol >= 2 && wcol < wl - 2) ? colmask : 0u)
                                        : ((wcol >= 1 && wcol < wl - 1) ? colmask : 0u);
    const unsigned row4 = (unsigned)nx * 4u;  // row pitch of an f32/u32 plane; offsets within a plane fit 32 bits
    // rows this (strip, row range) cell really uses: R0-2 .. R1+1 (two halo rows on each side).  The straight-line loads of the
    // warm-up and drain steps are clamped INTO that band, so that they touch lines the cell reads anyway instead of 3-5 rows of
    // its neighbours' (each such row costs HBM traffic and buys nothing)
    const int ylo = max(R0 - 2, 0), yhi = min(R1 + 1, ny - 1);
    // Row steps of both roles: r = R0 - 5 .. R0 + rows_wg - 1, rows_wg + 5 of them for every wave of the workgroup (in quad mode the
    // wave columns differ in R0 and R1, not in rows_wg), two barriers each.  The last does work: C of row yc = r + 2 <= R1 when
    // R1 = R0 + rows_wg, and the fit of row R1 - 1.  A step r = R0 + rows_wg would do nothing in either role -- A wants
    // r + 3 <= R1 + 1, C wants r + 2 <= R1, the fit role emits r < R1 -- and what the step before it reads from the rings at its
    // end (xnext, dq_next, ...) feeds that step alone.
    const int r_end = R0 + rows_wg + ((RIP_LEAN2 & 4) ? 0 : 1);

    // coefficient loader: raw loads at clamped source positions + validity mask for destination (y, c); `want` is wave-uniform.
    // The nine planes are walked in memory order (plane = 3*(1+dy) + (1+dx)) and land in the reference's term order
    // (rip_ipc_term): f32 coefficients as the five pairs kk[k / 2], f64 ones as nine scalars kk[k], with 8-byte loads.
    // kmin: terms below it are not loaded -- the fit role of a form with a partial K ring gets them through LDS.
    auto load_k = [&](const void *kern_base, int y, bool want, auto &kk, auto kmin_c) -> unsigned {
        constexpr int KMIN = decltype(kmin_c)::value;
        constexpr bool PAIRS = sizeof(kk) == sizeof(f2[5]);   // f2 kk[5], else double kk[9]
        constexpr unsigned ES = PAIRS ? 1u : 2u;   // element size in f32 words
        if constexpr (PAIRS) {
            if (dbg & 128) {
#pragma unroll
                for (int k = 0; k < 5; ++k) kk[k] = f2{(k == 0) ? 1.0f : 0.001f, 0.001f};
                return want ? lane_mask : 0u;
            }
        }
        unsigned rowoff[3];
        bool rok[3];
#pragma unroll
        for (int dyi = 0; dyi < 3; ++dyi) {
            const int sy = y - (dyi - 1);
            rok[dyi] = sy >= ay0 && sy < ay1;
            rowoff[dyi] = (unsigned)min(max(sy, ylo), yhi) * (row4 * ES);   // rows outside the range's own are never used: keep to lines it reads anyway
        }
        const unsigned rowbits = rip_ipc_row_mask(rok[0], rok[1], rok[2]);
        const __amdgpu_buffer_rsrc_t kr = c2_rsrc(kern_base);
        unsigned pofs = 0;
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            const int dy = p / 3 - 1, dx = p % 3 - 1;
            const int k = rip_ipc_term(dy, dx);
            if constexpr (PAIRS) {
                const float kv_ = c2_ld_f32(kr, cx4[dx + 1], pofs + rowoff[dy + 1]);
                if (k & 1)
                    kk[k / 2].y = kv_;
                else
                    kk[k / 2].x = kv_;
            } else {
                if (k >= KMIN) kk[k] = c2_ld_f64(kr, cx4[dx + 1] * 2u, pofs + rowoff[dy + 1]);
            }
            pofs += pl4 * ES;
        }
        const unsigned um = (want && y >= ay0 && y < ay1) ? rowbits : 0u;
        return lane_mask & um;
    };
    // validity mask of destination (y, c) alone, for the role that receives the coefficients through the K ring
    auto k_valid = [&](int y) -> unsigned {
        const bool r0 = (y + 1) >= ay0 && (y + 1) < ay1, r1 = y >= ay0 && y < ay1, r2 = (y - 1) >= ay0 && (y - 1) < ay1;
        return r1 ? (lane_mask & rip_ipc_row_mask(r0, r1, r2)) : 0u;
    };
#ifdef CH_STAMP
    unsigned long long st_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tl_ = __builtin_amdgcn_s_memtime();
#endif
    if (!fit_role) {
        // =========================================================================== ingest waves
        // plane p of the calibration slab at row yl: scalar offset p*pl4 + yl*row4; groups likewise in their arrays
        auto fetch_groups = [&](const RIP_K ChainArgs *ka, int y, int g0, int g1, RowRegs<NP, GE, BIAS> &rr) {
            if ((dbg & 64) && y > R0 - 2) return;   // timing experiment: every row works on the first row's (valid) values
            __builtin_amdgcn_sched_barrier(0);
            const unsigned yl = (unsigned)min(max(y, ylo), yhi);
            const __amdgpu_buffer_rsrc_t rs = c2_rsrc(ka->data), rq = c2_rsrc(ka->gdq), rd = c2_rsrc(ka->dark_data),
                                         rb = c2_rsrc(ka->bias, ka->bias_records);   // (BIAS = false: unused, no code)
            unsigned o4 = yl * row4 + (unsigned)g0 * pl4, o2 = yl * (row4 >> 1) + (unsigned)g0 * (pl4 >> 1),
                     o1 = yl * (row4 >> 2) + (unsigned)g0 * npix;
#pragma unroll
            for (int g = g0; g < g1; ++g) {
                if constexpr (GE > G) {
                    if (g >= G) continue;   // the dead half of an odd ramp's last pair is never loaded
                }
                const bool flags_only = SKIP0 && g == 0;   // a skipped first group keeps its flag byte, nothing else is loaded
                if (!flags_only) rr.S[g] = c2_ld_u16<SA>(rs, cc2, o2);
                rr.q[g] = c2_ld_u8<F::wring ? SA : 0>(rq, cc1, o1);   // (16 groups: the fit role reads these bytes again)
                if (!flags_only) {
                    rr.dk[g] = c2_ld_f32<SA>(rd, cc4, o4);
                    if constexpr (BIAS) rr.bs[g] = c2_ld_f32<SA>(rb, cc4, o4);
                }
                o4 += pl4;
                o2 += pl4 >> 1;
                o1 += npix;
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        // planes i0..i1-1 of [cf[0..NP-1], Smin, Smax, Sref, dq, gain]
        auto fetch_coefs = [&](const RIP_K ChainArgs *ka, int y, int i0, int i1, RowRegs<NP, GE, BIAS> &rr) {
            if ((dbg & 64) && y > R0 - 2) return;
            __builtin_amdgcn_sched_barrier(0);
            const unsigned yl = (unsigned)min(max(y, ylo), yhi);
            const __amdgpu_buffer_rsrc_t rp = c2_rsrc(ka->planes);
            unsigned o4 = yl * row4 + (unsigned)i0 * pl4;
#pragma unroll
            for (int i = i0; i < i1; ++i) {
                if (i < NP)
                    rr.cf[i] = c2_ld_f32<SA>(rp, cc4, o4);
                else if (i == NP)
                    rr.smin = c2_ld_f32<SA>(rp, cc4, o4);
                else if (i == NP + 1)
                    rr.smax = c2_ld_f32<SA>(rp, cc4, o4);
                else if (i == NP + 2)
                    rr.sref = c2_ld_f32<SA>(rp, cc4, o4);
                else if (i == NP + 3)   // the flag word: linearity dq merged with what the finish step ORs into pixeldq (RipCal)
                    rr.dq = c2_ld_u32<SA>(rp, cc4, yl * row4 + (unsigned)(NP + ka->merged_dq) * pl4);
                else
                    rr.gain = c2_ld_f32<F::wring ? SA : 0>(rp, cc4, o4);
                o4 += pl4;
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        auto fetch_row = [&](int y, RowRegs<NP, GE, BIAS> &rr) {  // prologue: the whole first row at once
            const RIP_K ChainArgs *ka = &kargs->a;
            fetch_coefs(ka, y, 0, NP + 5, rr);
            fetch_groups(ka, y, 0, G, rr);
        };
        constexpr int NCO = NP + 5;                 // coefficient-type planes per pixel
        constexpr int CO_STEP = (NCO + GP - 1) / GP;  // issued per pair of C
        RowRegs<NP, GE, BIAS> rr;
        if constexpr (GE > G) rr.S[G] = rr.q[G] = 0u, rr.dk[G] = 0.0f;
        if constexpr (SKIP0) rr.S[0] = 0u, rr.dk[0] = 0.0f;
        if constexpr (BIAS) {
            if constexpr (GE > G) rr.bs[G] = 0.0f;
            if constexpr (SKIP0) rr.bs[0] = 0.0f;
        }
        fetch_row(R0 - 2, rr);
        // The line values of a row, one per (channel of the window, group): lanes 0 .. NLC * GE - 1 of every ingest wave evaluate
        // them for the row ITS wave ingests next (quad mode: the wave columns are at different rows) into the wave's own table --
        // here for the first row, then in S2 of every step for row r + 4, which A reads in S1 of the step after.  Written and read
        // by the same wave, with a workgroup barrier between the two besides, so one buffer does.  Entries of a dead group are
        // never read (a skipped first group's lines are zeros in LN).
        const int lt_lane = tid & 63;
        double *lt_w = LTB + (tid >> 6) * (NLC * GE);
        auto line_values = [&](int y) {
            if constexpr (LT) {
                static_assert(NLC * GE <= 64, "one lane per (channel, group) of the wave's table");
                if (lt_lane < NLC * GE) {
                    const int ch = lt_lane / GE, g = lt_lane % GE;
                    const double *ln = LN + (ch * G + (g < G ? g : 0)) * 2;
                    lt_w[lt_lane] = rip_refpix_line(ln[0], ln[1], (double)y);
                }
            }
        };
        line_values(R0 - 2);
        int so_c = (R0 - 5 + 2 + 3000) % 3;  // O1 ring slot of row yc = r + 2
        double rcn[G];  // row corrections of the row the next step ingests
        {
            const RIP_K double *rt = rip_k(kargs->a.rowcorr_t) + (size_t)min(max(R0 - 2, 0), ny - 1) * G;
#pragma unroll
            for (int g = SKIP0 ? 1 : 0; g < G; ++g) rcn[g] = rt[g];   // (SKIP0: group 0's corrections are neither made nor read)
            if constexpr (SKIP0) rcn[0] = 0.0;
        }
        for (int r = R0 - 5; r < r_end; ++r, so_c = (so_c == 2) ? 0 : so_c + 1) {
            const RIP_K ChainArgs *ka = &c2_args(kargs)->a;  // S1 copy of the argument block
            const int yi = r + 3, yc = r + 2;
            const bool do_a = (yi >= R0 - 2) && (yi <= R1 + 1);
            const bool do_c = (yc >= R0 - 1) && (yc <= R1);
            // ---- S1: A (linearity of row yi from rr), then the loads S2 consumes
            // per-row reference-pixel correction of the G groups: wave-uniform, scalar loads (constant address space)
            double rc[G];  // loaded one step ahead: one wide scalar load from the row-major copy of the table
#pragma unroll
            for (int g = 0; g < G; ++g) rc[g] = rcn[g];
            {
                const RIP_K double *rt = rip_k(ka->rowcorr_t) + (size_t)min(max(yi + 1, 0), ny - 1) * G;
#pragma unroll
                for (int g = SKIP0 ? 1 : 0; g < G; ++g) rcn[g] = rt[g];
            }
            const bool a_full = do_a && yi >= 0 && yi < ny;  // wave-uniform
            // A: two pairs of groups at a time -- reference-pixel/bias arithmetic and z of both pairs, then their two
            // Legendre recurrences interleaved (independent chains), then the raw loads of the same groups of the next
            // row.  The loads are issued UNCONDITIONALLY between the blocks (the wait-count pass is path-insensitive: a
            // load that exists on one side of a branch only forces vmcnt(0) at later uses).  All lanes compute (lanes
            // beyond the frame edge work on the clamped column and store zeros).
            const int xslot = (so_c == 2) ? 0 : so_c + 1;    // 3-row rings (x and the per-pixel words): row yi = r + 3 takes the slot of row r
            f2 *xs = X2 + xslot * COLS + col;
            const bool act = col_act && yi >= ay0 && yi < ay1;
            uint32_t dq = rr.dq;
            uint32_t w[QW];  // the pixel's groupdq bytes, packed
#pragma unroll
            for (int i = 0; i < QW; ++i) w[i] = 0;
            const float smin = rr.smin;
            const float span = rr.smax - smin;
            const bool fastdiv = __all(rcp_safe(span));
            const float rspan = rip_rcp_mid(span);  // used only when every lane passes rcp_safe (2^-59.8 .. 2^59.8)
            const double yd = (double)yi;
            constexpr int PB = F::pb;   // pairs per block: their recurrences interleave
#pragma unroll
            for (int pb = 0; pb < GP; pb += PB) {
                f2 zz[PB], SS[PB];
                bool any_ex = false;
                if (a_full && !(dbg & 32)) {
                    f2 tt[PB], quo[PB];
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        const int p = pb + b;
                        float Sv[2];
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int g = 2 * p + e;
                            if constexpr (GE > G) {
                                if (g >= G) {   // dead half: a copy of its partner (same z: no exception of its own), zeroed below
                                    Sv[e] = Sv[0];
                                    continue;
                                }
                            }
                            if constexpr (SKIP0) {
                                if (g == 0) {   // skipped first group: its flag byte travels on, its value is its partner's (below)
                                    w[0] |= rr.q[0] & 0xffu;
                                    continue;
                                }
                            }
                            float S;
                            if constexpr (LT) {
                                S = rip_refpix_apply_iel((float)rr.S[g], rr.dk[g], rc[g], lt_w[chr * GE + g]);
                            } else {
                                const double *ln = LN + (chr * G + g) * 2;
                                S = rip_refpix_apply((float)rr.S[g], rr.dk[g], rc[g], ln[0], ln[1], yd);
                            }
                            if constexpr (BIAS) {
                                if (act) S = S - rr.bs[g];   // gen_cal_image.py:559-565
                            }
                            Sv[e] = S;
                            w[g / 4] |= (rr.q[g] & 0xffu) << (8 * (g & 3));
                        }
                        if constexpr (SKIP0) {
                            if (p == 0) Sv[0] = Sv[1];   // same z as its partner: no exception and no wave vote of its own
                        }
                        SS[b] = f2{Sv[0], Sv[1]};
                        const f2 t = SS[b] - f2{smin, smin};
                        tt[b] = t * 2.0f;
                    }
                    if (fastdiv) {  // one block: the PB reciprocal-division chains interleave
#pragma unroll
                        for (int b = 0; b < PB; ++b) quo[b] = div_rcp2(tt[b], span, rspan);
                    } else {
#pragma unroll
                        for (int b = 0; b < PB; ++b) quo[b] = f2{tt[b].x / span, tt[b].y / span};
                    }
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        f2 z = quo[b] + (-1.0f);
                        if constexpr (!SKIP0) {   // (SKIP0 implies do_not_flag_first; z.x is a copy of z.y there)
                            if (pb + b == 0 && a.do_not_flag_first) z.x = clip2<float>(z.x, -1.0f, 1.0f);
                        }
                        zz[b] = z;
                        any_ex = any_ex || (fabsf(z.x) > 1.0f) || (fabsf(z.y) > 1.0f);
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < PB; ++b) zz[b] = SS[b] = f2{0.0f, 0.0f};
                }
                // raw values of these groups of the next row (this row's are consumed)
                fetch_groups(ka, r + 4, 2 * pb, 2 * (pb + PB), rr);
                if (a_full && (dbg & 16)) {
#pragma unroll
                    for (int b = 0; b < PB; ++b) xs[(pb + b) * XR * COLS] = zz[b] + f2{1000.0f, 1100.0f};
                } else if (a_full) {
                    const bool slow = __any(any_ex);
                    f2 phi[PB];
                    bool ex[PB][2];
#pragma unroll
                    for (int b = 0; b < PB; ++b) ex[b][0] = ex[b][1] = false;
                    if (!slow) {
                        f2 pp[PB], pc[PB];
#pragma unroll
                        for (int b = 0; b < PB; ++b) {
                            phi[b] = f2{rr.cf[0], rr.cf[0]};
                            pp[b] = f2{1.0f, 1.0f};
                            pc[b] = zz[b];
                        }
#pragma unroll
                        for (int L = 1; L < NP; ++L) {
#pragma unroll
                            for (int b = 0; b < PB; ++b) {
                                const f2 term = pc[b] * rr.cf[L];
                                phi[b] = phi[b] + term;
                                const f2 u = zz[b] * c1[L];
                                const f2 pn = u * pc[b] - pp[b] * c2[L];
                                pp[b] = pc[b];
                                pc[b] = pn;
                            }
                        }
                    } else {
#pragma unroll
                        for (int b = 0; b < PB; ++b) {
                            float ph[2];
#pragma unroll
                            for (int e = 0; e < 2; ++e) {
                                if constexpr (SKIP0) {
                                    if (pb + b == 0 && e == 0) {   // skipped first group: no series
                                        ph[0] = 0.0f;
                                        continue;
                                    }
                                }
                                ph[e] = rip_legendre_series(e ? zz[b].y : zz[b].x, C2Legendre<NP>{rr.cf, c1, c2, chf}, ex[b][e]);
                            }
                            phi[b] = f2{ph[0], ph[1]};
                        }
                    }
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        const int p = pb + b;
                        const f2 fb = SS[b] - f2{rr.sref, rr.sref};
                        float vout[2];
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int g = 2 * p + e;
                            if constexpr (GE > G) {
                                if (g >= G) {   // dead half: zero in the ring, no flag
                                    vout[e] = 0.0f;
                                    continue;
                                }
                            }
                            if constexpr (SKIP0) {
                                if (g == 0) {   // skipped first group: zero in the ring; it raises no flag (do_not_flag_first)
                                    vout[e] = 0.0f;
                                    continue;
                                }
                            }
                            vout[e] = ((dq & bad) == 0) ? (e ? phi[b].y : phi[b].x) : (e ? fb.y : fb.x);
                            const bool first = (g == 0) && a.do_not_flag_first;
                            const uint32_t qg = w[g / 4] >> (8 * (g & 3));
                            if (!first && ex[b][e] && rip_lin_attempt(qg)) dq |= DQ_NO_LIN_CORR;
                        }
                        f2 xv = {vout[0], vout[1]};
                        if (act) xv = xv * rr.gain;
                        if constexpr (GE > G) {
                            if (2 * p + 1 >= G) xv.y = 0.0f;
                        }
                        if constexpr (SKIP0) {
                            if (p == 0) xv.x = 0.0f;
                        }
                        xs[p * XR * COLS] = col_ok ? xv : f2{0.0f, 0.0f};
                    }
                } else if (do_a) {
#pragma unroll
                    for (int b = 0; b < PB; ++b) xs[(pb + b) * XR * COLS] = f2{0.0f, 0.0f};
                }
            }
            if (do_a) {
                const bool keep = a_full && col_ok;
                DQ[xslot * COLS + col] = keep ? dq : 0u;
                if constexpr (F::wring) {
#pragma unroll
                    for (int i = 0; i < QW; ++i) QS[(xslot * QW + i) * COLS + col] = keep ? w[i] : 0u;
                    GN[xslot * COLS + col] = rr.gain;
                }
            }
            // IPC coefficients of row yc, consumed by C after the barrier; issued here so that their registers are not live
            // during A (requested at the top of the step instead: 0.949 against 0.945 ms, the latency is not on the critical path)
            f2 kC[5];
            double kCd[9];
            kC[4].y = 0.0f;
            unsigned vC;
            if constexpr (K64)
                vC = load_k(ka->kern, yc, do_c && wcol >= 1 && wcol < wl - 1, kCd, C2Int<0>{});
            else
                vC = load_k(ka->kern, yc, do_c && wcol >= 1 && wcol < wl - 1, kC, C2Int<0>{});
            CH_T(2)
            C2_SYNC();
            CH_T(3)
            const RIP_K ChainArgs *kb2 = &c2_args(kargs)->a;  // S2 copy
            // the share of the next row's coefficient planes that is requested beside pair p of C
            auto fetch_coefs_beside = [&](int p) { fetch_coefs(kb2, r + 4, p * CO_STEP, min(p * CO_STEP + CO_STEP, NCO), rr); };
            // ---- S2: issue the raw loads of row r+4 (consumed in S1 of the next step), then C of row yc
            CH_T(4)
            line_values(r + 4);   // the line values A of the next step subtracts
            {
                // every lane evaluates (lanes without valid terms produce values nobody reads); the coefficient planes of
                // the next row are requested between the pairs, unconditionally (see above)
                const bool all = __all(vC == 0x1ffu || vC == 0u);
                const int so = so_c;  // slot of row yc in both 3-row rings
                const int sm = (so == 0) ? 2 : so - 1, s0 = so, sp = (so == 2) ? 0 : so + 1;
                // hand the coefficients of destination row yc to the fit thread of this column (O2 of row yc, two steps on)
                if constexpr (KRN > 0) {
                    const int ks = yc & 1;
                    if constexpr (K64) {
#pragma unroll
                        for (int k = 0; k < KRN; ++k) KRd[(ks * KRN + k) * COLS + col] = kCd[k];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) KR2[(ks * 4 + i) * COLS + col] = kC[i];
                        KR1[ks * COLS + col] = kC[4].x;
                    }
                }
                if constexpr (K64) {
                    // PBC pairs in lockstep: their ring reads first, then interleaved f64 chains
                    constexpr int PBC = F::pbc;
#pragma unroll
                    for (int p0 = 0; p0 < GP; p0 += PBC) {
#pragma unroll
                        for (int q = 0; q < PBC; ++q)
                            fetch_coefs_beside(p0 + q);
                        if (do_c) {
                            float v[2 * PBC][9];
#pragma unroll
                            for (int q = 0; q < PBC; ++q) {
                                const f2 *xb = X2 + (p0 + q) * XR * COLS + col;
                                const f2 *xm_ = xb + sm * COLS, *x0_ = xb + s0 * COLS, *xp_ = xb + sp * COLS;
                                const f2 tt[9] = {x0_[0], xm_[0], xp_[0], x0_[-1], x0_[1], xm_[-1], xm_[1], xp_[-1], xp_[1]};
#pragma unroll
                                for (int k = 0; k < 9; ++k) v[2 * q][k] = tt[k].x, v[2 * q + 1][k] = tt[k].y;
                            }
                            double f[2 * PBC];
                            if (all)
                                c2_ipc9_batch<true, 2 * PBC>(v, kCd, vC, f);
                            else
                                c2_ipc9_batch<false, 2 * PBC>(v, kCd, vC, f);
#pragma unroll
                            for (int b = 0; b < 2 * PBC; ++b) {
                                const float xc = v[b][0];
                                // (SKIP0: group 0's iterate is a stored zero, its chain above is dead code)
                                O1d[((2 * p0 + b) * 3 + so) * COLS + col] = (SKIP0 && 2 * p0 + b == 0) ? 0.0 : (double)(xc + xc) - f[b];
                            }
                        }
                    }
                } else if (do_c && all && !(dbg & 1)) {
                    // interior wave: one straight-line block (see O2)
#pragma unroll
                    for (int i = 0; i < 5; ++i) asm volatile("" : "+v"(kC[i]));
#pragma unroll
                    for (int p0 = 0; p0 < GP; ++p0) {
                        fetch_coefs_beside(p0);
                        const f2 *xb = X2 + p0 * XR * COLS;
                        const f2 *xm[1] = {xb + sm * COLS}, *x0[1] = {xb + s0 * COLS}, *xp[1] = {xb + sp * COLS};
                        f2 f[1], xc[1];
                        fwd_rows_batch<1, true>(xm, x0, xp, col, kC, vC, f, xc);
                        f2 o1v = (xc[0] + xc[0]) - f[0];
                        if constexpr (SKIP0) {
                            if (p0 == 0) o1v.x = 0.0f;   // skipped first group: a stored zero, its half of the arithmetic is dead code
                        }
                        O12[(p0 * 3 + so) * COLS + col] = o1v;
                    }
                } else {
#pragma unroll
                    for (int p0 = 0; p0 < GP; ++p0) {
                        fetch_coefs_beside(p0);
                        if (do_c && !(dbg & 1)) {
                            const f2 *xb = X2 + p0 * XR * COLS;
                            const f2 *xm[1] = {xb + sm * COLS}, *x0[1] = {xb + s0 * COLS}, *xp[1] = {xb + sp * COLS};
                            f2 f[1], xc[1];
                            fwd_rows_batch<1, false>(xm, x0, xp, col, kC, vC, f, xc);
                            f2 o1v = (xc[0] + xc[0]) - f[0];
                            if constexpr (SKIP0) {
                                if (p0 == 0) o1v.x = 0.0f;
                            }
                            O12[(p0 * 3 + so) * COLS + col] = o1v;
                        }
                    }
                }
                if (GP * CO_STEP < NCO) fetch_coefs(kb2, r + 4, GP * CO_STEP, NCO, rr);
            }
            CH_T(5)
            CH_T(6)
            C2_SYNC();
            CH_T(7)
        }
    } else {
        // =========================================================================== fit waves
        f2 xnext[GP];  // x of (row r + 1, own column), read from the ring at the end of the step before (the ring holds 3 rows)
#pragma unroll
        for (int p0 = 0; p0 < GP; ++p0) xnext[p0] = f2{0.0f, 0.0f};
        const RipVariant v0 = rip_load_variant(vars, 0);
        const RipFitConst fc0 = rip_fit_const(h);
        constexpr int start = START;  // first group of the fit (exclude_first)
        float gain_next = 1.0f;   // gain, flag word and packed groupdq bytes of (row r + 1, own column): from the rings, like xnext
        uint32_t dq_next = 0, qw_next[QW];
#pragma unroll
        for (int i = 0; i < QW; ++i) qw_next[i] = 0;
        int o0_r = (R0 - 5 + 3000) % 3;  // O1 ring slot of row r
        uint32_t qb_next[F::wring ? 1 : G];   // 16 groups: the raw groupdq bytes of the next step's pixel
#pragma unroll
        for (int g = 0; g < (F::wring ? 1 : G); ++g) qb_next[g] = 0;
        f2 kn[5];       // narrow forms: the coefficients of the next step's row
        double kn_d[9];
#pragma unroll
        for (int i = 0; i < 5; ++i) kn[i] = f2{0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 9; ++k) kn_d[k] = 0.0;
        for (int r = R0 - 5; r < r_end; ++r, o0_r = (o0_r == 2) ? 0 : o0_r + 1) {
            const bool emit = (r >= R0) && (r < R1) && col_ok && (wcol >= 2 || c < 2) && (wcol < wl - 2 || c >= nx - 2);
            const RIP_K C2KernArgs *kf = c2_args(kargs);  // S1 copy of the argument block
            const unsigned rc_ = (unsigned)min(max(r, R0), yhi);   // (rows before R0 are warm-up steps: nothing is emitted there)
            const unsigned pe = rc_ * (unsigned)nx + cc1;
            // ---- S1: read noise of the pixel (used by the fit), then the second IPC iterate of row r
            const __amdgpu_buffer_rsrc_t rpl = c2_rsrc(kf->a.planes);
            const unsigned t_row = rc_ * row4;  // byte offset of row r in an f32 plane (uniform)
            const unsigned t_ld = (dbg & 256) ? 0u : t_row;   // timing experiment: the fit role's loads all hit row 0 (cached)
            const float e_read = c2_ld_f32<SA>(rpl, cc4, (unsigned)(NP + 5) * pl4 + t_ld);
            const float e_gain = gain_next;
            // calibration planes of the tail (finish) of the same pixel, consumed after the barrier
            const size_t t_row4 = (size_t)t_row;
            const size_t pe_row = (size_t)(rc_ * (unsigned)nx);   // element offset of row r
            const float e_dark = c2_ld_f32<SA>(rpl, cc4, (unsigned)(NP + 6) * pl4 + t_ld);
            // (flat flags and dark dq arrive with the linearity dq of the pixel: ChainArgs::merged_dq)
            const uint32_t e_pdq = c2_ld_u32<SA>(c2_rsrc(kf->a.pdq), cc4, t_ld);
            // flat / dark_dq == null: read the first slab plane instead (value unused), keeps the loads in one block
            const float e_flat_raw = c2_ld_f32<SA>(c2_rsrc(kf->a.flat ? (const void *)kf->a.flat : (const void *)kf->a.planes), cc4, t_ld);
            const float e_flat = kf->a.flat ? e_flat_raw : 1.0f;
            float d[GE];
            f2 dpair[GP];
            uint32_t qw[QW];  // the pixel's groupdq bytes, packed
#pragma unroll
            for (int i = 0; i < QW; ++i) qw[i] = 0;
            uint32_t lin_dq = 0;  // linearity dq of the pixel
            RipFitState fs;
            const bool act = emit && col_act && r >= ay0 && r < ay1;
            CH_T(0)
            C2_DRAIN()
            CH_T(1)
            // narrow forms: the fit role loads the coefficients the K ring does not carry itself (all lanes: clamped addresses),
            // requested at the end of the step before: they land across the barrier
            f2 kF[5];
            double kFd[9];
            kF[4].y = 0.0f;
            if constexpr (KFIT) {
#pragma unroll
                for (int k = 0; k < 9; ++k) kFd[k] = kn_d[k];
#pragma unroll
                for (int i = 0; i < 5; ++i) kF[i] = kn[i];
            }
            if (emit) {
                // the nine coefficients of destination (r, col) from the ingest thread of this column
                if constexpr (KRN > 0) {
                    const int ks = r & 1;
                    if constexpr (K64) {
#pragma unroll
                        for (int k = 0; k < KRN; ++k) kFd[k] = KRd[(ks * KRN + k) * COLS + col];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) kF[i] = KR2[(ks * 4 + i) * COLS + col];
                        kF[4].x = KR1[ks * COLS + col];
                    }
                }
                const unsigned vF = k_valid(r);
#pragma unroll
                for (int i = 0; i < QW; ++i) qw[i] = qw_next[i];
                if constexpr (!F::wring) {   // packed as the ingest role packs them
#pragma unroll
                    for (int i = 0; i < QW; ++i) qw[i] = 0;
#pragma unroll
                    for (int g = 0; g < G; ++g) qw[g / 4] |= (qb_next[g] & 0xffu) << (8 * (g & 3));
                }
                lin_dq = dq_next;
                const bool fastdiv = __all(rcp_safe(e_gain) || !act);
                const float rgain = rip_rcp_mid(e_gain);
                const bool all = __all(vF == 0x1ffu || !act);
                const int o0_ = o0_r, om_ = (o0_r == 0) ? 2 : o0_r - 1, op_ = (o0_r == 2) ? 0 : o0_r + 1;
                constexpr int NB = (GP % 2 == 0) ? 2 : 1;
                if constexpr (K64) {
                    // f64 iterate: (O1 + x) - fwd(O1) and the division by the gain in f64, one rounding to f32 at the end; NBO groups in
                    // lockstep (their ring reads, then interleaved chains), the divisions together at the end.  Lanes that are not
                    // active (border pixels) evaluate on whatever the rings hold there and keep x.
                    constexpr int NBO = F::nbo;
                    double o2v[GE];
#pragma unroll
                    for (int gb = 0; gb < GE; gb += NBO) {
                        double v[NBO][9];
#pragma unroll
                        for (int b = 0; b < NBO; ++b) {
                            const double *ob = O1d + (size_t)(gb + b) * 3 * COLS + col;
                            const double *om = ob + om_ * COLS, *o0 = ob + o0_ * COLS, *op = ob + op_ * COLS;
                            v[b][0] = o0[0], v[b][1] = om[0], v[b][2] = op[0], v[b][3] = o0[-1], v[b][4] = o0[1], v[b][5] = om[-1],
                            v[b][6] = om[1], v[b][7] = op[-1], v[b][8] = op[1];
                        }
                        double f[NBO];
                        if (all)
                            c2_ipc9_batch<true, NBO>(v, kFd, vF, f);
                        else
                            c2_ipc9_batch<false, NBO>(v, kFd, vF, f);
#pragma unroll
                        for (int b = 0; b < NBO; ++b) {
                            const float xc = ((gb + b) & 1) ? xnext[(gb + b) / 2].y : xnext[(gb + b) / 2].x;
                            o2v[gb + b] = (v[b][0] + (double)xc) - f[b];
                        }
                    }
                    float qf[GE];
                    if constexpr (GE > G) qf[G] = 0.0f;
                    if constexpr (SKIP0) qf[0] = 0.0f;
                    c2_div64_shared<G, GE, SKIP0 ? 1 : 0>(o2v, e_gain, act, qf);   // (a dead half takes no part in its range vote)
#pragma unroll
                    for (int g = 0; g < GE; ++g) {
                        const float xc = (g & 1) ? xnext[g / 2].y : xnext[g / 2].x;
                        d[g] = act ? qf[g] : xc;
                    }
#pragma unroll
                    for (int p0 = 0; p0 < GP; ++p0) dpair[p0] = f2{d[2 * p0], d[2 * p0 + 1]};
                } else if (all && fastdiv && __all(act) && !(dbg & 2)) {
                    // interior wave: one straight-line block (the coefficient pairs stay 64-bit registers whose halves the
                    // packed multiplies broadcast through op_sel)
#pragma unroll
                    for (int i = 0; i < 5; ++i) asm volatile("" : "+v"(kF[i]));
#pragma unroll
                    for (int p0 = 0; p0 < GP; p0 += NB) {
                        f2 xc[NB];
                        const f2 *om[NB], *o0[NB], *op[NB];
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            xc[b] = xnext[p0 + b];
                            const f2 *ob = O12 + (p0 + b) * 3 * COLS;
                            om[b] = ob + om_ * COLS, o0[b] = ob + o0_ * COLS, op[b] = ob + op_ * COLS;
                        }
                        f2 f[NB], oc[NB];
                        fwd_rows_batch<NB, true>(om, o0, op, col, kF, vF, f, oc);
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            const f2 val = div_rcp2((oc[b] + xc[b]) - f[b], e_gain, rgain);
                            d[2 * (p0 + b)] = val.x;
                            d[2 * (p0 + b) + 1] = val.y;
                            dpair[p0 + b] = val;
                        }
                    }
                } else {
                    constexpr int NBG = 1;  // boundary waves (rare): one pair at a time keeps this path's register demand low
#pragma unroll
                    for (int p0 = 0; p0 < GP; p0 += NBG) {
                        f2 xc[NBG], val[NBG];
#pragma unroll
                        for (int b = 0; b < NBG; ++b) val[b] = xc[b] = xnext[p0 + b];
                        if (act && !(dbg & 2)) {
                            const f2 *om[NBG], *o0[NBG], *op[NBG];
#pragma unroll
                            for (int b = 0; b < NBG; ++b) {
                                const f2 *ob = O12 + (p0 + b) * 3 * COLS;
                                om[b] = ob + om_ * COLS, o0[b] = ob + o0_ * COLS, op[b] = ob + op_ * COLS;
                            }
                            f2 f[NBG], oc[NBG];
                            if (all)
                                fwd_rows_batch<NBG, true>(om, o0, op, col, kF, vF, f, oc);
                            else
                                fwd_rows_batch<NBG, false>(om, o0, op, col, kF, vF, f, oc);
                            f2 o2[NBG];
#pragma unroll
                            for (int b = 0; b < NBG; ++b) o2[b] = (oc[b] + xc[b]) - f[b];
                            if (fastdiv) {
#pragma unroll
                                for (int b = 0; b < NBG; ++b) val[b] = div_rcp2(o2[b], e_gain, rgain);
                            } else {
#pragma unroll
                                for (int b = 0; b < NBG; ++b) val[b] = f2{o2[b].x / e_gain, o2[b].y / e_gain};
                            }
                        }
#pragma unroll
                        for (int b = 0; b < NBG; ++b) {
                            d[2 * (p0 + b)] = val[b].x;
                            d[2 * (p0 + b) + 1] = val[b].y;
                            dpair[p0 + b] = val[b];
                        }
                    }
                }
                // odd G: whatever the pair arithmetic left in the dead half (0 / gain), the fit sees a zero there
                if constexpr (GE > G) d[G] = 0.0f, dpair[GP - 1].y = 0.0f;
                // skipped first group: a zero that nothing below reads -- no weight, no tested difference, no refit term
                if constexpr (SKIP0) d[0] = 0.0f, dpair[0].x = 0.0f;
                // first half of the ramp fit (registers only): slope, errors, approximate jump significances
                const bool unsat = ((qw[(G - 1) / 4] >> (8 * ((G - 1) & 3))) & DQ_SATURATED) == 0;
                if (!(dbg & 4))
                    fit_full_pk_a<G, rip_full_valid<G, START>(), SKIP0>(dpair, fc0, v0, kf->a.dense, e_gain, e_read, unsat && act, kf->guard, fs);
            }
            CH_T(2)
            C2_SYNC();
            CH_T(3)
            const RIP_K C2KernArgs *kg = c2_args(kargs);  // S2 copy
            // ---- S2: the rest of pixel (r, c); at its end the per-pixel words of row r + 1 from the rings
            CH_T(4)
            C2_DRAIN()
            CH_T(5)
            // The tail of pixel (r, c), three steps in order.  (They stay lambdas: written out in place, the same code is given
            // another register assignment.)
            float s = 0.0f, er = 0.0f, ep = 0.0f;
            uint32_t jmask = 0, pdq = 0;
            // second half of the fit: exact pass where needed, jump mask; then the saturated refits
            auto part_fb = [&]() {
                if constexpr (!SKIP0) {   // (the launcher never takes SKIP0 for a call that wants the cube)
                    if (kg->a.cube_out) {
#pragma unroll
                        for (int g = 0; g < G; ++g) kg->a.cube_out[(unsigned)g * npix + pe] = d[g];
                    }
                }
                uint32_t qor = 0;
#pragma unroll
                for (int i = 0; i < QW; ++i) qor |= qw[i];
                const bool anysat = (qor & 0x02020202u) != 0u;
                const bool unsat = ((qw[(G - 1) / 4] >> (8 * ((G - 1) & 3))) & DQ_SATURATED) == 0;
                if (dbg & 4) {
                    s = d[0], er = e_read, ep = e_gain;
                } else {
                    fit_full_pk_b<G>(dpair, kg->h, fc0, kg->a.dense, kg->kvals + v0.k_ofs, kg->diffs + v0.diff_ofs, unsat && act,
                                     fs, jmask);
                    s = fs.s, er = fs.er, ep = fs.ep;
                    if (__any(anysat)) {
                        uint32_t qe[G];
#pragma unroll
                        for (int g = 0; g < G; ++g) qe[g] = (qw[g / 4] >> (8 * (g & 3))) & 0xffu;
                        trunc_layers<G, G - 1, GE, SKIP0>(d, qe, kg->h, kg->vars, kg->kvals, kg->diffs, e_gain, e_read, act, kg->guard, s, er,
                                                          ep, jmask);
                    }
                }
            };
            // T: flag propagation (fitting.py:339-353) and the stores of the group flags
            auto part_flags = [&]() {
                if (dbg & 8) return;
                uint8_t *gq = (kg->a.gdq_out && !(dbg & 512)) ? kg->a.gdq_out + pe_row : nullptr;
                pdq = propagate_flags_packed<G>(qw, jmask, start, e_pdq | lin_dq, gq, npix, c2_opaque(cc1));
            };
            // T: finish and the stores of the four planes
            auto part_finish = [&]() {
                if (dbg & 8) return;
                if (kg->a.finish) {
                    // gen_cal_image.py:458-475, 213-229, 607-629.  One wave vote selects the straight-line form built
                    // from the short exact operations (rip_rcp_mid, rip_sqrt_mid, sqrt(x*x) = x: tools/gpu_checks/
                    // fpcheck.hip); every intermediate then lies in their validated range 2^-100 .. 2^100 or is +0.
                    const float sd = (act && kg->a.dark_rate) ? s - e_dark : s;
                    const bool lean = kg->a.flat && __all(act && rip_mid36(sd) && (er == 0.0f || rip_mid36(er)) &&
                                                          (ep == 0.0f || rip_mid36(ep)) && e_flat > 0.0f && rip_mid36(e_flat));
                    if (lean) {
                        const float err = hypot_f32(er, ep);
                        const float ep2 = ep;  // sqrt(ep * ep)
                        const float e2 = err * err;
                        const float p2 = ep2 * ep2;
                        const float er2 = rip_sqrt_mid(clip_lo<float>(e2 - p2, 0.0f));
                        const float rflat = rip_rcp_mid(e_flat);
                        s = div_rcp(sd, e_flat, rflat);
                        er = div_rcp(er2, e_flat, rflat);
                        ep = div_rcp(ep2, e_flat, rflat);
                    } else {
                        rip_finish(act, [&] { return act && kg->a.dark_rate; }, e_dark, [&] { return kg->a.flat != nullptr; }, e_flat, s, er, ep);
                    }
                }
                const unsigned w4 = c2_opaque(cc4);
                // (dbg & 512: timing experiment without the plane stores; the test keeps the four values live)
                if (!(dbg & 512) || (s + er + ep == 12345.678f && pdq == 0xdeadbeefu)) {
                    *reinterpret_cast<float *>(reinterpret_cast<char *>(kg->a.slope) + t_row4 + w4) = s;
                    *reinterpret_cast<float *>(reinterpret_cast<char *>(kg->a.err_read) + t_row4 + w4) = er;
                    *reinterpret_cast<float *>(reinterpret_cast<char *>(kg->a.err_poisson) + t_row4 + w4) = ep;
                    *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(kg->a.pdq_out) + t_row4 + w4) = pdq;
                }
            };
            if (emit) {
                part_fb();
                part_flags();
                part_finish();
            }
            // x of (r + 1, own column) for the next step's O2: its ring slot is overwritten in S1 of that step (row r + 4)
            {
                const int sn = (o0_r == 2) ? 0 : o0_r + 1;
#pragma unroll
                for (int p0 = 0; p0 < GP; ++p0) xnext[p0] = X2[(p0 * XR + sn) * COLS + col];
                dq_next = DQ[sn * COLS + col];
                if constexpr (F::wring) {
#pragma unroll
                    for (int i = 0; i < QW; ++i) qw_next[i] = QS[(sn * QW + i) * COLS + col];
                    gain_next = GN[sn * COLS + col];
                } else {
                    // the fit role's own loads of row r + 1 (second read of lines its ingest role fetched three steps earlier):
                    // packed as the ingest role packs them; rows / columns outside the frame are never emitted
                    const unsigned yl = (unsigned)min(max((dbg & 1024) ? R0 : r + 1, ylo), yhi);   // (dbg 1024: timing, the re-read hits cache)
                    const __amdgpu_buffer_rsrc_t rq = c2_rsrc(kg->a.gdq);
                    unsigned o1 = yl * (row4 >> 2);
#pragma unroll
                    for (int g = 0; g < G; ++g) {   // (raw: packed at the top of the next step, when they have landed)
                        qb_next[g] = c2_ld_u8(rq, cc1, o1);
                        o1 += npix;
                    }
                    gain_next = c2_ld_f32(c2_rsrc(kg->a.planes), cc4, (unsigned)(NP + 4) * pl4 + yl * row4);
                }
            }
            // (two steps ahead instead -- half a step after the ingest role's read of the same lines: fabric traffic 1.44 -> 1.19 x
            // (f64), 1.50 -> 1.39 x (16 groups), 1.38 -> 1.27 x (both), and the kernels 3 % / 0 % / 10 % SLOWER: nine to eighteen more
            // live registers; not bound by bytes)
            if constexpr (KFIT) {
                if constexpr (K64)
                    (void)load_k(kg->a.kern, (dbg & 1024) ? R0 : r + 1, true, kn_d, C2Int<KRN>{});
                else
                    (void)load_k(kg->a.kern, (dbg & 1024) ? R0 : r + 1, true, kn, C2Int<0>{});
            }
            CH_T(6)
            C2_SYNC();
            CH_T(7)
        }
    }
#ifdef CH_STAMP
    if ((tid & 63) == 0 && a.dbg_buf) {
        unsigned long long *o = a.dbg_buf + ((size_t)blockIdx.x * (F::threads / 64) + (tid >> 6)) * 9;
        for (int i = 0; i < 9; ++i) o[i] += st_[i];
    }
#endif
}

template <int NP, int G, int START, typename KT, bool SKIP0 = false, bool BIAS = true>
static int launch_chain2_s(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a) {
    using F = C2Form<G + (G & 1), sizeof(KT) == 8>;
    const size_t lds = F::lds_bytes;
    if (a.nb < 2) return 1;   // (the frame-edge lanes of the first / last strip emit without neighbours: border pixels)
    ChainArgs ag = a;
    const long grid = c2_form_geometry<F>(ag, ctx->ncu, ctx->chain_reserve, ctx->chain_quad, ctx->last_geo);
    static bool lds_set[64] = {};   // per device, once per instantiation (contexts are used from one thread each)
    if (lds > 48 * 1024 && !lds_set[ctx->device & 63]) {
        RIP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(chain2_kernel<NP, G, START, KT, SKIP0, BIAS>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set[ctx->device & 63] = true;
    }
    hipLaunchKernelGGL((chain2_kernel<NP, G, START, KT, SKIP0, BIAS>), dim3((unsigned)grid), dim3(F::threads), lds, ctx->stream, ag,
                       reinterpret_cast<const RipPlanHeader *>(plan->dev), plan->d_variants, plan->d_k, plan->d_diffs,
                       ctx->guard_band);
    RIP_HIP(ctx, hipGetLastError());
    // the host's running total of the workgroups that will have counted themselves in (modulo 2^32, like the counter)
    if (ag.wg_counter) ctx->gate_total += (uint32_t)grid, ctx->gate_armed = true;
    return RIP_OK;
}

// returns the launch status, or 1 when the plan is not one the specialised kernel was compiled for: the dense table the kernel
// reads (plan.hip builds it from the plan's differences) must test exactly the differences of the compile-time mask -- for odd G
// too, where no tested difference may touch the dead half of the last pair
// skip0: take the form that skips group 0 (the caller has established that it may: rip_chain_may_skip_first, chain.hip)
// A call without a bias stream (bias_records == 0: calibrate.hip, from the screening of the set at upload, caldir.hip) takes the
// instantiation that has no biascorr loads and no subtraction where the form table names one (C2Form::nobias); in every other
// form the zero-record descriptor of the one instantiation drops the loads.
template <int NP, int G, typename KT, bool BIAS>
static int launch_chain2_b(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a, bool skip0) {
    if (plan->h.start == 0 && plan->dense.valid == rip_full_valid<G, 0>())
        return skip0 ? 1 : launch_chain2_s<NP, G, 0, KT, false, BIAS>(ctx, plan, a);
    if (plan->h.start == 1 && plan->dense.valid == rip_full_valid<G, 1>())
        return skip0 ? launch_chain2_s<NP, G, 1, KT, true, BIAS>(ctx, plan, a) : launch_chain2_s<NP, G, 1, KT, false, BIAS>(ctx, plan, a);
    return 1;
}
template <int NP, int G, typename KT>
static int launch_chain2(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a, bool skip0) {
    if constexpr (C2Form<G + (G & 1), sizeof(KT) == 8>::nobias) {
        if (a.bias_records == 0) return launch_chain2_b<NP, G, KT, false>(ctx, plan, a, skip0);
    }
    return launch_chain2_b<NP, G, KT, true>(ctx, plan, a, skip0);
}

// The fused kernel for NP Legendre planes and ipc4d coefficients of type KT, the group counts of part PART of the list
// (rip_common.h: RIP_CHAIN_G_PART*); chain.hip calls it for the configurations it lists, chain_np*.hip instantiate it.  Returns
// the launch status, or 1 when no instantiation fits (the caller then takes the stage kernels).
template <int NP, typename KT, int PART>
int rip_launch_chain2(rip_ctx *ctx, const RipPlan *plan, const ChainArgs &a, bool skip0) {
    static_assert(PART >= 0 && PART <= 2, "parts of RIP_CHAIN_G_ALL");
#define C2_CASE(g) \
    if (a.ngrp == g) return launch_chain2<NP, g, KT>(ctx, plan, a, skip0);
    if constexpr (PART == 0) {
        RIP_CHAIN_G_PART0(C2_CASE)
    } else if constexpr (PART == 1) {
        RIP_CHAIN_G_PART1(C2_CASE)
    } else {
        RIP_CHAIN_G_PART2(C2_CASE)
    }
#undef C2_CASE
    return 1;
}
