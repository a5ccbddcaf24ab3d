// The form table of the fused L1->L2 kernel (chain2_kernel.h): compile-time constants only, so that the dispatch (chain.hip) can
// ask about a form without instantiating a kernel.
#pragma once
#include "rip_common.h"

// The forms of the kernel, one per (group count, ipc4d dtype), and every choice that differs between them.  What does not fit the
// 256-column form's LDS twice per CU runs a NARROW form: one wide workgroup per CU that drops rings, and what a dropped ring
// carried the fit role loads itself, one step ahead (a second read of lines the ingest role fetched 1.5 steps earlier):
//   ipc4d  groups  narrow  columns  waves/SIMD  rings
//   f32    5-8     0       256      4           every ring, two workgroups per CU (the bench path)
//   f64    5-8     1       384      3           a PARTIAL K ring (krn; every ring at 256 columns: 120 KB, one workgroup per CU)
//   f32    9-16    2       384      3           no K ring, no gain / groupdq rings
//   f64    9-16    2       256      2           no K ring, no gain / groupdq rings
// A form is a function of the PADDED count GE = G rounded up to whole pairs (6, 8, 10, 12, 14, 16): 5 runs the form of 6, 7 of 8,
// 9 of 10 ... 15 of 16, and 10, 12, 14 are the 16-group form with fewer ring planes (narrow, columns, waves per SIMD, cache
// policy and ring set inherited from it unchanged; none of these was chosen by a timing run of its own).  Per form, from the
// compiler's resource report (VGPRs: range over the three Legendre orders and both starts; no form spills a vector register
// or uses scratch; 5 to 8 groups of f32 ipc4d: both the instantiation with and the one without a bias stream) and C2Form::lds_bytes:
//   G      f32 ipc4d: VGPRs  LDS bytes  pb      f64 ipc4d: VGPRs  LDS bytes  pb / pbc / nbo
//   5      101-103           68448      1       134-135           157056     1 / 1 / 2
//   6      104-111           68448      1       137               157056     1 / 1 / 2
//   7      111-124           81024      2       147               160256     2 / 1 / 2
//   8      115-128           81024      2       153               160256     2 / 1 / 2
//   9      120-124           97408      1       171               95712      1 / 1 / 2
//   10     122-128           97408      1       179               95712      1 / 1 / 2
//   11     131               115968     1       221               114240     3 / 2 / 4
//   12     139               115968     1       227               114240     3 / 2 / 4
//   13     135               134528     1       196               132768     1 / 1 / 2
//   14     139               134528     1       202               132768     1 / 1 / 2
//   15     145               153088     1       253-254           151296     4 / 2 / 4
//   16     149               153088     1       256               151296     4 / 2 / 4
// (budgets: 128 / 168 / 256 VGPRs at 4 / 3 / 2 waves per SIMD.)  What this leaves on the table, not chased here: the f64 forms of
// 9, 10, 13 and 14 groups run block factors 1 / 1 / 2 because 5 and 7 pairs have no other divisor -- a tail block would let them
// keep 4 / 2 / 4; and 9 to 14 groups at one workgroup per CU leave 26 to 65 KB of LDS unused, room for wider strips or a ring
// the 16-group form had to drop.
//
// ODD G: the pair machinery stays, with GP = (G + 1) / 2 pairs and the second half of the last pair DEAD.  The dead half is
//   - never loaded (the ingest role's group loads, the fit role's groupdq re-read and the row corrections stop at G),
//   - a copy of its partner inside the linearity block (same z, so it raises no exception and no wave vote of its own), then
//     a ZERO in the x ring; it sets no flag and its groupdq byte is never packed (the packed words carry zeros there),
//   - whatever 0 * k gives in the O1 ring and after the second iterate (possibly NaN for a non-finite coefficient or gain):
//     nobody reads it -- the f64 division's range vote looks at the G real quotients only, and the fit role overwrites the
//     dead half of its registers with zero before the fit,
//   - never stored: the cube and groupdq stores stop at G,
//   - outside the fit: no weight and no add in the slope sum (not even a signed zero), absent from rip_full_valid<G, START>
//     (no tested difference touches it: the launcher compares that mask with the plan's dense table and falls back to the
//     stage kernels on any mismatch), absent from the saturated refits (trunc_layers runs on the first G - 1 ... 3 real groups)
//     and from the flag propagation (propagate_flags_packed<G>: missing groups count as DO_NOT_USE in its all-groups test only).
// Every `g < G` test is a compile-time constant after unrolling; with even G the guarded code does not exist (if constexpr), so
// the 6-, 8- and 16-group kernels compile to the instruction streams they had before.
//
// SKIPPED FIRST GROUP (template parameter SKIP0 of the kernel, START = 1 only): the mirror image -- the FIRST half of pair 0 is
// dead.  With an excluded first group the fit gives d[0] the weight +-0 and tests no difference on it, so d[0] reaches the
// results only as 0 * (d[0] - d[1]) added to a sum that starts at +0: nothing, unless d[0] is not finite (or so large that the
// difference overflows).  The launcher takes this form only where |d[0]| < 2^103 is known without computing it: a CALDIR set
// that passed the screen at upload (caldir.hip: the bounds and the chain of bounds), a u16 cube, do_not_flag_first, no cube
// output, weight zero in every variant (calibrate.hip: choose_skip; chain.hip: rip_chain_may_skip_first).  Everything else
// runs the SKIP0 = false instantiation, which is the kernel as it was.  The same items as for odd G; group 0 is
//   - never loaded: cube, dark and biascorr samples, its row corrections (the scalar loads start at group 1) and its channel
//     lines (the LDS table holds zeros there) -- the pre-pass does not make the tables of group 0 in front of this form, so its
//     entries are unwritten memory.  Its groupdq BYTE stays live: loaded, packed, propagated and stored exactly as before,
//   - a copy of its partner inside the linearity block (same z: no exception and no wave vote of its own; the clip of
//     do_not_flag_first has nothing left to clip), its series is not evaluated, then a ZERO in the x ring; it sets no flag
//     (it set none before: do_not_flag_first),
//   - a stored zero in the O1 ring, and whatever the pair arithmetic gives after the second iterate: nobody reads it (the
//     arithmetic of a dead half has no consumer and is removed by the compiler: the x / O1 ring halves are unread in that sense),
//     outside the f64 division (not divided, not in its range vote), and the fit role overwrites d[0] with zero before the fit,
//   - outside the fit: no term in the slope sum of fit_full_pk_a_t (the sum starts with group 1's term added to +0, as it did
//     after (+0) + (+-0)), none in fit_full_regs / trunc_layers (the two-point weights have K[0] = 0 too), absent from
//     rip_full_valid<G, 1> as it always was.
// The pairs keep their positions (d1 = dA[0].y); with odd G both dead halves exist side by side.  Every test on SKIP0 is a
// compile-time constant, so the SKIP0 = false kernels compile to the instruction streams they had before.
// Round 3 ran the narrow forms as 128-column workgroups, three (two) per CU: 3 (2) waves per SIMD at <= 168 (256) VGPRs.  What they
// paid is windows at a 124-column pitch: a window row of a byte plane is one 128-byte line, misaligned it touches two (u16: two ->
// three, f32: four -> five), and the lines shared with the neighbouring strip have left L2 by the time that strip wants them -- a
// third of the algorithmic bytes fetched twice.  Round 4: ONE workgroup per CU of 384 columns (f64 x 16 groups: 256) -- the same
// waves per SIMD and LDS per CU, a third (half) of the seams: 6-8 % faster, same bits.  Same arithmetic as the 256-column form,
// which keeps 256 columns (128-column workgroups WITH every ring: 4 % slower, profiles/r03_summary.md; the narrow forms are slower
// there too: same 16 waves per CU).
// The half-step barrier falls after the first half of the fit in every form.  Same-box A/B of its place -- there / after the second
// half of the fit and the saturated refits / after the flag propagation and the group-flag stores: f32 ipc4d x 8 groups 0.884 /
// 0.887 / 0.895 ms (profiles/r03_summary.md); the wide narrow forms (round 4) 16 groups 1.704 / 1.770 / 1.751 ms per ramp, f64 x 16
// groups 2.251 / 2.278 / 2.302, f64 x 8 groups 1.138 / 1.145 / 1.153.
// largest block factor <= want that divides n: a blocked loop over n items then has no tail
constexpr int c2_block(int n, int want) {
    int d = want < 1 ? 1 : want;
    while (n % d) --d;
    return d;
}
// G here is the PADDED group count (whole pairs): an odd ramp runs the form of the next even count
template <int G, bool K64>
struct C2Form {
    static_assert(G % 2 == 0 && G > 4 && G <= 16, "forms exist for whole pairs of groups, 6 to 16");
    static constexpr int narrow = G > 8 ? 2 : (K64 ? 1 : 0);
    // columns of a workgroup's window, and its threads (two roles of one thread per column)
    static constexpr int cols = (narrow == 0 || (narrow == 2 && K64)) ? 256 : 384;
    static constexpr int threads = 2 * cols;
    // Strip geometry: the window of strip s starts at column s * outw; its lanes 2 .. cols-3 emit, lanes 0, 1 and cols-2, cols-1
    // are the halo of the two 3 x 3 passes -- except at the frame's edge, where columns 0, 1 and nx-2, nx-1 are emitted by those
    // lanes themselves (border pixels: no IPC, no neighbours needed; nb >= 2).  So n strips cover n * outw + 4 columns: 33 strips
    // of 128 columns cover 4096 exactly (34 with a uniform 2-column offset), 17 of 256.
    static constexpr int outw = cols - 4;
    static constexpr int nstrips(int nx) { return (nx - 4 + outw - 1) / outw < 1 ? 1 : (nx - 4 + outw - 1) / outw; }
    // waves per SIMD it is compiled for (register budget 512 / waves: 128, 168, 256 VGPRs) and launched with
    static constexpr int wps = narrow == 0 ? 4 : ((narrow == 2 && K64) ? 2 : 3);

    // The LDS layout, byte offsets; the ring slots of a row are `cols` columns wide:
    static constexpr int ks = K64 ? 8 : 4;                               // bytes of a coefficient and of an O1 value
    static constexpr int x_ofs = 0;                                      // [G/2][3] f2: x = gain*phi, pair-interleaved
    static constexpr int o1_ofs = x_ofs + G / 2 * 3 * cols * 8;          // [G/2][3] f2 (f64 ipc4d: [G][3] double): first iterate
    static constexpr int dq_ofs = o1_ofs + G * 3 * cols * ks;            // [3] u32: the flag word of the pixel
    // the packed groupdq bytes and the gain of the pixel travel from the ingest thread of a column to its fit thread too --
    // except in the 16-group forms, whose fit role loads them itself, like the coefficients
    static constexpr bool wring = narrow < 2;
    static constexpr int qs_ofs = dq_ofs + 3 * cols * 4;                          // [3][(G+3)/4] u32: groupdq bytes, packed
    static constexpr int gn_ofs = qs_ofs + (wring ? 3 * ((G + 3) / 4) * cols * 4 : 0);  // [3] f32: gain
    static constexpr int nlc = cols / RIP_CW + 1;                                 // channels a window can touch (not channel-aligned)
    static constexpr int ln_ofs = gn_ofs + (wring ? 3 * cols * 4 : 0);            // [nlc][G][2] double: channel lines of this strip
    static constexpr int kr_ofs = ln_ofs + nlc * G * 2 * 8;                       // [2][krn] KT: the K ring
    // Coefficients the K ring holds: all nine, or what the rest of the layout leaves of the 160 KB of a CU.  That cap matters at
    // f64 ipc4d x 8 groups (129.5 KB at 384 columns): the first five of the nine f64 coefficients travel from the ingest thread to
    // the fit thread through LDS, the fit role reads only the other four planes a second time -- 32 instead of 72 bytes per pixel of
    // re-read (traffic 1.33 -> 1.18 x), five loads fewer per step in flight in the fit role.  The 16-group forms have no K ring.
    static constexpr int krn_room = (160 * 1024 - kr_ofs) / (2 * cols * ks);
    static constexpr int krn = narrow == 2 ? 0 : (krn_room < 9 ? krn_room : 9);
    // The LEAN pieces of the 256-column form (f32 ipc4d, 5 to 8 groups), which is bound by the instructions it issues:
    //   - nobias: a second instantiation WITHOUT the biascorr stream (template parameter BIAS of the kernel) runs where the call
    //     has none (ChainArgs::bias_records == 0): no biascorr loads, no S - bs, no registers for them.  Every other form keeps
    //     the one instantiation, whose zero-record descriptor drops the loads in hardware.
    //   - lt: the channel-line values m * y + c of a row are computed once per (ingest wave, channel, group) and read from a
    //     table by the lanes, [cols / 64][nlc][G] doubles (a table per ingest wave: in quad mode every wave column marches down
    //     a row range of its own): 768 bytes at 8 groups, 81024 in all, still two workgroups per CU.  The narrow forms (f64
    //     ipc4d, and 9 to 16 groups) keep the per-lane evaluation: f64 ipc4d x 5 to 8 groups sizes its K ring from what the rest
    //     of the layout leaves of the CU's 160 KB (3.5 to 6.6 KB stay free), the forms of 9 to 16 groups have room; none of
    //     them was measured with a table, so none was changed.
    static constexpr bool nobias = narrow == 0;
    static constexpr bool lt = narrow == 0;
    static constexpr int lt_ofs = kr_ofs + 2 * krn * cols * ks;               // [cols / 64][nlc][G] double: line values of the row
    static constexpr int lds_bytes = lt_ofs + (lt ? (cols / 64) * nlc * G * 8 : 0);
    static_assert(lds_bytes <= (narrow == 0 ? 80 : 160) * 1024, "the 256-column form runs two workgroups per CU, the others one");

    // Cache policy of the ONCE-read arrays (aux bits of the buffer loads; 2 = nt: stream through the caches).  The narrow forms' fit
    // role reads the IPC coefficients (16 groups: gain and groupdq bytes too) a second time one row step after the ingest role; a
    // step of an XCD's 96 workgroups moves about 4 MB -- the size of its L2 -- so those lines have left L2 by then and come back
    // over the fabric (1.4-1.5 x the algorithmic bytes at ~5 TB/s of fabric traffic).  With the hint on everything read once,
    // same-box A/B (profiles/r04_summary.md): 16 groups 1.752 -> 1.730 / 1.780 -> 1.738 ms, f64 x 16 groups 2.414 -> 2.383 / 2.411 ->
    // 2.399 ms, f64 x 8 groups 1.179 -> 1.237 ms SLOWER -- so it is on for the 16-group forms only.  Results are identical either
    // way.  (256-column form, round 1: hints on the once-read arrays cost 11 %: no second read there.)
    static constexpr int stream_aux = narrow == 2 ? 2 : 0;
    // pairs per block of the linearity phase (their recurrences interleave): 2 at 128 and 168 registers; by same-box A/B at the
    // 16-group forms (profiles/r04_ab_runs.txt): at 168 registers 1 (1.697 against 1.710 ms; 4 spills: 3.46), f64 ipc4d at 256
    // registers 4 (2.24 against 2.27)
    // -- the largest such factor that divides the pair count (f64 ipc4d: 10 and 14 groups 1, 12 groups 3, 16 groups 4)
    static constexpr int pb = c2_block(G / 2, narrow == 2 ? (K64 ? 4 : 1) : 2);
    // f64 ipc4d: pairs the first iterate evaluates in lockstep -- two at 256 registers (f64 x 16 groups: 2.23 / 2.25 ms for 2 / 1),
    // one at 168
    static constexpr int pbc = c2_block(G / 2, wps == 2 ? 2 : 1);
    // f64 ipc4d: groups the second iterate evaluates in lockstep (16 groups: 256 registers, four)
    static constexpr int nbo = c2_block(G, G > 8 ? 4 : 2);
    // every blocked loop of the kernel steps by one of these over a count they divide: no block runs past its arrays or rings
    static_assert((G / 2) % pb == 0 && (G / 2) % pbc == 0 && G % nbo == 0, "block factors divide their counts");
};

// Launch geometry on `slots` co-resident workgroups, `reserve` of them left free where that costs nothing (the pre-pass of the NEXT
// ramp runs in them beside this kernel): every strip gets the same number of row ranges -- except a last strip of at most 64 live
// columns (nx = 4096 in the 256-column form: 16 strips of 252 + 64), which is covered in QUAD mode: nq workgroups whose wc wave
// columns take a row range each.  4096 x 4096: 16 x 31 ranges of 133 rows + 8 quad workgroups (32 ranges of 128 rows) = 504 workgroups
// of 139 steps; before (17 x 30 ranges of 137 rows): 510 of 143.  Returns the grid size.
static inline long chain2_geometry(ChainArgs &a, int nstrips, int live_last, int slots, int reserve, int wc = 4, bool quad_ok = true) {
    const int maxr = (a.ny + 7) / 8;   // at least 8 rows per range
    auto cdiv = [](int x, int y) { return (x + y - 1) / y; };
    int best_nr = 0, best_nq = 0, best_steps = 1 << 30;
    if (quad_ok && nstrips > 1 && live_last <= 64) {
        const int nfull = nstrips - 1;
        for (int pass = 0; pass < 2 && !best_nr; ++pass) {   // (second pass: without the reserve, when it leaves no room)
            const int avail = slots - (pass ? 0 : reserve);
            for (int nq = 1; wc * nq <= maxr && nq < avail; ++nq) {
                int nr = (avail - nq) / nfull;
                if (nr > maxr) nr = maxr;
                if (nr < 1) break;
                const int steps = cdiv(a.ny, nr) > cdiv(a.ny, wc * nq) ? cdiv(a.ny, nr) : cdiv(a.ny, wc * nq);
                if (steps < best_steps) best_steps = steps, best_nr = nr, best_nq = nq;
            }
        }
    }
    int nr_u = (slots - reserve) / nstrips;   // every strip alike
    if (nr_u < 1) nr_u = slots / nstrips;
    if (nr_u > maxr) nr_u = maxr;
    if (nr_u < 1) nr_u = 1;
    if (best_nr && best_steps < cdiv(a.ny, nr_u)) {
        a.geo_nr = best_nr, a.geo_rows = cdiv(a.ny, best_nr), a.geo_nq = best_nq, a.geo_rows_q = cdiv(a.ny, wc * best_nq);
        return (long)best_nr * (nstrips - 1) + best_nq;
    }
    a.geo_nr = nr_u, a.geo_rows = cdiv(a.ny, nr_u), a.geo_nq = 0, a.geo_rows_q = 0;
    return (long)nr_u * nstrips;
}

// The launch geometry of form F for the frame in a (ny, nx) on a device of ncu CUs: the workgroup slots of the form (per CU as many
// as the LDS holds, at most as many as its waves per SIMD allow), the reserve (narrow forms fill their CUs: none), the strip
// count and the live columns of the last strip.  THE one place that computes it: the launcher (chain2_kernel.h) and the query
// rip_chain_geometry_for (chain.hip) both call it.  Sets a.geo_*, returns the grid size; geo (may be null) receives window
// columns, strip count, live columns of the last strip, geo_nr, geo_rows, geo_nq, geo_rows_q, grid size.
template <typename F>
static inline long c2_form_geometry(ChainArgs &a, int ncu, int reserve, bool quad_ok, int *geo) {
    int per_cu = (160 * 1024) / F::lds_bytes;
    if (per_cu < 1) per_cu = 1;
    const int max_wg = 4 * F::wps / (F::threads / 64);
    if (per_cu > max_wg) per_cu = max_wg;
    const int nstrips = F::nstrips(a.nx), live_last = a.nx - (nstrips - 1) * F::outw;
    const long grid = chain2_geometry(a, nstrips, live_last, ncu * per_cu, F::narrow ? 0 : reserve, F::cols / 64, quad_ok);
    if (geo) {
        geo[0] = F::cols, geo[1] = nstrips, geo[2] = live_last, geo[3] = a.geo_nr, geo[4] = a.geo_rows, geo[5] = a.geo_nq,
        geo[6] = a.geo_rows_q, geo[7] = (int)grid;
    }
    return grid;
}
