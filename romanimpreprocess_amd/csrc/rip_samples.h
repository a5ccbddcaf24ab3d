// Raw 16-bit detector samples as every entry that reads a cube of them gets them (darkstack.hip, linfit.hip, noisestat.hip,
// corrstat.hip, rawframes.hip): the storage rule, the 8-sample load and the 16-byte access to the results.  Device code only;
// the host half (the band upload, the W8 dispatch) is in rip_host.h.  All of it moves integer bits: no order of swap and split
// changes a word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// `stored`, as rip_cal_raw_frame takes it (an entry's fits_be16 is stored = 1):
//   0  native uint16
//   1  FITS storage: big-endian int16 with BZERO = 32768 -- the unsigned sample is the swapped word with its top bit flipped
//   2  FITS int16 without BZERO: the bytes swapped only (an int16 whose bits numpy's cast to uint16 keeps)
// One dword holding two samples as stored -> the two native samples, in place.
__device__ __forceinline__ uint32_t decode_pair(uint32_t w, int stored) {
    if (stored != 0) w = ((w & 0x00FF00FFu) << 8) | ((w >> 8) & 0x00FF00FFu);
    if (stored == 1) w ^= 0x80008000u;
    return w;
}
// one sample (raw <= 0xFFFF)
__device__ __forceinline__ uint32_t decode_sample(uint32_t raw, int stored) { return decode_pair(raw, stored) & 0xFFFFu; }

// x[0 .. V-1]: the V samples at p, decoded.  V = 8 is the W8 form of the kernels, one 16-byte load (p is 16-byte aligned: the
// host checks, and that every row and frame starts on a multiple of 8 samples); V = 1 the one-sample form.
template <int V>
__device__ __forceinline__ void load_samples(const uint16_t *__restrict__ p, int stored, uint32_t (&x)[V]) {
    static_assert(V == 8 || V == 1, "one 16-byte load or one sample");
    if constexpr (V == 8) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t d = decode_pair(w[k], stored);
            x[2 * k] = d & 0xFFFFu;
            x[2 * k + 1] = d >> 16;
        }
    } else {
        x[0] = decode_sample(*p, stored);
    }
}

// p[k] += v[k] (ADD) or p[k] = v[k] for the first n of V adjacent results (n >= V: all of them).  wide: p is 16-byte aligned --
// then a whole vector of 8 goes in 16-byte pieces; a row's tail (n < V), an unaligned row and V = 1 go element by element.
// The defaults of add_results / store_results (n = V, wide = true) are the caller's promise that all V results exist and that p
// is 16-byte aligned where V = 8: its host entry checks that before it chooses the W8 form (rip_cal_noise_add, _frame_slopes).
template <bool ADD, typename T, int V>
__device__ __forceinline__ void put_results(T *__restrict__ p, const T (&v)[V], int n, bool wide) {
    static_assert(V == 8 || V == 1, "the forms of load_samples");
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "results of 4 or 8 bytes: 2 or 4 pieces of 16 bytes for V = 8");
    constexpr int PER = 16 / sizeof(T);
    if constexpr (V == 8) {
        if (wide && n >= V) {
            typedef T vec __attribute__((ext_vector_type(PER)));
#pragma unroll
            for (int j = 0; j < V / PER; ++j) {
                vec u = {};
                if constexpr (ADD) u = reinterpret_cast<vec *>(p)[j];
#pragma unroll
                for (int e = 0; e < PER; ++e) u[e] = ADD ? u[e] + v[j * PER + e] : v[j * PER + e];
                reinterpret_cast<vec *>(p)[j] = u;
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (k < n) p[k] = ADD ? p[k] + v[k] : v[k];
}
template <typename T, int V>
__device__ __forceinline__ void add_results(T *__restrict__ p, const T (&v)[V], int n = V, bool wide = true) {
    put_results<true>(p, v, n, wide);
}
template <typename T, int V>
__device__ __forceinline__ void store_results(T *__restrict__ p, const T (&v)[V], int n = V, bool wide = true) {
    put_results<false>(p, v, n, wide);
}
