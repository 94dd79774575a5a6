// The exact k-th-largest select over stored logits that p2t_sample_select (sample_select.hip) and p2t_beam_select (beam_select.hip)
// share: an order-preserving integer key, the column walk of a 1024-thread block, an 8-bit-per-pass radix select on per-wave
// integer histograms, and the fixed-order wave helpers.  Block-wide functions expect blockDim.x == 1024.
#pragma once
#include "common.h"

namespace p2t {

constexpr int kCap = 2048;                  // survivor table
constexpr int kNoIndex = 0x7fffffff;

// order-preserving key of a stored logit: a < b as numbers => key(a) < key(b) (-0 below +0: equal as numbers, harmless, the survivor
// test is on the float).  A bf16 value's key is decided by its upper 16 bits (the lower 16 are all 0 or all 1 with the sign).
template <typename T> struct KeyBits { static constexpr int N = sizeof(T) == 2 ? 16 : 32; };
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// f(value, column) for the columns of this thread: 16-byte pieces where `vec` says the row allows them, then the tail one by one
template <typename T, typename F>
__device__ __forceinline__ void for_each_column(const T* __restrict__ row, int V, bool vec, int tid, F f) {
    constexpr int PN = sizeof(T) == 2 ? 8 : 4;
    const int Vv = vec ? V / PN * PN : 0;
    for (int c = tid * PN; c < Vv; c += 1024 * PN) {
        float v[PN];
        if constexpr (PN == 8) load8(row + c, v);
        else load4(row + c, v);
#pragma unroll
        for (int e = 0; e < PN; ++e) f(v[e], c + e);
    }
    for (int c = Vv + tid; c < V; c += 1024) f(to_f32(row[c]), c);
}

// The k-th largest of the keys `each` hands to its callback (every thread its own share; at least k keys in all), by their upper
// BITS bits, 8 per pass from the top: per-wave integer histograms, a suffix count over the 256 digits by wave 0.  Block-wide call
// (barriers inside); hist and s_sel are free again on return.
template <int BITS, typename Each>
__device__ __forceinline__ uint32_t radix_select(int k, int (*hist)[256], int* s_sel, Each each) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t prefix = 0;
    int k_rem = k;
    for (int shift = 24; shift >= 32 - BITS; shift -= 8) {
        for (int i = tid; i < 16 * 256; i += 1024) (&hist[0][0])[i] = 0;
        if (tid == 0) { s_sel[0] = 0; s_sel[1] = 1; }
        __syncthreads();
        const uint32_t above = shift == 24 ? 0u : (0xffffffffu << (shift + 8));          // the digits already fixed
        each([&](uint32_t key) {
            if ((key & above) == prefix) atomicAdd(&hist[w][(key >> shift) & 255u], 1);
        });
        __syncthreads();
        if (tid < 256) {
            int t = 0;
#pragma unroll
            for (int ww = 0; ww < 16; ++ww) t += hist[ww][tid];
            hist[0][tid] = t;                                 // column tid of the table is this thread's alone
        }
        __syncthreads();
        if (w == 0) {                                         // lane l: digits 255 - 4 l .. 252 - 4 l; counts from the top down
            int cnt[4], tot = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) { cnt[i] = hist[0][255 - (4 * lane + i)]; tot += cnt[i]; }
            int incl = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            int run = incl - tot;                             // keys in digits above this lane's
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (run < k_rem && k_rem <= run + cnt[i]) { s_sel[0] = 255 - (4 * lane + i); s_sel[1] = k_rem - run; }
                run += cnt[i];
            }
        }
        __syncthreads();
        prefix |= (uint32_t)(s_sel[0] & 255) << shift;
        k_rem = s_sel[1];
        __syncthreads();
    }
    if (BITS == 16 && !(prefix & 0x80000000u)) prefix |= 0xffffu;       // a negative bf16 value: the lower key bits are ones
    return prefix;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
// inclusive scan over the 64 lanes in a fixed order
__device__ __forceinline__ float wave_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

}  // namespace p2t
