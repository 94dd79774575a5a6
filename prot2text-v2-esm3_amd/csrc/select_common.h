// The survivor-table pipeline that p2t_sample_select (sample_select.hip), p2t_beam_select (beam_select.hip) and p2t_beam_sample_select
// (beam_sample_select.hip) share, every step once: an order-preserving integer key, the column walk of a 1024-thread block, an
// 8-bit-per-pass radix select on per-wave integer histograms and the two-select k-th largest built on it, the survivor collection
// (slot counter, ordered fallback), the bitonic total order of the table, wave 0's fixed-order scan with the top-p cut, the row's lse,
// and the fixed-order wave helpers.  Block-wide functions expect blockDim.x == 1024.  The callers differ in functors only: what
// value a column stores, what happens to its score, and what e_j a rank has.
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

// ---- the table pipeline ---------------------------------------------------------------------------------------------------
struct NoColumnHook {
    template <typename... A> __device__ __forceinline__ void operator()(A...) const {}
};

// this thread's largest key of a row of stored logits; 0 (below every key of a number) for a thread without a column
template <typename T>
__device__ __forceinline__ uint32_t thread_max_key(const T* row, int V, bool vec, int tid) {
    uint32_t tmax = 0;
    for_each_column(row, V, vec, tid, [&](float v, int) { tmax = max(tmax, key_of(v)); });
    return tmax;
}

// The k-th largest (k <= 1024) of the keys key_at(value, column) of a row, in two selects: first over the 1024 per-thread maxima `tmax`
// (no row pass, no contention), whose k-th largest is a lower bound of the answer (at least k of the row's keys are that large); then
// over the row, counting only the keys at or above the bound -- some 60 of 128 256 at k = 50, a few thousand at k = 1024 -- so the
// histograms' same-address atomics stay few.  key_at may be recomputed per pass.
template <int BITS, typename T, typename KeyAt>
__device__ __forceinline__ uint32_t kth_largest_key(const T* row, int V, bool vec, int k, uint32_t tmax, int (*hist)[256],
                                                    int* s_sel, KeyAt key_at) {
    const int tid = threadIdx.x;
    const uint32_t floor_key = radix_select<BITS>(k, hist, s_sel, [&](auto count) { count(tmax); });
    return radix_select<BITS>(k, hist, s_sel, [&](auto count) {
        for_each_column(row, V, vec, tid, [&](float v, int c) {
            const uint32_t key = key_at(v, c);
            if (key >= floor_key) count(key);
        });
    });
}
// ... of the stored logits themselves
template <typename T>
__device__ __forceinline__ uint32_t kth_largest_stored(const T* row, int V, bool vec, int k, uint32_t tmax, int (*hist)[256],
                                                       int* s_sel) {
    return kth_largest_key<KeyBits<T>::N>(row, V, vec, k, tmax, hist, s_sel, [](float v, int) { return key_of(v); });
}

// Every column with x = value(stored logit, column) >= thr is a survivor: (x, column) goes into the table (val, idx) of kCap entries
// through an integer slot counter (any order; the sort undoes it), and seen(column, x, survivor) runs for every column.  Block-wide;
// -> the number of survivors (block-uniform).  More than kCap: the table is full and short of some, the caller goes on to
// collect_in_order (and decides about its flag).
template <typename T, typename Value, typename Seen = NoColumnHook>
__device__ __forceinline__ int collect_survivors(const T* row, int V, bool vec, float thr, float* val, int* idx, int* s_cnt, Value value,
                                                 Seen seen = {}) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    for_each_column(row, V, vec, tid, [&](float v, int c) {
        const float x = value(v, c);
        const bool keep = x >= thr;
        if (keep) {
            const int slot = atomicAdd(s_cnt, 1);
            if (slot < kCap) { val[slot] = x; idx[slot] = c; }
        }
        seen(c, x, keep);
    });
    __syncthreads();
    return *s_cnt;
}

// More than kCap values at or above thr: the table takes all above it (fewer than kCap), then the ties at thr in ascending column
// order by a ballot + per-wave-count scan until it is full; dropped(column) for a tie that found no slot.  Block-wide; -> the number
// of entries.
template <typename T, typename Value, typename Dropped = NoColumnHook>
__device__ __forceinline__ int collect_in_order(const T* row, int V, float thr, float* val, int* idx, int* s_cnt, int* s_wc,
                                                Value value, Dropped dropped = {}) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __syncthreads();
    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    for (int c = tid; c < V; c += 1024) {
        const float x = value(to_f32(row[c]), c);
        if (x > thr) {
            const int slot = atomicAdd(s_cnt, 1);
            if (slot < kCap) { val[slot] = x; idx[slot] = c; }
        }
    }
    __syncthreads();
    int base = min(*s_cnt, kCap);
    for (int c0 = 0; c0 < V; c0 += 1024) {
        const int c = c0 + tid;
        const bool eq = c < V && value(to_f32(row[c]), c) == thr;
        const unsigned long long b = __ballot(eq);
        if (lane == 0) s_wc[w] = __popcll(b);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int ww = 0; ww < 16; ++ww) {
            const int t = s_wc[ww];
            if (ww < w) off += t;
            tot += t;
        }
        if (eq) {
            const int slot = off + __popcll(b & ((1ull << lane) - 1ull));
            if (slot < kCap) { val[slot] = thr; idx[slot] = c; }
            else dropped(c);
        }
        base = min(base + tot, 2 * kCap);                     // saturated: only "full or not" matters from kCap on
        __syncthreads();
    }
    return min(base, kCap);
}

// bitonic sort of (val, idx)[0 .. P) by (value descending, index ascending): a total order; P a power of two in [64, kCap]; block-wide
__device__ __forceinline__ void sort_table(float* val, int* idx, int P, int tid) {
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < (P >> 1)) {
                const int i = ((tid / stride) * 2 * stride + (tid % stride)) & (kCap - 1), j = (i + stride) & (kCap - 1);
                const float va = val[i], vb = val[j];
                const int ia = idx[i], ib = idx[j];
                const bool b_first = vb > va || (vb == va && ib < ia);
                const bool a_first = va > vb || (va == vb && ia < ib);
                if (((i & size) == 0) ? b_first : a_first) { val[i] = vb; val[j] = va; idx[i] = ib; idx[j] = ia; }
            }
            __syncthreads();
        }
    }
}
// the n <= kCap entries padded with (-inf, kNoIndex) to a power of two P >= 64, then sorted; -> P
__device__ __forceinline__ int pad_and_sort_table(float* val, int* idx, int n, int tid) {
    int P = 64;
    while (P < n) P <<= 1;                                    // <= kCap
    for (int i = n + tid; i < P; i += 1024) { val[i] = -INFINITY; idx[i] = kNoIndex; }
    __syncthreads();
    sort_table(val, idx, P, tid);
    return P;
}

// Wave 0 alone, over the sorted ranks: se[j] = e_j = e_of(j) for j < n (0 up to P), a fixed-order scan of them (lane l adds its P / 64
// consecutive ranks l * per .., then a shuffle scan of the lane totals) and the top-p cut on the tail mass: rank j stays iff
// sum_{i >= j} e_i > (1 - top_p) * sum; rank 0 always.  -> the number of kept ranks; excl = the sum of the lanes before this one.
template <typename EOf>
__device__ __forceinline__ int top_p_cut(int n, int P, float top_p, float* se, int lane, float& excl, EOf e_of) {
    const int per = P >> 6, j0 = lane * per;
    float loc = 0.f;
    for (int i = 0; i < per; ++i) {
        const int j = j0 + i;
        const float e = j < n ? e_of(j) : 0.f;
        se[j] = e;
        loc += e;
    }
    const float incl = wave_scan(loc, lane);
    const float S = __shfl(incl, 63, 64);
    excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    if (!(top_p < 1.f)) return n;
    const float cut = (1.f - top_p) * S;
    float run = excl;
    int cnt = 0;
    for (int i = 0; i < per; ++i) {
        const int j = j0 + i;
        if (j < n) {
            cnt += (j == 0 || S - run > cut) ? 1 : 0;
            run += se[j];
        }
    }
    return min(max(wave_sum_int(cnt), 1), n);
}

// lse = logf(sum expf(v - mx)) over a row: every thread adds its columns in for_each_column's order, the lanes by a butterfly, the
// waves in wave order.  Block-wide; s_sum holds 16 floats.
template <typename T>
__device__ __forceinline__ float row_lse(const T* row, int V, bool vec, float mx, float* s_sum) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float part = 0.f;
    for_each_column(row, V, vec, tid, [&](float v, int) { part += expf(v - mx); });
    part = wave_sum(part);
    if (lane == 0) s_sum[w] = part;
    __syncthreads();
    float S = 0.f;
#pragma unroll
    for (int ww = 0; ww < 16; ++ww) S += s_sum[ww];
    return logf(S);
}

}  // namespace p2t
