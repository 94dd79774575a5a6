// Token selection by sampling (p2t_sample_select, p2t_sample_select_rows): HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper
// (transformers/generation/logits_process.py) and the multinomial draw of GenerationMixin._sample, one 1024-thread block per
// row, with greedy_select_kernel's step bookkeeping (llama_decode.hip).  The contract, every tie-break included, is the comment
// on p2t_sample_select in include/p2t_hip.h; tests/sampling_reference.py restates it in fp64.  Both kernels are one body over a row
// model (row_model.h): LockStepRows for p2t_sample_select, OwnRows -- greedy_select_rows_kernel's bookkeeping, every row on its own
// counter, a finished row left before its logits are read -- for p2t_sample_select_rows (tests/continuous_choice_reference.py).
//
// The draw of a row with key `key` at counter `step` (lock-step: key = row0 + r, step = step[0]; own rows: row_key[r], row_step[r]):
//     h = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ (uint64)key) ^ (uint64)(int64)step)                 (mix64: common.h)
//     hash24 = h >> 40,   u = (hash24 + 0.5) * 2^-24,   used as the nearest f32 (= float(2 hash24 + 1) * 2^-25)
// p2t_hip/synth.py sample_uniform(seed, key, step) is the same chain on the host.
//
// Filtered form (top_k on), sample_topk_kernel: the table pipeline of select_common.h, with x = stored logit / temperature as the
// value a column stores and its score written as it is seen; the draw is this file's own.
//   1. kth = the k-th largest STORED logit (thread_max_key, kth_largest_stored: a radix select over an order-preserving integer key,
//      8 bits per pass, first over the 1024 per-thread maxima, then over the row above that bound).  x -> x / temperature is
//      monotone, so the k-th largest x is kth / temperature, also where the division makes two different logits equal.  The row is
//      read with 16-byte loads where its pitch and base allow.
//   2. every column with x >= that is a survivor (collect_survivors): an LDS table of kCap (value, index) pairs.  More than kCap
//      survivors (>= 1025 exact ties): the ordered path (collect_in_order), bit 0 of the flags word, -inf as the score of a tie
//      that found no slot.
//   3. the table is sorted by (value descending, index ascending) (pad_and_sort_table): a total order, so the slot order is gone.
//   4. wave 0: e_j = exp(x_j - x_0), the fixed-order scan and the top-p cut on the tail mass (top_p_cut), then here the inverse CDF
//      at u over the kept ranks, on the se[] and the lane prefix the cut left.
// Unfiltered form (top_k off, top_p off), sample_full_kernel: the row maximum, then every wave scans one contiguous segment of
// columns in ascending order (64 columns per step, shuffle scan), the 16 segment sums are added in wave order, and the wave whose
// segment holds u * S walks it again with the same arithmetic to find the column.
// No float atomics; every float reduction has a fixed order: the same inputs give the same bits.  Every LDS index is bounded by
// kCap / 256 / 16 whatever the counts say, the written column is clamped, and the token is clamped to [0, V).
#include "row_model.h"
#include "select_common.h"

namespace p2t {
namespace {

__device__ __forceinline__ float draw_uniform(uint64_t seed, int64_t row, int step) {
    uint64_t h = mix64(seed + 0x9E3779B97F4A7C15ull);
    h = mix64(h ^ (uint64_t)row);
    h = mix64(h ^ (uint64_t)(int64_t)step);
    return (float)(int)(2u * (uint32_t)(h >> 40) + 1u) * 0x1p-25f;
}

template <typename T, typename Rows>
__global__ void __launch_bounds__(1024) sample_topk_kernel(const T* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ eos,
                                                           int n_eos, int64_t pad, int32_t* __restrict__ finished, int64_t* __restrict__ next,
                                                           int64_t* __restrict__ out_tokens, int64_t ld_tok, Rows rows,
                                                           int Gcap, float temperature, int top_k, float top_p, uint64_t seed,
                                                           float* __restrict__ scores, int64_t ld_scores, int32_t* __restrict__ flags) {
    __shared__ int hist[16][256];
    __shared__ float sv[kCap];            // survivors: x
    __shared__ int si[kCap];              //            column
    __shared__ float se[kCap];            //            exp(x - max)
    __shared__ int s_sel[2], s_cnt, s_wc[16], s_kept, s_tok;
    const int bb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = rows.engine_row(bb);
    if (!rows.enter(r, finished, next, pad, tid)) return;     // block-uniform; LockStepRows: never
    const T* row = logits + (int64_t)bb * ld;
    float* srow = scores ? scores + (int64_t)bb * ld_scores : nullptr;
    const int k = min(top_k, V);

    // ---- 1. the k-th largest stored logit ------------------------------------------------------------------------------
    const bool vec = ld % (16 / sizeof(T)) == 0 && ((uintptr_t)logits & 15u) == 0;
    const uint32_t kth_key = kth_largest_stored(row, V, vec, k, thread_max_key(row, V, vec, tid), hist, s_sel);
    const float xk = key_value(kth_key) / temperature;

    // ---- 2. survivors: x and its score; a tie the full table drops scores -inf ---------------------------------------------------
    auto x_of = [&](float v, int) { return v / temperature; };
    int n = collect_survivors(row, V, vec, xk, sv, si, &s_cnt, x_of, [&](int c, float x, bool keep) {
        if (srow) srow[c] = keep ? x : -INFINITY;
    });
    if (n > kCap) {                                           // block-uniform: >= 1025 exact ties at the k-th value
        if (tid == 0) atomicOr(flags, 1);
        n = collect_in_order(row, V, xk, sv, si, &s_cnt, s_wc, x_of, [&](int c) {
            if (srow) srow[c] = -INFINITY;
        });
    }
    if (n < 1) {                                              // only a row outside the contract (NaN) has no survivor
        if (tid == 0) { sv[0] = -INFINITY; si[0] = 0; }
        n = 1;
    }
    // ---- 3. total order: value descending, column ascending ----------------------------------------------------------------
    const int P = pad_and_sort_table(sv, si, n, tid);
    // ---- 4. top-p and the draw, one wave ---------------------------------------------------------------------------------
    const int step = rows.counter(r);
    if (w == 0) {
        const int per = P >> 6, j0 = lane * per;              // lane l: ranks l * per .. l * per + per - 1
        const float mx = sv[0];
        float excl;
        const int m = top_p_cut(n, P, top_p, se, lane, excl, [&](int j) { return expf(sv[j] - mx); });
        float run = excl, at_last = 0.f;
        for (int i = 0; i < per; ++i) {
            const int j = j0 + i;
            if (j < m) {
                run += se[j];
                if (j == m - 1) at_last = run;
            }
        }
        const float target = draw_uniform(seed, rows.key(r), step) * __shfl(at_last, (m - 1) / per, 64);
        int cand = kNoIndex;
        run = excl;
        for (int i = 0; i < per; ++i) {
            const int j = j0 + i;
            if (j < m) {
                run += se[j];
                if (run > target && cand == kNoIndex) cand = j;
            }
        }
        cand = wave_min_int(cand);
        if (cand >= m) cand = m - 1;                          // rounding left none: the last kept rank
        if (lane == 0) { s_kept = m; s_tok = si[cand & (kCap - 1)]; }
    }
    __syncthreads();
    if (srow) {
        const int m = s_kept;
        for (int j = m + tid; j < n; j += 1024) {
            const int c = si[j];
            if (c >= 0 && c < V) srow[c] = -INFINITY;
        }
    }
    if (tid == 0) rows.emit(r, s_tok, V, eos, n_eos, pad, finished, next, out_tokens, ld_tok, step, Gcap);
}

template <typename T, typename Rows>
__global__ void __launch_bounds__(1024) sample_full_kernel(const T* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ eos,
                                                           int n_eos, int64_t pad, int32_t* __restrict__ finished, int64_t* __restrict__ next,
                                                           int64_t* __restrict__ out_tokens, int64_t ld_tok, Rows rows,
                                                           int Gcap, float temperature, uint64_t seed, float* __restrict__ scores,
                                                           int64_t ld_scores) {
    __shared__ float s_max[16], s_sum[16];
    __shared__ int s_tok;
    const int bb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = rows.engine_row(bb);
    if (!rows.enter(r, finished, next, pad, tid)) return;     // block-uniform; LockStepRows: never
    const T* row = logits + (int64_t)bb * ld;
    float* srow = scores ? scores + (int64_t)bb * ld_scores : nullptr;
    float mx = -INFINITY;
    for (int c = tid; c < V; c += 1024) mx = fmaxf(mx, to_f32(row[c]) / temperature);
    mx = wave_max(mx);
    if (lane == 0) s_max[w] = mx;
    if (tid == 0) s_tok = V - 1;                              // rounding left none: the last column
    __syncthreads();
    mx = s_max[0];
#pragma unroll
    for (int ww = 1; ww < 16; ++ww) mx = fmaxf(mx, s_max[ww]);
    // wave w: columns [lo, hi), 64 per step in ascending order; cumulative mass of a column = base_w + (run + scan)
    const int seg = ((V + 15) / 16 + 63) / 64 * 64, lo = min(w * seg, V), hi = min(lo + seg, V);
    float run = 0.f;
    for (int c0 = lo; c0 < hi; c0 += 64) {
        const int c = c0 + lane;
        float e = 0.f;
        if (c < hi) {
            const float x = to_f32(row[c]) / temperature;
            e = expf(x - mx);
            if (srow) srow[c] = x;
        }
        run = run + __shfl(wave_scan(e, lane), 63, 64);
    }
    if (lane == 0) s_sum[w] = run;
    __syncthreads();
    float base = 0.f, S = 0.f;
#pragma unroll
    for (int ww = 0; ww < 16; ++ww) {
        if (ww == w) base = S;
        S += s_sum[ww];
    }
    const int step = rows.counter(r);
    const float target = draw_uniform(seed, rows.key(r), step) * S;
    // the wave whose segment holds the target: the cumulative mass before it does not pass the target, that of its last column does
    // (the running sums never decrease, so at most one wave; each wave judges for itself, on its own two numbers.  A block-uniform
    // "first ww with b + s_sum[ww] > target" loop over the 16 sums was miscompiled by hipcc: the v_cmp of its first round was followed
    // by an s_cselect on a stale SCC, and a target inside wave 0's segment was given to wave 2)
    if (!(base > target) && base + s_sum[w] > target) {       // wave-uniform
        run = 0.f;
        for (int c0 = lo; c0 < hi; c0 += 64) {
            const int c = c0 + lane;
            const float e = c < hi ? expf(to_f32(row[c]) / temperature - mx) : 0.f;
            const float sc = wave_scan(e, lane);
            const unsigned long long over = __ballot(c < hi && base + (run + sc) > target);
            if (over) {
                if (lane == 0) s_tok = c0 + (__ffsll((long long)over) - 1);
                break;
            }
            run = run + __shfl(sc, 63, 64);
        }
    }
    __syncthreads();
    if (tid == 0) rows.emit(r, s_tok, V, eos, n_eos, pad, finished, next, out_tokens, ld_tok, step, Gcap);
}

}  // namespace
}  // namespace p2t

using namespace p2t;

// the checks both entry points share (P2T_ERR_ARG, then P2T_ERR_UNSUPPORTED, before any GPU call)
static int sampler_args_check(const char* name, int V, const int64_t* eos_ids, int n_eos, int64_t ld_tokens, int G, float temperature, int top_k, float top_p,
                              const float* scores, int64_t ld_scores) {
    P2T_REQUIRE(G > 0 && ld_tokens >= G && n_eos >= 0 && (n_eos == 0 || eos_ids),
                "%s: G = %d, ld_tokens = %lld, n_eos = %d: needs G > 0, ld_tokens >= G, eos_ids for n_eos > 0", name, G, (long long)ld_tokens, n_eos);
    P2T_REQUIRE(temperature > 0.f && temperature < INFINITY, "%s: temperature %g is not a positive finite number", name, (double)temperature);
    P2T_REQUIRE(top_k >= 0 && top_k <= 1024, "%s: top_k = %d: 0 (off) or 1 .. 1024", name, top_k);
    P2T_REQUIRE(top_p > 0.f, "%s: top_p = %g: in (0, 1), or >= 1 for off", name, (double)top_p);
    P2T_REQUIRE(!scores || ld_scores >= V, "%s: ld_scores = %lld < V = %d", name, (long long)ld_scores, V);
    if (top_k == 0 && top_p < 1.f) {
        set_error("%s: top_p = %g without top_k needs a sort of the whole vocabulary: supported are top_k 1 .. 1024 (top_p on or off) "
                  "and both filters off", name, (double)top_p);
        return P2T_ERR_UNSUPPORTED;
    }
    return P2T_OK;
}

// one block per logits row: the filtered or the unfiltered kernel over the row model
template <typename Rows>
static void launch_sample(const void* logits, int dtype, int64_t ld, int V, int n, const int64_t* eos_ids, int n_eos, int64_t pad_id, int32_t* finished,
                          int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, Rows rows, int G, float temperature, int top_k, float top_p,
                          uint64_t seed, float* scores, int64_t ld_scores, int32_t* flags, hipStream_t s) {
#define P2T_SAMPLE_LAUNCH(T)                                                                                                                  \
    do {                                                                                                                                      \
        if (top_k > 0)                                                                                                                        \
            sample_topk_kernel<T, Rows><<<n, 1024, 0, s>>>((const T*)logits, ld, V, eos_ids, n_eos, pad_id, finished, next_tokens, out_tokens, \
                                                           ld_tokens, rows, G, temperature, top_k, top_p, seed, scores, ld_scores, flags);    \
        else                                                                                                                                  \
            sample_full_kernel<T, Rows><<<n, 1024, 0, s>>>((const T*)logits, ld, V, eos_ids, n_eos, pad_id, finished, next_tokens, out_tokens, \
                                                           ld_tokens, rows, G, temperature, seed, scores, ld_scores);                         \
    } while (0)
    if (dtype == P2T_BF16) P2T_SAMPLE_LAUNCH(bf16_t);
    else P2T_SAMPLE_LAUNCH(float);
#undef P2T_SAMPLE_LAUNCH
}

extern "C" int p2t_sample_select(const void* logits, int dtype, int64_t ld, int V, int BB, const int64_t* eos_ids, int n_eos, int64_t pad_id,
                                 int32_t* finished, int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, const int32_t* step, int G,
                                 float temperature, int top_k, float top_p, uint64_t seed, int64_t row0, float* scores, int64_t ld_scores,
                                 int32_t* flags, p2t_stream stream) {
    P2T_REQUIRE(logits && finished && next_tokens && out_tokens && step && flags, "p2t_sample_select: null argument");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_sample_select: dtype %d is neither P2T_F32 nor P2T_BF16", dtype);
    P2T_REQUIRE(BB > 0 && V > 0 && ld >= V, "p2t_sample_select: BB = %d, V = %d, ld = %lld: needs BB > 0, V > 0, ld >= V", BB, V, (long long)ld);
    P2T_TRY(sampler_args_check("p2t_sample_select", V, eos_ids, n_eos, ld_tokens, G, temperature, top_k, top_p, scores, ld_scores));
    launch_sample(logits, dtype, ld, V, BB, eos_ids, n_eos, pad_id, finished, next_tokens, out_tokens, ld_tokens, LockStepRows{step, row0}, G, temperature,
                  top_k, top_p, seed, scores, ld_scores, flags, (hipStream_t)stream);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_sample_select_rows(const void* logits, int dtype, int64_t ld, int V, int n, const int64_t* eos_ids, int n_eos, int64_t pad_id,
                                      int32_t* finished, int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, const int32_t* row_step,
                                      const int32_t* row_limit, const int32_t* row_map, const int64_t* row_key, int BB, int G, float temperature,
                                      int top_k, float top_p, uint64_t seed, float* scores, int64_t ld_scores, int32_t* flags, p2t_stream stream) {
    P2T_REQUIRE(logits && finished && next_tokens && out_tokens && row_step && row_limit && row_key && flags, "p2t_sample_select_rows: null argument");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_sample_select_rows: dtype %d is neither P2T_F32 nor P2T_BF16", dtype);
    P2T_REQUIRE(n > 0 && BB > 0 && n <= BB && (row_map || n == BB),
                "p2t_sample_select_rows: %d logits rows for %d engine rows (all of them, or a row_map subset)", n, BB);
    P2T_REQUIRE(V > 0 && ld >= V, "p2t_sample_select_rows: V = %d, ld = %lld: needs V > 0, ld >= V", V, (long long)ld);
    P2T_TRY(sampler_args_check("p2t_sample_select_rows", V, eos_ids, n_eos, ld_tokens, G, temperature, top_k, top_p, scores, ld_scores));
    launch_sample(logits, dtype, ld, V, n, eos_ids, n_eos, pad_id, finished, next_tokens, out_tokens, ld_tokens,
                  OwnRows{row_step, row_limit, row_map, row_key, BB}, G, temperature, top_k, top_p, seed, scores, ld_scores, flags, (hipStream_t)stream);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
