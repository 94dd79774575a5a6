// Beam sampling (p2t_beam_sample_select): one step of transformers' `_beam_search` with do_sample=True (beam-search multinomial
// sampling; 5.x, generation/utils.py `_get_top_k_continuations`) with an empty id prompt, as two launches that read every length on
// the device.  The contract, every tie-break included, is the comment on p2t_beam_sample_select in include/p2t_hip.h;
// tests/beam_sample_reference.py restates it in fp64.
//
// HF draws keep = max(2, 1 + n_eos) * nb continuations per prompt WITHOUT replacement from softmax(processed log-probabilities +
// running scores) over nb * V candidates.  Drawing without replacement is the descending order of acc + Gumbel noise (Plackett-Luce), so
// a select over perturbed keys does the whole draw; the noise of a candidate is a counter hash of (seed, prompt, step, beam * V + column).
//
// beam_sample_rows_kernel, one 1024-thread block per row (beam): the row maximum, lse in beam_rows_kernel's fixed order, then
//   top_k on:  sample_topk_kernel's two radix selects for the k-th largest stored logit, the survivor table, its bitonic sort by
//              (stored logit descending, column ascending), y = ((x - mx) - lse) / temperature and the top-p cut on the tail mass by wave 0;
//              then key = (y + running) + noise per kept entry and a second sort by (key descending, column ascending);
//   both off:  key for every column, the keep-th largest key by the same two selects over the keys (the noise is recomputed per pass:
//              a hash and two logf per column, next to a row read from L2), the keys at or above it collected and sorted.
//   The first `keep` (key, column) pairs of the sorted table go to the workspace with acc recomputed from the column (the same three
//   operations on the same numbers: the same bits), and the row's best acc.
// beam_sample_merge_kernel, one 256-thread block per prompt: beam_merge.h with the perturbed key as the rank key.
// No float atomics, fixed reduction orders: the same inputs give the same bits.  Every LDS index is bounded by kCap / 256 / 16 whatever
// the counts say, cur outside [0, max_length) counts as done, and columns are clamped to [0, V).
#include "beam_merge.h"
#include "select_common.h"

namespace p2t {
namespace {

// bitonic sort of (val, idx)[0 .. P) by (value descending, index ascending); P a power of two in [64, kCap]; block-wide
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

// More than kCap values at or above thr: the table takes all above it (fewer than kCap), then the ties at thr in ascending column
// order by a ballot + per-wave-count scan until it is full.  Block-wide; -> the number of entries.
template <typename At>
__device__ __forceinline__ int collect_in_order(int V, float thr, float* val, int* idx, int* s_cnt, int* s_wc, At at) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __syncthreads();
    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    for (int c = tid; c < V; c += 1024) {
        const float x = at(c);
        if (x > thr) {
            const int slot = atomicAdd(s_cnt, 1);
            if (slot < kCap) { val[slot] = x; idx[slot] = c; }
        }
    }
    __syncthreads();
    int base = min(*s_cnt, kCap);
    for (int c0 = 0; c0 < V; c0 += 1024) {
        const int c = c0 + tid;
        const bool eq = c < V && at(c) == thr;
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
        }
        base = min(base + tot, 2 * kCap);                     // saturated: only "full or not" matters from kCap on
        __syncthreads();
    }
    return min(base, kCap);
}

// the Gumbel noise of flat candidate index `flat` under the prompt-and-step hash h3
__device__ __forceinline__ float gumbel_noise(uint64_t h3, uint64_t flat) {
    const uint64_t h = mix64(h3 ^ flat);
    const float u = (float)(int)(2u * (uint32_t)(h >> 41) + 1u) * 0x1p-24f;           // an odd 24-bit integer * 2^-24: exact, inside (0, 1)
    return -logf(-logf(u));
}

template <typename T>
__global__ void __launch_bounds__(1024) beam_sample_rows_kernel(const T* __restrict__ logits, int64_t ld, int V, int nb, int keep, int max_length,
                                                                const int32_t* __restrict__ step_ptr, const int32_t* __restrict__ done,
                                                                const float* __restrict__ run_scores, int BB, float temperature, int top_k,
                                                                float top_p, uint64_t seed, int64_t prompt0, float* __restrict__ cand_key,
                                                                int32_t* __restrict__ cand_col, float* __restrict__ cand_acc,
                                                                float* __restrict__ row_best, float* __restrict__ scores, int64_t ld_scores,
                                                                int32_t* __restrict__ flags) {
    __shared__ int hist[16][256];
    __shared__ float sv[kCap];            // top_k on: the survivors' stored logits, then their y
    __shared__ int si[kCap];              // column
    __shared__ float se[kCap];            // top_k on: exp(y - y_0), then the perturbed keys; both off: the perturbed keys
    __shared__ int s_sel[2], s_cnt, s_wc[16], s_kept;
    __shared__ uint32_t s_wmax[16];
    __shared__ float s_sum[16];
    const int cur = step_ptr[0];
    if (done[0] != 0 || cur < 0 || cur >= max_length) return;              // block-uniform
    const int bb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const T* row = logits + (int64_t)bb * ld;
    float* srow = scores ? scores + (int64_t)bb * ld_scores : nullptr;
    const float run = run_scores[(int64_t)(cur & 1) * BB + bb];
    const int beam = bb % nb;
    uint64_t h3 = mix64(seed + 0x9E3779B97F4A7C15ull);
    h3 = mix64(h3 ^ (uint64_t)(prompt0 + bb / nb));
    h3 = mix64(h3 ^ (uint64_t)(int64_t)cur);
    const uint64_t flat0 = (uint64_t)beam * (uint64_t)V;
    const bool vec = ld % (16 / sizeof(T)) == 0 && ((uintptr_t)logits & 15u) == 0;

    // ---- 1. mx, lse: beam_rows_kernel's arithmetic (the maximum through the order-preserving key) ---------------------------------
    uint32_t tmax = 0;                                        // below every key of a number (a thread without a column keeps it)
    for_each_column(row, V, vec, tid, [&](float v, int) { tmax = max(tmax, key_of(v)); });
    uint32_t bmax = tmax;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bmax = max(bmax, (uint32_t)__shfl_xor((int)bmax, o, 64));
    if (lane == 0) s_wmax[w] = bmax;
    __syncthreads();
    bmax = s_wmax[0];
#pragma unroll
    for (int ww = 1; ww < 16; ++ww) bmax = max(bmax, s_wmax[ww]);
    const float mx = key_value(bmax);
    float part = 0.f;
    for_each_column(row, V, vec, tid, [&](float v, int) { part += expf(v - mx); });
    part = wave_sum(part);
    if (lane == 0) s_sum[w] = part;
    __syncthreads();
    float S = 0.f;
#pragma unroll
    for (int ww = 0; ww < 16; ++ww) S += s_sum[ww];
    const float lse = logf(S);
    const float y0 = (0.f - lse) / temperature;               // y of the row's largest logit
    auto y_of = [&](float v) { return ((v - mx) - lse) / temperature; };

    int n, m;                                                 // table entries, valid (kept) entries
    if (top_k > 0) {                                          // block-uniform
        // ---- 2a. the k-th largest stored logit and its survivors (sample_topk_kernel's steps 1-3 on the stored logits) --------------
        const int k = min(top_k, V);
        const uint32_t floor_key = radix_select<KeyBits<T>::N>(k, hist, s_sel, [&](auto count) { count(tmax); });
        const uint32_t kth_key = radix_select<KeyBits<T>::N>(k, hist, s_sel, [&](auto count) {
            for_each_column(row, V, vec, tid, [&](float v, int) {
                const uint32_t key = key_of(v);
                if (key >= floor_key) count(key);
            });
        });
        const float xk = key_value(kth_key);
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for_each_column(row, V, vec, tid, [&](float v, int c) {
            if (v >= xk) {
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < kCap) { sv[slot] = v; si[slot] = c; }
            }
            if (srow) srow[c] = -INFINITY;                    // the kept columns are written once the cut is known
        });
        __syncthreads();
        n = s_cnt;
        if (n > kCap) {                                       // block-uniform: >= 1025 exact ties at the k-th value
            if (tid == 0) atomicOr(flags, 1);
            n = collect_in_order(V, xk, sv, si, &s_cnt, s_wc, [&](int c) { return to_f32(row[c]); });
        }
        if (n < 1) {                                          // only a row outside the contract (NaN) has no survivor
            if (tid == 0) { sv[0] = -INFINITY; si[0] = 0; }
            n = 1;
        }
        int P = 64;
        while (P < n) P <<= 1;                                // <= kCap
        for (int i = n + tid; i < P; i += 1024) { sv[i] = -INFINITY; si[i] = kNoIndex; }
        __syncthreads();
        sort_table(sv, si, P, tid);
        // ---- 3a. y and the top-p cut, one wave (sample_topk_kernel's fixed-order scan) -------------------------------------------------
        if (w == 0) {
            const int per = P >> 6, j0 = lane * per;          // lane l: ranks l * per .. l * per + per - 1
            float loc = 0.f;
            for (int i = 0; i < per; ++i) {
                const int j = j0 + i;
                float e = 0.f;
                if (j < n) {
                    const float y = y_of(sv[j]);
                    sv[j] = y;
                    e = expf(y - y0);
                }
                se[j] = e;
                loc += e;
            }
            const float incl = wave_scan(loc, lane);
            const float tot = __shfl(incl, 63, 64);
            float excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 0.f;
            int kept = n;
            if (top_p < 1.f) {                                // rank j stays iff sum_{i >= j} e_i > (1 - top_p) sum; rank 0 always
                const float cut = (1.f - top_p) * tot;
                float acc = excl;
                int cnt = 0;
                for (int i = 0; i < per; ++i) {
                    const int j = j0 + i;
                    if (j < n) {
                        cnt += (j == 0 || tot - acc > cut) ? 1 : 0;
                        acc += se[j];
                    }
                }
                kept = min(max(wave_sum_int(cnt), 1), n);
            }
            if (lane == 0) s_kept = kept;
        }
        __syncthreads();
        m = s_kept;
        // ---- 4a. perturbed keys of the kept ranks, the draw order ---------------------------------------------------------------------
        for (int j = tid; j < P; j += 1024) {
            const int c = si[j];
            if (j < m && c >= 0 && c < V) {
                const float y = sv[j];
                if (srow) srow[c] = y;
                se[j] = (y + run) + gumbel_noise(h3, flat0 + (uint64_t)c);
            } else {
                se[j] = -INFINITY;
                si[j] = kNoIndex;
            }
        }
        __syncthreads();
        sort_table(se, si, P, tid);
    } else {
        // ---- 2b. both filters off: the keep-th largest perturbed key over all V columns ---------------------------------------------
        auto key_at = [&](float v, int c) { return (y_of(v) + run) + gumbel_noise(h3, flat0 + (uint64_t)c); };
        uint32_t kmax = 0;
        for_each_column(row, V, vec, tid, [&](float v, int c) {
            if (srow) srow[c] = y_of(v);
            kmax = max(kmax, key_of(key_at(v, c)));
        });
        const uint32_t floor_key = radix_select<32>(keep, hist, s_sel, [&](auto count) { count(kmax); });
        const float kth = key_value(radix_select<32>(keep, hist, s_sel, [&](auto count) {
            for_each_column(row, V, vec, tid, [&](float v, int c) {
                const uint32_t key = key_of(key_at(v, c));
                if (key >= floor_key) count(key);
            });
        }));
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for_each_column(row, V, vec, tid, [&](float v, int c) {
            const float key = key_at(v, c);
            if (key >= kth) {
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < kCap) { se[slot] = key; si[slot] = c; }
            }
        });
        __syncthreads();
        n = max(s_cnt, 0);
        // a running score of -1e9 (ulp 64) swallows y and the noise: thousands of equal keys.  Such a beam's candidates rank below every
        // live beam's, but its table is still a function of the inputs alone
        if (n > kCap) n = collect_in_order(V, kth, se, si, &s_cnt, s_wc, [&](int c) { return key_at(to_f32(row[c]), c); });
        m = n;
        int P = 64;
        while (P < n) P <<= 1;
        for (int i = n + tid; i < P; i += 1024) { se[i] = -INFINITY; si[i] = kNoIndex; }
        __syncthreads();
        sort_table(se, si, P, tid);
    }
    // ---- 5. the row's first `keep` draws (ranks keep .. 63 are never read) --------------------------------------------------------------
    if (tid < kKeepMax) {
        const int c = si[tid];
        const bool valid = tid < min(m, keep) && c >= 0 && c < V;
        const int cc = min(max(c, 0), V - 1);
        cand_key[(int64_t)bb * kKeepMax + tid] = valid ? se[tid] : -INFINITY;
        cand_acc[(int64_t)bb * kKeepMax + tid] = valid ? y_of(to_f32(row[cc])) + run : -INFINITY;
        cand_col[(int64_t)bb * kKeepMax + tid] = cc;
    }
    if (tid == 0) row_best[bb] = y0 + run;
}

struct SampleMergeArgs {
    MergeArgs m;
    int32_t* flags;
};

__global__ void __launch_bounds__(256) beam_sample_merge_kernel(SampleMergeArgs a) { beam_merge_body<true>(a.m, a.flags); }

}  // namespace
}  // namespace p2t

using namespace p2t;

extern "C" size_t p2t_beam_sample_workspace_bytes(int B0, int num_beams) {
    if (B0 <= 0 || num_beams <= 0) return 0;
    return (size_t)B0 * num_beams * (3 * kKeepMax + 1) * sizeof(float);
}

extern "C" int p2t_beam_sample_select(const void* logits, int dtype, int64_t ld, int B0, int num_beams, int V, const int64_t* eos_ids, int n_eos,
                                      int64_t pad_id, float length_penalty, int early_stopping, int max_length, int G, const int32_t* step,
                                      const p2t_beam_state* state, int64_t* next_tokens, int64_t* src_rows, float* scores, int64_t ld_scores,
                                      float temperature, int top_k, float top_p, uint64_t seed, int64_t prompt0, int32_t* flags,
                                      p2t_stream stream) {
    P2T_REQUIRE(logits && step && state && next_tokens && src_rows && flags, "p2t_beam_sample_select: null argument");
    P2T_REQUIRE(state->run_seq && state->run_idx && state->run_scores && state->fin_seq && state->fin_idx && state->fin_scores &&
                    state->is_finished && state->heuristic_open && state->done && state->sync && state->workspace,
                "p2t_beam_sample_select: null pointer in the state");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_beam_sample_select: dtype %d is neither P2T_F32 nor P2T_BF16", dtype);
    P2T_REQUIRE(B0 > 0 && num_beams > 0 && V > 0 && ld >= V,
                "p2t_beam_sample_select: B0 = %d, num_beams = %d, V = %d, ld = %lld: needs positive counts, ld >= V", B0, num_beams, V, (long long)ld);
    P2T_REQUIRE(n_eos >= 0 && (n_eos == 0 || eos_ids), "p2t_beam_sample_select: n_eos = %d: needs n_eos >= 0 and eos_ids for n_eos > 0", n_eos);
    P2T_REQUIRE(G > 0 && G % 64 == 0 && max_length > 0 && max_length <= G,
                "p2t_beam_sample_select: G = %d, max_length = %d: needs G a positive multiple of 64 and 1 <= max_length <= G", G, max_length);
    P2T_REQUIRE(length_penalty == length_penalty, "p2t_beam_sample_select: length_penalty is NaN");
    P2T_REQUIRE(early_stopping >= 0 && early_stopping <= 2, "p2t_beam_sample_select: early_stopping = %d: 0 (False), 1 (True) or 2 (\"never\")",
                early_stopping);
    P2T_REQUIRE(!scores || ld_scores >= V, "p2t_beam_sample_select: ld_scores = %lld < V = %d", (long long)ld_scores, V);
    P2T_REQUIRE(temperature > 0.f && temperature < INFINITY, "p2t_beam_sample_select: temperature %g is not a positive finite number",
                (double)temperature);
    P2T_REQUIRE(top_k >= 0 && top_k <= 1024, "p2t_beam_sample_select: top_k = %d: 0 (off) or 1 .. 1024", top_k);
    P2T_REQUIRE(top_p > 0.f, "p2t_beam_sample_select: top_p = %g: in (0, 1), or >= 1 for off", (double)top_p);
    if (top_k == 0 && top_p < 1.f) {
        set_error("p2t_beam_sample_select: top_p = %g without top_k needs a sort of the whole vocabulary: supported are top_k 1 .. 1024 (top_p on or "
                  "off) and both filters off", (double)top_p);
        return P2T_ERR_UNSUPPORTED;
    }
    const int64_t keep = (int64_t)(n_eos + 1 > 2 ? n_eos + 1 : 2) * num_beams;
    if (num_beams > kBeamsMax || keep > kKeepMax || V < keep || (int64_t)B0 * num_beams * V > 0x7fffffffll) {
        set_error("p2t_beam_sample_select: num_beams = %d, keep = max(2, 1 + n_eos) * num_beams = %lld, V = %d, B0 = %d: supported are 1 <= num_beams "
                  "<= %d, keep <= %d, V >= keep, B0 * num_beams * V < 2^31", num_beams, (long long)keep, V, B0, kBeamsMax, kKeepMax);
        return P2T_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    const int BB = B0 * num_beams;
    float* ws = state->workspace;
    float* cand_key = ws;
    int32_t* cand_col = reinterpret_cast<int32_t*>(ws + (int64_t)BB * kKeepMax);
    float* cand_acc = ws + 2 * (int64_t)BB * kKeepMax;
    float* row_best = ws + 3 * (int64_t)BB * kKeepMax;
    if (dtype == P2T_BF16)
        beam_sample_rows_kernel<bf16_t><<<BB, 1024, 0, s>>>((const bf16_t*)logits, ld, V, num_beams, (int)keep, max_length, step, state->done,
                                                            state->run_scores, BB, temperature, top_k, top_p, seed, prompt0, cand_key, cand_col,
                                                            cand_acc, row_best, scores, ld_scores, flags);
    else
        beam_sample_rows_kernel<float><<<BB, 1024, 0, s>>>((const float*)logits, ld, V, num_beams, (int)keep, max_length, step, state->done,
                                                           state->run_scores, BB, temperature, top_k, top_p, seed, prompt0, cand_key, cand_col,
                                                           cand_acc, row_best, scores, ld_scores, flags);
    P2T_LAUNCH_CHECK();
    SampleMergeArgs a{{*state, step, eos_ids, next_tokens, src_rows, pad_id, B0, num_beams, V, (int)keep, n_eos, G, max_length, early_stopping,
                       length_penalty}, flags};
    beam_sample_merge_kernel<<<B0, 256, 0, s>>>(a);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
