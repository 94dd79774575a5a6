// Beam sampling (p2t_beam_sample_select): one step of transformers' `_beam_search` with do_sample=True (beam-search multinomial
// sampling; 5.x, generation/utils.py `_get_top_k_continuations`) with an empty id prompt, as two launches that read every length on
// the device.  The contract, every tie-break included, is the comment on p2t_beam_sample_select in include/p2t_hip.h;
// tests/beam_sample_reference.py restates it in fp64.
//
// HF draws keep = max(2, 1 + n_eos) * nb continuations per prompt WITHOUT replacement from softmax(processed log-probabilities +
// running scores) over nb * V candidates.  Drawing without replacement is the descending order of acc + Gumbel noise (Plackett-Luce), so
// a select over perturbed keys does the whole draw; the noise of a candidate is a counter hash of (seed, prompt, step, beam * V + column).
//
// beam_sample_rows_kernel, one 1024-thread block per row (beam): the row maximum (here, through the order-preserving key), lse
// (row_lse), then the table pipeline of select_common.h; this file's own are the Gumbel keys and the second sort:
//   top_k on:  the pipeline on the stored logits (kth_largest_stored, collect_survivors -- the ordered path raises bit 0 of the flags
//              word --, pad_and_sort_table), then top_p_cut by wave 0 with e_j = exp(y_j - y_0), y = ((x - mx) - lse) / temperature
//              written over the stored logit; then key = (y + running) + noise per kept entry and a second sort_table by (key
//              descending, column ascending);
//   both off:  key for every column, the keep-th largest key by kth_largest_key over the 32-bit keys (the noise is recomputed per pass:
//              a hash and two logf per column, next to a row read from L2), the keys at or above it collected (bit 0 stays) and sorted.
//   The first `keep` (key, column) pairs of the sorted table go to the workspace with acc recomputed from the column (the same three
//   operations on the same numbers: the same bits), and the row's best acc.
// beam_sample_merge_kernel, one 256-thread block per prompt: beam_merge.h with the perturbed key as the rank key.
// No float atomics, fixed reduction orders: the same inputs give the same bits.  Every LDS index is bounded by kCap / 256 / 16 whatever
// the counts say, cur outside [0, max_length) counts as done, and columns are clamped to [0, V).
#include "beam_merge.h"
#include "select_common.h"

namespace p2t {
namespace {

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
    const uint32_t tmax = thread_max_key(row, V, vec, tid);
    uint32_t bmax = tmax;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bmax = max(bmax, (uint32_t)__shfl_xor((int)bmax, o, 64));
    if (lane == 0) s_wmax[w] = bmax;
    __syncthreads();
    bmax = s_wmax[0];
#pragma unroll
    for (int ww = 1; ww < 16; ++ww) bmax = max(bmax, s_wmax[ww]);
    const float mx = key_value(bmax);
    const float lse = row_lse(row, V, vec, mx, s_sum);
    const float y0 = (0.f - lse) / temperature;               // y of the row's largest logit
    auto y_of = [&](float v) { return ((v - mx) - lse) / temperature; };

    int n, m;                                                 // table entries, valid (kept) entries
    if (top_k > 0) {                                          // block-uniform
        // ---- 2a. the k-th largest stored logit, its survivors, their total order (select_common.h, on the stored logits) -------------
        const float xk = key_value(kth_largest_stored(row, V, vec, min(top_k, V), tmax, hist, s_sel));
        auto stored = [](float v, int) { return v; };
        n = collect_survivors(row, V, vec, xk, sv, si, &s_cnt, stored, [&](int c, float, bool) {
            if (srow) srow[c] = -INFINITY;                    // the kept columns are written once the cut is known
        });
        if (n > kCap) {                                       // block-uniform: >= 1025 exact ties at the k-th value
            if (tid == 0) atomicOr(flags, 1);
            n = collect_in_order(row, V, xk, sv, si, &s_cnt, s_wc, stored);
        }
        if (n < 1) {                                          // only a row outside the contract (NaN) has no survivor
            if (tid == 0) { sv[0] = -INFINITY; si[0] = 0; }
            n = 1;
        }
        const int P = pad_and_sort_table(sv, si, n, tid);
        // ---- 3a. y and the top-p cut, one wave ------------------------------------------------------------------------------------------
        if (w == 0) {
            float excl;
            const int kept = top_p_cut(n, P, top_p, se, lane, excl, [&](int j) {
                const float y = y_of(sv[j]);
                sv[j] = y;
                return expf(y - y0);
            });
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
        // ---- 2b. both filters off: the keep-th largest perturbed key over all V columns, the keys at or above it, sorted ------------
        auto key_at = [&](float v, int c) { return (y_of(v) + run) + gumbel_noise(h3, flat0 + (uint64_t)c); };
        uint32_t kmax = 0;
        for_each_column(row, V, vec, tid, [&](float v, int c) {
            if (srow) srow[c] = y_of(v);
            kmax = max(kmax, key_of(key_at(v, c)));
        });
        const float kth = key_value(kth_largest_key<32>(row, V, vec, keep, kmax, hist, s_sel, [&](float v, int c) { return key_of(key_at(v, c)); }));
        // a running score of -1e9 (ulp 64) swallows y and the noise: thousands of equal keys, the ordered path.  Such a beam's candidates
        // rank below every live beam's, but its table is still a function of the inputs alone (and bit 0 stays: no top-k boundary here)
        n = max(collect_survivors(row, V, vec, kth, se, si, &s_cnt, key_at), 0);
        if (n > kCap) n = collect_in_order(row, V, kth, se, si, &s_cnt, s_wc, key_at);
        m = n;
        pad_and_sort_table(se, si, n, tid);
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
    P2T_REQUIRE(flags, "p2t_beam_sample_select: null argument");
    P2T_REQUIRE(temperature > 0.f && temperature < INFINITY, "p2t_beam_sample_select: temperature %g is not a positive finite number",
                (double)temperature);
    P2T_REQUIRE(top_k >= 0 && top_k <= 1024, "p2t_beam_sample_select: top_k = %d: 0 (off) or 1 .. 1024", top_k);
    P2T_REQUIRE(top_p > 0.f, "p2t_beam_sample_select: top_p = %g: in (0, 1), or >= 1 for off", (double)top_p);
    BeamStep b;                                               // every argument error comes before either unsupported combination
    const int rc = beam_step_setup("p2t_beam_sample_select", logits, dtype, ld, B0, num_beams, V, eos_ids, n_eos, pad_id, length_penalty,
                                   early_stopping, max_length, G, step, state, next_tokens, src_rows, scores, ld_scores, &b);
    if (rc == P2T_ERR_ARG) return rc;
    if (top_k == 0 && top_p < 1.f) {
        set_error("p2t_beam_sample_select: top_p = %g without top_k needs a sort of the whole vocabulary: supported are top_k 1 .. 1024 (top_p on or "
                  "off) and both filters off", (double)top_p);
        return P2T_ERR_UNSUPPORTED;
    }
    P2T_TRY(rc);
    hipStream_t s = (hipStream_t)stream;
    float *cand_key = b.plane0, *cand_acc = b.plane2, *row_best = b.plane2 + (int64_t)b.BB * kKeepMax;
    if (dtype == P2T_BF16)
        beam_sample_rows_kernel<bf16_t><<<b.BB, 1024, 0, s>>>((const bf16_t*)logits, ld, V, num_beams, b.keep, max_length, step, state->done,
                                                              state->run_scores, b.BB, temperature, top_k, top_p, seed, prompt0, cand_key,
                                                              b.cand_col, cand_acc, row_best, scores, ld_scores, flags);
    else
        beam_sample_rows_kernel<float><<<b.BB, 1024, 0, s>>>((const float*)logits, ld, V, num_beams, b.keep, max_length, step, state->done,
                                                             state->run_scores, b.BB, temperature, top_k, top_p, seed, prompt0, cand_key,
                                                             b.cand_col, cand_acc, row_best, scores, ld_scores, flags);
    P2T_LAUNCH_CHECK();
    SampleMergeArgs a{b.merge, flags};
    beam_sample_merge_kernel<<<B0, 256, 0, s>>>(a);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
