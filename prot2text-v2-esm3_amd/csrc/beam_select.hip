// Beam-search selection (p2t_beam_select; p2t_beam_select_logprobs on rows that already hold processed log-probabilities, at the end):
// one step of transformers' `_beam_search` (5.x, vectorised form; generation/utils.py) with an empty id prompt, as two launches that
// read every length on the device.  The contract, every tie-break included, is the comment on p2t_beam_select in include/p2t_hip.h;
// tests/beam_reference.py restates it in fp64 (tests/beam_logprobs_reference.py: p2t_beam_select_logprobs in f32).
//
// beam_rows_kernel, one 1024-thread block per row (beam): the table pipeline of select_common.h on the stored logits -- the `keep`-th
// largest by two radix selects, the survivors at or above it, their sort by (value descending, column ascending) -- then max = rank 0
// and lse = logf(sum expf(x - max)) over the row (row_lse).  Its own: the write-out of the first 64 ranks as candidates, (max, lse)
// and optionally the row of log-probabilities.  x -> ((x - max) - lse) + running is monotone, so a prompt's `keep` best continuations
// lie among its beams' `keep` best each.
// beam_merge_kernel, one 256-thread block per prompt (beam_merge.h, shared with p2t_beam_sample_select, as are the argument checks and
// the workspace carving: beam_step_setup): the nb * keep candidates are ranked by counting, then the bookkeeping of the step on <= 64
// candidates, the table rows' move between the double-buffered halves and the stop condition over the prompts.
// No float atomics, fixed reduction orders: the same inputs give the same bits.  Every index is bounded whatever the inputs hold:
// cur outside [0, max_length) counts as done, columns are clamped to [0, V), ranks are only stored below their table sizes.
#include "beam_merge.h"
#include "select_common.h"

namespace p2t {
namespace {

// kLogprobs (p2t_beam_select_logprobs): the row already holds log-probabilities, so it is ranked as it stands: no row_lse, no scores
// write-out, and (mx, lse) = (0, 0), with which the merge's ((x - 0) - 0) + run is exactly x + run (for -inf and -0 as well).
template <typename T, bool kLogprobs = false>
__global__ void __launch_bounds__(1024) beam_rows_kernel(const T* __restrict__ logits, int64_t ld, int V, int keep, int max_length,
                                                         const int32_t* __restrict__ step_ptr, const int32_t* __restrict__ done,
                                                         float* __restrict__ cand_val, int32_t* __restrict__ cand_col,
                                                         float* __restrict__ row_stat, float* __restrict__ scores, int64_t ld_scores) {
    __shared__ int hist[16][256];
    __shared__ float sv[kCap];
    __shared__ int si[kCap];
    __shared__ int s_sel[2], s_cnt, s_wc[16];
    __shared__ float s_sum[16];
    const int cur = step_ptr[0];
    if (done[0] != 0 || cur < 0 || cur >= max_length) return;              // block-uniform
    const int bb = blockIdx.x, tid = threadIdx.x;
    const T* row = logits + (int64_t)bb * ld;
    const int k = min(keep, V);

    // ---- the keep-th largest stored logit, its survivors (more than kCap - keep exact ties there: the ordered path), the total order
    const bool vec = ld % (16 / sizeof(T)) == 0 && ((uintptr_t)logits & 15u) == 0;
    const float xk = key_value(kth_largest_stored(row, V, vec, k, thread_max_key(row, V, vec, tid), hist, s_sel));
    auto stored = [](float v, int) { return v; };
    int n = collect_survivors(row, V, vec, xk, sv, si, &s_cnt, stored);
    if (n > kCap) n = collect_in_order(row, V, xk, sv, si, &s_cnt, s_wc, stored);      // block-uniform
    n = max(n, 0);
    pad_and_sort_table(sv, si, n, tid);
    const float mx = sv[0];
    if (tid < kKeepMax) {                                     // ranks keep .. 63 are never read
        cand_val[(int64_t)bb * kKeepMax + tid] = sv[tid];
        cand_col[(int64_t)bb * kKeepMax + tid] = min(max(si[tid], 0), V - 1);
    }
    if constexpr (kLogprobs) {
        if (tid == 0) { row_stat[2 * bb] = 0.f; row_stat[2 * bb + 1] = 0.f; }
    } else {
        const float lse = row_lse(row, V, vec, mx, s_sum);
        if (tid == 0) { row_stat[2 * bb] = mx; row_stat[2 * bb + 1] = lse; }
        if (scores) {
            float* srow = scores + (int64_t)bb * ld_scores;
            for (int c = tid; c < V; c += 1024) srow[c] = (to_f32(row[c]) - mx) - lse;
        }
    }
}

__global__ void __launch_bounds__(256) beam_merge_kernel(MergeArgs a) { beam_merge_body<false>(a, nullptr); }

}  // namespace
}  // namespace p2t

using namespace p2t;

extern "C" size_t p2t_beam_workspace_bytes(int B0, int num_beams) {
    if (B0 <= 0 || num_beams <= 0) return 0;
    return (size_t)B0 * num_beams * (2 * kKeepMax + 2) * sizeof(float);
}

extern "C" int p2t_beam_select(const void* logits, int dtype, int64_t ld, int B0, int num_beams, int V, const int64_t* eos_ids, int n_eos,
                               int64_t pad_id, float length_penalty, int early_stopping, int max_length, int G, const int32_t* step,
                               const p2t_beam_state* state, int64_t* next_tokens, int64_t* src_rows, float* scores, int64_t ld_scores,
                               p2t_stream stream) {
    BeamStep b;
    P2T_TRY(beam_step_setup("p2t_beam_select", logits, dtype, ld, B0, num_beams, V, eos_ids, n_eos, pad_id, length_penalty, early_stopping, max_length,
                            G, step, state, next_tokens, src_rows, scores, ld_scores, &b));
    hipStream_t s = (hipStream_t)stream;
    float *cand_val = b.plane0, *row_stat = b.plane2;
    if (dtype == P2T_BF16)
        beam_rows_kernel<bf16_t><<<b.BB, 1024, 0, s>>>((const bf16_t*)logits, ld, V, b.keep, max_length, step, state->done, cand_val, b.cand_col,
                                                       row_stat, scores, ld_scores);
    else
        beam_rows_kernel<float><<<b.BB, 1024, 0, s>>>((const float*)logits, ld, V, b.keep, max_length, step, state->done, cand_val, b.cand_col,
                                                      row_stat, scores, ld_scores);
    P2T_LAUNCH_CHECK();
    beam_merge_kernel<<<B0, 256, 0, s>>>(b.merge);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_beam_select_logprobs(const float* lp, int64_t ld, int B0, int num_beams, int V, const int64_t* eos_ids, int n_eos, int64_t pad_id,
                                        float length_penalty, int early_stopping, int max_length, int G, const int32_t* step,
                                        const p2t_beam_state* state, int64_t* next_tokens, int64_t* src_rows, p2t_stream stream) {
    BeamStep b;
    P2T_TRY(beam_step_setup("p2t_beam_select_logprobs", lp, P2T_F32, ld, B0, num_beams, V, eos_ids, n_eos, pad_id, length_penalty, early_stopping,
                            max_length, G, step, state, next_tokens, src_rows, nullptr, 0, &b));
    hipStream_t s = (hipStream_t)stream;
    beam_rows_kernel<float, true><<<b.BB, 1024, 0, s>>>(lp, ld, V, b.keep, max_length, step, state->done, b.plane0, b.cand_col, b.plane2, nullptr, 0);
    P2T_LAUNCH_CHECK();
    beam_merge_kernel<<<B0, 256, 0, s>>>(b.merge);                 // unchanged: the candidates' keys are lp + running
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
