// Beam-search selection (p2t_beam_select): one step of transformers' `_beam_search` (5.x, vectorised form; generation/utils.py) with an
// empty id prompt, as two launches that read every length on the device.  The contract, every tie-break included, is the comment on
// p2t_beam_select in include/p2t_hip.h; tests/beam_reference.py restates it in fp64.
//
// beam_rows_kernel, one 1024-thread block per row (beam): the row's `keep` largest stored logits by sample_select's radix select
// (select_common.h), sorted by (value descending, column ascending), then max and lse = logf(sum expf(x - max)) over the row in a fixed
// order, and optionally the row of log-probabilities.  x -> ((x - max) - lse) + running is monotone, so a prompt's `keep` best
// continuations lie among its beams' `keep` best each.
// beam_merge_kernel, one 256-thread block per prompt (beam_merge.h, shared with p2t_beam_sample_select): the nb * keep candidates are
// ranked by counting, then the bookkeeping of the step on <= 64 candidates, the table rows' move between the double-buffered halves
// and the stop condition over the prompts.
// No float atomics, fixed reduction orders: the same inputs give the same bits.  Every index is bounded whatever the inputs hold:
// cur outside [0, max_length) counts as done, columns are clamped to [0, V), ranks are only stored below their table sizes.
#include "beam_merge.h"
#include "select_common.h"

namespace p2t {
namespace {

template <typename T>
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
    const int bb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const T* row = logits + (int64_t)bb * ld;
    const int k = min(keep, V);

    // ---- the keep-th largest stored logit (sample_topk_kernel's two selects) ----------------------------------------------
    const bool vec = ld % (16 / sizeof(T)) == 0 && ((uintptr_t)logits & 15u) == 0;
    uint32_t tmax = 0;
    for_each_column(row, V, vec, tid, [&](float v, int) { tmax = max(tmax, key_of(v)); });
    const uint32_t floor_key = radix_select<KeyBits<T>::N>(k, hist, s_sel, [&](auto count) { count(tmax); });
    const uint32_t kth_key = radix_select<KeyBits<T>::N>(k, hist, s_sel, [&](auto count) {
        for_each_column(row, V, vec, tid, [&](float v, int) {
            const uint32_t key = key_of(v);
            if (key >= floor_key) count(key);
        });
    });
    const float xk = key_value(kth_key);

    // ---- survivors: x >= xk ------------------------------------------------------------------------------------------------
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for_each_column(row, V, vec, tid, [&](float v, int c) {
        if (v >= xk) {
            const int slot = atomicAdd(&s_cnt, 1);
            if (slot < kCap) { sv[slot] = v; si[slot] = c; }
        }
    });
    __syncthreads();
    int n = s_cnt;
    if (n > kCap) {                                           // block-uniform: more than kCap - keep exact ties at the keep-th value
        __syncthreads();
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int c = tid; c < V; c += 1024) {
            const float x = to_f32(row[c]);
            if (x > xk) {                                     // fewer than keep of them
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < kCap) { sv[slot] = x; si[slot] = c; }
            }
        }
        __syncthreads();
        int base = min(s_cnt, kCap);
        for (int c0 = 0; c0 < V; c0 += 1024) {                // the ties, ascending column, until the table is full
            const int c = c0 + tid;
            const bool eq = c < V && to_f32(row[c]) == xk;
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
                if (slot < kCap) { sv[slot] = xk; si[slot] = c; }
            }
            base = min(base + tot, 2 * kCap);
            __syncthreads();
        }
        n = min(base, kCap);
    }
    n = max(n, 0);
    // ---- total order: value descending, column ascending -----------------------------------------------------------------------
    int P = 64;
    while (P < n) P <<= 1;                                    // <= kCap
    for (int i = n + tid; i < P; i += 1024) { sv[i] = -INFINITY; si[i] = kNoIndex; }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < (P >> 1)) {
                const int i = ((tid / stride) * 2 * stride + (tid % stride)) & (kCap - 1), j = (i + stride) & (kCap - 1);
                const float va = sv[i], vb = sv[j];
                const int ia = si[i], ib = si[j];
                const bool b_first = vb > va || (vb == va && ib < ia);
                const bool a_first = va > vb || (va == vb && ia < ib);
                if (((i & size) == 0) ? b_first : a_first) { sv[i] = vb; sv[j] = va; si[i] = ib; si[j] = ia; }
            }
            __syncthreads();
        }
    }
    const float mx = sv[0];
    if (tid < kKeepMax) {                                     // ranks keep .. 63 are never read
        cand_val[(int64_t)bb * kKeepMax + tid] = sv[tid];
        cand_col[(int64_t)bb * kKeepMax + tid] = min(max(si[tid], 0), V - 1);
    }
    // ---- lse: every thread adds its columns in for_each_column's order, the lanes by a butterfly, the waves in wave order --------
    float part = 0.f;
    for_each_column(row, V, vec, tid, [&](float v, int) { part += expf(v - mx); });
    part = wave_sum(part);
    if (lane == 0) s_sum[w] = part;
    __syncthreads();
    float S = 0.f;
#pragma unroll
    for (int ww = 0; ww < 16; ++ww) S += s_sum[ww];
    const float lse = logf(S);
    if (tid == 0) { row_stat[2 * bb] = mx; row_stat[2 * bb + 1] = lse; }
    if (scores) {
        float* srow = scores + (int64_t)bb * ld_scores;
        for (int c = tid; c < V; c += 1024) srow[c] = (to_f32(row[c]) - mx) - lse;
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
    P2T_REQUIRE(logits && step && state && next_tokens && src_rows, "p2t_beam_select: null argument");
    P2T_REQUIRE(state->run_seq && state->run_idx && state->run_scores && state->fin_seq && state->fin_idx && state->fin_scores &&
                    state->is_finished && state->heuristic_open && state->done && state->sync && state->workspace,
                "p2t_beam_select: null pointer in the state");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_beam_select: dtype %d is neither P2T_F32 nor P2T_BF16", dtype);
    P2T_REQUIRE(B0 > 0 && num_beams > 0 && V > 0 && ld >= V, "p2t_beam_select: B0 = %d, num_beams = %d, V = %d, ld = %lld: needs positive counts, ld >= V",
                B0, num_beams, V, (long long)ld);
    P2T_REQUIRE(n_eos >= 0 && (n_eos == 0 || eos_ids), "p2t_beam_select: n_eos = %d: needs n_eos >= 0 and eos_ids for n_eos > 0", n_eos);
    P2T_REQUIRE(G > 0 && G % 64 == 0 && max_length > 0 && max_length <= G,
                "p2t_beam_select: G = %d, max_length = %d: needs G a positive multiple of 64 and 1 <= max_length <= G", G, max_length);
    P2T_REQUIRE(length_penalty == length_penalty, "p2t_beam_select: length_penalty is NaN");
    P2T_REQUIRE(early_stopping >= 0 && early_stopping <= 2, "p2t_beam_select: early_stopping = %d: 0 (False), 1 (True) or 2 (\"never\")", early_stopping);
    P2T_REQUIRE(!scores || ld_scores >= V, "p2t_beam_select: ld_scores = %lld < V = %d", (long long)ld_scores, V);
    const int64_t keep = (int64_t)(n_eos + 1 > 2 ? n_eos + 1 : 2) * num_beams;
    if (num_beams > kBeamsMax || keep > kKeepMax || V < keep || (int64_t)B0 * num_beams * V > 0x7fffffffll) {
        set_error("p2t_beam_select: num_beams = %d, keep = max(2, 1 + n_eos) * num_beams = %lld, V = %d, B0 = %d: supported are 1 <= num_beams <= %d, "
                  "keep <= %d, V >= keep, B0 * num_beams * V < 2^31", num_beams, (long long)keep, V, B0, kBeamsMax, kKeepMax);
        return P2T_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    const int BB = B0 * num_beams;
    float* ws = state->workspace;
    float* cand_val = ws;
    int32_t* cand_col = reinterpret_cast<int32_t*>(ws + (int64_t)BB * kKeepMax);
    float* row_stat = ws + 2 * (int64_t)BB * kKeepMax;
    if (dtype == P2T_BF16)
        beam_rows_kernel<bf16_t><<<BB, 1024, 0, s>>>((const bf16_t*)logits, ld, V, (int)keep, max_length, step, state->done, cand_val, cand_col, row_stat,
                                                     scores, ld_scores);
    else
        beam_rows_kernel<float><<<BB, 1024, 0, s>>>((const float*)logits, ld, V, (int)keep, max_length, step, state->done, cand_val, cand_col, row_stat,
                                                    scores, ld_scores);
    P2T_LAUNCH_CHECK();
    MergeArgs a{*state, step, eos_ids, next_tokens, src_rows, pad_id, B0, num_beams, V, (int)keep, n_eos, G, max_length, early_stopping, length_penalty};
    beam_merge_kernel<<<B0, 256, 0, s>>>(a);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
