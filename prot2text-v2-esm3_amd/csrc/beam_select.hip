// Beam-search selection (p2t_beam_select): one step of transformers' `_beam_search` (5.x, vectorised form; generation/utils.py) with an
// empty id prompt, as two launches that read every length on the device.  The contract, every tie-break included, is the comment on
// p2t_beam_select in include/p2t_hip.h; tests/beam_reference.py restates it in fp64.
//
// beam_rows_kernel, one 1024-thread block per row (beam): the row's `keep` largest stored logits by sample_select's radix select
// (select_common.h), sorted by (value descending, column ascending), then max and lse = logf(sum expf(x - max)) over the row in a fixed
// order, and optionally the row of log-probabilities.  x -> ((x - max) - lse) + running is monotone, so a prompt's `keep` best
// continuations lie among its beams' `keep` best each.
// beam_merge_kernel, one 256-thread block per prompt: the nb * keep candidates are ranked by counting (every rank is a total order, so
// the result does not depend on the thread schedule), then the bookkeeping of the step on <= 64 candidates, then the table rows move
// between beams.  The tables are double-buffered on the parity of the step counter: a step reads half cur & 1 and writes the other,
// so no row is read after another beam has overwritten it.  Columns above cur hold the caller's fill in both halves (no step
// writes past its own column), so only columns 0 .. cur are copied.
// The stop condition spans the prompts: every block leaves its three flags in sync[1 + b] and takes a ticket from sync[0] (an integer
// atomic); the block that takes the last one combines them in prompt order, raises done and resets the ticket.
// No float atomics, fixed reduction orders: the same inputs give the same bits.  Every index is bounded whatever the inputs hold:
// cur outside [0, max_length) counts as done, columns are clamped to [0, V), ranks are only stored below their table sizes.
#include "select_common.h"

namespace p2t {
namespace {

constexpr int kKeepMax = 64;                // candidates per row / per prompt after the first cut
constexpr int kBeamsMax = 16;
constexpr float kMask = -1.0e9f;

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

struct MergeArgs {
    p2t_beam_state st;
    const int32_t* step;
    const int64_t* eos;
    int64_t* next_tokens;
    int64_t* src_rows;
    int64_t pad;
    int B0, nb, V, keep, n_eos, G, max_length, early_stopping;
    float length_penalty;
};

// rank of entry i of val[0 .. n) under (value descending, position ascending)
__device__ __forceinline__ int rank_of(const float* val, int n, int i) {
    const float v = val[i];
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const float u = val[j];
        r += (u > v || (u == v && j < i)) ? 1 : 0;
    }
    return r;
}

__global__ void __launch_bounds__(256) beam_merge_kernel(MergeArgs a) {
    __shared__ float c_acc[kBeamsMax * kKeepMax];             // the nb * keep candidates, in (beam, rank inside the beam) order
    __shared__ int top[kKeepMax];                             // the first cut: candidate index per rank
    __shared__ float t_lp[kKeepMax], t_live[kKeepMax], m_sc[kBeamsMax + kKeepMax];
    __shared__ int t_tok[kKeepMax], t_beam[kKeepMax], t_hit[kKeepMax], t_just[kKeepMax];
    __shared__ int nxt[kBeamsMax], sel[kBeamsMax], fin_old[kBeamsMax], fin_new[kBeamsMax];
    __shared__ float sc_new[kBeamsMax];
    __shared__ int s_last;
    const int b = blockIdx.x, tid = threadIdx.x, nb = a.nb, keep = a.keep, G = a.G;
    const int cur = a.step[0];
    if (a.st.done[0] != 0 || cur < 0 || cur >= a.max_length) {             // stopped: the state stays, pad and the identity come out
        for (int r = tid; r < nb; r += 256) {
            a.next_tokens[b * nb + r] = a.pad;
            a.src_rows[b * nb + r] = b * nb + r;
        }
        return;
    }
    const int rd = cur & 1, wr = rd ^ 1;
    const int64_t tab = (int64_t)a.B0 * nb * G;               // one half of a table
    const int64_t vecn = (int64_t)a.B0 * nb;                   // one half of a per-beam vector
    const float* run_sc = a.st.run_scores + rd * vecn + b * nb;
    const float* cand_val = a.st.workspace;
    const int32_t* cand_col = reinterpret_cast<const int32_t*>(a.st.workspace + (int64_t)a.B0 * nb * kKeepMax);
    const float* row_stat = a.st.workspace + 2 * (int64_t)a.B0 * nb * kKeepMax;

    // ---- candidates and the first cut ------------------------------------------------------------------------------------------
    const int n = nb * keep;
    for (int i = tid; i < n; i += 256) {
        const int beam = i / keep, r = i - beam * keep, row = b * nb + beam;
        const float x = cand_val[(int64_t)row * kKeepMax + r];
        c_acc[i] = ((x - row_stat[2 * row]) - row_stat[2 * row + 1]) + run_sc[beam];
    }
    if (tid < kKeepMax) top[tid] = 0;
    if (tid < kBeamsMax) { nxt[tid] = 0; sel[tid] = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int r = rank_of(c_acc, n, i);
        if (r < keep) top[r] = i;
    }
    __syncthreads();
    // ---- stopping hits, the beams that go on, the finished candidates -------------------------------------------------------------
    int all_fin_old = 1;
    for (int j = 0; j < nb; ++j) all_fin_old &= a.st.is_finished[rd * vecn + b * nb + j] != 0;
    const int open_old = a.st.heuristic_open[b] != 0;
    const float len_pow = (float)pow((double)(cur + 1), (double)a.length_penalty);
    if (tid < keep) {
        const int i = top[tid], beam = i / keep, r = i - beam * keep;
        const float lp = c_acc[i];
        const int tok = cand_col[(int64_t)(b * nb + beam) * kKeepMax + r];
        int hit = cur + 1 >= a.max_length;
        for (int e = 0; e < a.n_eos; ++e) hit |= (int64_t)tok == a.eos[e];
        const int just = hit && tid < nb;
        float fin = lp / len_pow;
        fin = fin + ((all_fin_old && a.early_stopping == 1) ? kMask : -0.f);
        fin = fin + (open_old ? -0.f : kMask);
        fin = fin + (just ? -0.f : kMask);
        t_lp[tid] = lp; t_tok[tid] = tok; t_beam[tid] = beam; t_hit[tid] = hit; t_just[tid] = just;
        t_live[tid] = lp + (hit ? kMask : -0.f);
        m_sc[nb + tid] = fin;
    }
    if (tid < nb) {
        m_sc[tid] = a.st.fin_scores[rd * vecn + b * nb + tid];
        fin_old[tid] = a.st.is_finished[rd * vecn + b * nb + tid];
    }
    __syncthreads();
    if (tid < keep) {
        const int r = rank_of(t_live, keep, tid);
        if (r < nb) nxt[r] = tid;
    }
    if (tid < nb + keep) {
        const int r = rank_of(m_sc, nb + keep, tid);
        if (r < nb) sel[r] = tid;
    }
    __syncthreads();
    // ---- the tables: half rd -> half wr -----------------------------------------------------------------------------------------
    const int64_t* run_seq_r = a.st.run_seq + rd * tab + (int64_t)b * nb * G;
    const int32_t* run_idx_r = a.st.run_idx + rd * tab + (int64_t)b * nb * G;
    const int64_t* fin_seq_r = a.st.fin_seq + rd * tab + (int64_t)b * nb * G;
    const int32_t* fin_idx_r = a.st.fin_idx + rd * tab + (int64_t)b * nb * G;
    int64_t* run_seq_w = a.st.run_seq + wr * tab + (int64_t)b * nb * G;
    int32_t* run_idx_w = a.st.run_idx + wr * tab + (int64_t)b * nb * G;
    int64_t* fin_seq_w = a.st.fin_seq + wr * tab + (int64_t)b * nb * G;
    int32_t* fin_idx_w = a.st.fin_idx + wr * tab + (int64_t)b * nb * G;
    for (int r = 0; r < nb; ++r) {
        const int kq = nxt[r], sb = t_beam[kq];               // running row r <- candidate kq: beam sb's row and one more token
        for (int c = tid; c <= cur; c += 256) {
            run_seq_w[r * G + c] = c == cur ? (int64_t)t_tok[kq] : run_seq_r[sb * G + c];
            run_idx_w[r * G + c] = c == cur ? b * nb + sb : run_idx_r[sb * G + c];
        }
        const int s = sel[r];
        if (s < nb) {                                         // a finished slot that stays (maybe in another place)
            for (int c = tid; c <= cur; c += 256) {
                fin_seq_w[r * G + c] = fin_seq_r[s * G + c];
                fin_idx_w[r * G + c] = fin_idx_r[s * G + c];
            }
        } else {
            const int kf = s - nb, fb = t_beam[kf];
            for (int c = tid; c <= cur; c += 256) {
                fin_seq_w[r * G + c] = c == cur ? (int64_t)t_tok[kf] : run_seq_r[fb * G + c];
                fin_idx_w[r * G + c] = c == cur ? b * nb + fb : run_idx_r[fb * G + c];
            }
        }
    }
    if (tid < nb) {
        const int kq = nxt[tid], s = sel[tid];
        a.st.run_scores[wr * vecn + b * nb + tid] = t_live[kq];
        a.next_tokens[b * nb + tid] = t_tok[kq];
        a.src_rows[b * nb + tid] = b * nb + t_beam[kq];
        const float sc = m_sc[s];
        const int f = s < nb ? fin_old[s] : t_just[s - nb];
        a.st.fin_scores[wr * vecn + b * nb + tid] = sc;
        a.st.is_finished[wr * vecn + b * nb + tid] = f;
        sc_new[tid] = sc;
        fin_new[tid] = f;
    }
    __syncthreads();
    // ---- can a running beam still beat the worst finished one; the stop condition over all prompts -------------------------------
    if (tid == 0) {
        const int best_len = (a.early_stopping == 2 && a.length_penalty > 0.f) ? a.max_length : cur + 1;
        const float best_running = t_live[nxt[0]] / (float)pow((double)best_len, (double)a.length_penalty);
        float lo = sc_new[0];
        int all_fin = 1, all_hits = 1, any_better = 0;
        for (int j = 1; j < nb; ++j) lo = fminf(lo, sc_new[j]);
        for (int j = 0; j < nb; ++j) {
            all_fin &= fin_new[j] != 0;
            any_better |= best_running > (fin_new[j] ? lo : kMask);
        }
        for (int j = 0; j < keep; ++j) all_hits &= t_hit[j];
        const int open = open_old && any_better;
        a.st.heuristic_open[b] = open;
        a.st.sync[1 + b] = open | (all_fin << 1) | (all_hits << 2);
        __threadfence();
        s_last = atomicAdd(&a.st.sync[0], 1) == a.B0 - 1;
        if (s_last) {
            __threadfence();
            int any_open = 0, fin_all = 1, hits_all = 1;
            for (int p = 0; p < a.B0; ++p) {
                const int f = __atomic_load_n(&a.st.sync[1 + p], __ATOMIC_RELAXED);
                any_open |= f & 1;
                fin_all &= (f >> 1) & 1;
                hits_all &= (f >> 2) & 1;
            }
            const int go_on = any_open && !(fin_all && a.early_stopping == 1) && !hits_all;
            a.st.sync[0] = 0;
            if (!go_on || cur + 1 >= a.max_length) {
                a.st.done[1] = cur + 1;
                a.st.done[0] = 1;
            }
        }
    }
}

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
