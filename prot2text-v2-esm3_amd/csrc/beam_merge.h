// The per-prompt half of a beam step, shared by p2t_beam_select (beam_select.hip) and p2t_beam_sample_select (beam_sample_select.hip):
// the nb * keep candidates the rows kernel left in the workspace are ranked by counting (every rank is a total order, so the result
// does not depend on the thread schedule), then the bookkeeping of the step on <= 64 candidates, then the table rows move between beams.
// The tables are double-buffered on the parity of the step counter: a step reads half cur & 1 and writes the other, so no row is read
// after another beam has overwritten it.  Columns above cur hold the caller's fill in both halves (no step writes past its own
// column), so only columns 0 .. cur are copied.
// The stop condition spans the prompts: every block leaves its three flags in sync[1 + b] and takes a ticket from sync[0] (an integer
// atomic); the block that takes the last one combines them in prompt order, raises done and resets the ticket.
// kSample = false: the workspace holds {stored logit [BB][64], column [BB][64], (mx, lse) [BB][2]}; a candidate's rank key is its
// accumulated score ((x - mx) - lse) + running.  p2t_beam_select_logprobs leaves log-probabilities and (mx, lse) = (0, 0) there: the
// same expression is then exactly x + running.
// kSample = true: {perturbed key [BB][64], column [BB][64], accumulated score [BB][64], the row's best accumulated score [BB]}; the
// rank key is the perturbed key, the score that goes on is the unperturbed one, and bit 1 of *flags is raised when the keep-th
// candidate is absent or more than 100 below the prompt's best accumulated score.
// The host half of both entry points is here too (beam_step_setup, at the end): the argument checks, keep, the supported range and the
// workspace planes they have in common.
#pragma once
#include "common.h"

namespace p2t {
namespace {

constexpr int kKeepMax = 64;                // candidates per row / per prompt after the first cut
constexpr int kBeamsMax = 16;
constexpr float kMask = -1.0e9f;

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

// the body of a 256-thread block, one block per prompt
template <bool kSample>
__device__ __forceinline__ void beam_merge_body(const MergeArgs& a, int32_t* __restrict__ flags) {
    __shared__ float c_acc[kBeamsMax * kKeepMax];             // the nb * keep candidates' rank keys, in (beam, rank inside the beam) order
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
    const float* row_stat = a.st.workspace + 2 * (int64_t)a.B0 * nb * kKeepMax;      // kSample: the accumulated scores
    const float* row_best = a.st.workspace + 3 * (int64_t)a.B0 * nb * kKeepMax;      // kSample only

    // ---- candidates and the first cut ------------------------------------------------------------------------------------------
    const int n = nb * keep;
    for (int i = tid; i < n; i += 256) {
        const int beam = i / keep, r = i - beam * keep, row = b * nb + beam;
        const float x = cand_val[(int64_t)row * kKeepMax + r];
        if constexpr (kSample) c_acc[i] = x;
        else c_acc[i] = ((x - row_stat[2 * row]) - row_stat[2 * row + 1]) + run_sc[beam];
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
        float lp;
        if constexpr (kSample) {
            lp = row_stat[(int64_t)(b * nb + beam) * kKeepMax + r];
            if (tid == keep - 1) {                            // the last draw: absent (-inf) or of probability 0 in f32
                float best = row_best[b * nb];
                for (int j = 1; j < nb; ++j) best = fmaxf(best, row_best[b * nb + j]);
                if (!(lp >= best - 100.f)) atomicOr(flags, 2);
            }
        } else {
            lp = c_acc[i];
        }
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

// ---- host: what the two entry points check and set up alike ----------------------------------------------------------------------
struct BeamStep {
    int BB, keep;
    float *plane0, *plane2;                                   // workspace planes [BB][64]: candidate keys; (mx, lse) [BB][2] or acc [BB][64]
    int32_t* cand_col;                                        // plane 1: candidate columns
    MergeArgs merge;
};

// The argument checks of entry point `name` (P2T_ERR_ARG), its supported range (P2T_ERR_UNSUPPORTED), keep and the workspace's common part.
inline int beam_step_setup(const char* name, const void* logits, int dtype, int64_t ld, int B0, int num_beams, int V, const int64_t* eos_ids,
                           int n_eos, int64_t pad_id, float length_penalty, int early_stopping, int max_length, int G, const int32_t* step,
                           const p2t_beam_state* state, int64_t* next_tokens, int64_t* src_rows, const float* scores, int64_t ld_scores,
                           BeamStep* out) {
    P2T_REQUIRE(logits && step && state && next_tokens && src_rows, "%s: null argument", name);
    P2T_REQUIRE(state->run_seq && state->run_idx && state->run_scores && state->fin_seq && state->fin_idx && state->fin_scores &&
                    state->is_finished && state->heuristic_open && state->done && state->sync && state->workspace,
                "%s: null pointer in the state", name);
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "%s: dtype %d is neither P2T_F32 nor P2T_BF16", name, dtype);
    P2T_REQUIRE(B0 > 0 && num_beams > 0 && V > 0 && ld >= V, "%s: B0 = %d, num_beams = %d, V = %d, ld = %lld: needs positive counts, ld >= V", name,
                B0, num_beams, V, (long long)ld);
    P2T_REQUIRE(n_eos >= 0 && (n_eos == 0 || eos_ids), "%s: n_eos = %d: needs n_eos >= 0 and eos_ids for n_eos > 0", name, n_eos);
    P2T_REQUIRE(G > 0 && G % 64 == 0 && max_length > 0 && max_length <= G,
                "%s: G = %d, max_length = %d: needs G a positive multiple of 64 and 1 <= max_length <= G", name, G, max_length);
    P2T_REQUIRE(length_penalty == length_penalty, "%s: length_penalty is NaN", name);
    P2T_REQUIRE(early_stopping >= 0 && early_stopping <= 2, "%s: early_stopping = %d: 0 (False), 1 (True) or 2 (\"never\")", name, early_stopping);
    P2T_REQUIRE(!scores || ld_scores >= V, "%s: ld_scores = %lld < V = %d", name, (long long)ld_scores, V);
    const int64_t keep = (int64_t)(n_eos + 1 > 2 ? n_eos + 1 : 2) * num_beams;
    if (num_beams > kBeamsMax || keep > kKeepMax || V < keep || (int64_t)B0 * num_beams * V > 0x7fffffffll) {
        set_error("%s: num_beams = %d, keep = max(2, 1 + n_eos) * num_beams = %lld, V = %d, B0 = %d: supported are 1 <= num_beams <= %d, "
                  "keep <= %d, V >= keep, B0 * num_beams * V < 2^31", name, num_beams, (long long)keep, V, B0, kBeamsMax, kKeepMax);
        return P2T_ERR_UNSUPPORTED;
    }
    const int BB = B0 * num_beams;
    float* ws = state->workspace;
    *out = BeamStep{BB, (int)keep, ws, ws + 2 * (int64_t)BB * kKeepMax, reinterpret_cast<int32_t*>(ws + (int64_t)BB * kKeepMax),
                    MergeArgs{*state, step, eos_ids, next_tokens, src_rows, pad_id, B0, num_beams, V, (int)keep, n_eos, G, max_length, early_stopping,
                              length_penalty}};
    return P2T_OK;
}

}  // namespace
}  // namespace p2t
