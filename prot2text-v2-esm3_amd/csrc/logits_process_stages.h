// Stages 2 - 5 of the logits processors, shared by p2t_logits_process (logits_process.hip: on the stored logits, history = the rows'
// out_tokens) and p2t_beam_logprobs_process (beam_process.hip: on the log-probabilities, history = the beam's running sequence): HF's
// RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> NoBadWordsLogitsProcessor (SuppressTokensLogitsProcessor folded in
// as one-token words) -> MinNewTokensLengthLogitsProcessor on the f32 row y[0 .. V) of one 1024-thread block, with the history
// hist[0 .. cur).  The caller fills y first and puts a barrier in front of every stage (one block owns the row, so the block's own
// order is all that is needed).  Stages 3 - 5 only ever write -inf, stage 2 writes one value per column: whatever the thread order,
// the same inputs give the same bits.  Every column written is checked against [0, V), every history index lies in [0, cur), every
// word offset is checked against [0, n_word_ids].
#pragma once
#include "common.h"

namespace p2t {

struct ProcessorArgs {
    float penalty;
    int ngram, min_new;
    const int64_t* eos;
    int n_eos;
    const int64_t* words;
    const int32_t* offsets;
    int n_words, n_word_ids;
};

// 2. repetition penalty: thread i of the history writes y_t = x_t < 0 ? x_t * penalty : x_t / penalty with x_t = x_of(t) recomputed from
//    the SOURCE row, never read back from y, so two threads holding the same token write the same bits (no de-duplication, no atomics)
template <typename XOf>
__device__ __forceinline__ void penalty_stage(float* __restrict__ y, int V, const int64_t* __restrict__ hist, int cur, float penalty, int tid,
                                              XOf x_of) {
    if (penalty != 1.f) {
        for (int i = tid; i < cur; i += 1024) {
            const int64_t t = hist[i];
            if (t >= 0 && t < V) {
                const float x = x_of((int)t);
                y[t] = x < 0.f ? x * penalty : x / penalty;
            }
        }
    }
}

// 3. no repeated n-gram: windows i .. i + n - 1 inside the history, i <= cur - n; thread i compares history[i .. i + n - 1) with the last
//    n - 1 tokens and writes -inf at history[i + n - 1]
__device__ __forceinline__ void ngram_stage(float* __restrict__ y, int V, const int64_t* __restrict__ hist, int cur, int ngram, int tid) {
    if (ngram > 0 && cur >= ngram) {
        const int64_t* last = hist + (cur - (ngram - 1));         // the last n - 1 tokens
        for (int i = tid; i <= cur - ngram; i += 1024) {
            bool same = true;
            for (int j = 0; j < ngram - 1 && same; ++j) same = hist[i + j] == last[j];
            if (same) {
                const int64_t t = hist[i + ngram - 1];
                if (t >= 0 && t < V) y[t] = -INFINITY;
            }
        }
    }
}

// 4. bad words (a suppressed token is a word of one token): thread w compares all but the last token of word w with the end of the
//    history and writes -inf at its last token
__device__ __forceinline__ void bad_words_stage(float* __restrict__ y, int V, const int64_t* __restrict__ hist, int cur,
                                                const int64_t* __restrict__ words, const int32_t* __restrict__ offsets, int n_words,
                                                int n_word_ids, int tid) {
    for (int w = tid; w < n_words; w += 1024) {
        const int lo = offsets[w], hi = offsets[w + 1];
        if (lo < 0 || hi <= lo || hi > n_word_ids) continue;
        const int L = hi - lo;
        if (L > 1 && L > cur) continue;                           // HF: "the sequence is longer than the context, ignore"
        bool same = true;
        for (int j = 0; j < L - 1 && same; ++j) same = words[lo + j] == hist[cur - (L - 1) + j];
        if (same) {
            const int64_t t = words[hi - 1];
            if (t >= 0 && t < V) y[t] = -INFINITY;
        }
    }
}

// 5. no eos before min_new_tokens: thread e writes -inf at eos id e while cur < min_new_tokens
__device__ __forceinline__ void min_new_stage(float* __restrict__ y, int V, int cur, int min_new, const int64_t* __restrict__ eos, int n_eos,
                                              int tid) {
    if (cur < min_new) {
        for (int e = tid; e < n_eos; e += 1024) {
            const int64_t t = eos[e];
            if (t >= 0 && t < V) y[t] = -INFINITY;
        }
    }
}

// stages 2 - 5 on a filled row; block-wide (barriers inside, the first one closes the caller's fill)
template <typename XOf>
__device__ __forceinline__ void processor_stages(float* __restrict__ y, int V, const int64_t* __restrict__ hist, int cur, const ProcessorArgs& p,
                                                 int tid, XOf x_of) {
    __syncthreads();
    penalty_stage(y, V, hist, cur, p.penalty, tid, x_of);
    __syncthreads();
    ngram_stage(y, V, hist, cur, p.ngram, tid);
    __syncthreads();
    bad_words_stage(y, V, hist, cur, p.words, p.offsets, p.n_words, p.n_word_ids, tid);
    __syncthreads();
    min_new_stage(y, V, cur, p.min_new, p.eos, p.n_eos, tid);
}

// the processor settings' argument checks, alike in both entry points (P2T_ERR_ARG before any GPU call)
inline int processor_args_check(const char* name, float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens, const int64_t* eos_ids,
                                int n_eos, const int64_t* word_ids, const int32_t* word_offsets, int n_words, int n_word_ids) {
    P2T_REQUIRE(repetition_penalty > 0.f && repetition_penalty < INFINITY, "%s: repetition_penalty %g is not a positive finite number", name,
                (double)repetition_penalty);
    P2T_REQUIRE(no_repeat_ngram_size >= 0 && min_new_tokens >= 0, "%s: no_repeat_ngram_size = %d, min_new_tokens = %d: needs both >= 0 (0: off)", name,
                no_repeat_ngram_size, min_new_tokens);
    P2T_REQUIRE(n_eos >= 0 && (n_eos == 0 || eos_ids), "%s: n_eos = %d: needs n_eos >= 0, eos_ids for n_eos > 0", name, n_eos);
    P2T_REQUIRE(n_words >= 0 && n_word_ids >= 0 && (n_words == 0 || (word_ids && word_offsets && n_word_ids > 0)),
                "%s: n_words = %d, n_word_ids = %d: needs both >= 0, word_ids, word_offsets and n_word_ids > 0 for n_words > 0", name, n_words,
                n_word_ids);
    return P2T_OK;
}

}  // namespace p2t
