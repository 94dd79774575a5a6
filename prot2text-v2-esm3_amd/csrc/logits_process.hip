// Logits processors in front of the token selectors (p2t_logits_process, p2t_logits_process_rows): HF's RepetitionPenaltyLogitsProcessor ->
// NoRepeatNGramLogitsProcessor -> NoBadWordsLogitsProcessor (SuppressTokensLogitsProcessor folded in as one-token words) ->
// MinNewTokensLengthLogitsProcessor (transformers/generation/logits_process.py, in the order of GenerationMixin._get_logits_processor),
// one 1024-thread block per row.  The contract is the comment on p2t_logits_process in include/p2t_hip.h;
// tests/logits_process_reference.py restates it in numpy float32.
//
// The row's history is out_tokens[r, 0 .. cur), cur = clamp(step[0], 0, G): the tokens the selectors wrote, read on the device, so
// the launch can sit inside the captured step graph.  One body over a row model (row_model.h): LockStepRows for p2t_logits_process;
// OwnRows for p2t_logits_process_rows (continuous batching): logits row i is engine row r = row_map[i], cur = clamp(row_step[r], 0, G),
// and a finished row is left before anything is read or written (the selectors do not read its row).  The stored logits are never edited: the block writes an f32 row of its own
// and the selectors read that.
//   1. copy: y_c = float(logit_c), 16-byte loads and stores where pitch and base of both rows allow them.
//   2. penalty: thread i of the history writes y_t = x_t < 0 ? x_t * penalty : x_t / penalty with x_t read from the SOURCE row, so two
//      threads holding the same token write the same bits (no de-duplication, no atomics).
//   3. n-gram: thread i compares history[i .. i + n - 1) with the last n - 1 tokens and writes -inf at history[i + n - 1].
//   4. bad words: thread w compares all but the last token of word w with the end of the history and writes -inf at its last token.
//   5. min new tokens: thread e writes -inf at eos id e while cur < min_new_tokens.
// Stages 2 - 5 are logits_process_stages.h, shared with p2t_beam_logprobs_process (beam_process.hip).  Stages 3 - 5 only ever write
// -inf, stage 2 writes one value per column: whatever the thread order, the same inputs give the same bits.  A barrier separates the
// stages (one block owns the row, so the block's own order is all that is needed).  Every column written is checked against [0, V),
// every history index against [0, cur), every word offset against [0, n_word_ids].
#include "logits_process_stages.h"
#include "row_model.h"

namespace p2t {
namespace {

template <typename T, typename Rows>
__global__ void __launch_bounds__(1024) logits_process_kernel(const T* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ out_tokens,
                                                              int64_t ld_tok, Rows rows, const int32_t* __restrict__ finished, int G,
                                                              float* __restrict__ out, int64_t ld_out, float penalty, int ngram, int min_new,
                                                              const int64_t* __restrict__ eos, int n_eos, const int64_t* __restrict__ words,
                                                              const int32_t* __restrict__ offsets, int n_words, int n_word_ids) {
    const int bb = blockIdx.x, tid = threadIdx.x;
    const int r = rows.engine_row(bb);
    if (!rows.enter(r, finished, nullptr, 0, tid)) return;        // block-uniform; LockStepRows: never
    const T* row = logits + (int64_t)bb * ld;
    float* y = out + (int64_t)bb * ld_out;
    const int64_t* hist = out_tokens + (int64_t)r * ld_tok;
    const int cur = min(max(rows.counter(r), 0), G);

    // ---- 1. copy ----------------------------------------------------------------------------------------------------------
    constexpr int PN = sizeof(T) == 2 ? 8 : 4;
    const bool vec = ld % PN == 0 && ((uintptr_t)logits & 15u) == 0 && ld_out % 4 == 0 && ((uintptr_t)out & 15u) == 0;
    const int nvec = vec ? V / PN : 0, Vv = nvec * PN;           // 16-byte pieces of the source row
    // one block streams the whole row, so the copy is bound by load latency, not bandwidth: kUnroll loads per thread are in flight
    // before the first store (128 256 columns in bf16: 16 pieces per thread, two rounds)
    constexpr int kUnroll = 8;
    const uint4* src = reinterpret_cast<const uint4*>(row);
    for (int p0 = tid; p0 < nvec; p0 += 1024 * kUnroll) {
        uint4 t[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int p = p0 + u * 1024;
            t[u] = p < nvec ? src[p] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int p = p0 + u * 1024;
            if (p >= nvec) continue;
            float* d = y + (int64_t)p * PN;
            if constexpr (PN == 8) {                              // bf16 -> f32: the 16 bits above 16 zeros
                *reinterpret_cast<float4*>(d) = make_float4(__uint_as_float(t[u].x << 16), __uint_as_float(t[u].x & 0xFFFF0000u),
                                                            __uint_as_float(t[u].y << 16), __uint_as_float(t[u].y & 0xFFFF0000u));
                *reinterpret_cast<float4*>(d + 4) = make_float4(__uint_as_float(t[u].z << 16), __uint_as_float(t[u].z & 0xFFFF0000u),
                                                                __uint_as_float(t[u].w << 16), __uint_as_float(t[u].w & 0xFFFF0000u));
            } else {
                *reinterpret_cast<uint4*>(d) = t[u];
            }
        }
    }
    for (int c = Vv + tid; c < V; c += 1024) y[c] = to_f32(row[c]);

    // ---- 2 - 5. penalty (x_t the STORED logit), n-gram, bad words, min new tokens: logits_process_stages.h -----------------------------
    const ProcessorArgs p{penalty, ngram, min_new, eos, n_eos, words, offsets, n_words, n_word_ids};
    processor_stages(y, V, hist, cur, p, tid, [&](int t) { return to_f32(row[t]); });
}

}  // namespace
}  // namespace p2t

using namespace p2t;

// one block per logits row over the row model
template <typename Rows>
static void launch_process(const void* logits, int dtype, int64_t ld, int V, int n, const int64_t* out_tokens, int64_t ld_tokens, Rows rows,
                           const int32_t* finished, int G, float* out, int64_t ld_out, float penalty, int ngram, int min_new, const int64_t* eos_ids, int n_eos,
                           const int64_t* word_ids, const int32_t* word_offsets, int n_words, int n_word_ids, hipStream_t s) {
    if (dtype == P2T_BF16)
        logits_process_kernel<bf16_t, Rows><<<n, 1024, 0, s>>>((const bf16_t*)logits, ld, V, out_tokens, ld_tokens, rows, finished, G, out, ld_out, penalty, ngram,
                                                               min_new, eos_ids, n_eos, word_ids, word_offsets, n_words, n_word_ids);
    else
        logits_process_kernel<float, Rows><<<n, 1024, 0, s>>>((const float*)logits, ld, V, out_tokens, ld_tokens, rows, finished, G, out, ld_out, penalty, ngram,
                                                              min_new, eos_ids, n_eos, word_ids, word_offsets, n_words, n_word_ids);
}

extern "C" int p2t_logits_process(const void* logits, int dtype, int64_t ld, int V, int BB, const int64_t* out_tokens, int64_t ld_tokens,
                                  const int32_t* step, int G, float* out, int64_t ld_out, float repetition_penalty, int no_repeat_ngram_size,
                                  int min_new_tokens, const int64_t* eos_ids, int n_eos, const int64_t* word_ids, const int32_t* word_offsets,
                                  int n_words, int n_word_ids, p2t_stream stream) {
    P2T_REQUIRE(logits && out_tokens && step && out, "p2t_logits_process: null argument");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_logits_process: dtype %d is neither P2T_F32 nor P2T_BF16", dtype);
    P2T_REQUIRE(BB > 0 && V > 0 && ld >= V && ld_out >= V,
                "p2t_logits_process: BB = %d, V = %d, ld = %lld, ld_out = %lld: needs BB > 0, V > 0, ld >= V, ld_out >= V", BB, V, (long long)ld,
                (long long)ld_out);
    P2T_REQUIRE(G > 0 && ld_tokens >= G, "p2t_logits_process: G = %d, ld_tokens = %lld: needs G > 0, ld_tokens >= G", G, (long long)ld_tokens);
    P2T_TRY(processor_args_check("p2t_logits_process", repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_ids, n_eos, word_ids, word_offsets,
                                 n_words, n_word_ids));
    launch_process(logits, dtype, ld, V, BB, out_tokens, ld_tokens, LockStepRows{step, 0}, nullptr, G, out, ld_out, repetition_penalty, no_repeat_ngram_size,
                   min_new_tokens, eos_ids, n_eos, word_ids, word_offsets, n_words, n_word_ids, (hipStream_t)stream);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_logits_process_rows(const void* logits, int dtype, int64_t ld, int V, int n, const int64_t* out_tokens, int64_t ld_tokens,
                                       const int32_t* row_step, const int32_t* row_map, const int32_t* finished, int BB, int G, float* out,
                                       int64_t ld_out, float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens, const int64_t* eos_ids,
                                       int n_eos, const int64_t* word_ids, const int32_t* word_offsets, int n_words, int n_word_ids, p2t_stream stream) {
    P2T_REQUIRE(logits && out_tokens && row_step && out, "p2t_logits_process_rows: null argument");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_logits_process_rows: dtype %d is neither P2T_F32 nor P2T_BF16", dtype);
    P2T_REQUIRE(n > 0 && BB > 0 && n <= BB && (row_map || n == BB),
                "p2t_logits_process_rows: %d logits rows for %d engine rows (all of them, or a row_map subset)", n, BB);
    P2T_REQUIRE(V > 0 && ld >= V && ld_out >= V, "p2t_logits_process_rows: V = %d, ld = %lld, ld_out = %lld: needs V > 0, ld >= V, ld_out >= V", V,
                (long long)ld, (long long)ld_out);
    P2T_REQUIRE(G > 0 && ld_tokens >= G, "p2t_logits_process_rows: G = %d, ld_tokens = %lld: needs G > 0, ld_tokens >= G", G, (long long)ld_tokens);
    P2T_TRY(processor_args_check("p2t_logits_process_rows", repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_ids, n_eos, word_ids, word_offsets,
                                 n_words, n_word_ids));
    launch_process(logits, dtype, ld, V, n, out_tokens, ld_tokens, OwnRows{row_step, nullptr, row_map, nullptr, BB}, finished, G, out, ld_out,
                   repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_ids, n_eos, word_ids, word_offsets, n_words, n_word_ids, (hipStream_t)stream);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
