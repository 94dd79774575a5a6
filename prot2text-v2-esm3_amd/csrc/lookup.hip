// Prompt-lookup decoding (include/p2t_hip.h "prompt-lookup decoding"): the two small kernels around p2t_llama_decode_step_multi.
//   * p2t_lookup_draft_rows: a row's next k tokens guessed from its own generated text -- HF's PromptLookupCandidateGenerator: the
//     longest trailing n-gram (n down to 1) that occurs earlier, at its EARLIEST occurrence with a non-empty continuation;
//   * p2t_lookup_verify_rows: the model's greedy token behind each of the step's Q = k + 1 tokens, the longest agreeing prefix of the
//     draft, the new tokens' bookkeeping in greedy_select_rows_kernel's terms (eos bit 1, limit bit 2) and the row's counter.
// Both read every length on the device and enqueue only: they sit inside the replayed step graph.
#include "common.h"
#include "greedy_argmax.h"
#include "kernels.h"

namespace p2t {
namespace {

constexpr int kDraftThreads = 256, kNoMatch = 0x7fffffff;

// One block per row.  History h[0 .. s] = out_tokens[r, 0 .. s], s = row_step[r]; h[s] is the token chosen last and the step's token 0.
__global__ void __launch_bounds__(kDraftThreads) lookup_draft_rows_kernel(const int64_t* __restrict__ out_tokens, int64_t ld_tok,
                                                                          const int32_t* __restrict__ row_step, const int32_t* __restrict__ finished,
                                                                          int Gcap, int k, int ngram, int64_t pad, int64_t* __restrict__ step_tokens,
                                                                          int32_t* __restrict__ draft_len) {
    __shared__ int first;
    const int r = blockIdx.x, Q = k + 1, tid = threadIdx.x;
    const int64_t* h = out_tokens + (int64_t)r * ld_tok;
    int64_t* dst = step_tokens + (int64_t)r * Q;
    if (finished[r]) {                                   // the whole block: a finished row feeds pads and drafts nothing
        if (tid < Q) dst[tid] = pad;
        if (tid == 0) draft_len[r] = 0;
        return;
    }
    const int s = min(max(row_step[r], 0), Gcap - 1);
    int start = 0, c = 0;                                // the continuation h[start .. start + c)
    for (int m = min(ngram, s); m >= 1; --m) {
        if (tid == 0) first = kNoMatch;
        __syncthreads();
        // a match at i <= s - m leaves at least h[i + m] to continue with; i = s - m + 1 is the suffix itself
        for (int i = tid; i + m <= s; i += kDraftThreads) {
            bool eq = true;
            for (int e = 0; e < m; ++e) eq = eq && h[i + e] == h[s - m + 1 + e];
            if (eq) { atomicMin(&first, i); break; }     // ascending i per thread: its later matches cannot be earlier
        }
        __syncthreads();
        const int f = first;
        __syncthreads();                                 // every thread has read `first` before the next round resets it
        if (f != kNoMatch) {
            start = f + m;
            c = min(k, s + 1 - start);
            break;
        }
    }
    if (tid < Q) dst[tid] = tid == 0 ? h[s] : (tid <= c ? h[start + tid - 1] : pad);
    if (tid == 0) draft_len[r] = c;
}

// the greedy token of every logits row (BB * Q blocks of 1024 threads), p2t_greedy_select's tie rule
template <typename T>
__global__ void __launch_bounds__(1024) lookup_argmax_kernel(const T* __restrict__ logits, int64_t ld, int V, int32_t* __restrict__ choice) {
    const int idx = greedy_argmax<T>(logits + (int64_t)blockIdx.x * ld, ld, V);
    if (threadIdx.x == 0) choice[blockIdx.x] = idx;
}

// One thread per row: choice[r, j] is the model's token behind the step's token j.  A finished row writes nothing but its pad.
__global__ void __launch_bounds__(64) lookup_verify_tail_kernel(const int32_t* __restrict__ choice, const int64_t* __restrict__ step_tokens,
                                                                const int32_t* __restrict__ draft_len, int BB, int Q,
                                                                const int64_t* __restrict__ eos, int n_eos, int64_t pad,
                                                                int32_t* __restrict__ finished, int64_t* __restrict__ next,
                                                                int64_t* __restrict__ out_tokens, int64_t ld_tok, int32_t* __restrict__ row_step,
                                                                const int32_t* __restrict__ row_limit, int Gcap, int32_t* __restrict__ stats) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= BB) return;
    if (finished[r]) { next[r] = pad; return; }
    const int s = min(max(row_step[r], 0), Gcap - 1), c = min(max(draft_len[r], 0), Q - 1);
    const int limit = min(max(row_limit[r], 1), Gcap);
    // the draft tokens the model agrees with: g_a decides t_(a + 1) and is itself token s + a + 1 -- one behind the limit decides nothing
    int a = 0;
    while (a < c && s + a + 1 < limit && (int64_t)choice[r * Q + a] == step_tokens[(int64_t)r * Q + a + 1]) ++a;
    int n_new = 0, fin = 0;
    int64_t last = pad;
    for (int j = 0; j <= a && !fin; ++j) {               // g_0 .. g_a, cut behind the first eos and at the row's limit
        const int idx = s + 1 + j;
        if (idx >= limit) { fin |= 2; break; }           // (a live row has s + 1 < limit: never at j = 0)
        last = choice[r * Q + j];
        out_tokens[(int64_t)r * ld_tok + idx] = last;
        ++n_new;
        for (int e = 0; e < n_eos; ++e)
            if (last == eos[e]) fin |= 1;
        if (idx + 1 >= limit) fin |= 2;
    }
    row_step[r] = s + n_new;
    next[r] = last;
    if (fin) finished[r] |= fin;
    stats[3 * r] += 1;                                   // verify steps, drafted tokens, accepted tokens (a: before the eos / limit cut)
    stats[3 * r + 1] += c;
    stats[3 * r + 2] += a;
}

}  // namespace
}  // namespace p2t

using namespace p2t;

extern "C" int p2t_lookup_draft_rows(const int64_t* out_tokens, int64_t ld_tokens, const int32_t* row_step, const int32_t* finished, int BB, int G,
                                     int num_tokens, int max_ngram, int64_t pad_id, int64_t* step_tokens, int32_t* draft_len, p2t_stream stream) {
    P2T_REQUIRE(out_tokens && row_step && finished && step_tokens && draft_len, "p2t_lookup_draft_rows: null argument");
    P2T_REQUIRE(BB > 0 && G > 0 && ld_tokens >= G, "p2t_lookup_draft_rows: bad shape arguments (BB %d, G %d, ld_tokens %lld)", BB, G, (long long)ld_tokens);
    P2T_REQUIRE(num_tokens >= 1 && num_tokens <= 7, "p2t_lookup_draft_rows: num_tokens %d outside 1 .. 7", num_tokens);
    P2T_REQUIRE(max_ngram >= 1 && max_ngram <= 4, "p2t_lookup_draft_rows: max_ngram %d outside 1 .. 4", max_ngram);
    lookup_draft_rows_kernel<<<BB, kDraftThreads, 0, (hipStream_t)stream>>>(out_tokens, ld_tokens, row_step, finished, G, num_tokens, max_ngram, pad_id,
                                                                            step_tokens, draft_len);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_lookup_verify_rows(const void* logits, int dtype, int64_t ld, int V, int BB, int q_tokens, const int64_t* step_tokens,
                                      const int32_t* draft_len, const int64_t* eos_ids, int n_eos, int64_t pad_id, int32_t* finished,
                                      int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, int32_t* row_step, const int32_t* row_limit, int G,
                                      int32_t* stats, int32_t* choice, p2t_stream stream) {
    P2T_REQUIRE(logits && step_tokens && draft_len && finished && next_tokens && out_tokens && row_step && row_limit && stats && choice,
                "p2t_lookup_verify_rows: null argument");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_lookup_verify_rows: logits are f32 or bf16 (got dtype %d)", dtype);
    P2T_REQUIRE(q_tokens >= 2 && q_tokens <= 8, "p2t_lookup_verify_rows: q_tokens %d outside 2 .. 8", q_tokens);
    P2T_REQUIRE(BB > 0 && V > 0 && ld >= V && G > 0 && ld_tokens >= G && n_eos >= 0 && (n_eos == 0 || eos_ids), "p2t_lookup_verify_rows: bad shape arguments");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == P2T_BF16) lookup_argmax_kernel<bf16_t><<<BB * q_tokens, 1024, 0, s>>>((const bf16_t*)logits, ld, V, choice);
    else lookup_argmax_kernel<float><<<BB * q_tokens, 1024, 0, s>>>((const float*)logits, ld, V, choice);
    P2T_LAUNCH_CHECK();
    lookup_verify_tail_kernel<<<(unsigned)ceil_div(BB, 64), 64, 0, s>>>(choice, step_tokens, draft_len, BB, q_tokens, eos_ids, n_eos, pad_id, finished,
                                                                        next_tokens, out_tokens, ld_tokens, row_step, row_limit, G, stats);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
