// Logits processors under beam search (p2t_beam_logprobs_process): HF's `_beam_search` takes the log-softmax of the step's logits and
// runs the processors on THAT, with the beam's running sequence as the history (transformers 5.15, generation/utils.py); the
// processed rows are what the search then ranks (p2t_beam_select_logprobs, beam_select.hip) and what it returns as the step's
// scores.  The contract is the comment on p2t_beam_logprobs_process in include/p2t_hip.h; tests/logits_process_reference.py on the
// `scores` rows of p2t_beam_select restates it.  One 1024-thread block per row (beam):
//   1. mx = the row maximum (every thread's largest key, a block reduction: exact), lse = row_lse (select_common.h): step 1 of
//      p2t_beam_select with its summation order, so lp_c = (x_c - mx) - lse has the bits p2t_beam_select(scores=) writes.  The row is
//      written as f32, 16-byte loads and stores where pitch and base of both rows allow them.
//   2 - 5. logits_process_stages.h on that row with the history run_seq[cur & 1][row][0 .. cur), cur = step[0]: the half is chosen on the
//      device, since a captured graph holds two steps of different parities.  The penalty's x_t is recomputed from the stored logit as
//      (float(logit_t) - mx) - lse, never read back from the row: duplicates in the history write the same bits.
// done[0] set or cur outside [0, max_length): nothing is written (beam_rows_kernel's early return).  Every column written is checked
// against [0, V); cur < max_length <= G bounds every history index; every word offset is checked against [0, n_word_ids].
#include "beam_merge.h"
#include "logits_process_stages.h"
#include "select_common.h"

namespace p2t {
namespace {

template <typename T>
__global__ void __launch_bounds__(1024) beam_logprobs_kernel(const T* __restrict__ logits, int64_t ld, int V, int max_length, int G, int64_t tab,
                                                             const int32_t* __restrict__ step_ptr, const int32_t* __restrict__ done,
                                                             const int64_t* __restrict__ run_seq, float* __restrict__ lp, int64_t ld_lp,
                                                             ProcessorArgs p) {
    __shared__ uint32_t s_key[16];
    __shared__ float s_sum[16];
    const int cur = step_ptr[0];
    if (done[0] != 0 || cur < 0 || cur >= max_length) return;              // block-uniform
    const int bb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const T* row = logits + (int64_t)bb * ld;
    float* y = lp + (int64_t)bb * ld_lp;
    const int64_t* hist = run_seq + (int64_t)(cur & 1) * tab + (int64_t)bb * G;      // cur < max_length <= G columns of it are read

    // ---- 1. mx, lse: the loads of beam_rows_kernel (same `vec`), so the same summation order ------------------------------------
    constexpr int PN = sizeof(T) == 2 ? 8 : 4;
    const bool vec = ld % PN == 0 && ((uintptr_t)logits & 15u) == 0;
    uint32_t key = thread_max_key(row, V, vec, tid);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, 64));
    if (lane == 0) s_key[w] = key;
    __syncthreads();
    key = s_key[0];
#pragma unroll
    for (int ww = 1; ww < 16; ++ww) key = max(key, s_key[ww]);
    const float mx = key_value(key);
    const float lse = row_lse(row, V, vec, mx, s_sum);

    // ---- the row of log-probabilities -------------------------------------------------------------------------------------------
    const bool vst = vec && ld_lp % 4 == 0 && ((uintptr_t)lp & 15u) == 0;
    const int nvec = vst ? V / PN : 0, Vv = nvec * PN;          // 16-byte pieces of the source row
    // one block streams the whole row, so the pass is bound by load latency, not bandwidth: kUnroll loads per thread are in flight
    // before the first store (128 256 columns in bf16: 16 pieces per thread, two rounds)
    constexpr int kUnroll = 8;
    const uint4* src = reinterpret_cast<const uint4*>(row);
    for (int p0 = tid; p0 < nvec; p0 += 1024 * kUnroll) {
        uint4 t[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int q = p0 + u * 1024;
            t[u] = q < nvec ? src[q] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int q = p0 + u * 1024;
            if (q >= nvec) continue;
            float* d = y + (int64_t)q * PN;
            const uint32_t r[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
            if constexpr (PN == 8) {                              // bf16 -> f32: the 16 bits above 16 zeros
                float v[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[2 * e] = (__uint_as_float(r[e] << 16) - mx) - lse;
                    v[2 * e + 1] = (__uint_as_float(r[e] & 0xFFFF0000u) - mx) - lse;
                }
                *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
            } else {
                *reinterpret_cast<float4*>(d) = make_float4((__uint_as_float(r[0]) - mx) - lse, (__uint_as_float(r[1]) - mx) - lse,
                                                            (__uint_as_float(r[2]) - mx) - lse, (__uint_as_float(r[3]) - mx) - lse);
            }
        }
    }
    for (int c = Vv + tid; c < V; c += 1024) y[c] = (to_f32(row[c]) - mx) - lse;

    // ---- 2 - 5. the processors on the log-probabilities ---------------------------------------------------------------------------
    processor_stages(y, V, hist, cur, p, tid, [&](int t) { return (to_f32(row[t]) - mx) - lse; });
}

}  // namespace
}  // namespace p2t

using namespace p2t;

extern "C" int p2t_beam_logprobs_process(const void* logits, int dtype, int64_t ld, int B0, int num_beams, int V, const int32_t* step, int G,
                                         int max_length, const p2t_beam_state* state, float repetition_penalty, int no_repeat_ngram_size,
                                         int min_new_tokens, const int64_t* eos_ids, int n_eos, const int64_t* word_ids, const int32_t* word_offsets,
                                         int n_words, int n_word_ids, float* lp, int64_t ld_lp, p2t_stream stream) {
    const char* name = "p2t_beam_logprobs_process";
    P2T_REQUIRE(logits && step && state && lp, "%s: null argument", name);
    P2T_REQUIRE(state->run_seq && state->done, "%s: null pointer in the state (run_seq and done are read)", name);
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "%s: dtype %d is neither P2T_F32 nor P2T_BF16", name, dtype);
    P2T_REQUIRE(B0 > 0 && num_beams > 0 && V > 0 && ld >= V && ld_lp >= V,
                "%s: B0 = %d, num_beams = %d, V = %d, ld = %lld, ld_lp = %lld: needs positive counts, ld >= V, ld_lp >= V", name, B0, num_beams, V,
                (long long)ld, (long long)ld_lp);
    P2T_REQUIRE(G > 0 && G % 64 == 0 && max_length > 0 && max_length <= G,
                "%s: G = %d, max_length = %d: needs G a positive multiple of 64 and 1 <= max_length <= G", name, G, max_length);
    P2T_TRY(processor_args_check(name, repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_ids, n_eos, word_ids, word_offsets, n_words,
                                 n_word_ids));
    if (num_beams > kBeamsMax || (int64_t)B0 * num_beams * V > 0x7fffffffll) {
        set_error("%s: num_beams = %d, V = %d, B0 = %d: supported are 1 <= num_beams <= %d, B0 * num_beams * V < 2^31", name, num_beams, V, B0,
                  kBeamsMax);
        return P2T_ERR_UNSUPPORTED;
    }
    const int BB = B0 * num_beams;
    const int64_t tab = (int64_t)BB * G;                          // one half of run_seq
    const ProcessorArgs p{repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_ids, n_eos, word_ids, word_offsets, n_words, n_word_ids};
    hipStream_t s = (hipStream_t)stream;
    if (dtype == P2T_BF16)
        beam_logprobs_kernel<bf16_t><<<BB, 1024, 0, s>>>((const bf16_t*)logits, ld, V, max_length, G, tab, step, state->done, state->run_seq, lp, ld_lp,
                                                         p);
    else
        beam_logprobs_kernel<float><<<BB, 1024, 0, s>>>((const float*)logits, ld, V, max_length, G, tab, step, state->done, state->run_seq, lp, ld_lp, p);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
