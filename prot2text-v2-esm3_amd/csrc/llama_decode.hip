// Generation with a KV cache: what `llama_decoder.generate(inputs_embeds=..., attention_mask=...)` runs under
// Esm2LlamaInstructForCausalLM.generate (reference models/modeling_esm2llama_instruct.py:217-251; HF GenerationMixin + the cached
// LlamaAttention path, transformers/models/llama/modeling_llama.py).  This file: the prefill doors, the decode step, the quantised LM
// head and the greedy selectors.  The cache's layout and maintenance are kv_cache.hip, the step's attention attn_decode.hip.
//
// Where a step appends and how far it attends is counted on the device:
//   * every row generates in lock-step: ONE device counter `step` = generated tokens already in the cache.  A decode step reads it on
//     the device (so the whole step replays as a HIP graph without a host round trip), appends at index `step`, attends to
//     prompt_len[b0] + step + 1 keys and increments it last;
//   * opt-in (continuous batching, p2t_llama_decode_step_rows; group == 1): every row carries its OWN counter, row_step[row], beside the
//     cache -- the same kernels read step[row * stride] with stride 1 where the lock-step entry points pass stride 0.  A finished row
//     is frozen (it re-appends at its own index and does not advance).
#include "common.h"
#include "greedy_argmax.h"
#include "kernels.h"

namespace p2t {
namespace {

// last valid row of every prompt: out[b] = x[b, len[b] - 1]
__global__ void __launch_bounds__(256) gather_last_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int T, int H,
                                                          float* __restrict__ out) {
    const int b = blockIdx.x;
    const int t = max(0, min(T, lens[b]) - 1);
    const float* s = x + ((int64_t)b * T + t) * H;
    for (int c = threadIdx.x; c < H; c += 256) out[(int64_t)b * H + c] = s[c];
}

// ---------------------------------------------------------------------------------------------
// one new token per row: rotation at its position + append to the generated segment
// ---------------------------------------------------------------------------------------------
// One wave per (row, head slot): lane j < d/2 holds the rotary pair (j, j + d/2).  qkv: the f32 result of the QKV projection in the
// ROW ORDER OF qkv_w (for head_dim 128 without q/k norm: the packed order of p2t_llama_layer).  `round_first`: the prefill of this
// model rounds the projection to the model dtype before the rotation (its unfused path), so the step does too.
template <typename T>
__global__ void __launch_bounds__(256) rope_append_kernel(const float* __restrict__ qkv, int64_t ldq, const float* __restrict__ inv_freq,
                                                          const float* __restrict__ qw, const float* __restrict__ kw, float eps,
                                                          const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ step_ptr,
                                                          int step_stride, int group, T* __restrict__ qbuf, T* __restrict__ kg, T* __restrict__ vtg, int BB,
                                                          int nh, int nkv, int d, int dp, int G, float q_scale, int packed128,
                                                          int round_first, int q_tokens) {
    const int lane = threadIdx.x & 63, heads = nh + 2 * nkv, half = d / 2;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= BB * heads) return;
    // m: the projection's row (BB of them); bb: its cache row -- several tokens per row: token m % q_tokens of row m / q_tokens
    const int m = row / heads, hh = row - m * heads, bb = q_tokens > 1 ? m / q_tokens : m;
    // stride 0: the shared counter, 1: row bb's own (+ the token's place among the row's new ones)
    const int step = min(max(step_ptr[(int64_t)bb * step_stride], 0) + (m - bb * q_tokens), G - 1);
    const int pos = prompt_len[bb / group] + step;
    const float* src = qkv + (int64_t)m * ldq + (int64_t)hh * d;
    auto at = [&](int j) {
        int p = j;
        if (packed128) { const int blk = j >> 5; p = blk == 1 ? j + 32 : (blk == 2 ? j - 32 : j); }
        const float v = src[p];
        return round_first ? to_f32(from_f32<T>(v)) : v;
    };
    float x1 = 0.f, x2 = 0.f;
    if (lane < half) { x1 = at(lane); x2 = at(lane + half); }
    if (hh < nh + nkv) {
        const bool is_q = hh < nh;
        const float qs = is_q ? q_scale : 1.0f;
        float c = 1.f, s = 0.f;
        if (lane < half) {
            const float a = __fmul_rn((float)pos, inv_freq[lane]);
            c = cosf(a);
            s = sinf(a);
        }
        float o1, o2;
        if (qw) {                                   // Qwen3: RMSNorm over the head, rotation, then the folded scale (qk_norm_rope_kernel)
            const float* w = is_q ? qw : kw;
            const float ss = wave_sum(x1 * x1 + x2 * x2);
            const float rstd = rsqrtf(ss / (float)d + eps);
            const float a1 = lane < half ? w[lane] * (x1 * rstd) : 0.f, a2 = lane < half ? w[lane + half] * (x2 * rstd) : 0.f;
            o1 = (a1 * c - a2 * s) * qs;
            o2 = (a2 * c + a1 * s) * qs;
        } else {                                    // scale first, then the rotation (the QKV + RoPE epilogue / qkv_post_kernel)
            const float a1 = x1 * qs, a2 = x2 * qs;
            o1 = a1 * c - a2 * s;
            o2 = a2 * c + a1 * s;
        }
        T* dst = is_q ? qbuf + ((int64_t)m * nh + hh) * dp : kg + (((int64_t)bb * nkv + (hh - nh)) * G + step) * dp;
        if (lane < half) { dst[lane] = from_f32<T>(o1); dst[lane + half] = from_f32<T>(o2); }
        for (int cc = d + lane; cc < dp; cc += 64) dst[cc] = from_f32<T>(0.f);
    } else {
        T* dst = vtg + ((int64_t)bb * nkv + (hh - nh - nkv)) * dp * G + step;
        if (lane < half) { dst[(int64_t)lane * G] = from_f32<T>(x1); dst[(int64_t)(lane + half) * G] = from_f32<T>(x2); }
        for (int cc = d + lane; cc < dp; cc += 64) dst[(int64_t)cc * G] = from_f32<T>(0.f);
    }
}

// ---------------------------------------------------------------------------------------------
// token selection (greedy) and step bookkeeping
// ---------------------------------------------------------------------------------------------
// torch.argmax semantics over the first V columns (lowest index among equal maxima), then HF's finished-row rule
// (generation/utils.py, _sample: next = next * unfinished + pad * (1 - unfinished); a row finishes once it emits an eos id).
template <typename T>
__global__ void __launch_bounds__(1024) greedy_select_kernel(const T* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ eos,
                                                             int n_eos, int64_t pad, int32_t* __restrict__ finished,
                                                             int64_t* __restrict__ next, int64_t* __restrict__ out_tokens, int64_t ld_tok,
                                                             const int32_t* __restrict__ step_ptr, int Gcap) {
    const int bb = blockIdx.x;
    const int idx = greedy_argmax<T>(logits + (int64_t)bb * ld, ld, V);
    if (threadIdx.x == 0) {
        int64_t tok = idx;
        const int fin = finished[bb];
        if (fin) tok = pad;
        next[bb] = tok;
        const int st = min(max(step_ptr[0], 0), Gcap - 1);
        out_tokens[(int64_t)bb * ld_tok + st] = tok;
        if (!fin) {
            for (int e = 0; e < n_eos; ++e)
                if (tok == eos[e]) finished[bb] = 1;
        }
    }
}

// The greedy choice of rows that carry their OWN counters (continuous batching): logits row blockIdx.x belongs to engine row
// row_map[blockIdx.x] (nullptr: itself).  A finished row emits pad and writes no token -- its counter no longer moves, and the token
// at it is its last one; a live row writes its token at its own index and picks up the eos bit (1) and the limit bit (2).
template <typename T>
__global__ void __launch_bounds__(1024) greedy_select_rows_kernel(const T* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ eos,
                                                                  int n_eos, int64_t pad, int32_t* __restrict__ finished,
                                                                  int64_t* __restrict__ next, int64_t* __restrict__ out_tokens, int64_t ld_tok,
                                                                  const int32_t* __restrict__ row_step, const int32_t* __restrict__ row_limit,
                                                                  const int32_t* __restrict__ row_map, int BB, int Gcap) {
    const int r = row_map ? row_map[blockIdx.x] : (int)blockIdx.x;
    if (r < 0 || r >= BB) return;                        // the whole block: a row the engine does not have touches nothing
    const int idx = greedy_argmax<T>(logits + (int64_t)blockIdx.x * ld, ld, V);
    if (threadIdx.x == 0) {
        if (finished[r]) { next[r] = pad; return; }
        const int64_t tok = idx;
        const int st = min(max(row_step[r], 0), Gcap - 1);
        next[r] = tok;
        out_tokens[(int64_t)r * ld_tok + st] = tok;
        int fin = 0;
        for (int e = 0; e < n_eos; ++e)
            if (tok == eos[e]) fin |= 1;
        if (st + 1 >= min(max(row_limit[r], 1), Gcap)) fin |= 2;
        if (fin) finished[r] |= fin;
    }
}

// n counters `stride` apart (lock-step: ONE, <<<1, 1>>>; per-row counters: BB at stride 1); a frozen row keeps its own
__global__ void advance_kernel(int32_t* step, int stride, const int32_t* __restrict__ frozen, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !(frozen && frozen[i])) step[(int64_t)i * stride] += 1;
}

struct DecodeBuffers {
    float* x; void* h; float* qkv; void* qb; void* ao; void* act; float* inv_freq;
    uint8_t* hq; uint8_t* hs; uint8_t* aoq; uint8_t* aos; uint8_t* actq; uint8_t* acts;      // gemm_fp8: e4m3 rows + their E8M0 scales
};

size_t decode_plan(const p2t_llama_config* c, int BB, int Tp, int Gcap, Arena* ar, DecodeBuffers* b) {
    const size_t e = dtype_size(c->dtype);
    const int64_t H = c->hidden, F = c->ffn, Hp = round_up(H, 64), Fp = round_up(F, 64);
    const int d = c->head_dim, dp = head_dim_padded(d), nh = c->heads, nkv = c->kv_heads;
    const int64_t QO = round_up((int64_t)nh * d, 64), NQKV = (int64_t)(nh + 2 * nkv) * d;
    Arena local(nullptr, ~(size_t)0 >> 1);
    Arena& a = ar ? *ar : local;
    DecodeBuffers t;
    t.x = (float*)a.take(sizeof(float) * (size_t)BB * H);
    t.h = a.take(e * (size_t)BB * Hp);
    t.qkv = (float*)a.take(sizeof(float) * (size_t)BB * NQKV);
    t.qb = a.take(e * (size_t)BB * nh * dp);
    t.ao = a.take(e * (size_t)BB * QO);
    t.act = a.take(e * (size_t)BB * Fp);
    t.inv_freq = (float*)a.take(sizeof(float) * (d / 2 + 1));
    t.hq = t.hs = t.aoq = t.aos = t.actq = t.acts = nullptr;
    if (c->gemm_fp8) {
        const int64_t Hq = round_up(H, 128), Fq = round_up(F, 128), QOq = round_up((int64_t)nh * d, 128);
        t.hq = (uint8_t*)a.take((size_t)BB * Hq);    t.hs = (uint8_t*)a.take((size_t)BB);
        t.aoq = (uint8_t*)a.take((size_t)BB * QOq);  t.aos = (uint8_t*)a.take((size_t)BB);
        t.actq = (uint8_t*)a.take((size_t)BB * Fq);  t.acts = (uint8_t*)a.take((size_t)BB);
    }
    if (b) *b = t;
    return a.off + 256;
}

// the two-launch form's second launch: rotation + cache append of the f32 projection `qkv`, to where `ra` points (model dtype `dt`)
template <typename T>
void rope_append_t(const float* qkv, int64_t ldq, const SkinnyRope& ra, const p2t_llama_layer& L, float eps, int BB, int dp, int round_first,
                   hipStream_t s) {
    const unsigned grid = (unsigned)ceil_div((int64_t)BB * (ra.nh + 2 * ra.nkv), 4);
    rope_append_kernel<T><<<grid, 256, 0, s>>>(qkv, ldq, ra.inv_freq, L.q_norm_w, L.k_norm_w, eps, ra.prompt_len, ra.step, ra.step_stride, ra.group, (T*)ra.q,
                                               (T*)ra.k, (T*)ra.vt, BB, ra.nh, ra.nkv, ra.d, dp, ra.G, ra.q_scale, ra.d == 128 && !L.q_norm_w, round_first,
                                               ra.q_tokens);
}
int launch_rope_append(const float* qkv, int64_t ldq, const SkinnyRope& ra, const p2t_llama_layer& L, float eps, int BB, int dp, int round_first, int dt,
                       hipStream_t s) {
    if (dt == P2T_BF16) rope_append_t<bf16_t>(qkv, ldq, ra, L, eps, BB, dp, round_first, s);
    else rope_append_t<float>(qkv, ldq, ra, L, eps, BB, dp, round_first, s);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

}  // namespace
}  // namespace p2t

using namespace p2t;

extern "C" size_t p2t_llama_prefill_workspace_bytes(const p2t_llama_config* cfg, int B, int T) {
    if (!cfg || B <= 0 || T <= 0) return 0;
    return p2t_llama_workspace_bytes(cfg, B, T) + sizeof(float) * (size_t)B * T * cfg->hidden + 512;
}

extern "C" int p2t_llama_prefill(const p2t_llama_config* c, const p2t_llama_weights* w, const float* inputs_embeds, const int64_t* mask, int B,
                                 int T, const p2t_kv_cache* cache, float* last_hidden, void* workspace, size_t workspace_bytes,
                                 p2t_stream stream) {
    P2T_REQUIRE(c && w && inputs_embeds && mask && last_hidden && workspace && B > 0 && T > 0, "p2t_llama_prefill: null/empty argument");
    P2T_TRY(check_cache(c, cache, "p2t_llama_prefill"));
    P2T_REQUIRE(cache->B0 == B && T <= cache->Tp, "p2t_llama_prefill: cache holds %d rows x %d tokens, the prompt batch is %d x %d", cache->B0,
                cache->Tp, B, T);
    P2T_REQUIRE(workspace_bytes >= p2t_llama_prefill_workspace_bytes(c, B, T), "p2t_llama_prefill: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Arena ar(workspace, workspace_bytes);
    float* out = (float*)ar.take(sizeof(float) * (size_t)B * T * c->hidden);
    void* rest = ar.take(p2t_llama_workspace_bytes(c, B, T));
    P2T_REQUIRE(!ar.overflow, "p2t_llama_prefill: workspace overflow");
    P2T_TRY(llama_forward_impl(c, w, nullptr, inputs_embeds, mask, B, T, c->n_layers, out, rest, p2t_llama_workspace_bytes(c, B, T), stream, nullptr,
                               cache));
    gather_last_kernel<<<B, 256, 0, s>>>(out, cache->prompt_len, T, c->hidden, last_hidden);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" size_t p2t_llama_prefill_packed_workspace_bytes(const p2t_llama_config* cfg, int R, int Tpk) {
    return p2t_llama_prefill_workspace_bytes(cfg, R, Tpk);
}

// p2t_llama_prefill over packed rows: the same layers on R x Tpk tokens, attention and rotation confined per prompt by docs, the keys and
// values scattered to each prompt's cache row.  Every refusal stands in front of the first launch.
extern "C" int p2t_llama_prefill_packed(const p2t_llama_config* c, const p2t_llama_weights* w, const float* inputs_embeds, const int64_t* mask,
                                        const int32_t* docs, int R, int Tpk, int n, const int32_t* place, const p2t_kv_cache* cache, float* last_hidden,
                                        void* workspace, size_t workspace_bytes, p2t_stream stream) {
    P2T_REQUIRE(c && w && inputs_embeds && mask && docs && place && last_hidden && workspace && R > 0 && Tpk > 0 && n > 0,
                "p2t_llama_prefill_packed: null/empty argument");
    P2T_TRY(check_cache(c, cache, "p2t_llama_prefill_packed"));
    if (c->gemm_fp8) {
        set_error("p2t_llama_prefill_packed: the packed prefill runs the model-dtype GEMMs; gemm_fp8 models (fp8 / MXFP4 weights) take p2t_llama_prefill");
        return P2T_ERR_UNSUPPORTED;
    }
    P2T_REQUIRE(cache->B0 == n, "p2t_llama_prefill_packed: cache holds %d rows, the packed batch %d prompts", cache->B0, n);
    PackedPrompts pp;
    P2T_TRY(place_table(place, n, R, Tpk, cache->Tp, "p2t_llama_prefill_packed", &pp));
    P2T_REQUIRE((int64_t)n * c->kv_heads <= 65535, "p2t_llama_prefill_packed: %d prompts x %d kv heads exceed one launch", n, c->kv_heads);
    P2T_REQUIRE(workspace_bytes >= p2t_llama_prefill_packed_workspace_bytes(c, R, Tpk), "p2t_llama_prefill_packed: workspace too small");
    Arena ar(workspace, workspace_bytes);
    float* out = (float*)ar.take(sizeof(float) * (size_t)R * Tpk * c->hidden);
    void* rest = ar.take(p2t_llama_workspace_bytes(c, R, Tpk));
    P2T_REQUIRE(!ar.overflow, "p2t_llama_prefill_packed: workspace overflow");
    P2T_TRY(llama_forward_impl(c, w, nullptr, inputs_embeds, mask, R, Tpk, c->n_layers, out, rest, p2t_llama_workspace_bytes(c, R, Tpk), stream, nullptr,
                               cache, docs, &pp));
    return launch_gather_last_packed(out, Tpk, c->hidden, pp, last_hidden, (hipStream_t)stream);
}

extern "C" size_t p2t_llama_decode_workspace_bytes(const p2t_llama_config* cfg, int BB, int Tp, int G) {
    if (!cfg || BB <= 0 || Tp <= 0 || G <= 0) return 0;
    return decode_plan(cfg, BB, Tp, G, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// The quantised LM head (include/p2t_hip.h, p2t_lm_head_q): final RMSNorm written as e4m3 rows + E8M0 row scales, then the weight
// stream of gemm_skinny.hip on e4m3 / MXFP4 codes (<= 64 rows) or the general fp8 GEMM on e4m3 codes (more rows; never a stream copy).
static int64_t lm_head_q_kq(int64_t H) { return round_up(H, 128); }
static size_t lm_head_q_ws_bytes(int64_t M, int64_t H) {
    return M > 0 && H > 0 ? (size_t)round_up(M * lm_head_q_kq(H), 256) + (size_t)round_up(M, 256) + 512 : 0;
}

// every refusal of a head call, before any launch.  `who`: the entry point's name
static int lm_head_q_check(const p2t_lm_head_q* h, int64_t M, int64_t H, int64_t V, int64_t ld_logits, int out_dtype, const char* who) {
    P2T_REQUIRE(h, "%s: null head descriptor", who);
    P2T_REQUIRE(h->format == P2T_LM_HEAD_E4M3 || h->format == P2T_LM_HEAD_MXFP4, "%s: head format %d is neither P2T_LM_HEAD_E4M3 nor P2T_LM_HEAD_MXFP4", who,
                h->format);
    P2T_REQUIRE(M > 0 && H > 0 && H % 8 == 0 && H < (1 << 30) && V > 0 && V < (1 << 30), "%s: bad head shape (rows %lld, hidden %lld %% 8, vocab %lld)", who,
                (long long)M, (long long)H, (long long)V);
    P2T_REQUIRE(ld_logits >= V && ld_logits % 4 == 0, "%s: ld_logits %lld must be a multiple of 4 that holds vocab %lld", who, (long long)ld_logits, (long long)V);
    const int64_t Kq = lm_head_q_kq(H);
    const bool mx = h->format == P2T_LM_HEAD_MXFP4;
    P2T_REQUIRE(h->codes && ((uintptr_t)h->codes & 15) == 0, "%s: null or misaligned head codes (16-byte alignment)", who);
    P2T_REQUIRE(h->scales || (mx && h->stream_order), "%s: null head scales (only an interleaved MXFP4 stream copy carries its own)", who);
    P2T_REQUIRE(h->stream_order || (h->ld % 16 == 0 && h->ld >= (mx ? Kq / 2 : Kq)), "%s: head ld %lld must be a multiple of 16 and at least %lld bytes", who,
                (long long)h->ld, (long long)(mx ? Kq / 2 : Kq));
    P2T_REQUIRE(!h->codes_e4m3 == !h->scales_e4m3, "%s: codes_e4m3 and scales_e4m3 go together", who);
    P2T_REQUIRE(!h->codes_e4m3 || mx, "%s: codes_e4m3 is the MXFP4 head's copy for more than 64 rows (an e4m3 head serves them itself)", who);
    if (out_dtype != P2T_BF16) {
        set_error("%s: the quantised LM head serves bf16 models only", who);
        return P2T_ERR_UNSUPPORTED;
    }
    if (M > 64 && h->stream_order) {
        set_error("%s: a stream-order LM head serves at most 64 rows (got %lld): pass the row-major one", who, (long long)M);
        return P2T_ERR_UNSUPPORTED;
    }
    if (M > 64 && mx && !h->codes_e4m3) {
        set_error("%s: an MXFP4 LM head serves more than 64 rows (got %lld) through its e4m3 copy (codes_e4m3, scales_e4m3)", who, (long long)M);
        return P2T_ERR_UNSUPPORTED;
    }
    if (M > 64 && V % 16) {
        set_error("%s: more than 64 rows run the general GEMM, which takes a vocabulary that is a multiple of 16 (got %lld)", who, (long long)V);
        return P2T_ERR_UNSUPPORTED;
    }
    if (M > 64 && !mx && h->ld != Kq) {
        set_error("%s: more than 64 rows read the e4m3 head at ld = hidden rounded up to 128 (%lld, got %lld)", who, (long long)Kq, (long long)h->ld);
        return P2T_ERR_UNSUPPORTED;
    }
    return P2T_OK;
}

// checked arguments only.  norm_w == nullptr: x holds rows that are normalised already (the prefill's last hidden rows)
static int lm_head_q_run(const float* x, int64_t ld_x, const float* norm_w, float eps, const p2t_lm_head_q* h, int64_t M, int64_t H, int64_t V, void* logits,
                         int64_t ld_logits, uint8_t* aq, uint8_t* as, hipStream_t s) {
    const int64_t Kq = lm_head_q_kq(H);
    if (norm_w) P2T_TRY(launch_rmsnorm_fp8_few(x, ld_x, norm_w, eps, aq, Kq, as, M, H, s));
    else P2T_TRY(launch_quant_rows_few(x, P2T_F32, ld_x, M, H, aq, Kq, as, s));
    if (M <= 64) {
        if (h->format == P2T_LM_HEAD_MXFP4)
            return launch_gemm_skinny_mxfp4(aq, Kq, as, h->codes, h->ld, h->scales, logits, ld_logits, M, V, Kq, P2T_BF16, P2T_EPI_STORE, nullptr, s,
                                            h->stream_order != 0);
        return launch_gemm_skinny_fp8(aq, Kq, as, h->codes, h->ld, h->scales, logits, ld_logits, M, V, Kq, P2T_BF16, P2T_EPI_STORE, nullptr, s,
                                      h->stream_order != 0);
    }
    const bool mx = h->format == P2T_LM_HEAD_MXFP4;
    return p2t::gemm_nt(gemm_args_fp8(aq, Kq, as, mx ? h->codes_e4m3 : h->codes, mx ? h->scales_e4m3 : h->scales, M, V, Kq, logits, ld_logits, P2T_BF16,
                                      P2T_EPI_STORE), s);
}

// the step's last launch: the shared counter (stride 0: one thread, as ever), or every row's own where it is not frozen
static int launch_advance(int32_t* step, int stride, const int32_t* frozen, int BB, hipStream_t s) {
    if (stride == 0) advance_kernel<<<1, 1, 0, s>>>(step, 0, nullptr, 1);
    else advance_kernel<<<(unsigned)ceil_div(BB, 256), 256, 0, s>>>(step, stride, frozen, BB);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

// One call of the step: the doors fill it in by name, and what a door does not have stays nullptr
struct StepCall {
    const char* who = nullptr;                                // the entry point's name, for the messages
    const p2t_llama_config* c = nullptr; const p2t_llama_weights* w = nullptr;
    const p2t_llama_layer_stream* ws_layers = nullptr;        // stream-order copies of the projections
    const p2t_llama_layer_mxfp4* mx = nullptr;                // their MXFP4 form (a gemm_fp8 model, at most 64 rows)
    const void* lm_head = nullptr; int64_t ld_head = 0; int lm_head_preshuffled = 0;
    const p2t_lm_head_q* head_q = nullptr;                    // the quantised head, in lm_head's place
    const p2t_kv_cache* cache = nullptr; const float* x_in = nullptr; void* logits = nullptr; int64_t ld_logits = 0; int flags = 0;
    void* workspace = nullptr; size_t workspace_bytes = 0;
    int32_t* row_step = nullptr; const int32_t* frozen = nullptr;       // per-row counters (p2t_llama_decode_step_rows)
    const uint8_t* ancestry = nullptr;                                  // the beam group's ancestry table (p2t_llama_decode_step_beams)
    int q_tokens = 0;                                                   // tokens per row, row_step read only (p2t_llama_decode_step_multi); 0: one, as ever
    p2t_stream stream = nullptr;
};
// the arguments that all four doors have, under the same names
#define P2T_STEP_CALL(a, name)                                                                                                                    \
    StepCall a;                                                                                                                                   \
    a.who = name; a.c = c; a.w = w; a.lm_head = lm_head; a.ld_head = ld_head; a.lm_head_preshuffled = lm_head_preshuffled; a.cache = cache;        \
    a.x_in = x_in; a.logits = logits; a.ld_logits = ld_logits; a.flags = flags; a.workspace = workspace; a.workspace_bytes = workspace_bytes;      \
    a.stream = stream

// One projection's weight: the row-major matrix w at row stride ld (+ its row scales, gemm_fp8), its stream-order copy or nullptr, its
// MXFP4 codes (+ block scales) or nullptr
struct StepWeight { const void* w; int64_t ld; const uint8_t* row_scale; const void* stream; const void* mx; const uint8_t* mx_bs; };

// what the MXFP4 form of the projections asks of the call
static int check_mx(const p2t_llama_config* c, const p2t_kv_cache* cache, const p2t_llama_layer_mxfp4* mx, const char* who, int q_tokens) {
    P2T_REQUIRE(c && cache, "%s: null argument", who);
    P2T_REQUIRE(c->gemm_fp8 && c->dtype == P2T_BF16, "%s: mx_layers need a gemm_fp8 configuration with bf16 activations", who);
    P2T_REQUIRE((int64_t)cache->B0 * cache->group * q_tokens <= 64, "%s: mx_layers serve at most 64 rows (got %lld): beyond that the e4m3 weights serve", who,
                (long long)cache->B0 * cache->group * q_tokens);
    for (int l = 1; l < c->n_layers; ++l) P2T_REQUIRE(!mx[l].stream_order == !mx[0].stream_order, "%s: layers differ in stream_order", who);
    return P2T_OK;
}

// Every refusal of the step, before its first enqueue (under stream capture a later one would leave a half-recorded graph behind) --
// the workspace's included, so this pass also carves it: what it hands back is all the launch sequence needs beside the call.
// -> kc: the cache the launches read -- with per-row counters row_step stands where the shared counter does, and the cache's own is
// neither read nor written; b: the workspace, carved.
static int check_step(const StepCall& a, p2t_kv_cache* kc, DecodeBuffers* b, uint8_t** head_aq, uint8_t** head_as) {
    const char* who = a.who;
    const p2t_llama_config* c = a.c;
    P2T_REQUIRE(!(a.ws_layers && a.mx), "%s: w_stream and mx_layers are two forms of the same projections: pass one", who);
    const int Q = a.q_tokens ? a.q_tokens : 1;
    if (a.q_tokens) {                                    // before anything multiplies by it
        P2T_REQUIRE(c && a.cache, "%s: null argument", who);
        P2T_TRY(check_multi(a.q_tokens, c->kv_heads > 0 ? c->heads / c->kv_heads : 0, who));
    }
    if (a.mx) P2T_TRY(check_mx(c, a.cache, a.mx, who, Q));
    P2T_REQUIRE(c && a.w && a.w->layers && a.w->final_norm_w && (a.lm_head || a.head_q) && a.x_in && a.logits && a.workspace, "%s: null argument", who);
    if (a.cache) *kc = *a.cache;
    if (a.cache && a.row_step) kc->step = a.row_step;
    P2T_TRY(check_cache(c, a.cache ? kc : nullptr, who));
    if (a.row_step && kc->group != 1) {
        set_error("%s: per-row counters serve group == 1 only (got %d)", who, kc->group);
        return P2T_ERR_UNSUPPORTED;
    }
    if (a.ancestry) P2T_TRY(check_ancestry(a.ancestry, kc->group, c->heads / c->kv_heads, who));
    P2T_REQUIRE(!c->gemm_fp8 || c->dtype == P2T_BF16, "%s: gemm_fp8 needs bf16 activations (dtype = P2T_BF16)", who);
    const int BB = kc->B0 * kc->group * Q;               // the step's rows: Q tokens per cache row
    if (a.q_tokens && BB > 64) {
        set_error("%s: %d rows x %d tokens exceed the 64 rows of one weight-streaming step", who, kc->B0, Q);
        return P2T_ERR_UNSUPPORTED;
    }
    const int64_t H = c->hidden, Hp = round_up(H, 64);
    P2T_REQUIRE((a.head_q || a.lm_head_preshuffled || a.ld_head >= Hp) && a.ld_logits >= c->vocab, "%s: ld_head %lld < %lld or ld_logits %lld < vocab", who,
                (long long)a.ld_head, (long long)Hp, (long long)a.ld_logits);
    if (a.head_q) {
        P2T_TRY(lm_head_q_check(a.head_q, BB, H, c->vocab, a.ld_logits, c->dtype, who));
    } else {
        P2T_REQUIRE(!a.lm_head_preshuffled || c->dtype == P2T_BF16, "%s: pre-shuffled weights are a bf16 layout", who);
        // the stream-order copy is only readable by the skinny kernels (<= 64 rows): beyond that the general GEMM would read the
        // shuffled tiles as a row-major [vocab, Hp] matrix and return wrong logits without an error
        P2T_REQUIRE(!a.lm_head_preshuffled || BB <= 64, "%s: a pre-shuffled LM head serves at most 64 rows (got %d): pass the row-major one", who, BB);
    }
    // the quantised head's e4m3 rows + row scales sit behind the step's own buffers
    P2T_REQUIRE(a.workspace_bytes >= decode_plan(c, BB, kc->Tp, kc->G, nullptr, nullptr) + (a.head_q ? lm_head_q_ws_bytes(BB, H) : 0),
                "%s: workspace too small", who);
    for (int l = 0; l < c->n_layers; ++l) {
        const p2t_llama_layer& L = a.w->layers[l];
        P2T_REQUIRE(!c->gemm_fp8 || (L.qkv_ws && L.o_ws && L.gu_ws && L.down_ws), "%s: gemm_fp8 needs the row scales of layer %d", who, l);
        P2T_REQUIRE(!L.q_norm_w == !L.k_norm_w, "%s: q_norm_w and k_norm_w go together (layer %d)", who, l);
        if (!a.mx) continue;
        const p2t_llama_layer_mxfp4& X = a.mx[l];
        P2T_REQUIRE(X.qkv_w && X.o_w && X.gu_w && X.down_w && (a.mx->stream_order || (X.qkv_bs && X.o_bs && X.gu_bs && X.down_bs)),
                    "%s: null codes / block scales in layer %d", who, l);
    }
    Arena ar(a.workspace, a.workspace_bytes);
    decode_plan(c, BB, kc->Tp, kc->G, &ar, b);
    *head_aq = a.head_q ? (uint8_t*)ar.take((size_t)BB * lm_head_q_kq(H)) : nullptr;
    *head_as = a.head_q ? (uint8_t*)ar.take((size_t)BB) : nullptr;
    P2T_REQUIRE(!ar.overflow, "%s: workspace overflow", who);
    return P2T_OK;
}

static int decode_step(const StepCall& a) {
    p2t_kv_cache kc;
    DecodeBuffers b;
    uint8_t *head_aq, *head_as;
    P2T_TRY(check_step(a, &kc, &b, &head_aq, &head_as));
    const p2t_llama_config* c = a.c;
    const p2t_llama_weights* w = a.w;
    hipStream_t s = (hipStream_t)a.stream;
    const bool fp8 = c->gemm_fp8, fuse_rope = !(a.flags & P2T_DECODE_NO_ROPE_FUSION);
    const int Q = a.q_tokens ? a.q_tokens : 1;           // tokens per cache row: BB rows of activations, BB / Q rows of cache
    const int sstride = a.row_step ? 1 : 0, BB = kc.B0 * kc.group * Q, dt = c->dtype;
    const int64_t M = BB, H = c->hidden, F = c->ffn, Hp = round_up(H, 64), Fp = round_up(F, 64);
    const int d = c->head_dim, dp = head_dim_padded(d), nh = c->heads, nkv = c->kv_heads;
    const int64_t NQKV = (int64_t)(nh + 2 * nkv) * d, QO = round_up((int64_t)nh * d, 64);
    const float* inv_freq = w->inv_freq;
    if (!inv_freq) {
        P2T_TRY(launch_inv_freq(b.inv_freq, d / 2, c->rope_theta, c->rope_llama3, c->rope_factor, c->rope_low_freq_factor, c->rope_high_freq_factor,
                                (float)c->rope_original_max_pos, s));
        inv_freq = b.inv_freq;
    }
    const float scale = 1.0f / sqrtf((float)d);
    const int l2s = dt == P2T_BF16;                      // as the prefill: scale * log2(e) folded into q for bf16 models
    const float q_fold = l2s ? scale * kLog2e : 1.0f, c_exp = l2s ? 1.0f : scale * kLog2e;
    P2T_CHECK_HIP(hipMemcpyAsync(b.x, a.x_in, sizeof(float) * (size_t)BB * H, hipMemcpyDeviceToDevice, s));
    P2T_CHECK_HIP(hipMemsetAsync(b.ao, 0, dtype_size(dt) * (size_t)BB * QO, s));
    // the SwiGLU epilogues write columns [0, F) of act and the down projection reads K = Fp of them against zero weight columns: what
    // the caller's workspace held in [F, Fp) must not reach it (NaN x 0)
    if (Fp > F) P2T_CHECK_HIP(hipMemsetAsync(b.act, 0, dtype_size(dt) * (size_t)BB * Fp, s));
    // gemm_fp8 models (e4m3 weights AND GEMM operands, bf16 activations elsewhere): the same step with every
    // projection on the e4m3 stream (half the weight bytes of a step); rows are quantised by the RMSNorm / a quantise pass as in the prefill
    const int64_t Hq = round_up(H, 128), Fq = round_up(F, 128), QOq = round_up((int64_t)nh * d, 128);
    const Operand h = fp8 ? Operand{b.hq, Hq, b.hs} : Operand{b.h, Hp, nullptr};
    const Operand ao = fp8 ? Operand{b.aoq, QOq, b.aos} : Operand{b.ao, QO, nullptr};
    const Operand act = fp8 ? Operand{b.actq, Fq, b.acts} : Operand{b.act, Fp, nullptr};
    // the towers' two helpers (towers.hip) on the launchers for a few rows
    auto norm_into_h = [&](const float* ln_w) {
        return fp8 ? launch_rmsnorm_fp8_few(b.x, H, ln_w, c->rms_norm_eps, b.hq, Hq, b.hs, M, H, s)
                   : launch_rmsnorm_few_rows(b.x, H, ln_w, c->rms_norm_eps, b.h, Hp, M, H, dt, s);
    };
    auto quantise_into = [&](const Operand& o, const void* x, int64_t ld, int64_t cols) {
        return o.scale ? launch_quant_rows_few(x, dt, ld, M, cols, o.p, o.ld, o.scale, s) : (int)P2T_OK;
    };
    // out[M, N] = epilogue(x . W^T): the weight-streaming kernel (gemm_skinny.hip) first; where it answers UNSUPPORTED (more than 64
    // rows, an f32 model) the general GEMM on the row-major matrix.  Neither the fused-rotation form (`rope`: QKV + rotation + cache
    // append in one launch) nor MXFP4 has a general form: their answer goes back to the caller as it is
    const bool stream_w = a.ws_layers && dt == P2T_BF16;
    const int mx_stream = a.mx && a.mx->stream_order;
    auto project = [&](const Operand& x, const StepWeight& W, int64_t N, void* out, int64_t ldc, int out_dtype, int epi, const SkinnyRope* rope) {
        const int64_t K = x.ld;
        const void* wt = W.stream ? W.stream : W.w;
        const int pre = W.stream != nullptr;
        if (W.mx) return launch_gemm_skinny_mxfp4(x.p, K, x.scale, W.mx, K / 2, W.mx_bs, out, ldc, M, N, K, out_dtype, epi, rope, s, mx_stream);
        const int r = x.scale ? launch_gemm_skinny_fp8(x.p, K, x.scale, wt, W.ld, W.row_scale, out, ldc, M, N, K, out_dtype, epi, rope, s, pre)
                      : rope  ? launch_gemm_skinny_qkv_rope(x.p, K, wt, W.ld, M, N, K, *rope, s, pre)
                              : launch_gemm_skinny(x.p, K, wt, W.ld, out, ldc, M, N, K, dt, out_dtype, epi, s, pre);
        if (r != P2T_ERR_UNSUPPORTED || rope) return r;
        GemmArgs g = projection(x, W.w, W.row_scale, M, N, dt, out, ldc, out_dtype, epi);
        g.ldw = W.ld;
        if (epi == P2T_EPI_STORE_F32) g.n_zero = (int)N;
        return gemm_nt(g, s);
    };
    const size_t per_g = (size_t)(BB / Q) * nkv * kc.G * dp * dtype_size(dt);  // one layer of the generated segment, bytes
    for (int l = 0; l < c->n_layers; ++l) {
        const p2t_llama_layer& L = w->layers[l];
        const p2t_llama_layer_stream S = stream_w ? a.ws_layers[l] : p2t_llama_layer_stream{};
        const p2t_llama_layer_mxfp4 X = a.mx ? a.mx[l] : p2t_llama_layer_mxfp4{};
        const StepWeight Wqkv{L.qkv_w, h.ld, L.qkv_ws, S.qkv_w, X.qkv_w, X.qkv_bs}, Wo{L.o_w, ao.ld, L.o_ws, S.o_w, X.o_w, X.o_bs},
            Wgu{L.gu_w, h.ld, L.gu_ws, S.gu_w, X.gu_w, X.gu_bs}, Wdown{L.down_w, act.ld, L.down_ws, S.down_w, X.down_w, X.down_bs};
        // the prefill of this layer rotates in its QKV epilogue (towers.hip): the step then rotates the unrounded projection too
        const int fused_prefill = !L.q_norm_w && (d == 64 || d == 128);
        SkinnyRope ra;                                   // where this layer's rotation reads its position and appends
        ra.inv_freq = inv_freq; ra.prompt_len = kc.prompt_len; ra.step = kc.step; ra.step_stride = sstride; ra.group = kc.group;
        ra.nh = nh; ra.nkv = nkv; ra.d = d; ra.G = kc.G; ra.q_scale = q_fold; ra.q_tokens = Q;
        ra.q = b.qb; ra.k = (char*)kc.k_gen + per_g * l; ra.vt = (char*)kc.vt_gen + per_g * l;
        P2T_TRY(norm_into_h(L.ln1_w));
        int r = P2T_ERR_UNSUPPORTED;
        if (fused_prefill && dt == P2T_BF16 && fuse_rope) r = project(h, Wqkv, NQKV, nullptr, 0, dt, 0, &ra);      // SK_QKV_ROPE
        if (r == P2T_ERR_UNSUPPORTED) {                  // two launches: the f32 projection, then rotation + append
            P2T_TRY(project(h, Wqkv, NQKV, b.qkv, NQKV, P2T_F32, P2T_EPI_STORE_F32, nullptr));
            r = launch_rope_append(b.qkv, NQKV, ra, L, c->rms_norm_eps, BB, dp, !fused_prefill, dt, s);
        }
        P2T_TRY(r);
        if (a.ancestry) P2T_TRY(launch_attn_decode_beams(c, b.qb, b.ao, QO, &kc, l, c_exp, dt == P2T_BF16, 1, a.ancestry, s));
        else if (a.q_tokens) P2T_TRY(launch_attn_decode_multi(c, b.qb, b.ao, QO, &kc, l, c_exp, dt == P2T_BF16, 1, Q, s));
        else P2T_TRY(launch_attn_decode(c, b.qb, b.ao, QO, &kc, l, c_exp, dt == P2T_BF16, 1, sstride, s));
        P2T_TRY(quantise_into(ao, b.ao, QO, (int64_t)nh * d));
        P2T_TRY(project(ao, Wo, H, b.x, H, P2T_F32, P2T_EPI_RESID, nullptr));
        P2T_TRY(norm_into_h(L.ln2_w));
        P2T_TRY(project(h, Wgu, 2 * F, b.act, Fp, dt, P2T_EPI_SWIGLU, nullptr));
        P2T_TRY(quantise_into(act, b.act, Fp, F));
        P2T_TRY(project(act, Wdown, H, b.x, H, P2T_F32, P2T_EPI_RESID, nullptr));
    }
    if (a.head_q) {                                      // the e4m3 / MXFP4 head on the residual stream
        P2T_TRY(lm_head_q_run(b.x, H, w->final_norm_w, c->rms_norm_eps, a.head_q, M, H, c->vocab, a.logits, a.ld_logits, head_aq, head_as, s));
    } else {                                             // the model-dtype head, of a gemm_fp8 model too
        const StepWeight Whead{a.lm_head, a.ld_head, nullptr, a.lm_head_preshuffled ? a.lm_head : nullptr, nullptr, nullptr};
        P2T_TRY(launch_rmsnorm_few_rows(b.x, H, w->final_norm_w, c->rms_norm_eps, b.h, Hp, M, H, dt, s));
        P2T_TRY(project(Operand{b.h, Hp, nullptr}, Whead, c->vocab, a.logits, a.ld_logits, dt, P2T_EPI_STORE, nullptr));
    }
    if (a.q_tokens) return P2T_OK;                       // the counters are the verify kernel's to advance (p2t_lookup_verify_rows)
    return launch_advance(kc.step, sstride, a.frozen, BB, s);
}

extern "C" int p2t_llama_decode_step(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers,
                                     const void* lm_head, int64_t ld_head, int lm_head_preshuffled, const p2t_kv_cache* cache, const float* x_in, void* logits, int64_t ld_logits, int flags, void* workspace,
                                     size_t workspace_bytes, p2t_stream stream) {
    P2T_STEP_CALL(a, "p2t_llama_decode_step");
    a.ws_layers = ws_layers;
    return decode_step(a);
}

// The step of a gemm_fp8 model whose four projections per layer stream MXFP4 weights (include/p2t_hip.h): everything else -- the
// row quantisers, the attention, the bf16 LM head -- is p2t_llama_decode_step's.
extern "C" int p2t_llama_decode_step_mxfp4(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_mxfp4* mx_layers,
                                           const void* lm_head, int64_t ld_head, int lm_head_preshuffled, const p2t_kv_cache* cache, const float* x_in,
                                           void* logits, int64_t ld_logits, int flags, void* workspace, size_t workspace_bytes, p2t_stream stream) {
    P2T_REQUIRE(mx_layers, "p2t_llama_decode_step_mxfp4: null argument");
    P2T_STEP_CALL(a, "p2t_llama_decode_step_mxfp4");
    a.mx = mx_layers;
    return decode_step(a);
}

// Both steps behind one door, plus the quantised LM head: w_stream or mx_layers (either may be NULL, not both set); head_q == NULL is
// the existing step, launch for launch.
extern "C" int p2t_llama_decode_step_q(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers,
                                       const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                                       const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x_in, void* logits, int64_t ld_logits, int flags,
                                       void* workspace, size_t workspace_bytes, p2t_stream stream) {
    P2T_STEP_CALL(a, "p2t_llama_decode_step_q");
    a.ws_layers = ws_layers; a.mx = mx_layers; a.head_q = head_q;
    return decode_step(a);
}

// p2t_llama_decode_step_q for rows that carry their own counters (continuous batching, include/p2t_hip.h): the same launches, every
// `step[0]` read as row_step[row]; the last launch advances the rows that are not frozen.
extern "C" int p2t_llama_decode_step_rows(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers,
                                          const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                                          const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x_in, void* logits, int64_t ld_logits,
                                          int flags, void* workspace, size_t workspace_bytes, int32_t* row_step, const int32_t* frozen,
                                          p2t_stream stream) {
    P2T_REQUIRE(row_step, "p2t_llama_decode_step_rows: null row_step");
    P2T_STEP_CALL(a, "p2t_llama_decode_step_rows");
    a.ws_layers = ws_layers; a.mx = mx_layers; a.head_q = head_q; a.row_step = row_step; a.frozen = frozen;
    return decode_step(a);
}

// p2t_llama_decode_step_q for a beam group whose generated keys stay in the rows that wrote them (include/p2t_hip.h): the same launches
// but the attention's, which reads the ancestry table.
extern "C" int p2t_llama_decode_step_beams(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers,
                                           const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                                           const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x_in, void* logits, int64_t ld_logits,
                                           int flags, void* workspace, size_t workspace_bytes, const uint8_t* ancestry, p2t_stream stream) {
    P2T_REQUIRE(ancestry, "p2t_llama_decode_step_beams: null ancestry table");
    P2T_STEP_CALL(a, "p2t_llama_decode_step_beams");
    a.ws_layers = ws_layers; a.mx = mx_layers; a.head_q = head_q; a.ancestry = ancestry;
    return decode_step(a);
}

// p2t_llama_decode_step_rows for q_tokens tokens per row (include/p2t_hip.h): the launches of a step of B0 * q_tokens rows, the rotation
// and the attention indexed by (row, token); row_step is read only.
extern "C" int p2t_llama_decode_step_multi(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers,
                                           const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                                           const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x_in, void* logits, int64_t ld_logits,
                                           int flags, void* workspace, size_t workspace_bytes, const int32_t* row_step, int q_tokens,
                                           p2t_stream stream) {
    P2T_REQUIRE(row_step, "p2t_llama_decode_step_multi: null row_step");
    P2T_REQUIRE(q_tokens >= 1, "p2t_llama_decode_step_multi: q_tokens %d outside 1 .. 64", q_tokens);
    P2T_STEP_CALL(a, "p2t_llama_decode_step_multi");
    a.ws_layers = ws_layers; a.mx = mx_layers; a.head_q = head_q; a.row_step = const_cast<int32_t*>(row_step); a.q_tokens = q_tokens;
    return decode_step(a);
}

#undef P2T_STEP_CALL

extern "C" size_t p2t_lm_head_q_workspace_bytes(int64_t M, int64_t hidden) { return lm_head_q_ws_bytes(M, hidden); }

extern "C" int p2t_lm_head_logits_q(const float* x, int64_t ld_x, const float* norm_w, float eps, const p2t_lm_head_q* head, int64_t M, int64_t hidden,
                                    int64_t vocab, void* logits, int64_t ld_logits, int out_dtype, uint8_t* act_codes, uint8_t* act_scales, void* workspace,
                                    size_t workspace_bytes, p2t_stream stream) {
    P2T_REQUIRE(x && logits, "p2t_lm_head_logits_q: null x / logits");
    P2T_TRY(lm_head_q_check(head, M, hidden, vocab, ld_logits, out_dtype, "p2t_lm_head_logits_q"));
    P2T_REQUIRE(ld_x >= hidden && ld_x % 8 == 0 && ((uintptr_t)x & 15) == 0, "p2t_lm_head_logits_q: ld_x %lld must be a multiple of 8 that holds hidden %lld (x 16-byte aligned)",
                (long long)ld_x, (long long)hidden);
    P2T_REQUIRE(!act_codes == !act_scales, "p2t_lm_head_logits_q: act_codes and act_scales go together");
    P2T_REQUIRE(!act_codes || ((uintptr_t)act_codes & 15) == 0, "p2t_lm_head_logits_q: act_codes must be 16-byte aligned");
    uint8_t* aq = act_codes;
    uint8_t* as = act_scales;
    if (!aq) {
        P2T_REQUIRE(workspace && workspace_bytes >= lm_head_q_ws_bytes(M, hidden), "p2t_lm_head_logits_q: workspace too small (p2t_lm_head_q_workspace_bytes)");
        Arena ar(workspace, workspace_bytes);
        aq = (uint8_t*)ar.take((size_t)M * lm_head_q_kq(hidden));
        as = (uint8_t*)ar.take((size_t)M);
        P2T_REQUIRE(!ar.overflow, "p2t_lm_head_logits_q: workspace overflow");
    }
    return lm_head_q_run(x, ld_x, norm_w, eps, head, M, hidden, vocab, logits, ld_logits, aq, as, (hipStream_t)stream);
}

extern "C" int p2t_greedy_select(const void* logits, int dtype, int64_t ld, int V, int BB, const int64_t* eos_ids, int n_eos, int64_t pad_id,
                                 int32_t* finished, int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, const int32_t* step, int G,
                                 p2t_stream stream) {
    P2T_REQUIRE(logits && finished && next_tokens && out_tokens && step && BB > 0 && V > 0 && ld >= V && G > 0 && ld_tokens >= G && n_eos >= 0 &&
                    (n_eos == 0 || eos_ids),
                "p2t_greedy_select: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == P2T_BF16)
        greedy_select_kernel<bf16_t><<<BB, 1024, 0, s>>>((const bf16_t*)logits, ld, V, eos_ids, n_eos, pad_id, finished, next_tokens, out_tokens,
                                                        ld_tokens, step, G);
    else
        greedy_select_kernel<float><<<BB, 1024, 0, s>>>((const float*)logits, ld, V, eos_ids, n_eos, pad_id, finished, next_tokens, out_tokens,
                                                       ld_tokens, step, G);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_greedy_select_rows(const void* logits, int dtype, int64_t ld, int V, int n, const int64_t* eos_ids, int n_eos, int64_t pad_id,
                                      int32_t* finished, int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, const int32_t* row_step,
                                      const int32_t* row_limit, const int32_t* row_map, int BB, int G, p2t_stream stream) {
    P2T_REQUIRE(logits && finished && next_tokens && out_tokens && row_step && row_limit, "p2t_greedy_select_rows: null argument");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_greedy_select_rows: logits are f32 or bf16 (got dtype %d)", dtype);
    P2T_REQUIRE(n > 0 && BB > 0 && n <= BB && (row_map || n == BB), "p2t_greedy_select_rows: %d logits rows for %d engine rows (all of them, or a row_map subset)", n,
                BB);
    P2T_REQUIRE(V > 0 && ld >= V && G > 0 && ld_tokens >= G && n_eos >= 0 && (n_eos == 0 || eos_ids), "p2t_greedy_select_rows: bad shape arguments");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == P2T_BF16)
        greedy_select_rows_kernel<bf16_t><<<n, 1024, 0, s>>>((const bf16_t*)logits, ld, V, eos_ids, n_eos, pad_id, finished, next_tokens, out_tokens,
                                                            ld_tokens, row_step, row_limit, row_map, BB, G);
    else
        greedy_select_rows_kernel<float><<<n, 1024, 0, s>>>((const float*)logits, ld, V, eos_ids, n_eos, pad_id, finished, next_tokens, out_tokens,
                                                           ld_tokens, row_step, row_limit, row_map, BB, G);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

