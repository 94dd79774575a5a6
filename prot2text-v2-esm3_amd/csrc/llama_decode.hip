// Generation with a KV cache: what `llama_decoder.generate(inputs_embeds=..., attention_mask=...)` runs under
// Esm2LlamaInstructForCausalLM.generate (reference models/modeling_esm2llama_instruct.py:217-251; HF GenerationMixin + the cached
// LlamaAttention path, transformers/models/llama/modeling_llama.py).
//
// Layout (sized for 288 GB of HBM: nothing is paged, nothing is re-laid-out per step):
//   * prompts are COMPACTED first (p2t_compact_rows): the valid tokens of every row move to the front in order, so positions are
//     0..len-1 -- exactly HF's `position_ids = cumsum(attention_mask) - 1` on the tokens under the mask, for left padding, right
//     padding or holes alike -- and every row's keys are a prefix of its cache row;
//   * the cache has two segments: the PROMPT segment [layer][B0][kv_head][Tp][dp] (keys, post-rotation) + the same transposed
//     [layer][B0][kv_head][dp][Tp] (values: the decode kernel reads 8 consecutive keys of one feature with one 16-byte load), written
//     once by the prefill; and the GENERATED segment [layer][BB][kv_head][G][dp] / [..][dp][G] with BB = B0 * group rows (group =
//     beams per prompt: all beams of a prompt share its prompt segment, beam re-ordering touches the generated segment only);
//   * every row generates in lock-step: ONE device counter `step` = generated tokens already in the cache.  A decode step reads it on
//     the device (so the whole step replays as a HIP graph without a host round trip), appends at index `step`, attends to
//     prompt_len[b0] + step + 1 keys and increments it last;
//   * opt-in (continuous batching, p2t_llama_decode_step_rows; group == 1): every row carries its OWN counter, row_step[row], beside the
//     cache -- the same kernels read step[row * stride] with stride 1 where the lock-step entry points pass stride 0.  A finished row
//     is frozen (it re-appends at its own index and does not advance); p2t_kv_slot_load copies a freshly prefilled prompt segment from a
//     staging cache into its slot and resets its counters, between two replays of the step graph;
//   * opt-in for bf16 models (p2t_kv_cache's scale arrays set): the PROMPT segment as e4m3 codes in the same index order + one E8M0 scale
//     byte per key for K and for V -- quantised by the prefill's store (kv_quant_store_kernel), read by the F8 tiles of the attention.
#include "common.h"
#include "kernels.h"
#include "quant_fp8.h"

namespace p2t {
namespace {

// ---------------------------------------------------------------------------------------------
// compaction of the prompt rows
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) compact_index_kernel(const int64_t* __restrict__ mask, int T, int32_t* __restrict__ dst,
                                                            int64_t* __restrict__ out_mask, int32_t* __restrict__ lens) {
    __shared__ int cnt[256];
    __shared__ int total;
    const int b = blockIdx.x, tid = threadIdx.x, per = (T + 255) / 256;
    const int t0 = min(T, tid * per), t1 = min(T, t0 + per);
    const int64_t* m = mask + (int64_t)b * T;
    int c = 0;
    for (int t = t0; t < t1; ++t) c += m[t] != 0;
    cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int a = 0;
        for (int i = 0; i < 256; ++i) { const int v = cnt[i]; cnt[i] = a; a += v; }
        total = a;
        lens[b] = a;
    }
    __syncthreads();
    int a = cnt[tid];
    for (int t = t0; t < t1; ++t) dst[(int64_t)b * T + t] = m[t] != 0 ? a++ : -1;
    const int n = total;
    for (int t = tid; t < T; t += 256) out_mask[(int64_t)b * T + t] = t < n ? 1 : 0;
}

__global__ void __launch_bounds__(256) compact_copy_kernel(const float* __restrict__ x, const int32_t* __restrict__ dst, int T, int H,
                                                           float* __restrict__ out) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int to = dst[(int64_t)b * T + t];
    if (to < 0) return;
    const float4* s = reinterpret_cast<const float4*>(x + ((int64_t)b * T + t) * H);
    float4* d = reinterpret_cast<float4*>(out + ((int64_t)b * T + to) * H);
    for (int c = threadIdx.x; c < H / 4; c += 256) d[c] = s[c];
}

// last valid row of every prompt: out[b] = x[b, len[b] - 1]
__global__ void __launch_bounds__(256) gather_last_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int T, int H,
                                                          float* __restrict__ out) {
    const int b = blockIdx.x;
    const int t = max(0, min(T, lens[b]) - 1);
    const float* s = x + ((int64_t)b * T + t) * H;
    for (int c = threadIdx.x; c < H; c += 256) out[(int64_t)b * H + c] = s[c];
}

// v [BH][seq][dp] -> vt [BH][dp][Tp] (columns 0..seq-1)
template <typename T>
__global__ void __launch_bounds__(256) v_transpose_store_kernel(const T* __restrict__ v, T* __restrict__ vt, int seq, int dp, int Tp) {
    __shared__ T tile[64][130];
    const int bh = blockIdx.y, t0 = blockIdx.x * 64;
    for (int i = threadIdx.x; i < 64 * dp; i += 256) {
        const int tl = i / dp, c = i - tl * dp;
        tile[tl][c] = t0 + tl < seq ? v[((int64_t)bh * seq + t0 + tl) * dp + c] : from_f32<T>(0.f);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * dp; i += 256) {
        const int c = i >> 6, tl = i & 63;
        if (t0 + tl < Tp) vt[((int64_t)bh * dp + c) * Tp + t0 + tl] = tile[tl][c];
    }
}

// fp8 prompt segment (p2t_kv_cache with the scale arrays set): k, v bf16 [BH][seq][DP] -> K codes [BH][Tp][DP], V codes transposed
// [BH][DP][Tp], one E8M0 byte per key each; quant_rows_kernel's arithmetic on every key row (amax -> e8m0_of_amax -> x * 2^-e ->
// v_cvt_pk_fp8_f32), columns d .. DP zero.  grid (64-key tiles, BH); DP / 8 lanes share a key (8 features each) and reduce its
// maximum among themselves; the V codes cross LDS for the transpose.  Positions < seq only.
template <int DP>
__global__ void __launch_bounds__(256) kv_quant_store_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, uint8_t* __restrict__ kq,
                                                             uint8_t* __restrict__ vtq, uint8_t* __restrict__ ks, uint8_t* __restrict__ vs, int seq,
                                                             int d, int Tp) {
    constexpr int LG = DP / 8, KPP = 256 / LG;                        // lanes per key, keys per pass
    __shared__ __attribute__((aligned(16))) uint8_t tile[DP][68];     // V codes [feature][key of the tile]
    const int bh = blockIdx.y, t0 = blockIdx.x * 64;
    const int sub = threadIdx.x % LG, kl = threadIdx.x / LG;
    auto quant8 = [&](const bf16_t* src, bool ok, int& E) {           // 8 features of one key -> their codes; E of the whole key
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
        if (ok) load8(src, x);
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[e] = 8 * sub + e < d ? x[e] : 0.f;
            amax = fmaxf(amax, fabsf(x[e]));
        }
#pragma unroll
        for (int o = LG / 2; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        E = e8m0_of_amax(amax);
        const float inv = pow2_neg(E);
        return make_uint2(pack_fp8x4(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv), pack_fp8x4(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv));
    };
#pragma unroll
    for (int pass = 0; pass < 64 / KPP; ++pass) {
        const int tl = pass * KPP + kl, t = t0 + tl;
        const bool ok = t < seq;                                      // the same for the lanes of a key
        const int64_t in = ((int64_t)bh * seq + t) * DP + 8 * sub, row = (int64_t)bh * Tp + t;
        int E;
        const uint2 kc = quant8(k + in, ok, E);
        if (ok) {
            *reinterpret_cast<uint2*>(kq + row * DP + 8 * sub) = kc;
            if (sub == 0) ks[row] = (uint8_t)E;
        }
        const uint2 vc = quant8(v + in, ok, E);
        if (ok && sub == 0) vs[row] = (uint8_t)E;
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[8 * sub + e][tl] = (uint8_t)((e < 4 ? vc.x : vc.y) >> (8 * (e & 3)));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DP * 16; i += 256) {
        const int c = i >> 4, t = t0 + 4 * (i & 15);
        const unsigned w = *reinterpret_cast<const unsigned*>(&tile[c][4 * (i & 15)]);
        uint8_t* dst = vtq + ((int64_t)bh * DP + c) * Tp + t;
        if (t + 4 <= seq) {
            *reinterpret_cast<unsigned*>(dst) = w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e < seq) dst[e] = (uint8_t)(w >> (8 * e));
        }
    }
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
                                                          int round_first) {
    const int lane = threadIdx.x & 63, heads = nh + 2 * nkv, half = d / 2;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= BB * heads) return;
    const int bb = row / heads, hh = row - bb * heads;
    const int step = min(max(step_ptr[(int64_t)bb * step_stride], 0), G - 1);      // stride 0: the shared counter, 1: row bb's own
    const int pos = prompt_len[bb / group] + step;
    const float* src = qkv + (int64_t)bb * ldq + (int64_t)hh * d;
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
        T* dst = is_q ? qbuf + ((int64_t)bb * nh + hh) * dp : kg + (((int64_t)bb * nkv + (hh - nh)) * G + step) * dp;
        if (lane < half) { dst[lane] = from_f32<T>(o1); dst[lane + half] = from_f32<T>(o2); }
        for (int cc = d + lane; cc < dp; cc += 64) dst[cc] = from_f32<T>(0.f);
    } else {
        T* dst = vtg + ((int64_t)bb * nkv + (hh - nh - nkv)) * dp * G + step;
        if (lane < half) { dst[(int64_t)lane * G] = from_f32<T>(x1); dst[(int64_t)(lane + half) * G] = from_f32<T>(x2); }
        for (int cc = d + lane; cc < dp; cc += 64) dst[(int64_t)cc * G] = from_f32<T>(0.f);
    }
}

// ---------------------------------------------------------------------------------------------
// attention of ONE query token per row over the two cache segments
// ---------------------------------------------------------------------------------------------
// grid (BB * nkv, head chunks): ONE block owns all keys of a (row, kv head) -- cut into 64-key tiles (prompt segment, then generated
// segment), tile t goes to wave t mod NW.  A wave keeps a running (max, sum, output) per query head of the GQA group -- they all read
// the same keys -- in base-2 form; the waves are merged in LDS in wave order (decode_merge): no atomics, nothing through memory.
//   scores: lane = key, 16-byte pieces of its K row against q (f32 in LDS, broadcast reads);
//   values: lane = feature (rows of the transposed segment), 16-byte pieces = 8 (bf16) / 4 (f32) consecutive keys against P in LDS.
template <typename T> struct Piece;
template <> struct Piece<bf16_t> { static constexpr int N = 8; };
template <> struct Piece<float> { static constexpr int N = 4; };
template <typename T, int N> __device__ __forceinline__ void load_piece(const T* p, float (&v)[N]) {
    if constexpr (N == 8) load8(p, v); else load4(p, v);
}

// Merge of a block's per-wave results (red[w][head][0..DP-1] = un-normalised output, [DP] = running max, [DP + 1] = sum; base-2 form),
// in wave order, and the store of the normalised rows.  One block owns ALL keys of its (row, kv head): a split over several blocks
// with a last-arriver merge through global memory was measured at 42 us per launch against 24 for this form at 8 x 1121 keys -- three
// more dependent round trips to memory and a release fence per block cost more than the idle CUs.
template <typename T, int DP, int GH, int NW>
__device__ __forceinline__ void decode_merge(float (&red)[NW][GH][DP + 2], int bb, int h0, int nhead, int d, T* __restrict__ out, int64_t ld_out) {
    for (int i = threadIdx.x; i < GH * DP; i += NW * 64) {
        const int g = i / DP, c = i - g * DP;
        if (g >= nhead || c >= d) continue;
        float M = -INFINITY;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) M = fmaxf(M, red[ww][g][DP]);
        float o = 0.f, L = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) {
            const float mw = red[ww][g][DP];
            if (mw > -INFINITY) {
                const float f = exp2f(mw - M);
                o += f * red[ww][g][c];
                L += f * red[ww][g][DP + 1];
            }
        }
        out[(int64_t)bb * ld_out + (int64_t)(h0 + g) * d + c] = from_f32<T>(o / L);
    }
}

template <typename T, int DP, int GH>
__global__ void __launch_bounds__(512) attn_decode_kernel(const T* __restrict__ q, const T* __restrict__ kp, const T* __restrict__ vtp,
                                                          const T* __restrict__ kg, const T* __restrict__ vtg,
                                                          const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ step_ptr,
                                                          int step_stride, int group, int nh, int nkv, int G, int Tp, int Gcap, float c_exp, int round_p,
                                                          T* __restrict__ out, int64_t ld_out, int d) {
    constexpr int PN = Piece<T>::N, R = DP > 64 ? DP / 64 : 1, PW = DP + 2, NW = 8;
    __shared__ float sq[GH][DP];
    __shared__ float sp[NW][GH][64];
    __shared__ float red[NW][GH][PW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pair = blockIdx.x, bb = pair / nkv, kvh = pair - bb * nkv, b0 = bb / group;
    const int hc = blockIdx.y;
    const int h0 = kvh * G + hc * GH, nhead = min(GH, G - hc * GH);          // query heads h0 .. h0 + nhead - 1
    for (int i = threadIdx.x; i < GH * DP; i += NW * 64) {
        const int g = i / DP, c = i - g * DP;
        sq[g][c] = g < nhead ? to_f32(q[((int64_t)bb * nh + h0 + g) * DP + c]) : 0.f;
    }
    __syncthreads();
    const int n0 = min(max(prompt_len[b0], 0), Tp), n1 = min(max(step_ptr[(int64_t)bb * step_stride], 0) + 1, Gcap);
    const int tiles0 = (n0 + 63) >> 6, tiles = tiles0 + ((n1 + 63) >> 6);
    const T* k_seg0 = kp + ((int64_t)b0 * nkv + kvh) * Tp * DP;
    const T* k_seg1 = kg + ((int64_t)bb * nkv + kvh) * Gcap * DP;
    const T* v_seg0 = vtp + ((int64_t)b0 * nkv + kvh) * DP * Tp;
    const T* v_seg1 = vtg + ((int64_t)bb * nkv + kvh) * DP * Gcap;

    float m_run[GH], l_run[GH], acc[GH][R];
#pragma unroll
    for (int g = 0; g < GH; ++g) {
        m_run[g] = -INFINITY;
        l_run[g] = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[g][r] = 0.f;
    }
    for (int t = w; t < tiles; t += NW) {
        const int sg = t >= tiles0, tt = sg ? t - tiles0 : t, n = sg ? n1 : n0, cap = sg ? Gcap : Tp;
        const int key = tt * 64 + lane;
        const bool valid = key < n, full = tt * 64 + 64 <= n;
        const T* krow = (sg ? k_seg1 : k_seg0) + (int64_t)key * DP;
        float sc[GH];
#pragma unroll
        for (int g = 0; g < GH; ++g) sc[g] = 0.f;
        if (valid) {
#pragma unroll 4
            for (int c = 0; c < DP; c += PN) {
                float kv[PN];
                load_piece<T, PN>(krow + c, kv);
#pragma unroll
                for (int g = 0; g < GH; ++g) {
#pragma unroll
                    for (int e = 0; e < PN; ++e) sc[g] = fmaf(kv[e], sq[g][c + e], sc[g]);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int g = 0; g < GH; ++g) {
            const float e2 = valid ? sc[g] * c_exp : -INFINITY;
            const float m_new = fmaxf(m_run[g], wave_max(e2));            // every tile holds at least one valid key
            const float alpha = exp2f(m_run[g] - m_new);
            float p = valid ? exp2f(e2 - m_new) : 0.f;
            l_run[g] = l_run[g] * alpha + p;
            if (round_p) p = to_f32(from_f32<T>(p));                      // the MFMA forward feeds P to the matrix pipe in bf16
            sp[w][g][lane] = p;
            m_run[g] = m_new;
#pragma unroll
            for (int r = 0; r < R; ++r) acc[g][r] *= alpha;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int dim = lane + 64 * r;
            if (dim < DP) {
                const T* vrow = (sg ? v_seg1 : v_seg0) + (int64_t)dim * cap + tt * 64;
#pragma unroll 2
                for (int j = 0; j < 64; j += PN) {
                    float vv[PN];
                    load_piece<T, PN>(vrow + j, vv);
                    if (!full) {
#pragma unroll
                        for (int e = 0; e < PN; ++e) vv[e] = tt * 64 + j + e < n ? vv[e] : 0.f;
                    }
#pragma unroll
                    for (int g = 0; g < GH; ++g) {
#pragma unroll
                        for (int e = 0; e < PN; ++e) acc[g][r] = fmaf(sp[w][g][j + e], vv[e], acc[g][r]);
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int g = 0; g < GH; ++g) {
        const float l = wave_sum(l_run[g]);
        if (lane == 0) { red[w][g][DP] = m_run[g]; red[w][g][DP + 1] = l; }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (lane + 64 * r < DP) red[w][g][lane + 64 * r] = acc[g][r];
    }
    __syncthreads();
    decode_merge<T, DP, GH, NW>(red, bb, h0, nhead, d, out, ld_out);
}

// bf16 form on the matrix pipe (`v_mfma_f32_16x16x32_bf16`, fragments straight from global memory -- no LDS staging, the step is a
// stream).  Per wave and 64-key tile:
//   S[key, head] = K . q^T: A = 16 keys x 32 features of K (a lane: 16 bytes of one key row), B = q (16 head slots, the group's G
//     real heads first, zeros behind), so a lane holds 4 keys of ONE head slot -- the softmax statistics of a head live in the four
//     lanes l, l + 16, l + 32, l + 48;
//   the A rows of the sub-tiles are permuted (row 4 g + r of sub-tile t <-> key 32 (t / 2) + 8 g + 4 (t % 2) + r), so that the eight
//     probabilities a lane holds after two sub-tiles are 8 CONSECUTIVE keys: exactly the B operand of
//   O[feature, head] += V^T . P: A = 16 features x 32 keys of the transposed value segment (a lane: 16 bytes = 8 consecutive keys of
//     one feature), no exchange between lanes anywhere.
//
// F8 tiles (the fp8 prompt segment: e4m3 codes + one E8M0 byte per key for K and for V) feed the same two products: the codes are widened
// to bf16 (exact) right in front of the MFMA that takes them, the K scale multiplies the key's f32 score and the V scale the key's
// probability once the row sum has taken the unscaled one -- powers of two, so nothing rounds differently from the bf16 tile on the
// dequantised operands.  A lane's loads stay 16 bytes of one row, which now hold 16 elements, so both contraction orders are permuted
// (any order serves a sum as long as the two operands agree):
//   S: lane g reads the features 64 (kk / 2) + 16 g + 8 (kk % 2) .. of its key for step kk (DP 32: 8 g ..) -- `qf` is then the query in
//     that order (the kernel's qp);
//   A rows: row 4 g + r of sub-tile t <-> key 16 g + 4 t + r, so a lane's sixteen scores are the keys 16 g .. 16 g + 15: one 16-byte
//     load of each scale array, one 16-byte load per feature of the transposed codes, P in that key order.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(unsigned lo, unsigned hi) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), e = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    return __builtin_bit_cast(bf16x8, u32x4{pack_bf16x2(a[0], a[1]), pack_bf16x2(b[0], b[1]), pack_bf16x2(c[0], c[1]), pack_bf16x2(e[0], e[1])});
}
__device__ __forceinline__ float e8m0_byte_to_f32(unsigned word, int byte) {       // 2^(E - 127) for E = 1 .. 254; E = 0 -> 0
    return __uint_as_float(((word >> (8 * byte)) & 0xFFu) << 23);
}

// One 64-key tile `tt` of a segment of `cap` keys, `n` of them valid, into a wave's running (max, sum, output).
template <int DP, bool F8>
__device__ __forceinline__ void decode_tile(const void* __restrict__ k_seg, const void* __restrict__ v_seg, const uint8_t* __restrict__ ks_seg,
                                            const uint8_t* __restrict__ vs_seg, int tt, int n, int cap, const bf16x8 (&qf)[DP / 32], float c_exp, int j,
                                            int g, float& m_run, float& l_run, f32x4 (&acc)[DP / 16]) {
    constexpr int KK = DP / 32, DT = DP / 16;
    const bool full = tt * 64 + 64 <= n;
    f32x4 sc[4];
    // all fragments of the tile first (32 loads of 16 bytes in flight per lane for bf16), then the arithmetic
    bf16x8 kf[F8 ? 1 : 4][F8 ? 1 : KK], vf[F8 ? 1 : 2][F8 ? 1 : DT];
    unsigned kw[F8 ? 4 : 1][2 * KK];
    u32x4 vw[F8 ? DT : 1], ksw = {}, vsw = {};
    if constexpr (F8) {
        const uint8_t* kb = (const uint8_t*)k_seg + (int64_t)(tt * 64 + 16 * (j >> 2) + (j & 3)) * DP;
        const uint8_t* vb = (const uint8_t*)v_seg + (int64_t)tt * 64 + 16 * g;
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            if constexpr (DP == 32) {
                const uint2 t2 = *reinterpret_cast<const uint2*>(kb + 4 * st * DP + 8 * g);
                kw[st][0] = t2.x; kw[st][1] = t2.y;
            } else {
#pragma unroll
                for (int h = 0; h < KK / 2; ++h) {
                    const u32x4 t4 = *reinterpret_cast<const u32x4*>(kb + 4 * st * DP + 64 * h + 16 * g);
#pragma unroll
                    for (int i = 0; i < 4; ++i) kw[st][4 * h + i] = t4[i];
                }
            }
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) vw[dt] = *reinterpret_cast<const u32x4*>(vb + (int64_t)(16 * dt + j) * cap);
        ksw = *reinterpret_cast<const u32x4*>(ks_seg + tt * 64 + 16 * g);
        vsw = *reinterpret_cast<const u32x4*>(vs_seg + tt * 64 + 16 * g);
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            sc[st] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                sc[st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(e4m3x8_to_bf16(kw[st][2 * kk], kw[st][2 * kk + 1]), qf[kk], sc[st], 0, 0, 0);
        }
    } else {
        // A rows of S: lane row i = j <-> key offset 8 (i / 4) + (i % 4) inside a 32-key half, + 4 for the odd sub-tile
        const int krow = 8 * (j >> 2) + (j & 3);
        const bf16_t* kb = (const bf16_t*)k_seg + (int64_t)tt * 64 * DP + 8 * g;
        const bf16_t* vb = (const bf16_t*)v_seg + (int64_t)tt * 64 + 8 * g;
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                kf[st][kk] = *reinterpret_cast<const bf16x8*>(kb + (int64_t)(32 * (st >> 1) + 4 * (st & 1) + krow) * DP + 32 * kk);
#pragma unroll
        for (int hv = 0; hv < 2; ++hv)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) vf[hv][dt] = *reinterpret_cast<const bf16x8*>(vb + (int64_t)(16 * dt + j) * cap + 32 * hv);
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            sc[st] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) sc[st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[st][kk], qf[kk], sc[st], 0, 0, 0);
        }
    }
    // lane (head j, g): sc[st][r] is the key 32 (st / 2) + 8 g + 4 (st % 2) + r of the tile (F8: 16 g + 4 st + r)
    float mx = -INFINITY;
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = F8 ? 16 * g + 4 * st + r : 32 * (st >> 1) + 8 * g + 4 * (st & 1) + r;
            const bool ok = full || tt * 64 + key < n;
            float s = sc[st][r];
            if constexpr (F8) s *= e8m0_byte_to_f32(ksw[st], r);
            sc[st][r] = ok ? s * c_exp : -INFINITY;                   // a select: what a key behind the prefix holds goes no further
            mx = fmaxf(mx, sc[st][r]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);                          // every tile holds at least one valid key
    const float alpha = exp2f(m_run - m_new);
    m_run = m_new;
    if (F8 && !full) {                                             // code and scale bytes behind the valid prefix -> 0 (0 x garbage must stay 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int nv = n - (tt * 64 + 16 * g + 4 * i);         // valid keys among the word's four
            const unsigned keep = nv >= 4 ? ~0u : (nv <= 0 ? 0u : (1u << (8 * nv)) - 1u);
            vsw[i] &= keep;
#pragma unroll
            for (int dt = 0; dt < (F8 ? DT : 1); ++dt) vw[dt][i] &= keep;
        }
    }
    float psum = 0.f;
    bf16x8 pf[2];
#pragma unroll
    for (int hv = 0; hv < 2; ++hv) {
        float p[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            p[e] = exp2f(sc[2 * hv + (e >> 2)][e & 3] - m_new);
            psum += p[e];
            if constexpr (F8) p[e] *= e8m0_byte_to_f32(vsw[2 * hv + (e >> 2)], e & 3);      // after the sum took the unscaled p
        }
        pf[hv] = __builtin_bit_cast(bf16x8, u32x4{pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), pack_bf16x2(p[4], p[5]), pack_bf16x2(p[6], p[7])});
    }
    l_run = l_run * alpha + psum;
    if (!F8 && !full) {                                            // keys behind the valid prefix: 0 x garbage must stay 0
#pragma unroll
        for (int hv = 0; hv < 2; ++hv)
#pragma unroll
            for (int dt = 0; dt < (F8 ? 1 : DT); ++dt) {
                typedef short s16x8 __attribute__((ext_vector_type(8)));
                s16x8 v = __builtin_bit_cast(s16x8, vf[hv][dt]);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = tt * 64 + 32 * hv + 8 * g + e < n ? v[e] : (short)0;
                vf[hv][dt] = __builtin_bit_cast(bf16x8, v);
            }
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        acc[dt] *= alpha;
#pragma unroll
        for (int hv = 0; hv < 2; ++hv) {
            if constexpr (F8) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(e4m3x8_to_bf16(vw[dt][2 * hv], vw[dt][2 * hv + 1]), pf[hv], acc[dt], 0, 0, 0);
            else acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[hv][dt], pf[hv], acc[dt], 0, 0, 0);
        }
    }
}

// P8: the prompt segment is the fp8 form (kp / vtp: e4m3 bytes, kps / vps: their scale bytes [B0][kv heads][Tp]); the generated
// segment's tiles are the bf16 ones either way.
template <int DP, int GH, int NW, bool P8>
__global__ void __launch_bounds__(NW * 64) attn_decode_mfma_kernel(const bf16_t* __restrict__ q, const void* __restrict__ kp,
                                                               const void* __restrict__ vtp, const bf16_t* __restrict__ kg,
                                                               const bf16_t* __restrict__ vtg, const uint8_t* __restrict__ kps,
                                                               const uint8_t* __restrict__ vps, const int32_t* __restrict__ prompt_len,
                                                               const int32_t* __restrict__ step_ptr, int step_stride, int group, int nh, int nkv, int G,
                                                               int Tp, int Gcap, float c_exp, bf16_t* __restrict__ out, int64_t ld_out, int d) {
    constexpr int PW = DP + 2, KK = DP / 32, DT = DP / 16, EP = P8 ? 1 : 2;       // EP: bytes per element of the prompt segment
    __shared__ float red[NW][GH][PW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
    const int pair = blockIdx.x, bb = pair / nkv, kvh = pair - bb * nkv, b0 = bb / group;
    const int hc = blockIdx.y;
    const int h0 = kvh * G + hc * GH, nhead = min(GH, G - hc * GH);
    const bf16x8 zero8 = {};
    const bf16_t* qrow = q + ((int64_t)bb * nh + h0 + j) * DP;
    auto load_q = [&](bf16x8 (&qf)[KK], bool f8_order) {            // B operand of S: head slot j, features 32 kk + 8 g .. (or the F8 tiles' order)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int f = f8_order && DP > 32 ? 64 * (kk >> 1) + 16 * g + 8 * (kk & 1) : 32 * kk + 8 * g;
            qf[kk] = j < nhead ? *reinterpret_cast<const bf16x8*>(qrow + f) : zero8;
        }
    };
    bf16x8 qf[KK];
    load_q(qf, P8);
    const int n0 = min(max(prompt_len[b0], 0), Tp), n1 = min(max(step_ptr[(int64_t)bb * step_stride], 0) + 1, Gcap);
    const int tiles0 = (n0 + 63) >> 6, tiles = tiles0 + ((n1 + 63) >> 6);
    const char* k_seg0 = (const char*)kp + ((int64_t)b0 * nkv + kvh) * Tp * DP * EP;
    const bf16_t* k_seg1 = kg + ((int64_t)bb * nkv + kvh) * Gcap * DP;
    const char* v_seg0 = (const char*)vtp + ((int64_t)b0 * nkv + kvh) * DP * Tp * EP;
    const bf16_t* v_seg1 = vtg + ((int64_t)bb * nkv + kvh) * DP * Gcap;
    const uint8_t* ks_seg0 = P8 ? kps + ((int64_t)b0 * nkv + kvh) * Tp : nullptr;
    const uint8_t* vs_seg0 = P8 ? vps + ((int64_t)b0 * nkv + kvh) * Tp : nullptr;
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (P8) {
        // a wave's tiles in the same order as below: its prompt tiles, then (q in the bf16 tiles' feature order) its generated ones
        int t = w;
        for (; t < tiles0; t += NW) decode_tile<DP, true>(k_seg0, v_seg0, ks_seg0, vs_seg0, t, n0, Tp, qf, c_exp, j, g, m_run, l_run, acc);
        if (t < tiles) load_q(qf, false);
        for (; t < tiles; t += NW) decode_tile<DP, false>(k_seg1, v_seg1, nullptr, nullptr, t - tiles0, n1, Gcap, qf, c_exp, j, g, m_run, l_run, acc);
    } else {
        for (int t = w; t < tiles; t += NW) {
            const int sg = t >= tiles0, tt = sg ? t - tiles0 : t;
            decode_tile<DP, false>(sg ? (const void*)k_seg1 : (const void*)k_seg0, sg ? (const void*)v_seg1 : (const void*)v_seg0, nullptr, nullptr, tt,
                                   sg ? n1 : n0, sg ? Gcap : Tp, qf, c_exp, j, g, m_run, l_run, acc);
        }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (j < GH) {                                                     // lane (head j, g) holds the features 16 dt + 4 g + r of its head
        if (g == 0) { red[w][j][DP] = m_run; red[w][j][DP + 1] = l_run; }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[w][j][16 * dt + 4 * g + r] = acc[dt][r];
    }
    __syncthreads();
    decode_merge<bf16_t, DP, GH, NW>(red, bb, h0, nhead, d, out, ld_out);
}

// ---------------------------------------------------------------------------------------------
// token selection (greedy) and step bookkeeping
// ---------------------------------------------------------------------------------------------
// torch.argmax semantics over the first V columns (lowest index among equal maxima), then HF's finished-row rule
// (generation/utils.py, _sample: next = next * unfinished + pad * (1 - unfinished); a row finishes once it emits an eos id).
// argmax of one logits row by a block of 1024 threads; thread 0 returns it (the other threads' value is their wave's or their own)
template <typename T>
__device__ __forceinline__ int greedy_argmax(const T* __restrict__ row, int64_t ld, int V) {
    constexpr int PN = Piece<T>::N, kNone = 0x7fffffff;
    __shared__ float bv[16];
    __shared__ int bi[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float best = -INFINITY;
    int idx = kNone;
    auto take = [&](float v, int c) {                   // ascending c per thread: a later equal value never replaces an earlier one
        if (idx == kNone || v > best) { best = v; idx = c; }
    };
    const int Vv = (ld % PN == 0) ? V / PN * PN : 0;     // 16-byte pieces while the row pitch keeps them aligned
    for (int c = tid * PN; c < Vv; c += 1024 * PN) {
        float v[PN];
        load_piece<T, PN>(row + c, v);
#pragma unroll
        for (int e = 0; e < PN; ++e) take(v[e], c + e);
    }
    for (int c = Vv + tid; c < V; c += 1024) take(to_f32(row[c]), c);
    auto better = [](float v, int i, float bvv, int bii) { return i != kNone && (bii == kNone || v > bvv || (v == bvv && i < bii)); };
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(best, o, 64);
        const int i2 = __shfl_xor(idx, o, 64);
        if (better(v, i2, best, idx)) { best = v; idx = i2; }
    }
    if (lane == 0) { bv[w] = best; bi[w] = idx; }
    __syncthreads();
    if (tid == 0) {
        for (int ww = 1; ww < 16; ++ww)
            if (better(bv[ww], bi[ww], best, idx)) { best = bv[ww]; idx = bi[ww]; }
    }
    return idx;
}

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

// Staging row i's prompt segment -> slot tab.slot[i] of the engine's cache, every layer: per (layer, i) the kv heads of a tensor are ONE
// contiguous run in both caches (K [kv][Tp][dp], V^T [kv][dp][Tp], the scale bytes [kv][Tp]), a multiple of 16 bytes since Tp % 64 == 0.
// grid (pieces, layers * k, tensors): 16-byte loads and stores, whole capacity Tp -- nothing of the slot's previous occupant stays.
// The slots and limits travel in the launch's arguments (host arrays, checked there): no copy, no allocation.
constexpr int kSlotLoadMax = 256;
struct SlotTable { int32_t slot[kSlotLoadMax]; int32_t limit[kSlotLoadMax]; };

__global__ void __launch_bounds__(256) kv_slot_load_kernel(const char* __restrict__ ks, const char* __restrict__ vs, const char* __restrict__ kss,
                                                           const char* __restrict__ vss, char* __restrict__ kd, char* __restrict__ vd, char* __restrict__ ksd,
                                                           char* __restrict__ vsd, int64_t seg_bytes, int64_t scale_bytes, int k, int B0,
                                                           const int32_t* __restrict__ len_src, int32_t* __restrict__ len_dst, int32_t* __restrict__ row_step,
                                                           int32_t* __restrict__ finished, int32_t* __restrict__ row_limit, SlotTable tab) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const int l = blockIdx.y / k, i = blockIdx.y - l * k, which = blockIdx.z;
    const int slot = tab.slot[i];                        // 0 .. B0 - 1, distinct: checked on the host before the launch
    const int64_t n = which < 2 ? seg_bytes : scale_bytes;
    const char* src = (which == 0 ? ks : which == 1 ? vs : which == 2 ? kss : vss) + ((int64_t)l * k + i) * n;
    char* dst = (which == 0 ? kd : which == 1 ? vd : which == 2 ? ksd : vsd) + ((int64_t)l * B0 + slot) * n;
    for (int64_t o = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16; o < n; o += (int64_t)gridDim.x * 256 * 16)
        *reinterpret_cast<u32x4*>(dst + o) = *reinterpret_cast<const u32x4*>(src + o);
    if (blockIdx.x == 0 && blockIdx.y == 0 && which == 0) {
        for (int j = threadIdx.x; j < k; j += 256) {
            const int s = tab.slot[j];
            len_dst[s] = len_src[j];
            row_step[s] = 0;
            finished[s] = 0;
            row_limit[s] = tab.limit[j];
        }
    }
}

// beam re-ordering of the generated segment: grid (layers * BB * kv_heads)
template <typename T>
__global__ void __launch_bounds__(256) kv_reorder_kernel(const T* __restrict__ ks, const T* __restrict__ vs, T* __restrict__ kd, T* __restrict__ vd,
                                                         const int64_t* __restrict__ src_row, const int32_t* __restrict__ step_ptr, int BB, int nkv,
                                                         int dp, int G) {
    const int n = min(max(step_ptr[0], 0), G);
    const int idx = blockIdx.x, kvh = idx % nkv, r = (idx / nkv) % BB, l = idx / (nkv * BB);
    int64_t sr = src_row[r];
    if (sr < 0 || sr >= BB) sr = r;
    const int64_t to = (((int64_t)l * BB + r) * nkv + kvh) * (int64_t)G * dp, from = (((int64_t)l * BB + sr) * nkv + kvh) * (int64_t)G * dp;
    for (int i = threadIdx.x; i < n * dp; i += 256) kd[to + i] = ks[from + i];
    for (int i = threadIdx.x; i < n * dp; i += 256) {
        const int c = i / n, j = i - c * n;
        vd[to + (int64_t)c * G + j] = vs[from + (int64_t)c * G + j];
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
    int ZC, GH;
};

int pick_gh(int G) { return G <= 1 ? 1 : (G <= 2 ? 2 : (G <= 4 ? 4 : 8)); }

// GH query heads of a GQA group per block, ZC chunks of them (more than 8 heads per kv head: the keys are read once per chunk)
void attn_decode_plan(int nh, int nkv, int* ZC, int* GH) {
    const int G = nh / nkv;
    *GH = pick_gh(G);
    *ZC = (G + *GH - 1) / *GH;
}

size_t decode_plan(const p2t_llama_config* c, int BB, int Tp, int Gcap, Arena* ar, DecodeBuffers* b) {
    const size_t e = dtype_size(c->dtype);
    const int64_t H = c->hidden, F = c->ffn, Hp = round_up(H, 64), Fp = round_up(F, 64);
    const int d = c->head_dim, dp = head_dim_padded(d), nh = c->heads, nkv = c->kv_heads;
    const int64_t QO = round_up((int64_t)nh * d, 64), NQKV = (int64_t)(nh + 2 * nkv) * d;
    Arena local(nullptr, ~(size_t)0 >> 1);
    Arena& a = ar ? *ar : local;
    DecodeBuffers t;
    attn_decode_plan(nh, nkv, &t.ZC, &t.GH);
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

template <typename T>
int launch_attn_decode_t(const DecodeBuffers& b, const p2t_kv_cache* kc, int layer, int BB, int nh, int nkv, int d, int dp, float c_exp, int round_p,
                         int64_t QO, hipStream_t s, int use_mfma = 1, int step_stride = 0) {
    const int G = nh / nkv;
    const size_t per_p = (size_t)kc->B0 * nkv * kc->Tp * dp, per_g = (size_t)BB * nkv * kc->G * dp;
    const T* kp = (const T*)kc->k_prompt + per_p * layer;
    const T* vtp = (const T*)kc->vt_prompt + per_p * layer;
    const T* kg = (const T*)kc->k_gen + per_g * layer;
    const T* vtg = (const T*)kc->vt_gen + per_g * layer;
    const dim3 grid((unsigned)(BB * nkv), (unsigned)b.ZC);
    if constexpr (sizeof(T) == 2) {
        if (use_mfma) {                      // (0: the lane-per-key kernel below, the form every dtype can run)
            // the fp8 prompt segment (the cache carries scales): the same index order in bytes, one scale byte per key
            const size_t per_s = (size_t)kc->B0 * nkv * kc->Tp;
            const uint8_t* kp8 = (const uint8_t*)kc->k_prompt + per_p * layer;
            const uint8_t* vtp8 = (const uint8_t*)kc->vt_prompt + per_p * layer;
            const uint8_t* kps = kc->k_prompt_scale ? kc->k_prompt_scale + per_s * layer : nullptr;
            const uint8_t* vps = kc->k_prompt_scale ? kc->v_prompt_scale + per_s * layer : nullptr;
#define P2T_ADM(DPV, GHV, P8V)                                                                                                        \
    attn_decode_mfma_kernel<DPV, GHV, (GHV <= 4 && DPV <= 64 ? 16 : 8), P8V><<<grid, (GHV <= 4 && DPV <= 64 ? 16 : 8) * 64, 0, s>>>(    \
        (const bf16_t*)b.qb, P8V ? (const void*)kp8 : (const void*)kp, P8V ? (const void*)vtp8 : (const void*)vtp, (const bf16_t*)kg,  \
        (const bf16_t*)vtg, kps, vps, kc->prompt_len, kc->step, step_stride, kc->group, nh, nkv, G, kc->Tp, kc->G, c_exp, (bf16_t*)b.ao, QO, d)
#define P2T_ADM_G(DPV, P8V)                                                                                                           \
    do {                                                                                                                              \
        if (b.GH == 1) P2T_ADM(DPV, 1, P8V); else if (b.GH == 2) P2T_ADM(DPV, 2, P8V); else if (b.GH == 4) P2T_ADM(DPV, 4, P8V);       \
        else P2T_ADM(DPV, 8, P8V);                                                                                                    \
    } while (0)
            if (kps) {
                if (dp == 32) P2T_ADM_G(32, true); else if (dp == 64) P2T_ADM_G(64, true); else P2T_ADM_G(128, true);
            } else {
                if (dp == 32) P2T_ADM_G(32, false); else if (dp == 64) P2T_ADM_G(64, false); else P2T_ADM_G(128, false);
            }
#undef P2T_ADM_G
#undef P2T_ADM
            P2T_LAUNCH_CHECK();
            return P2T_OK;
        }
    }
    P2T_REQUIRE(!kc->k_prompt_scale, "attention over an fp8 prompt segment: the matrix-pipe kernel only");
#define P2T_AD(DPV, GHV)                                                                                                              \
    attn_decode_kernel<T, DPV, GHV><<<grid, 512, 0, s>>>((const T*)b.qb, kp, vtp, kg, vtg, kc->prompt_len, kc->step, step_stride, kc->group, nh, nkv, G, \
                                                         kc->Tp, kc->G, c_exp, round_p, (T*)b.ao, QO, d)
#define P2T_AD_G(DPV)                                                                                                                 \
    do {                                                                                                                              \
        if (b.GH == 1) P2T_AD(DPV, 1); else if (b.GH == 2) P2T_AD(DPV, 2); else if (b.GH == 4) P2T_AD(DPV, 4); else P2T_AD(DPV, 8);      \
    } while (0)
    if (dp == 32) P2T_AD_G(32); else if (dp == 64) P2T_AD_G(64); else P2T_AD_G(128);
#undef P2T_AD_G
#undef P2T_AD
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

int check_cache(const p2t_llama_config* c, const p2t_kv_cache* kc, const char* who) {
    P2T_REQUIRE(kc && kc->k_prompt && kc->vt_prompt && kc->k_gen && kc->vt_gen && kc->prompt_len && kc->step, "%s: null cache field", who);
    P2T_REQUIRE(kc->B0 > 0 && kc->group > 0 && kc->Tp > 0 && kc->G > 0 && kc->Tp % 64 == 0 && kc->G % 64 == 0,
                "%s: cache capacities must be positive multiples of 64 (Tp %d, G %d)", who, kc->Tp, kc->G);
    P2T_REQUIRE(c->heads % c->kv_heads == 0 && c->head_dim % 2 == 0 && c->head_dim <= 128, "%s: unsupported head shape", who);
    P2T_REQUIRE(!kc->k_prompt_scale == !kc->v_prompt_scale, "%s: k_prompt_scale and v_prompt_scale go together (the fp8 prompt segment)", who);
    if (kc->k_prompt_scale && c->dtype != P2T_BF16) {
        set_error("%s: the fp8 prompt segment serves bf16 models only", who);
        return P2T_ERR_UNSUPPORTED;
    }
    P2T_REQUIRE(!kc->k_prompt_scale || (((uintptr_t)kc->k_prompt | (uintptr_t)kc->vt_prompt | (uintptr_t)kc->k_prompt_scale | (uintptr_t)kc->v_prompt_scale) & 15) == 0,
                "%s: the fp8 prompt segment's buffers must be 16-byte aligned", who);
    return P2T_OK;
}

int launch_kv_quant_store(const void* k, const void* v, int BH, int T, int d, int Tp, uint8_t* kq, uint8_t* vtq, uint8_t* ks, uint8_t* vs, hipStream_t s) {
    const int dp = head_dim_padded(d);
    const dim3 grid((unsigned)ceil_div(T, 64), (unsigned)BH);
#define P2T_KVQ(DPV) kv_quant_store_kernel<DPV><<<grid, 256, 0, s>>>((const bf16_t*)k, (const bf16_t*)v, kq, vtq, ks, vs, T, d, Tp)
    if (dp == 32) P2T_KVQ(32); else if (dp == 64) P2T_KVQ(64); else P2T_KVQ(128);
#undef P2T_KVQ
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

}  // namespace

// prefill hook of llama_forward_impl (towers.hip): layer l's rotated keys / values -> prompt segment
int llama_kv_store(const p2t_llama_config* c, const p2t_kv_cache* kc, int layer, const void* k, const void* v, int B, int T, hipStream_t s) {
    const int dp = head_dim_padded(c->head_dim), nkv = c->kv_heads;
    const size_t e = dtype_size(c->dtype), per = (size_t)kc->B0 * nkv * kc->Tp * dp;
    if (kc->k_prompt_scale) {                 // fp8 prompt segment: codes + scales of both in one launch (check_cache: a bf16 model)
        const size_t per_s = (size_t)kc->B0 * nkv * kc->Tp;
        return launch_kv_quant_store(k, v, B * nkv, T, c->head_dim, kc->Tp, (uint8_t*)kc->k_prompt + per * layer, (uint8_t*)kc->vt_prompt + per * layer,
                                     kc->k_prompt_scale + per_s * layer, kc->v_prompt_scale + per_s * layer, s);
    }
    char* kd = (char*)kc->k_prompt + per * layer * e;
    P2T_CHECK_HIP(hipMemcpy2DAsync(kd, (size_t)kc->Tp * dp * e, k, (size_t)T * dp * e, (size_t)T * dp * e, (size_t)B * nkv, hipMemcpyDeviceToDevice, s));
    const dim3 grid((unsigned)ceil_div(T, 64), (unsigned)(B * nkv));
    if (c->dtype == P2T_BF16)
        v_transpose_store_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)v, (bf16_t*)kc->vt_prompt + per * layer, T, dp, kc->Tp);
    else
        v_transpose_store_kernel<float><<<grid, 256, 0, s>>>((const float*)v, (float*)kc->vt_prompt + per * layer, T, dp, kc->Tp);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_compact_rows(const float* x, const int64_t* mask, int B, int T, int H, float* out, int64_t* out_mask, int32_t* lens,
                                int32_t* scratch, p2t_stream stream) {
    P2T_REQUIRE(x && mask && out && out_mask && lens && scratch && B > 0 && T > 0 && H > 0 && H % 4 == 0 && x != out,
                "p2t_compact_rows: bad arguments (H must be a multiple of 4, out of place)");
    hipStream_t s = (hipStream_t)stream;
    P2T_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * T * H, s));
    compact_index_kernel<<<B, 256, 0, s>>>(mask, T, scratch, out_mask, lens);
    P2T_LAUNCH_CHECK();
    compact_copy_kernel<<<dim3((unsigned)T, (unsigned)B), 256, 0, s>>>(x, scratch, T, H, out);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

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

// mx: the MXFP4 form of the projections (p2t_llama_decode_step_mxfp4; a gemm_fp8 model, at most 64 rows) or nullptr
static int decode_step_impl(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers, const p2t_llama_layer_mxfp4* mx,
                            const void* lm_head, int64_t ld_head, int lm_head_preshuffled, const p2t_kv_cache* cache, const float* x_in, void* logits,
                            int64_t ld_logits, int flags, void* workspace, size_t workspace_bytes, p2t_stream stream, const p2t_lm_head_q* head_q = nullptr,
                            const char* who = "p2t_llama_decode_step", int32_t* row_step = nullptr, const int32_t* frozen = nullptr) {
    P2T_REQUIRE(c && w && w->layers && w->final_norm_w && (lm_head || head_q) && x_in && logits && workspace, "%s: null argument", who);
    const bool fuse_rope = !(flags & P2T_DECODE_NO_ROPE_FUSION);
    // per-row counters (p2t_llama_decode_step_rows): the same launches read row_step[row] where the lock-step ones read step[0]; the
    // cache's own counter is neither read nor written
    p2t_kv_cache rows_cache;
    const int sstride = row_step ? 1 : 0;
    if (row_step) {
        P2T_REQUIRE(cache, "%s: null cache", who);
        rows_cache = *cache;
        rows_cache.step = row_step;
        cache = &rows_cache;
    }
    P2T_TRY(check_cache(c, cache, who));
    if (row_step && cache->group != 1) {
        set_error("%s: per-row counters serve group == 1 only (got %d)", who, cache->group);
        return P2T_ERR_UNSUPPORTED;
    }
    P2T_REQUIRE(!c->gemm_fp8 || c->dtype == P2T_BF16, "%s: gemm_fp8 needs bf16 activations (dtype = P2T_BF16)", who);
    const int BB = cache->B0 * cache->group;
    const int dt = c->dtype;
    const int64_t H = c->hidden, F = c->ffn, Hp = round_up(H, 64), Fp = round_up(F, 64);
    const int d = c->head_dim, dp = head_dim_padded(d), nh = c->heads, nkv = c->kv_heads;
    const int64_t NQKV = (int64_t)(nh + 2 * nkv) * d, QO = round_up((int64_t)nh * d, 64);
    P2T_REQUIRE((head_q || lm_head_preshuffled || ld_head >= Hp) && ld_logits >= c->vocab, "%s: ld_head %lld < %lld or ld_logits %lld < vocab", who, (long long)ld_head,
                (long long)Hp, (long long)ld_logits);
    // the quantised head: every refusal before the first launch; its e4m3 rows + row scales sit behind the step's own buffers
    if (head_q) P2T_TRY(lm_head_q_check(head_q, BB, H, c->vocab, ld_logits, dt, who));
    P2T_REQUIRE(workspace_bytes >= decode_plan(c, BB, cache->Tp, cache->G, nullptr, nullptr) + (head_q ? lm_head_q_ws_bytes(BB, H) : 0),
                "%s: workspace too small", who);
    hipStream_t s = (hipStream_t)stream;
    Arena ar(workspace, workspace_bytes);
    DecodeBuffers b;
    decode_plan(c, BB, cache->Tp, cache->G, &ar, &b);
    uint8_t* head_aq = head_q ? (uint8_t*)ar.take((size_t)BB * lm_head_q_kq(H)) : nullptr;
    uint8_t* head_as = head_q ? (uint8_t*)ar.take((size_t)BB) : nullptr;
    P2T_REQUIRE(!ar.overflow, "%s: workspace overflow", who);
    const float* inv_freq = w->inv_freq;
    if (!inv_freq) {
        P2T_TRY(launch_inv_freq(b.inv_freq, d / 2, c->rope_theta, c->rope_llama3, c->rope_factor, c->rope_low_freq_factor, c->rope_high_freq_factor,
                                (float)c->rope_original_max_pos, s));
        inv_freq = b.inv_freq;
    }
    const float scale = 1.0f / sqrtf((float)d);
    const int l2s = dt == P2T_BF16;                      // as the prefill: scale * log2(e) folded into q for bf16 models
    const float q_fold = l2s ? scale * kLog2e : 1.0f, c_exp = l2s ? 1.0f : scale * kLog2e;
    P2T_CHECK_HIP(hipMemcpyAsync(b.x, x_in, sizeof(float) * (size_t)BB * H, hipMemcpyDeviceToDevice, s));
    P2T_CHECK_HIP(hipMemsetAsync(b.ao, 0, dtype_size(dt) * (size_t)BB * QO, s));
    // the SwiGLU epilogues write columns [0, F) of act and the down projection reads K = Fp of them against zero weight columns: what
    // the caller's workspace held in [F, Fp) must not reach it (NaN x 0)
    if (Fp > F) P2T_CHECK_HIP(hipMemsetAsync(b.act, 0, dtype_size(dt) * (size_t)BB * Fp, s));
    const int64_t M = BB;
    // the step's projections: the weight-streaming kernel (gemm_skinny.hip) for bf16 models, the general GEMM otherwise
    // `pre`: the pre-shuffled stream copy of the same weight (p2t_preshuffle_w), when the caller built one
    auto gemm_nt = [&](const GemmArgs& a, hipStream_t st, const void* pre = nullptr) {
        const int r = launch_gemm_skinny(a.A, a.lda, pre ? pre : a.W, a.ldw, a.out, a.ldc, a.M, a.N, a.K, a.dtype, a.out_dtype, a.epilogue, st, pre != nullptr);
        return r == P2T_ERR_UNSUPPORTED ? p2t::gemm_nt(a, st) : r;
    };
    const bool stream_w = ws_layers && dt == P2T_BF16;
    // gemm_fp8 models (e4m3 weights AND GEMM operands, bf16 activations elsewhere): the same step with every
    // projection on the e4m3 stream (half the weight bytes of a step); rows are quantised by the RMSNorm / a quantise pass as in the prefill
    const int64_t Hq = round_up(H, 128), Fq = round_up(F, 128), QOq = round_up((int64_t)nh * d, 128);
    struct MxProj { const void* w; const uint8_t* bs; };   // one projection of p2t_llama_layer_mxfp4; w == nullptr: the e4m3 stream
    auto gemm8 = [&](const uint8_t* A, int64_t lda, const uint8_t* as, const void* W, const uint8_t* wsc, const void* pre, void* out, int64_t ldc,
                     int64_t N, int64_t K, int out_dtype, int epi, const SkinnyRope* ra, hipStream_t st, MxProj m4 = MxProj{nullptr, nullptr}) {
        // no general 4-bit GEMM behind this one: only the fused-rotation form may answer UNSUPPORTED (the caller then takes two launches)
        if (m4.w) return launch_gemm_skinny_mxfp4(A, lda, as, m4.w, K / 2, m4.bs, out, ldc, M, N, K, out_dtype, epi, ra, st, mx->stream_order != 0);
        const int r = launch_gemm_skinny_fp8(A, lda, as, pre ? pre : W, K, wsc, out, ldc, M, N, K, out_dtype, epi, ra, st, pre != nullptr);
        if (r != P2T_ERR_UNSUPPORTED || ra) return r;
        GemmArgs g = gemm_args_fp8(A, lda, as, W, wsc, M, N, K, out, ldc, out_dtype, epi);
        if (epi == P2T_EPI_STORE_F32) g.n_zero = (int)N;
        return p2t::gemm_nt(g, st);
    };
    for (int l = 0; c->gemm_fp8 && l < c->n_layers; ++l) {
        const p2t_llama_layer& L = w->layers[l];
        P2T_REQUIRE(L.qkv_ws && L.o_ws && L.gu_ws && L.down_ws, "%s: gemm_fp8 needs the row scales of layer %d", who, l);
        P2T_REQUIRE(!L.q_norm_w == !L.k_norm_w, "%s: q_norm_w and k_norm_w go together (layer %d)", who, l);
        const int fused_prefill = !L.q_norm_w && (d == 64 || d == 128);
        const p2t_llama_layer_stream* S = ws_layers ? ws_layers + l : nullptr;
        const MxProj xq{mx ? mx[l].qkv_w : nullptr, mx ? mx[l].qkv_bs : nullptr}, xo{mx ? mx[l].o_w : nullptr, mx ? mx[l].o_bs : nullptr},
            xg{mx ? mx[l].gu_w : nullptr, mx ? mx[l].gu_bs : nullptr}, xd{mx ? mx[l].down_w : nullptr, mx ? mx[l].down_bs : nullptr};
        P2T_REQUIRE(!mx || (xq.w && xo.w && xg.w && xd.w && (mx->stream_order || (xq.bs && xo.bs && xg.bs && xd.bs))),
                    "p2t_llama_decode_step_mxfp4: null codes / block scales in layer %d", l);
        const size_t per_g = (size_t)BB * nkv * cache->G * dp;
        P2T_TRY(launch_rmsnorm_fp8_few(b.x, H, L.ln1_w, c->rms_norm_eps, b.hq, Hq, b.hs, M, H, s));
        bool roped = false;
        if (fused_prefill && fuse_rope) {
            SkinnyRope ra;
            ra.inv_freq = inv_freq; ra.prompt_len = cache->prompt_len; ra.step = cache->step; ra.step_stride = sstride; ra.group = cache->group;
            ra.nh = nh; ra.nkv = nkv; ra.d = d; ra.G = cache->G; ra.q_scale = q_fold;
            ra.q = b.qb; ra.k = (bf16_t*)cache->k_gen + per_g * l; ra.vt = (bf16_t*)cache->vt_gen + per_g * l;
            const int r = gemm8(b.hq, Hq, b.hs, L.qkv_w, L.qkv_ws, S ? S->qkv_w : nullptr, nullptr, 0, NQKV, Hq, dt, 0, &ra, s, xq);
            if (r != P2T_ERR_UNSUPPORTED) { P2T_TRY(r); roped = true; }
        }
        if (!roped) {
            P2T_TRY(gemm8(b.hq, Hq, b.hs, L.qkv_w, L.qkv_ws, S ? S->qkv_w : nullptr, b.qkv, NQKV, NQKV, Hq, P2T_F32, P2T_EPI_STORE_F32, nullptr, s, xq));
            const unsigned grid = (unsigned)ceil_div((int64_t)BB * (nh + 2 * nkv), 4);
            rope_append_kernel<bf16_t><<<grid, 256, 0, s>>>(b.qkv, NQKV, inv_freq, L.q_norm_w, L.k_norm_w, c->rms_norm_eps, cache->prompt_len, cache->step,
                                                            sstride, cache->group, (bf16_t*)b.qb, (bf16_t*)cache->k_gen + per_g * l, (bf16_t*)cache->vt_gen + per_g * l,
                                                            BB, nh, nkv, d, dp, cache->G, q_fold, d == 128 && !L.q_norm_w, !fused_prefill);
            P2T_LAUNCH_CHECK();
        }
        P2T_TRY(launch_attn_decode_t<bf16_t>(b, cache, l, BB, nh, nkv, d, dp, c_exp, 1, QO, s, 1, sstride));
        P2T_TRY(launch_quant_rows_few(b.ao, dt, QO, M, (int64_t)nh * d, b.aoq, QOq, b.aos, s));
        P2T_TRY(gemm8(b.aoq, QOq, b.aos, L.o_w, L.o_ws, S ? S->o_w : nullptr, b.x, H, H, QOq, P2T_F32, P2T_EPI_RESID, nullptr, s, xo));
        P2T_TRY(launch_rmsnorm_fp8_few(b.x, H, L.ln2_w, c->rms_norm_eps, b.hq, Hq, b.hs, M, H, s));
        P2T_TRY(gemm8(b.hq, Hq, b.hs, L.gu_w, L.gu_ws, S ? S->gu_w : nullptr, b.act, Fp, 2 * F, Hq, dt, P2T_EPI_SWIGLU, nullptr, s, xg));
        P2T_TRY(launch_quant_rows_few(b.act, dt, Fp, M, F, b.actq, Fq, b.acts, s));
        P2T_TRY(gemm8(b.actq, Fq, b.acts, L.down_w, L.down_ws, S ? S->down_w : nullptr, b.x, H, H, Fq, P2T_F32, P2T_EPI_RESID, nullptr, s, xd));
    }
    for (int l = 0; !c->gemm_fp8 && l < c->n_layers; ++l) {
        const p2t_llama_layer& L = w->layers[l];
        P2T_REQUIRE(!L.q_norm_w == !L.k_norm_w, "%s: q_norm_w and k_norm_w go together (layer %d)", who, l);
        const int fused_prefill = !L.q_norm_w && (d == 64 || d == 128);
        P2T_TRY(launch_rmsnorm_few_rows(b.x, H, L.ln1_w, c->rms_norm_eps, b.h, Hp, M, H, dt, s));
        bool roped = false;
        if (fused_prefill && dt == P2T_BF16 && fuse_rope) {   // projection + rotation + cache append in one launch (SK_QKV_ROPE)
            const size_t per_g = (size_t)BB * nkv * cache->G * dp;
            SkinnyRope ra;
            ra.inv_freq = inv_freq; ra.prompt_len = cache->prompt_len; ra.step = cache->step; ra.step_stride = sstride; ra.group = cache->group;
            ra.nh = nh; ra.nkv = nkv; ra.d = d; ra.G = cache->G; ra.q_scale = q_fold;
            ra.q = b.qb; ra.k = (bf16_t*)cache->k_gen + per_g * l; ra.vt = (bf16_t*)cache->vt_gen + per_g * l;
            const int r = launch_gemm_skinny_qkv_rope(b.h, Hp, stream_w ? ws_layers[l].qkv_w : L.qkv_w, Hp, M, NQKV, Hp, ra, s, stream_w);
            if (r != P2T_ERR_UNSUPPORTED) { P2T_TRY(r); roped = true; }
        }
        if (!roped) {
            GemmArgs g1(b.h, Hp, L.qkv_w, Hp, M, NQKV, Hp, dt, b.qkv, NQKV, P2T_F32, P2T_EPI_STORE_F32);
            g1.n_zero = (int)NQKV;
            P2T_TRY(gemm_nt(g1, s, stream_w ? ws_layers[l].qkv_w : nullptr));
            {
                const unsigned grid = (unsigned)ceil_div((int64_t)BB * (nh + 2 * nkv), 4);
                const size_t per_g = (size_t)BB * nkv * cache->G * dp;
                if (dt == P2T_BF16)
                    rope_append_kernel<bf16_t><<<grid, 256, 0, s>>>(b.qkv, NQKV, inv_freq, L.q_norm_w, L.k_norm_w, c->rms_norm_eps, cache->prompt_len,
                                                                    cache->step, sstride, cache->group, (bf16_t*)b.qb, (bf16_t*)cache->k_gen + per_g * l,
                                                                    (bf16_t*)cache->vt_gen + per_g * l, BB, nh, nkv, d, dp, cache->G, q_fold,
                                                                    d == 128 && !L.q_norm_w, !fused_prefill);
                else
                    rope_append_kernel<float><<<grid, 256, 0, s>>>(b.qkv, NQKV, inv_freq, L.q_norm_w, L.k_norm_w, c->rms_norm_eps, cache->prompt_len,
                                                                   cache->step, sstride, cache->group, (float*)b.qb, (float*)cache->k_gen + per_g * l,
                                                                   (float*)cache->vt_gen + per_g * l, BB, nh, nkv, d, dp, cache->G, q_fold,
                                                                   d == 128 && !L.q_norm_w, 0);
                P2T_LAUNCH_CHECK();
            }
        }
        if (dt == P2T_BF16) P2T_TRY(launch_attn_decode_t<bf16_t>(b, cache, l, BB, nh, nkv, d, dp, c_exp, 1, QO, s, 1, sstride));
        else P2T_TRY(launch_attn_decode_t<float>(b, cache, l, BB, nh, nkv, d, dp, c_exp, 0, QO, s, 1, sstride));
        GemmArgs g2(b.ao, QO, L.o_w, QO, M, H, QO, dt, b.x, H, P2T_F32, P2T_EPI_RESID);
        P2T_TRY(gemm_nt(g2, s, stream_w ? ws_layers[l].o_w : nullptr));
        P2T_TRY(launch_rmsnorm_few_rows(b.x, H, L.ln2_w, c->rms_norm_eps, b.h, Hp, M, H, dt, s));
        GemmArgs g3(b.h, Hp, L.gu_w, Hp, M, 2 * F, Hp, dt, b.act, Fp, dt, P2T_EPI_SWIGLU);
        P2T_TRY(gemm_nt(g3, s, stream_w ? ws_layers[l].gu_w : nullptr));
        GemmArgs g4(b.act, Fp, L.down_w, Fp, M, H, Fp, dt, b.x, H, P2T_F32, P2T_EPI_RESID);
        P2T_TRY(gemm_nt(g4, s, stream_w ? ws_layers[l].down_w : nullptr));
    }
    if (head_q) {                                        // one more branch after the layer loops: the e4m3 / MXFP4 head on the residual stream
        P2T_TRY(lm_head_q_run(b.x, H, w->final_norm_w, c->rms_norm_eps, head_q, M, H, c->vocab, logits, ld_logits, head_aq, head_as, s));
        return launch_advance(cache->step, sstride, frozen, BB, s);
    }
    P2T_REQUIRE(!lm_head_preshuffled || dt == P2T_BF16, "%s: pre-shuffled weights are a bf16 layout", who);
    // the stream-order copy is only readable by the skinny kernels (<= 64 rows): beyond that the general GEMM would read the
    // shuffled tiles as a row-major [vocab, Hp] matrix and return wrong logits without an error
    P2T_REQUIRE(!lm_head_preshuffled || M <= 64, "%s: a pre-shuffled LM head serves at most 64 rows (got %lld): pass the row-major one", who,
                (long long)M);
    P2T_TRY(launch_rmsnorm_few_rows(b.x, H, w->final_norm_w, c->rms_norm_eps, b.h, Hp, M, H, dt, s));
    GemmArgs gh(b.h, Hp, lm_head, ld_head, M, c->vocab, Hp, dt, logits, ld_logits, dt, P2T_EPI_STORE);
    P2T_TRY(gemm_nt(gh, s, lm_head_preshuffled ? lm_head : nullptr));
    return launch_advance(cache->step, sstride, frozen, BB, s);
}

extern "C" int p2t_llama_decode_step(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers,
                                     const void* lm_head, int64_t ld_head, int lm_head_preshuffled, const p2t_kv_cache* cache, const float* x_in, void* logits, int64_t ld_logits, int flags, void* workspace,
                                     size_t workspace_bytes, p2t_stream stream) {
    return decode_step_impl(c, w, ws_layers, nullptr, lm_head, ld_head, lm_head_preshuffled, cache, x_in, logits, ld_logits, flags, workspace, workspace_bytes,
                            stream);
}

// The step of a gemm_fp8 model whose four projections per layer stream MXFP4 weights (include/p2t_hip.h): everything else -- the
// row quantisers, the attention, the bf16 LM head -- is p2t_llama_decode_step's.
extern "C" int p2t_llama_decode_step_mxfp4(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_mxfp4* mx_layers,
                                           const void* lm_head, int64_t ld_head, int lm_head_preshuffled, const p2t_kv_cache* cache, const float* x_in,
                                           void* logits, int64_t ld_logits, int flags, void* workspace, size_t workspace_bytes, p2t_stream stream) {
    P2T_REQUIRE(c && mx_layers && cache, "p2t_llama_decode_step_mxfp4: null argument");
    P2T_REQUIRE(c->gemm_fp8 && c->dtype == P2T_BF16, "p2t_llama_decode_step_mxfp4: needs a gemm_fp8 configuration with bf16 activations");
    P2T_REQUIRE((int64_t)cache->B0 * cache->group <= 64, "p2t_llama_decode_step_mxfp4: at most 64 rows (got %lld): beyond that the e4m3 weights serve",
                (long long)cache->B0 * cache->group);
    for (int l = 1; l < c->n_layers; ++l)
        P2T_REQUIRE(!mx_layers[l].stream_order == !mx_layers[0].stream_order, "p2t_llama_decode_step_mxfp4: layers differ in stream_order");
    return decode_step_impl(c, w, nullptr, mx_layers, lm_head, ld_head, lm_head_preshuffled, cache, x_in, logits, ld_logits, flags, workspace,
                            workspace_bytes, stream);
}

// Both steps behind one door, plus the quantised LM head: w_stream or mx_layers (either may be NULL, not both set); head_q == NULL is
// the existing step, launch for launch.
extern "C" int p2t_llama_decode_step_q(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers,
                                       const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                                       const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x_in, void* logits, int64_t ld_logits, int flags,
                                       void* workspace, size_t workspace_bytes, p2t_stream stream) {
    P2T_REQUIRE(!(ws_layers && mx_layers), "p2t_llama_decode_step_q: w_stream and mx_layers are two forms of the same projections: pass one");
    if (mx_layers) {
        P2T_REQUIRE(c && cache, "p2t_llama_decode_step_q: null argument");
        P2T_REQUIRE(c->gemm_fp8 && c->dtype == P2T_BF16, "p2t_llama_decode_step_q: mx_layers need a gemm_fp8 configuration with bf16 activations");
        P2T_REQUIRE((int64_t)cache->B0 * cache->group <= 64, "p2t_llama_decode_step_q: mx_layers serve at most 64 rows (got %lld): beyond that the e4m3 weights serve",
                    (long long)cache->B0 * cache->group);
        for (int l = 1; l < c->n_layers; ++l)
            P2T_REQUIRE(!mx_layers[l].stream_order == !mx_layers[0].stream_order, "p2t_llama_decode_step_q: layers differ in stream_order");
    }
    return decode_step_impl(c, w, ws_layers, mx_layers, lm_head, ld_head, lm_head_preshuffled, cache, x_in, logits, ld_logits, flags, workspace, workspace_bytes,
                            stream, head_q, "p2t_llama_decode_step_q");
}

// p2t_llama_decode_step_q for rows that carry their own counters (continuous batching, include/p2t_hip.h): the same launches, every
// `step[0]` read as row_step[row]; the last launch advances the rows that are not frozen.
extern "C" int p2t_llama_decode_step_rows(const p2t_llama_config* c, const p2t_llama_weights* w, const p2t_llama_layer_stream* ws_layers,
                                          const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                                          const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x_in, void* logits, int64_t ld_logits,
                                          int flags, void* workspace, size_t workspace_bytes, int32_t* row_step, const int32_t* frozen,
                                          p2t_stream stream) {
    P2T_REQUIRE(row_step, "p2t_llama_decode_step_rows: null row_step");
    P2T_REQUIRE(!(ws_layers && mx_layers), "p2t_llama_decode_step_rows: w_stream and mx_layers are two forms of the same projections: pass one");
    if (mx_layers) {
        P2T_REQUIRE(c && cache, "p2t_llama_decode_step_rows: null argument");
        P2T_REQUIRE(c->gemm_fp8 && c->dtype == P2T_BF16, "p2t_llama_decode_step_rows: mx_layers need a gemm_fp8 configuration with bf16 activations");
        P2T_REQUIRE((int64_t)cache->B0 * cache->group <= 64, "p2t_llama_decode_step_rows: mx_layers serve at most 64 rows (got %lld): beyond that the e4m3 weights serve",
                    (long long)cache->B0 * cache->group);
        for (int l = 1; l < c->n_layers; ++l)
            P2T_REQUIRE(!mx_layers[l].stream_order == !mx_layers[0].stream_order, "p2t_llama_decode_step_rows: layers differ in stream_order");
    }
    return decode_step_impl(c, w, ws_layers, mx_layers, lm_head, ld_head, lm_head_preshuffled, cache, x_in, logits, ld_logits, flags, workspace, workspace_bytes,
                            stream, head_q, "p2t_llama_decode_step_rows", row_step, frozen);
}

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

extern "C" int p2t_kv_slot_load(const p2t_llama_config* c, const p2t_kv_cache* staging, const p2t_kv_cache* cache, const int32_t* slots,
                                const int32_t* limits, int k, int32_t* row_step, int32_t* finished, int32_t* row_limit, p2t_stream stream) {
    P2T_REQUIRE(c && staging && cache && slots && limits && row_step && finished && row_limit, "p2t_kv_slot_load: null argument");
    P2T_REQUIRE(c->n_layers > 0 && c->kv_heads > 0, "p2t_kv_slot_load: empty model");
    p2t_kv_cache from = *staging, to = *cache;           // neither cache's own counter is read or written: the rows' counters stand in for the check
    from.step = to.step = row_step;
    P2T_TRY(check_cache(c, &from, "p2t_kv_slot_load (staging)"));
    P2T_TRY(check_cache(c, &to, "p2t_kv_slot_load"));
    P2T_REQUIRE(cache->group == 1, "p2t_kv_slot_load: group == 1 only (got %d)", cache->group);
    P2T_REQUIRE(staging->Tp == cache->Tp, "p2t_kv_slot_load: the staging cache holds %d prompt tokens per row, the engine's %d", staging->Tp, cache->Tp);
    P2T_REQUIRE(!staging->k_prompt_scale == !cache->k_prompt_scale,
                "p2t_kv_slot_load: the two caches differ in the prompt segment's format (scale arrays on one of them only)");
    P2T_REQUIRE(k > 0 && k == staging->B0 && k <= cache->B0, "p2t_kv_slot_load: %d slots from a staging cache of %d rows into %d slots", k, staging->B0, cache->B0);
    if (k > kSlotLoadMax || (int64_t)c->n_layers * k > 65535) {
        set_error("p2t_kv_slot_load: at most %d slots per call and 65535 (layer, slot) pairs (got %d slots)", kSlotLoadMax, k);
        return P2T_ERR_UNSUPPORTED;
    }
    SlotTable tab;
    for (int i = 0; i < k; ++i) {
        P2T_REQUIRE(slots[i] >= 0 && slots[i] < cache->B0, "p2t_kv_slot_load: slot %d (entry %d) outside [0, %d)", slots[i], i, cache->B0);
        for (int j = 0; j < i; ++j) P2T_REQUIRE(slots[j] != slots[i], "p2t_kv_slot_load: slot %d is named twice (entries %d and %d)", slots[i], j, i);
        P2T_REQUIRE(limits[i] >= 1 && limits[i] <= cache->G, "p2t_kv_slot_load: row limit %d (entry %d) outside 1 .. %d", limits[i], i, cache->G);
        tab.slot[i] = slots[i];
        tab.limit[i] = limits[i];
    }
    for (int i = k; i < kSlotLoadMax; ++i) tab.slot[i] = tab.limit[i] = 0;
    const void* bufs[] = {staging->k_prompt, staging->vt_prompt, staging->k_prompt_scale, staging->v_prompt_scale, cache->k_prompt, cache->vt_prompt,
                          cache->k_prompt_scale, cache->v_prompt_scale};
    for (const void* p : bufs) P2T_REQUIRE(((uintptr_t)p & 15) == 0, "p2t_kv_slot_load: the prompt segments' buffers must be 16-byte aligned");
    const bool f8 = cache->k_prompt_scale != nullptr;
    const int dp = head_dim_padded(c->head_dim);
    const int64_t scale_bytes = (int64_t)c->kv_heads * cache->Tp, seg_bytes = scale_bytes * dp * (f8 ? 1 : (int64_t)dtype_size(c->dtype));
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(seg_bytes, 256 * 16), 64), (unsigned)(c->n_layers * k), f8 ? 4u : 2u);
    kv_slot_load_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const char*)staging->k_prompt, (const char*)staging->vt_prompt, (const char*)staging->k_prompt_scale,
                                                              (const char*)staging->v_prompt_scale, (char*)cache->k_prompt, (char*)cache->vt_prompt,
                                                              (char*)cache->k_prompt_scale, (char*)cache->v_prompt_scale, seg_bytes, scale_bytes, k, cache->B0,
                                                              staging->prompt_len, const_cast<int32_t*>(cache->prompt_len), row_step, finished, row_limit, tab);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_kv_reorder(const p2t_llama_config* c, const p2t_kv_cache* cache, const int64_t* src_row, void* k_dst, void* vt_dst,
                              p2t_stream stream) {
    P2T_REQUIRE(c && src_row && k_dst && vt_dst, "p2t_kv_reorder: null argument");
    P2T_TRY(check_cache(c, cache, "p2t_kv_reorder"));
    P2T_REQUIRE(k_dst != cache->k_gen && vt_dst != cache->vt_gen, "p2t_kv_reorder: out of place only");
    const int BB = cache->B0 * cache->group, nkv = c->kv_heads, dp = head_dim_padded(c->head_dim);
    const unsigned grid = (unsigned)((int64_t)c->n_layers * BB * nkv);
    hipStream_t s = (hipStream_t)stream;
    if (c->dtype == P2T_BF16)
        kv_reorder_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)cache->k_gen, (const bf16_t*)cache->vt_gen, (bf16_t*)k_dst, (bf16_t*)vt_dst, src_row,
                                                       cache->step, BB, nkv, dp, cache->G);
    else
        kv_reorder_kernel<float><<<grid, 256, 0, s>>>((const float*)cache->k_gen, (const float*)cache->vt_gen, (float*)k_dst, (float*)vt_dst, src_row,
                                                     cache->step, BB, nkv, dp, cache->G);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

static int attention_decode_impl(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                 const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp, int G,
                                 float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out, const uint8_t* k_prompt_scale,
                                 const uint8_t* v_prompt_scale, p2t_stream stream, int step_stride = 0) {
    P2T_REQUIRE(q && out && (dtype == P2T_F32 || dtype == P2T_BF16) && nkv > 0 && nh % nkv == 0 && ld_out >= (int64_t)nh * head_dim,
                "p2t_attention_decode: bad arguments");
    p2t_llama_config c{};
    c.heads = nh; c.kv_heads = nkv; c.head_dim = head_dim; c.dtype = dtype;
    p2t_kv_cache kc{const_cast<void*>(k_prompt), const_cast<void*>(vt_prompt), const_cast<void*>(k_gen), const_cast<void*>(vt_gen), prompt_len,
                    const_cast<int32_t*>(step), B0, group, Tp, G, const_cast<uint8_t*>(k_prompt_scale), const_cast<uint8_t*>(v_prompt_scale)};
    P2T_TRY(check_cache(&c, &kc, "p2t_attention_decode"));
    if (k_prompt_scale && use_mfma == 0) {
        set_error("p2t_attention_decode_prompt_fp8: the matrix-pipe kernel only (use_mfma = 0: the lane-per-key kernel reads no fp8 segment)");
        return P2T_ERR_UNSUPPORTED;
    }
    const int BB = B0 * group, dp = head_dim_padded(head_dim);
    DecodeBuffers b{};
    attn_decode_plan(nh, nkv, &b.ZC, &b.GH);
    b.qb = const_cast<void*>(q);
    b.ao = out;
    hipStream_t s = (hipStream_t)stream;
    const float c_exp = log2_scores ? 1.0f : scale * kLog2e;
    if (dtype == P2T_BF16) return launch_attn_decode_t<bf16_t>(b, &kc, 0, BB, nh, nkv, head_dim, dp, c_exp, 1, ld_out, s, use_mfma != 0, step_stride);
    P2T_REQUIRE(use_mfma <= 0, "p2t_attention_decode: the matrix-pipe kernel is bf16 only");
    return launch_attn_decode_t<float>(b, &kc, 0, BB, nh, nkv, head_dim, dp, c_exp, 0, ld_out, s, 1, step_stride);
}

extern "C" int p2t_attention_decode(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                    const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp, int G,
                                    float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out, p2t_stream stream) {
    return attention_decode_impl(q, k_prompt, vt_prompt, k_gen, vt_gen, prompt_len, step, B0, group, nh, nkv, head_dim, Tp, G, scale, log2_scores, dtype,
                                 use_mfma, out, ld_out, nullptr, nullptr, stream);
}

extern "C" int p2t_attention_decode_prompt_fp8(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                               const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp,
                                               int G, float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                                               const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, p2t_stream stream) {
    P2T_REQUIRE(!k_prompt_scale == !v_prompt_scale, "p2t_attention_decode_prompt_fp8: k_prompt_scale and v_prompt_scale go together");
    P2T_REQUIRE(k_prompt_scale, "p2t_attention_decode_prompt_fp8: null scale arrays (p2t_attention_decode serves the bf16 prompt segment)");
    return attention_decode_impl(q, k_prompt, vt_prompt, k_gen, vt_gen, prompt_len, step, B0, group, nh, nkv, head_dim, Tp, G, scale, log2_scores, dtype,
                                 use_mfma, out, ld_out, k_prompt_scale, v_prompt_scale, stream);
}

// p2t_attention_decode / p2t_attention_decode_prompt_fp8 (the scale arrays both set) with one counter per row: group == 1
extern "C" int p2t_attention_decode_rows(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                         const int32_t* prompt_len, const int32_t* row_step, int B0, int nh, int nkv, int head_dim, int Tp, int G,
                                         float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                                         const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, p2t_stream stream) {
    P2T_REQUIRE(row_step, "p2t_attention_decode_rows: null row_step");
    P2T_REQUIRE(!k_prompt_scale == !v_prompt_scale, "p2t_attention_decode_rows: k_prompt_scale and v_prompt_scale go together");
    return attention_decode_impl(q, k_prompt, vt_prompt, k_gen, vt_gen, prompt_len, row_step, B0, 1, nh, nkv, head_dim, Tp, G, scale, log2_scores, dtype,
                                 use_mfma, out, ld_out, k_prompt_scale, v_prompt_scale, stream, 1);
}

extern "C" int p2t_kv_quant_store(const void* k, const void* v, int B, int kv_heads, int T, int head_dim, int Tp, void* k_codes, void* vt_codes,
                                  uint8_t* k_scale, uint8_t* v_scale, p2t_stream stream) {
    P2T_REQUIRE(k && v && k_codes && vt_codes && k_scale && v_scale && B > 0 && kv_heads > 0 && T > 0, "p2t_kv_quant_store: null/empty argument");
    P2T_REQUIRE(head_dim > 0 && head_dim % 2 == 0 && head_dim <= 128 && Tp % 64 == 0 && T <= Tp,
                "p2t_kv_quant_store: head_dim %d must be even and <= 128, Tp %d a multiple of 64 that holds T %d", head_dim, Tp, T);
    P2T_REQUIRE((((uintptr_t)k | (uintptr_t)v | (uintptr_t)k_codes | (uintptr_t)vt_codes) & 15) == 0, "p2t_kv_quant_store: buffers must be 16-byte aligned");
    return launch_kv_quant_store(k, v, B * kv_heads, T, head_dim, Tp, (uint8_t*)k_codes, (uint8_t*)vt_codes, k_scale, v_scale, (hipStream_t)stream);
}
