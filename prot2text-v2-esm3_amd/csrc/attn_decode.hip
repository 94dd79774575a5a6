// The attention of the decode step: ONE query token per row over the two segments of the KV cache (kv_cache.hip has the layout;
// llama_decode.hip's step is the caller, the p2t_attention_decode* doors below serve tests and benchmarks):
//   * the shared lock-step counter `step` = generated tokens already in the cache, read on the device (so the whole step replays as a
//     HIP graph without a host round trip): a row attends to prompt_len[b0] + step + 1 keys;
//   * per-row counters (continuous batching): the same kernels read step[row * stride] with stride 1 where the lock-step entry points
//     pass stride 0;
//   * a beam group under an ancestry table (p2t_attention_decode_beams, the lock-step counter): the generated keys of ALL rows of the
//     prompt are streamed and key i of physical row p counts for beam row r where ancestry[r][i] == p; the matrix-pipe kernel then runs one
//     block per (prompt, kv head) with (beam, head) pairs as its 16 head slots (attn_decode_beams_mfma_kernel);
//   * the fp8 prompt segment (bf16 models, the cache's scale arrays set) is read by the F8 tiles of the matrix-pipe kernel.
#include "common.h"
#include "kernels.h"

namespace p2t {
namespace {

// ---------------------------------------------------------------------------------------------
// attention of ONE query token per row over the two cache segments
// ---------------------------------------------------------------------------------------------
// grid (BB * nkv, head chunks): ONE block owns all keys of a (row, kv head) -- cut into 64-key tiles (prompt segment, then generated
// segment), tile t goes to wave t mod NW.  A wave keeps a running (max, sum, output) per query head of the GQA group -- they all read
// the same keys -- in base-2 form; the waves are merged in LDS in wave order (decode_merge): no atomics, nothing through memory.
//   scores: lane = key, 16-byte pieces of its K row against q (f32 in LDS, broadcast reads);
//   values: lane = feature (rows of the transposed segment), 16-byte pieces = 8 (bf16) / 4 (f32) consecutive keys against P in LDS.

// Merge of a block's per-wave results (red[w][head][0..DP-1] = un-normalised output, [DP] = running max, [DP + 1] = sum; base-2 form),
// in wave order, and the store of the normalised rows.  One block owns ALL keys of its (row, kv head): a split over several blocks
// with a last-arriver merge through global memory was measured at 42 us per launch against 24 for this form at 8 x 1121 keys -- three
// more dependent round trips to memory and a release fence per block cost more than the idle CUs.
template <int DP, int GH, int NW>
__device__ __forceinline__ float merged_output(const float (&red)[NW][GH][DP + 2], int g, int c) {      // feature c of head slot g, normalised
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
    return o / L;
}

template <typename T, int DP, int GH, int NW>
__device__ __forceinline__ void decode_merge(float (&red)[NW][GH][DP + 2], int bb, int h0, int nhead, int d, T* __restrict__ out, int64_t ld_out) {
    for (int i = threadIdx.x; i < GH * DP; i += NW * 64) {
        const int g = i / DP, c = i - g * DP;
        if (g >= nhead || c >= d) continue;
        out[(int64_t)bb * ld_out + (int64_t)(h0 + g) * d + c] = from_f32<T>(merged_output<DP, GH, NW>(red, g, c));
    }
}

// The same for the beam kernel's 16 head slots: slot j = (beam beam0 + j / G, head j % G) of prompt b0 writes its own row
template <int DP, int NW>
__device__ __forceinline__ void decode_merge_beams(float (&red)[NW][16][DP + 2], int b0, int group, int beam0, int BC, int kvh, int G, int d,
                                                   bf16_t* __restrict__ out, int64_t ld_out) {
    for (int i = threadIdx.x; i < 16 * DP; i += NW * 64) {
        const int j = i / DP, c = i - j * DP, sb = j / G, sh = j - sb * G;
        if (sb >= BC || beam0 + sb >= group || c >= d) continue;
        out[(int64_t)(b0 * group + beam0 + sb) * ld_out + (int64_t)(kvh * G + sh) * d + c] = from_f32<bf16_t>(merged_output<DP, 16, NW>(red, j, c));
    }
}

// ANC (a beam group under an ancestry table, `anc` u8 [BB][Gcap]): the generated tiles are those of ALL `group` physical rows of the
// row's prompt, and key i of physical row p counts where anc[bb][i] == p -- a tile may then hold no visible key at all.
// MQ (q_tokens query tokens per cache row, p2t_attention_decode_multi): the grid's rows are VIRTUAL rows m = row * q_tokens + j -- q and
// out are indexed by m, the cache by row m / q_tokens, and token j sees step[row] + j + 1 generated keys: every other line is the
// per-row kernel's, so virtual row m computes what that kernel computes for a row whose counter is step[row] + j, bit for bit.
template <typename T, int DP, int GH, bool ANC = false, bool MQ = false>
__global__ void __launch_bounds__(512) attn_decode_kernel(const T* __restrict__ q, const T* __restrict__ kp, const T* __restrict__ vtp,
                                                          const T* __restrict__ kg, const T* __restrict__ vtg,
                                                          const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ step_ptr,
                                                          int step_stride, int group, int nh, int nkv, int G, int Tp, int Gcap, float c_exp, int round_p,
                                                          T* __restrict__ out, int64_t ld_out, int d, const uint8_t* __restrict__ anc, int q_tokens) {
    static_assert(!(ANC && MQ), "a beam group decodes one token per row");
    constexpr int PN = Piece<T>::N, R = DP > 64 ? DP / 64 : 1, PW = DP + 2, NW = 8;
    __shared__ float sq[GH][DP];
    __shared__ float sp[NW][GH][64];
    __shared__ float red[NW][GH][PW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pair = blockIdx.x, vrow = pair / nkv, kvh = pair - vrow * nkv;  // vrow: the row of q and out
    const int bb = MQ ? vrow / q_tokens : vrow, b0 = bb / group;              // bb: the cache row
    const int hc = blockIdx.y;
    const int h0 = kvh * G + hc * GH, nhead = min(GH, G - hc * GH);          // query heads h0 .. h0 + nhead - 1
    for (int i = threadIdx.x; i < GH * DP; i += NW * 64) {
        const int g = i / DP, c = i - g * DP;
        sq[g][c] = g < nhead ? to_f32(q[((int64_t)vrow * nh + h0 + g) * DP + c]) : 0.f;
    }
    __syncthreads();
    const int n0 = min(max(prompt_len[b0], 0), Tp);
    const int n1 = min(max(step_ptr[(int64_t)bb * step_stride], 0) + (MQ ? vrow - bb * q_tokens : 0) + 1, Gcap);
    const int tiles0 = (n0 + 63) >> 6, tiles1 = (n1 + 63) >> 6, tiles = tiles0 + (ANC ? group : 1) * tiles1;
    const int64_t seg1 = (int64_t)nkv * Gcap * DP;                            // one row of the generated segment
    const T* k_seg0 = kp + ((int64_t)b0 * nkv + kvh) * Tp * DP;
    const T* k_seg1 = kg + ((int64_t)(ANC ? b0 * group : bb) * nkv + kvh) * Gcap * DP;      // ANC: the prompt's physical row 0
    const T* v_seg0 = vtp + ((int64_t)b0 * nkv + kvh) * DP * Tp;
    const T* v_seg1 = vtg + ((int64_t)(ANC ? b0 * group : bb) * nkv + kvh) * DP * Gcap;

    float m_run[GH], l_run[GH], acc[GH][R];
#pragma unroll
    for (int g = 0; g < GH; ++g) {
        m_run[g] = -INFINITY;
        l_run[g] = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[g][r] = 0.f;
    }
    for (int t = w; t < tiles; t += NW) {
        const int sg = t >= tiles0, n = sg ? n1 : n0, cap = sg ? Gcap : Tp;
        const int phys = ANC && sg ? (t - tiles0) / tiles1 : 0;               // ANC: which physical row of the prompt the tile lies in
        const int tt = sg ? (ANC ? t - tiles0 - phys * tiles1 : t - tiles0) : t;
        const int key = tt * 64 + lane;
        bool valid = key < n;
        const bool full = tt * 64 + 64 <= n;
        if (ANC && sg) valid = valid && anc[(int64_t)bb * Gcap + key] == phys;
        const T* krow = (sg ? (ANC ? k_seg1 + phys * seg1 : k_seg1) : k_seg0) + (int64_t)key * DP;
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
            const float m_new = fmaxf(m_run[g], wave_max(e2));            // every tile holds at least one valid key -- unless ANC:
            const float m_ref = ANC && m_new == -INFINITY ? 0.f : m_new;  // nothing visible so far: alpha = 0 on (l, acc) = 0, no -inf - -inf
            const float alpha = exp2f(m_run[g] - m_ref);
            float p = valid ? exp2f(e2 - m_ref) : 0.f;
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
                const T* vrow = (sg ? (ANC ? v_seg1 + phys * seg1 : v_seg1) : v_seg0) + (int64_t)dim * cap + tt * 64;
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
    decode_merge<T, DP, GH, NW>(red, vrow, h0, nhead, d, out, ld_out);
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
// ANC (bf16 tiles of a beam group's generated segment, attn_decode_beams_mfma_kernel): the segment is physical row `phys` of the prompt
// and key i counts for the lane's head slot where anc_row[i] == phys (anc_row: the ancestry row of the slot's beam).  Two things differ
// from the other tiles: a slot may see NO key of the tile, and then keeps (m_run, l_run, acc) exactly; and masked keys inside n hold
// other beams' finite values, which p = 0 silences without zeroing V.
// MQ (bf16 tiles of the generated segment under several query tokens per row, attn_decode_multi_mfma_kernel): `n` is the LANE'S head
// slot's own count -- the slot's query sees the keys in front of it and itself -- and n_v >= n the count of the chunk's last query.  As
// under ANC a slot may see no key of the tile and then keeps (m_run, l_run, acc) exactly; the keys between n and n_v are this step's
// own finite ones, which p = 0 silences, and V is zeroed behind n_v only.
template <int DP, bool F8, bool ANC = false, bool MQ = false>
__device__ __forceinline__ void decode_tile(const void* __restrict__ k_seg, const void* __restrict__ v_seg, const uint8_t* __restrict__ ks_seg,
                                            const uint8_t* __restrict__ vs_seg, int tt, int n, int cap, const bf16x8 (&qf)[DP / 32], float c_exp, int j,
                                            int g, float& m_run, float& l_run, f32x4 (&acc)[DP / 16], const uint8_t* __restrict__ anc_row = nullptr,
                                            int phys = 0, int n_v = 0) {
    static_assert(!(F8 && (ANC || MQ)) && !(ANC && MQ), "the generated segment is bf16; a beam group decodes one token per row");
    constexpr bool EMPTY = ANC || MQ;        // a slot may see no key of the tile
    constexpr int KK = DP / 32, DT = DP / 16;
    const bool full = tt * 64 + 64 <= n;
    f32x4 sc[4];
    uint2 aw[ANC ? 2 : 1] = {};              // the table bytes of the lane's two runs of 8 keys (32 hv + 8 g ..)
    if constexpr (ANC) {
#pragma unroll
        for (int hv = 0; hv < 2; ++hv) aw[hv] = *reinterpret_cast<const uint2*>(anc_row + tt * 64 + 32 * hv + 8 * g);
    }
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
            bool ok = full || tt * 64 + key < n;
            if constexpr (ANC) ok = ok && (int)((((st & 1) ? aw[st >> 1].y : aw[st >> 1].x) >> (8 * r)) & 0xFFu) == phys;
            float s = sc[st][r];
            if constexpr (F8) s *= e8m0_byte_to_f32(ksw[st], r);
            sc[st][r] = ok ? s * c_exp : -INFINITY;                   // a select: what a key behind the prefix holds goes no further
            mx = fmaxf(mx, sc[st][r]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float m_new = fmaxf(m_run, mx);                                // every tile holds at least one valid key -- unless ANC / MQ:
    const float alpha = exp2f(m_run - (EMPTY && m_new == -INFINITY ? 0.f : m_new));    // nothing visible so far: 0 on (l, acc) = 0, no -inf - -inf
    m_run = m_new;
    if (EMPTY && m_new == -INFINITY) m_new = 0.f;                  // ... and p = exp2(-inf - 0) = 0
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
    const int nz = MQ ? n_v : n;                                   // V is zeroed behind the last count any slot of the wave has
    if (!F8 && (MQ ? tt * 64 + 64 > nz : !full)) {                 // keys behind the valid prefix: 0 x garbage must stay 0
#pragma unroll
        for (int hv = 0; hv < 2; ++hv)
#pragma unroll
            for (int dt = 0; dt < (F8 ? 1 : DT); ++dt) {
                typedef short s16x8 __attribute__((ext_vector_type(8)));
                s16x8 v = __builtin_bit_cast(s16x8, vf[hv][dt]);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = tt * 64 + 32 * hv + 8 * g + e < nz ? v[e] : (short)0;
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

// A beam group under an ancestry table (include/p2t_hip.h): grid (B0 * nkv, beam chunks), ONE block per (prompt, kv head) and chunk of
// BC = 16 / G beams.  The 16 head slots of the products above are (beam, head) pairs -- slot j = (beam beam0 + j / G, head j % G), its
// own q row -- so the prompt segment is streamed once for all beams of the chunk; then the generated tiles of the prompt's `group`
// physical rows, each with the table as one more condition of the score select (decode_tile's ANC form).  Tile t of that one list goes
// to wave t mod NW; the merge is decode_merge's, per slot.  LDS: red[NW][16][DP + 2] f32 = 66.5 KB at (NW 8, DP 128) and 67.6 KB at
// (16, 64), of the CU's 160 KB.
template <int DP, int NW, bool P8>
__global__ void __launch_bounds__(NW * 64) attn_decode_beams_mfma_kernel(const bf16_t* __restrict__ q, const void* __restrict__ kp,
                                                                     const void* __restrict__ vtp, const bf16_t* __restrict__ kg,
                                                                     const bf16_t* __restrict__ vtg, const uint8_t* __restrict__ kps,
                                                                     const uint8_t* __restrict__ vps, const int32_t* __restrict__ prompt_len,
                                                                     const int32_t* __restrict__ step_ptr, const uint8_t* __restrict__ anc, int group,
                                                                     int nh, int nkv, int G, int Tp, int Gcap, float c_exp, bf16_t* __restrict__ out,
                                                                     int64_t ld_out, int d) {
    constexpr int PW = DP + 2, KK = DP / 32, DT = DP / 16, EP = P8 ? 1 : 2;
    __shared__ float red[NW][16][PW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
    const int pair = blockIdx.x, b0 = pair / nkv, kvh = pair - b0 * nkv;
    const int BC = 16 / G, beam0 = blockIdx.y * BC, sb = j / G, sh = j - sb * G;
    const bool live = sb < BC && beam0 + sb < group;
    // a slot without a beam reads a real row's table and a zero q: its numbers stay finite and decode_merge_beams stores none of them
    const int row = b0 * group + min(beam0 + sb, group - 1);
    const bf16x8 zero8 = {};
    const bf16_t* qrow = q + ((int64_t)row * nh + kvh * G + sh) * DP;
    auto load_q = [&](bf16x8 (&qf)[KK], bool f8_order) {            // attn_decode_mfma_kernel's, per slot
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int f = f8_order && DP > 32 ? 64 * (kk >> 1) + 16 * g + 8 * (kk & 1) : 32 * kk + 8 * g;
            qf[kk] = live ? *reinterpret_cast<const bf16x8*>(qrow + f) : zero8;
        }
    };
    bf16x8 qf[KK];
    load_q(qf, P8);
    const int n0 = min(max(prompt_len[b0], 0), Tp), n1 = min(max(step_ptr[0], 0) + 1, Gcap);
    const int tiles0 = (n0 + 63) >> 6, tiles1 = (n1 + 63) >> 6, tiles = tiles0 + group * tiles1;
    const char* k_seg0 = (const char*)kp + ((int64_t)b0 * nkv + kvh) * Tp * DP * EP;
    const char* v_seg0 = (const char*)vtp + ((int64_t)b0 * nkv + kvh) * DP * Tp * EP;
    const uint8_t* ks_seg0 = P8 ? kps + ((int64_t)b0 * nkv + kvh) * Tp : nullptr;
    const uint8_t* vs_seg0 = P8 ? vps + ((int64_t)b0 * nkv + kvh) * Tp : nullptr;
    const int64_t seg1 = (int64_t)nkv * Gcap * DP;                    // one row of the generated segment (K and V^T alike)
    const bf16_t* k_grp = kg + (int64_t)b0 * group * seg1 + (int64_t)kvh * Gcap * DP;       // physical row 0 of the prompt
    const bf16_t* v_grp = vtg + (int64_t)b0 * group * seg1 + (int64_t)kvh * DP * Gcap;
    const uint8_t* anc_row = anc + (int64_t)row * Gcap;
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto gen_tile = [&](int u) {                                     // tile u of the generated list: physical row u / tiles1
        const int p = u / tiles1, tt = u - p * tiles1;
        decode_tile<DP, false, true>(k_grp + p * seg1, v_grp + p * seg1, nullptr, nullptr, tt, n1, Gcap, qf, c_exp, j, g, m_run, l_run, acc, anc_row, p);
    };
    int t = w;
    for (; t < tiles0; t += NW) decode_tile<DP, P8>(k_seg0, v_seg0, ks_seg0, vs_seg0, t, n0, Tp, qf, c_exp, j, g, m_run, l_run, acc);
    if (P8 && t < tiles) load_q(qf, false);                          // the bf16 tiles' feature order
    for (; t < tiles; t += NW) gen_tile(t - tiles0);
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (g == 0) { red[w][j][DP] = m_run; red[w][j][DP + 1] = l_run; }       // lane (slot j, g) holds the features 16 dt + 4 g + r of its slot
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w][j][16 * dt + 4 * g + r] = acc[dt][r];
    __syncthreads();
    decode_merge_beams<DP, NW>(red, b0, group, beam0, BC, kvh, G, d, out, ld_out);
}

// Several query tokens per cache row (include/p2t_hip.h, p2t_attention_decode_multi): q / out row m = row * Q + i is token i of cache row
// `row`, which sees the prompt and the generated keys 0 .. step[row] + i.  grid (BB * nkv, query chunks), ONE block per (row, kv head)
// and chunk of QC = 16 / G queries: head slot j = (query q0 + j / G, head j % G), so the row's keys and values are streamed once for QC
// queries.  Prompt tiles count for every slot; the generated tile list runs to the chunk's last query and every slot brings its own count
// (decode_tile's MQ form).  Tile t goes to wave t mod NW and the merge is per slot, with the per-row kernel's NW for the same head shape:
// a slot's tiles, their waves and their order are those of attn_decode_mfma_kernel for a row whose counter is step[row] + i, and a tile
// behind the slot's count changes nothing -- the same bits.  Idle slots (16 % G, Q's last chunk) read a zero q and store nothing.
template <int DP, int NW, bool P8>
__global__ void __launch_bounds__(NW * 64) attn_decode_multi_mfma_kernel(const bf16_t* __restrict__ q, const void* __restrict__ kp,
                                                                     const void* __restrict__ vtp, const bf16_t* __restrict__ kg,
                                                                     const bf16_t* __restrict__ vtg, const uint8_t* __restrict__ kps,
                                                                     const uint8_t* __restrict__ vps, const int32_t* __restrict__ prompt_len,
                                                                     const int32_t* __restrict__ step_ptr, int Q, int nh, int nkv, int G, int Tp,
                                                                     int Gcap, float c_exp, bf16_t* __restrict__ out, int64_t ld_out, int d) {
    constexpr int PW = DP + 2, KK = DP / 32, DT = DP / 16, EP = P8 ? 1 : 2;
    __shared__ float red[NW][16][PW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
    const int pair = blockIdx.x, bb = pair / nkv, kvh = pair - bb * nkv;
    const int QC = 16 / G, q0 = blockIdx.y * QC, sq = j / G, sh = j - sq * G;
    const int q_last = min(q0 + QC, Q) - 1;                           // the chunk's last query
    const bool live = sq < QC && q0 + sq <= q_last;
    const int qi = min(q0 + sq, q_last);                              // an idle slot: a real query's count, a zero q
    const bf16x8 zero8 = {};
    const bf16_t* qrow = q + (((int64_t)bb * Q + qi) * nh + kvh * G + sh) * DP;
    auto load_q = [&](bf16x8 (&qf)[KK], bool f8_order) {            // attn_decode_mfma_kernel's, per slot
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int f = f8_order && DP > 32 ? 64 * (kk >> 1) + 16 * g + 8 * (kk & 1) : 32 * kk + 8 * g;
            qf[kk] = live ? *reinterpret_cast<const bf16x8*>(qrow + f) : zero8;
        }
    };
    bf16x8 qf[KK];
    load_q(qf, P8);
    const int st = max(step_ptr[bb], 0);
    const int n0 = min(max(prompt_len[bb], 0), Tp), n1 = min(st + qi + 1, Gcap), n1_last = min(st + q_last + 1, Gcap);
    const int tiles0 = (n0 + 63) >> 6, tiles = tiles0 + ((n1_last + 63) >> 6);
    const char* k_seg0 = (const char*)kp + ((int64_t)bb * nkv + kvh) * Tp * DP * EP;
    const bf16_t* k_seg1 = kg + ((int64_t)bb * nkv + kvh) * Gcap * DP;
    const char* v_seg0 = (const char*)vtp + ((int64_t)bb * nkv + kvh) * DP * Tp * EP;
    const bf16_t* v_seg1 = vtg + ((int64_t)bb * nkv + kvh) * DP * Gcap;
    const uint8_t* ks_seg0 = P8 ? kps + ((int64_t)bb * nkv + kvh) * Tp : nullptr;
    const uint8_t* vs_seg0 = P8 ? vps + ((int64_t)bb * nkv + kvh) * Tp : nullptr;
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int t = w;
    for (; t < tiles0; t += NW) decode_tile<DP, P8>(k_seg0, v_seg0, ks_seg0, vs_seg0, t, n0, Tp, qf, c_exp, j, g, m_run, l_run, acc);
    if (P8 && t < tiles) load_q(qf, false);                          // the bf16 tiles' feature order
    for (; t < tiles; t += NW)
        decode_tile<DP, false, false, true>(k_seg1, v_seg1, nullptr, nullptr, t - tiles0, n1, Gcap, qf, c_exp, j, g, m_run, l_run, acc, nullptr, 0, n1_last);
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (g == 0) { red[w][j][DP] = m_run; red[w][j][DP + 1] = l_run; }       // lane (slot j, g) holds the features 16 dt + 4 g + r of its slot
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w][j][16 * dt + 4 * g + r] = acc[dt][r];
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * DP; i += NW * 64) {             // decode_merge_beams' store, slot = (query, head)
        const int jj = i / DP, c = i - jj * DP, s2 = jj / G, h2 = jj - s2 * G;
        if (s2 >= QC || q0 + s2 > q_last || c >= d) continue;
        out[((int64_t)bb * Q + q0 + s2) * ld_out + (int64_t)(kvh * G + h2) * d + c] = from_f32<bf16_t>(merged_output<DP, 16, NW>(red, jj, c));
    }
}

int pick_gh(int G) { return G <= 1 ? 1 : (G <= 2 ? 2 : (G <= 4 ? 4 : 8)); }

template <typename T>
int launch_attn_decode_t(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp, int round_p,
                         int use_mfma, int step_stride, hipStream_t s) {
    const int nh = c->heads, nkv = c->kv_heads, d = c->head_dim, dp = head_dim_padded(d), G = nh / nkv, BB = kc->B0 * kc->group;
    // GH query heads of a GQA group per block, ZC chunks of them (more than 8 heads per kv head: the keys are read once per chunk)
    const int GH = pick_gh(G), ZC = (G + GH - 1) / GH;
    const size_t per_p = (size_t)kc->B0 * nkv * kc->Tp * dp, per_g = (size_t)BB * nkv * kc->G * dp;
    const T* kp = (const T*)kc->k_prompt + per_p * layer;
    const T* vtp = (const T*)kc->vt_prompt + per_p * layer;
    const T* kg = (const T*)kc->k_gen + per_g * layer;
    const T* vtg = (const T*)kc->vt_gen + per_g * layer;
    const dim3 grid((unsigned)(BB * nkv), (unsigned)ZC);
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
        (const bf16_t*)q, P8V ? (const void*)kp8 : (const void*)kp, P8V ? (const void*)vtp8 : (const void*)vtp, (const bf16_t*)kg,  \
        (const bf16_t*)vtg, kps, vps, kc->prompt_len, kc->step, step_stride, kc->group, nh, nkv, G, kc->Tp, kc->G, c_exp, (bf16_t*)out, ld_out, d)
#define P2T_ADM_G(DPV, P8V)                                                                                                           \
    do {                                                                                                                              \
        if (GH == 1) P2T_ADM(DPV, 1, P8V); else if (GH == 2) P2T_ADM(DPV, 2, P8V); else if (GH == 4) P2T_ADM(DPV, 4, P8V);       \
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
    attn_decode_kernel<T, DPV, GHV><<<grid, 512, 0, s>>>((const T*)q, kp, vtp, kg, vtg, kc->prompt_len, kc->step, step_stride, kc->group, nh, nkv, G, \
                                                         kc->Tp, kc->G, c_exp, round_p, (T*)out, ld_out, d, nullptr, 1)
#define P2T_AD_G(DPV)                                                                                                                 \
    do {                                                                                                                              \
        if (GH == 1) P2T_AD(DPV, 1); else if (GH == 2) P2T_AD(DPV, 2); else if (GH == 4) P2T_AD(DPV, 4); else P2T_AD(DPV, 8);      \
    } while (0)
    if (dp == 32) P2T_AD_G(32); else if (dp == 64) P2T_AD_G(64); else P2T_AD_G(128);
#undef P2T_AD_G
#undef P2T_AD
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

// launch_attn_decode_t for a beam group under an ancestry table (checked: group 2 .. 16, G <= 16, the shared counter)
template <typename T>
int launch_attn_decode_beams_t(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp,
                               int round_p, int use_mfma, const uint8_t* anc, hipStream_t s) {
    const int nh = c->heads, nkv = c->kv_heads, d = c->head_dim, dp = head_dim_padded(d), G = nh / nkv, BB = kc->B0 * kc->group;
    const size_t per_p = (size_t)kc->B0 * nkv * kc->Tp * dp, per_g = (size_t)BB * nkv * kc->G * dp;
    const T* kg = (const T*)kc->k_gen + per_g * layer;
    const T* vtg = (const T*)kc->vt_gen + per_g * layer;
    if constexpr (sizeof(T) == 2) {
        if (use_mfma) {
            const int BC = 16 / G;                   // beams per block: its 16 head slots are (beam, head) pairs
            const dim3 grid((unsigned)(kc->B0 * nkv), (unsigned)ceil_div(kc->group, BC));
            const size_t per_s = (size_t)kc->B0 * nkv * kc->Tp, e = kc->k_prompt_scale ? 1 : 2;
            const char* kp = (const char*)kc->k_prompt + per_p * layer * e;
            const char* vtp = (const char*)kc->vt_prompt + per_p * layer * e;
            const uint8_t* kps = kc->k_prompt_scale ? kc->k_prompt_scale + per_s * layer : nullptr;
            const uint8_t* vps = kc->k_prompt_scale ? kc->v_prompt_scale + per_s * layer : nullptr;
#define P2T_ADB(DPV, P8V)                                                                                                             \
    attn_decode_beams_mfma_kernel<DPV, (DPV <= 64 ? 16 : 8), P8V><<<grid, (DPV <= 64 ? 16 : 8) * 64, 0, s>>>(                          \
        (const bf16_t*)q, kp, vtp, (const bf16_t*)kg, (const bf16_t*)vtg, kps, vps, kc->prompt_len, kc->step, anc, kc->group, nh, nkv, G, kc->Tp,   \
        kc->G, c_exp, (bf16_t*)out, ld_out, d)
            if (kps) {
                if (dp == 32) P2T_ADB(32, true); else if (dp == 64) P2T_ADB(64, true); else P2T_ADB(128, true);
            } else {
                if (dp == 32) P2T_ADB(32, false); else if (dp == 64) P2T_ADB(64, false); else P2T_ADB(128, false);
            }
#undef P2T_ADB
            P2T_LAUNCH_CHECK();
            return P2T_OK;
        }
    }
    P2T_REQUIRE(!kc->k_prompt_scale, "attention over an fp8 prompt segment: the matrix-pipe kernel only");
    const int GH = pick_gh(G), ZC = (G + GH - 1) / GH;
    const dim3 grid((unsigned)(BB * nkv), (unsigned)ZC);
    const T* kp = (const T*)kc->k_prompt + per_p * layer;
    const T* vtp = (const T*)kc->vt_prompt + per_p * layer;
#define P2T_ADL(DPV, GHV)                                                                                                             \
    attn_decode_kernel<T, DPV, GHV, true><<<grid, 512, 0, s>>>((const T*)q, kp, vtp, kg, vtg, kc->prompt_len, kc->step, 0, kc->group, nh, nkv, G, kc->Tp, \
                                                               kc->G, c_exp, round_p, (T*)out, ld_out, d, anc, 1)
#define P2T_ADL_G(DPV)                                                                                                                \
    do {                                                                                                                              \
        if (GH == 1) P2T_ADL(DPV, 1); else if (GH == 2) P2T_ADL(DPV, 2); else if (GH == 4) P2T_ADL(DPV, 4); else P2T_ADL(DPV, 8);  \
    } while (0)
    if (dp == 32) P2T_ADL_G(32); else if (dp == 64) P2T_ADL_G(64); else P2T_ADL_G(128);
#undef P2T_ADL_G
#undef P2T_ADL
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

// launch_attn_decode_t for Q query tokens per row (checked: group 1, per-row counters, 1 <= G <= 16)
template <typename T>
int launch_attn_decode_multi_t(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp,
                               int round_p, int use_mfma, int Q, hipStream_t s) {
    const int nh = c->heads, nkv = c->kv_heads, d = c->head_dim, dp = head_dim_padded(d), G = nh / nkv, BB = kc->B0;
    const int GH = pick_gh(G), ZC = (G + GH - 1) / GH;
    const size_t per_p = (size_t)kc->B0 * nkv * kc->Tp * dp, per_g = (size_t)BB * nkv * kc->G * dp;
    const T* kg = (const T*)kc->k_gen + per_g * layer;
    const T* vtg = (const T*)kc->vt_gen + per_g * layer;
    if constexpr (sizeof(T) == 2) {
        if (use_mfma) {
            const int QC = 16 / G;                   // queries per block: its 16 head slots are (query, head) pairs
            const dim3 grid((unsigned)(BB * nkv), (unsigned)ceil_div(Q, QC));
            const size_t per_s = (size_t)kc->B0 * nkv * kc->Tp, e = kc->k_prompt_scale ? 1 : 2;
            const char* kp = (const char*)kc->k_prompt + per_p * layer * e;
            const char* vtp = (const char*)kc->vt_prompt + per_p * layer * e;
            const uint8_t* kps = kc->k_prompt_scale ? kc->k_prompt_scale + per_s * layer : nullptr;
            const uint8_t* vps = kc->k_prompt_scale ? kc->v_prompt_scale + per_s * layer : nullptr;
            const bool nw16 = GH <= 4 && dp <= 64;   // the per-row kernel's waves for this head shape (the same tile -> wave map)
#define P2T_ADQ(DPV, NWV, P8V)                                                                                                        \
    attn_decode_multi_mfma_kernel<DPV, NWV, P8V><<<grid, NWV * 64, 0, s>>>((const bf16_t*)q, kp, vtp, (const bf16_t*)kg, (const bf16_t*)vtg, kps, vps, \
                                                                           kc->prompt_len, kc->step, Q, nh, nkv, G, kc->Tp, kc->G, c_exp,     \
                                                                           (bf16_t*)out, ld_out, d)
#define P2T_ADQ_D(P8V)                                                                                                                \
    do {                                                                                                                              \
        if (dp == 32) { if (nw16) P2T_ADQ(32, 16, P8V); else P2T_ADQ(32, 8, P8V); }                                                   \
        else if (dp == 64) { if (nw16) P2T_ADQ(64, 16, P8V); else P2T_ADQ(64, 8, P8V); }                                              \
        else P2T_ADQ(128, 8, P8V);                                                                                                    \
    } while (0)
            if (kps) P2T_ADQ_D(true); else P2T_ADQ_D(false);
#undef P2T_ADQ_D
#undef P2T_ADQ
            P2T_LAUNCH_CHECK();
            return P2T_OK;
        }
    }
    P2T_REQUIRE(!kc->k_prompt_scale, "attention over an fp8 prompt segment: the matrix-pipe kernel only");
    const dim3 grid((unsigned)(BB * Q * nkv), (unsigned)ZC);
    const T* kp = (const T*)kc->k_prompt + per_p * layer;
    const T* vtp = (const T*)kc->vt_prompt + per_p * layer;
#define P2T_ADV(DPV, GHV)                                                                                                             \
    attn_decode_kernel<T, DPV, GHV, false, true><<<grid, 512, 0, s>>>((const T*)q, kp, vtp, kg, vtg, kc->prompt_len, kc->step, 1, 1, nh, nkv, G, kc->Tp, \
                                                                      kc->G, c_exp, round_p, (T*)out, ld_out, d, nullptr, Q)
#define P2T_ADV_G(DPV)                                                                                                                \
    do {                                                                                                                              \
        if (GH == 1) P2T_ADV(DPV, 1); else if (GH == 2) P2T_ADV(DPV, 2); else if (GH == 4) P2T_ADV(DPV, 4); else P2T_ADV(DPV, 8);  \
    } while (0)
    if (dp == 32) P2T_ADV_G(32); else if (dp == 64) P2T_ADV_G(64); else P2T_ADV_G(128);
#undef P2T_ADV_G
#undef P2T_ADV
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

}  // namespace

int launch_attn_decode_multi(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp,
                             int round_p, int use_mfma, int q_tokens, hipStream_t s) {
    return c->dtype == P2T_BF16 ? launch_attn_decode_multi_t<bf16_t>(c, q, out, ld_out, kc, layer, c_exp, round_p, use_mfma, q_tokens, s)
                                : launch_attn_decode_multi_t<float>(c, q, out, ld_out, kc, layer, c_exp, round_p, use_mfma, q_tokens, s);
}

// what a call with several query tokens per row asks: 1 .. 64 of them, at most 16 query heads per kv head
int check_multi(int q_tokens, int heads_per_kv, const char* who) {
    P2T_REQUIRE(q_tokens >= 1 && q_tokens <= 64, "%s: q_tokens %d outside 1 .. 64", who, q_tokens);
    if (heads_per_kv > 16) {
        set_error("%s: several query tokens per row serve at most 16 query heads per kv head (got %d)", who, heads_per_kv);
        return P2T_ERR_UNSUPPORTED;
    }
    return P2T_OK;
}

int launch_attn_decode_beams(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp,
                             int round_p, int use_mfma, const uint8_t* ancestry, hipStream_t s) {
    return c->dtype == P2T_BF16 ? launch_attn_decode_beams_t<bf16_t>(c, q, out, ld_out, kc, layer, c_exp, round_p, use_mfma, ancestry, s)
                                : launch_attn_decode_beams_t<float>(c, q, out, ld_out, kc, layer, c_exp, round_p, use_mfma, ancestry, s);
}

// one layer's attention of the step (llama_decode.hip) or of the doors below: c says the head shape and the dtype, kc the cache
int launch_attn_decode(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp, int round_p,
                       int use_mfma, int step_stride, hipStream_t s) {
    return c->dtype == P2T_BF16 ? launch_attn_decode_t<bf16_t>(c, q, out, ld_out, kc, layer, c_exp, round_p, use_mfma, step_stride, s)
                                : launch_attn_decode_t<float>(c, q, out, ld_out, kc, layer, c_exp, round_p, use_mfma, step_stride, s);
}

}  // namespace p2t

using namespace p2t;

static int attention_decode_impl(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                 const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp, int G,
                                 float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out, const uint8_t* k_prompt_scale,
                                 const uint8_t* v_prompt_scale, int step_stride, const uint8_t* ancestry, p2t_stream stream, int q_tokens = 0) {
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
    P2T_REQUIRE(dtype == P2T_BF16 || use_mfma <= 0, "p2t_attention_decode: the matrix-pipe kernel is bf16 only");
    const float c_exp = log2_scores ? 1.0f : scale * kLog2e;
    if (ancestry) return launch_attn_decode_beams(&c, q, out, ld_out, &kc, 0, c_exp, dtype == P2T_BF16, use_mfma != 0, ancestry, (hipStream_t)stream);
    if (q_tokens) return launch_attn_decode_multi(&c, q, out, ld_out, &kc, 0, c_exp, dtype == P2T_BF16, use_mfma != 0, q_tokens, (hipStream_t)stream);
    return launch_attn_decode(&c, q, out, ld_out, &kc, 0, c_exp, dtype == P2T_BF16, use_mfma != 0, step_stride, (hipStream_t)stream);
}

extern "C" int p2t_attention_decode(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                    const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp, int G,
                                    float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out, p2t_stream stream) {
    return attention_decode_impl(q, k_prompt, vt_prompt, k_gen, vt_gen, prompt_len, step, B0, group, nh, nkv, head_dim, Tp, G, scale, log2_scores, dtype,
                                 use_mfma, out, ld_out, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int p2t_attention_decode_prompt_fp8(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                               const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp,
                                               int G, float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                                               const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, p2t_stream stream) {
    P2T_REQUIRE(!k_prompt_scale == !v_prompt_scale, "p2t_attention_decode_prompt_fp8: k_prompt_scale and v_prompt_scale go together");
    P2T_REQUIRE(k_prompt_scale, "p2t_attention_decode_prompt_fp8: null scale arrays (p2t_attention_decode serves the bf16 prompt segment)");
    return attention_decode_impl(q, k_prompt, vt_prompt, k_gen, vt_gen, prompt_len, step, B0, group, nh, nkv, head_dim, Tp, G, scale, log2_scores, dtype,
                                 use_mfma, out, ld_out, k_prompt_scale, v_prompt_scale, 0, nullptr, stream);
}

// p2t_attention_decode / p2t_attention_decode_prompt_fp8 (the scale arrays both set) with one counter per row: group == 1
extern "C" int p2t_attention_decode_rows(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                         const int32_t* prompt_len, const int32_t* row_step, int B0, int nh, int nkv, int head_dim, int Tp, int G,
                                         float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                                         const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, p2t_stream stream) {
    P2T_REQUIRE(row_step, "p2t_attention_decode_rows: null row_step");
    P2T_REQUIRE(!k_prompt_scale == !v_prompt_scale, "p2t_attention_decode_rows: k_prompt_scale and v_prompt_scale go together");
    return attention_decode_impl(q, k_prompt, vt_prompt, k_gen, vt_gen, prompt_len, row_step, B0, 1, nh, nkv, head_dim, Tp, G, scale, log2_scores, dtype,
                                 use_mfma, out, ld_out, k_prompt_scale, v_prompt_scale, 1, nullptr, stream);
}

// p2t_attention_decode_rows for q_tokens query tokens per row: q / out row r * q_tokens + j is token j of cache row r
extern "C" int p2t_attention_decode_multi(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                          const int32_t* prompt_len, const int32_t* row_step, int B0, int nh, int nkv, int head_dim, int Tp, int G,
                                          float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                                          const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, int q_tokens, p2t_stream stream) {
    P2T_REQUIRE(row_step, "p2t_attention_decode_multi: null row_step");
    P2T_REQUIRE(nkv > 0 && nh > 0, "p2t_attention_decode_multi: bad arguments");
    P2T_TRY(check_multi(q_tokens, nh / nkv, "p2t_attention_decode_multi"));
    P2T_REQUIRE(!k_prompt_scale == !v_prompt_scale, "p2t_attention_decode_multi: k_prompt_scale and v_prompt_scale go together");
    return attention_decode_impl(q, k_prompt, vt_prompt, k_gen, vt_gen, prompt_len, row_step, B0, 1, nh, nkv, head_dim, Tp, G, scale, log2_scores, dtype,
                                 use_mfma, out, ld_out, k_prompt_scale, v_prompt_scale, 1, nullptr, stream, q_tokens);
}

// p2t_attention_decode / p2t_attention_decode_prompt_fp8 for a beam group whose generated keys stay in the rows that wrote them
extern "C" int p2t_attention_decode_beams(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                          const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp, int G,
                                          float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                                          const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, const uint8_t* ancestry, p2t_stream stream) {
    P2T_REQUIRE(nkv > 0 && nh > 0, "p2t_attention_decode_beams: bad arguments");
    P2T_TRY(check_ancestry(ancestry, group, nh / nkv, "p2t_attention_decode_beams"));
    P2T_REQUIRE(!k_prompt_scale == !v_prompt_scale, "p2t_attention_decode_beams: k_prompt_scale and v_prompt_scale go together");
    return attention_decode_impl(q, k_prompt, vt_prompt, k_gen, vt_gen, prompt_len, step, B0, group, nh, nkv, head_dim, Tp, G, scale, log2_scores, dtype,
                                 use_mfma, out, ld_out, k_prompt_scale, v_prompt_scale, 0, ancestry, stream);
}
