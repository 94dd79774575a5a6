// The KV cache of generation (p2t_kv_cache): prompt compaction, the prefill's store into the prompt segment, and the maintenance between
// steps (beam re-ordering, slot refill).  The step that appends to it is llama_decode.hip, the attention that reads it attn_decode.hip.
//
// Layout (sized for 288 GB of HBM: nothing is paged, nothing is re-laid-out per step):
//   * prompts are COMPACTED first (p2t_compact_rows): the valid tokens of every row move to the front in order, so positions are
//     0..len-1 -- exactly HF's `position_ids = cumsum(attention_mask) - 1` on the tokens under the mask, for left padding, right
//     padding or holes alike -- and every row's keys are a prefix of its cache row;
//   * the cache has two segments: the PROMPT segment [layer][B0][kv_head][Tp][dp] (keys, post-rotation) + the same transposed
//     [layer][B0][kv_head][dp][Tp] (values: the decode kernel reads 8 consecutive keys of one feature with one 16-byte load), written
//     once by the prefill; and the GENERATED segment [layer][BB][kv_head][G][dp] / [..][dp][G] with BB = B0 * group rows (group =
//     beams per prompt: all beams of a prompt share its prompt segment, beam re-ordering touches the generated segment only);
//   * opt-in (continuous batching; group == 1): every row carries its OWN counter, row_step[row], beside the cache; p2t_kv_slot_load
//     copies a freshly prefilled prompt segment from a staging cache into its slot and resets its counters, between two replays of the
//     step graph;
//   * opt-in (beam groups, group >= 2): the generated keys and values STAY in the row that wrote them and an ancestry table beside the
//     cache, u8 [BB][G], names the row of the prompt that holds key i of a beam's history; p2t_kv_ancestry_update stands where the
//     re-ordering copy stood, and the attention reads the table as a mask (attn_decode.hip);
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
    if (!out_mask) return;                               // p2t_prompt_index: the destinations and the lengths alone
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
// packed prompt rows (include/p2t_hip.h, p2t_pack_rows): prompts back to back in a few long rows, placed by a PlaceTable
// ---------------------------------------------------------------------------------------------
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// x [B][T][H] -> packed [R][Tpk][H], mask, position_ids, every output element written ONCE.  grid (max(T, Tpk), B + R):
//   * y < B, the copy blocks: token x of prompt y, the r-th under its mask (dst from compact_index_kernel), goes to token start + r of
//     its packed row with mask 1 and position r -- straight from the original row, 16-byte loads and stores;
//   * y >= B, the fill blocks: token x of packed row y - B that no prompt covers becomes zeros with mask 0 and position 0.
__global__ void __launch_bounds__(256) pack_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ dst, const int32_t* __restrict__ lens,
                                                        int B, int T, int H, int Tpk, float* __restrict__ out, int64_t* __restrict__ out_mask,
                                                        int32_t* __restrict__ pos, PlaceTable tab) {
    const int t = blockIdx.x, y = blockIdx.y;
    if (y < B) {
        if (t >= T) return;
        const int r = dst[(int64_t)y * T + t];
        if (r < 0 || r >= min(lens[y], tab.len[y])) return;           // (the host planned from these lengths: a guard, not a case)
        const int64_t to = (int64_t)tab.row[y] * Tpk + tab.start[y] + r;
        const float4* s = reinterpret_cast<const float4*>(x + ((int64_t)y * T + t) * H);
        float4* d = reinterpret_cast<float4*>(out + to * H);
        for (int c = threadIdx.x; c < H / 4; c += 256) d[c] = s[c];
        if (threadIdx.x == 0) { out_mask[to] = 1; pos[to] = r; }
        return;
    }
    if (t >= Tpk) return;
    const int row = y - B;
    for (int i = 0; i < B; ++i)                                       // uniform over the block: scalar reads of the launch arguments
        if (tab.row[i] == row && t >= tab.start[i] && t < tab.start[i] + tab.len[i]) return;
    const int64_t to = (int64_t)row * Tpk + t;
    float4* d = reinterpret_cast<float4*>(out + to * H);
    for (int c = threadIdx.x; c < H / 4; c += 256) d[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x == 0) { out_mask[to] = 0; pos[to] = 0; }
}

// last_hidden[i] = x[row_i][start_i + len_i - 1]: gather_last_kernel (llama_decode.hip) on packed rows
__global__ void __launch_bounds__(256) gather_last_packed_kernel(const float* __restrict__ x, int Tpk, int H, float* __restrict__ out, PlaceTable tab) {
    const int i = blockIdx.x;
    const float* s = x + ((int64_t)tab.row[i] * Tpk + tab.start[i] + tab.len[i] - 1) * H;
    for (int c = threadIdx.x; c < H; c += 256) out[(int64_t)i * H + c] = s[c];
}

// One layer's keys and values from packed rows into every prompt's own row of the prompt segment, ONE launch: k, v [R][nkv][Tpk][dp] ->
// K [n][nkv][Tp][dp] rows 0 .. len - 1, V^T [n][nkv][dp][Tp] columns 0 .. len - 1.  grid (64-key tiles of the longest prompt, n * nkv).
// A tile's source starts at token start + 64 * tile of the packed row -- any token, but a token is dp elements, so 16-byte pieces stay
// aligned; its destination starts at key 64 * tile of a row whose capacity is a multiple of 64, so whole 16-byte groups of a V^T column
// are aligned stores and only the last group of a prompt goes element by element.  Nothing at or behind len is written.
template <typename T>
__global__ void __launch_bounds__(256) kv_store_packed_kernel(const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ kd, T* __restrict__ vtd,
                                                              int nkv, int Tpk, int dp, int Tp, PlaceTable tab) {
    constexpr int N = 16 / (int)sizeof(T);                            // elements per 16-byte piece
    __shared__ __attribute__((aligned(16))) T tile[128][64 + N];      // V [feature][key of the tile]
    const int i = blockIdx.y / nkv, kvh = blockIdx.y - i * nkv, t0 = blockIdx.x * 64;
    const int cnt = min(64, tab.len[i] - t0);                         // keys of this tile
    if (cnt <= 0) return;
    const int64_t from = (((int64_t)tab.row[i] * nkv + kvh) * Tpk + tab.start[i] + t0) * dp, bh = (int64_t)i * nkv + kvh;
    const u32x4_t* ks = reinterpret_cast<const u32x4_t*>(k + from);
    u32x4_t* kt = reinterpret_cast<u32x4_t*>(kd + (bh * Tp + t0) * dp);
    const int ppk = dp / N;                                           // pieces per key
    for (int p = threadIdx.x; p < cnt * ppk; p += 256) kt[p] = ks[p];
    const u32x4_t* vs = reinterpret_cast<const u32x4_t*>(v + from);
    for (int p = threadIdx.x; p < cnt * ppk; p += 256) {
        const int tl = p / ppk, c0 = (p - tl * ppk) * N;
        const u32x4_t w = vs[p];
        T e[N];
        __builtin_memcpy(e, &w, 16);
#pragma unroll
        for (int j = 0; j < N; ++j) tile[c0 + j][tl] = e[j];
    }
    __syncthreads();
    constexpr int GPC = 64 / N;                                       // 16-byte groups per column of the tile
    for (int p = threadIdx.x; p < dp * GPC; p += 256) {
        const int c = p / GPC, t = (p - c * GPC) * N;
        if (t >= cnt) continue;
        T* dst = vtd + (bh * dp + c) * Tp + t0 + t;
        if (t + N <= cnt) {
            *reinterpret_cast<u32x4_t*>(dst) = *reinterpret_cast<const u32x4_t*>(&tile[c][t]);
        } else {
            for (int j = 0; t + j < cnt; ++j) dst[j] = tile[c][t + j];
        }
    }
}

// The same into an fp8 prompt segment: kv_quant_store_kernel's arithmetic on every key (amax over the key's d features among the DP / 8
// lanes that share it -> e8m0_of_amax -> x * 2^-e -> pack_fp8x4; columns d .. DP zero codes; one scale byte per key for K and for V), read
// from where the prompt lies in its packed row and written to the prompt's own cache row.  Codes and scales are bit-equal to
// kv_quant_store_kernel's on the same keys laid out one prompt per row.
template <int DP>
__global__ void __launch_bounds__(256) kv_quant_store_packed_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, uint8_t* __restrict__ kq,
                                                                    uint8_t* __restrict__ vtq, uint8_t* __restrict__ ks, uint8_t* __restrict__ vs, int nkv,
                                                                    int Tpk, int d, int Tp, PlaceTable tab) {
    constexpr int LG = DP / 8, KPP = 256 / LG;                        // lanes per key, keys per pass
    __shared__ __attribute__((aligned(16))) uint8_t tile[DP][68];     // V codes [feature][key of the tile]
    const int i = blockIdx.y / nkv, kvh = blockIdx.y - i * nkv, t0 = blockIdx.x * 64;
    const int seq = tab.len[i];
    if (t0 >= seq) return;
    const int64_t from = ((int64_t)tab.row[i] * nkv + kvh) * Tpk + tab.start[i], bh = (int64_t)i * nkv + kvh;
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
        const int64_t in = (from + t) * DP + 8 * sub, row = bh * Tp + t;
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
    for (int p = threadIdx.x; p < DP * 16; p += 256) {
        const int c = p >> 4, t = t0 + 4 * (p & 15);
        const unsigned w = *reinterpret_cast<const unsigned*>(&tile[c][4 * (p & 15)]);
        uint8_t* dst = vtq + (bh * DP + c) * Tp + t;
        if (t + 4 <= seq) {
            *reinterpret_cast<unsigned*>(dst) = w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e < seq) dst[e] = (uint8_t)(w >> (8 * e));
        }
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

// The ancestry table of a beam group (include/p2t_hip.h), updated where kv_reorder_kernel would copy: grid (columns / 256, prompts), ONE
// thread per (prompt, column <= s).  Column i of a prompt's rows depends on column i of the same rows only, so a thread that reads its
// group bytes and then writes them is an in-place update without a barrier.
constexpr int kAncestryGroupMax = 16;
__global__ void __launch_bounds__(256) kv_ancestry_update_kernel(uint8_t* __restrict__ anc, const int64_t* __restrict__ src_rows,
                                                                 const int32_t* __restrict__ step_ptr, int group, int G) {
    const int s = min(max(step_ptr[0], 0), G - 1);
    const int i = blockIdx.x * 256 + threadIdx.x, b0 = blockIdx.y;
    if (i > s) return;
    uint8_t* col = anc + (int64_t)b0 * group * G + i;
    uint8_t v[kAncestryGroupMax];
#pragma unroll
    for (int g = 0; g < kAncestryGroupMax; ++g) {
        if (g >= group) continue;
        const int64_t sr = min(max(src_rows[b0 * group + g] - (int64_t)b0 * group, (int64_t)0), (int64_t)group - 1);      // clamped into the prompt
        v[g] = i == s ? (uint8_t)g : col[sr * G];
    }
#pragma unroll
    for (int g = 0; g < kAncestryGroupMax; ++g)
        if (g < group) col[(int64_t)g * G] = v[g];
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

int check_ancestry(const void* ancestry, int group, int heads_per_kv, const char* who) {
    P2T_REQUIRE(ancestry && ((uintptr_t)ancestry & 15) == 0, "%s: null ancestry table (or not 16-byte aligned)", who);
    P2T_REQUIRE(group >= 2, "%s: an ancestry table serves beam groups (group >= 2, got %d)", who, group);
    if (group > kAncestryGroupMax || heads_per_kv > 16) {
        set_error("%s: an ancestry table serves at most %d rows per prompt and 16 query heads per kv head (got group %d, %d heads)", who,
                  kAncestryGroupMax, group, heads_per_kv);
        return P2T_ERR_UNSUPPORTED;
    }
    return P2T_OK;
}

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

int place_table(const int32_t* place, int n, int R, int Tpk, int Tp, const char* who, PackedPrompts* pp) {
    P2T_REQUIRE(place && n > 0 && R > 0 && Tpk > 0, "%s: null/empty placement (%d prompts in %d rows of %d tokens)", who, n, R, Tpk);
    if (n > kPackedPromptsMax) {
        set_error("%s: at most %d prompts per call (got %d)", who, kPackedPromptsMax, n);
        return P2T_ERR_UNSUPPORTED;
    }
    pp->n = n;
    pp->longest = 0;
    for (int i = 0; i < n; ++i) {
        const int row = place[3 * i], start = place[3 * i + 1], len = place[3 * i + 2];
        P2T_REQUIRE(row >= 0 && row < R, "%s: prompt %d lies in packed row %d, outside [0, %d)", who, i, row, R);
        P2T_REQUIRE(len >= 1, "%s: prompt %d has %d tokens (every prompt needs at least one)", who, i, len);
        P2T_REQUIRE(start >= 0 && (int64_t)start + len <= Tpk, "%s: prompt %d (start %d, %d tokens) does not fit a packed row of %d tokens", who, i, start, len,
                    Tpk);
        P2T_REQUIRE(Tp <= 0 || len <= Tp, "%s: prompt %d has %d tokens, the cache's prompt segment holds %d", who, i, len, Tp);
        for (int j = 0; j < i; ++j)
            P2T_REQUIRE(pp->tab.row[j] != row || start >= pp->tab.start[j] + pp->tab.len[j] || pp->tab.start[j] >= start + len,
                        "%s: prompts %d and %d overlap in packed row %d", who, j, i, row);
        pp->tab.row[i] = row;
        pp->tab.start[i] = start;
        pp->tab.len[i] = len;
        pp->longest = std::max(pp->longest, len);
    }
    for (int i = n; i < kPackedPromptsMax; ++i) pp->tab.row[i] = pp->tab.start[i] = pp->tab.len[i] = 0;
    return P2T_OK;
}

// packed prefill hook of llama_forward_impl (towers.hip): layer l's rotated keys / values -> every prompt's row of the prompt segment
int llama_kv_store_packed(const p2t_llama_config* c, const p2t_kv_cache* kc, int layer, const void* k, const void* v, int Tpk, const PackedPrompts& pp,
                          hipStream_t s) {
    const int dp = head_dim_padded(c->head_dim), nkv = c->kv_heads;
    const size_t per = (size_t)kc->B0 * nkv * kc->Tp * dp, per_s = (size_t)kc->B0 * nkv * kc->Tp;
    const dim3 grid((unsigned)ceil_div(pp.longest, 64), (unsigned)(pp.n * nkv));
    if (kc->k_prompt_scale) {                 // fp8 prompt segment (check_cache: a bf16 model)
        uint8_t *kq = (uint8_t*)kc->k_prompt + per * layer, *vtq = (uint8_t*)kc->vt_prompt + per * layer;
        uint8_t *ks = kc->k_prompt_scale + per_s * layer, *vs = kc->v_prompt_scale + per_s * layer;
#define P2T_KVQP(DPV) kv_quant_store_packed_kernel<DPV><<<grid, 256, 0, s>>>((const bf16_t*)k, (const bf16_t*)v, kq, vtq, ks, vs, nkv, Tpk, c->head_dim, kc->Tp, pp.tab)
        if (dp == 32) P2T_KVQP(32); else if (dp == 64) P2T_KVQP(64); else P2T_KVQP(128);
#undef P2T_KVQP
    } else if (c->dtype == P2T_BF16) {
        kv_store_packed_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)k, (const bf16_t*)v, (bf16_t*)kc->k_prompt + per * layer,
                                                            (bf16_t*)kc->vt_prompt + per * layer, nkv, Tpk, dp, kc->Tp, pp.tab);
    } else {
        kv_store_packed_kernel<float><<<grid, 256, 0, s>>>((const float*)k, (const float*)v, (float*)kc->k_prompt + per * layer,
                                                           (float*)kc->vt_prompt + per * layer, nkv, Tpk, dp, kc->Tp, pp.tab);
    }
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

int launch_gather_last_packed(const float* x, int Tpk, int H, const PackedPrompts& pp, float* out, hipStream_t s) {
    gather_last_packed_kernel<<<pp.n, 256, 0, s>>>(x, Tpk, H, out, pp.tab);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_prompt_index(const int64_t* mask, int B, int T, int32_t* index, int32_t* lens, p2t_stream stream) {
    P2T_REQUIRE(mask && index && lens && B > 0 && T > 0, "p2t_prompt_index: null/empty argument");
    compact_index_kernel<<<B, 256, 0, (hipStream_t)stream>>>(mask, T, index, nullptr, lens);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_pack_rows(const float* x, const int32_t* index, const int32_t* lens, int B, int T, int H, const int32_t* place, int R, int Tpk,
                             float* out, int64_t* out_mask, int32_t* position_ids, p2t_stream stream) {
    P2T_REQUIRE(x && index && lens && out && out_mask && position_ids && B > 0 && T > 0 && H > 0 && H % 4 == 0 && x != out,
                "p2t_pack_rows: bad arguments (H must be a multiple of 4, out of place)");
    P2T_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "p2t_pack_rows: x and out must be 16-byte aligned");
    PackedPrompts pp;
    P2T_TRY(place_table(place, B, R, Tpk, 0, "p2t_pack_rows", &pp));
    for (int i = 0; i < B; ++i) {            // the packed mask must be a prefix (p2t_doc_prepare): every prompt starts at 0 or where another ends
        bool ok = pp.tab.start[i] == 0;
        for (int j = 0; j < B && !ok; ++j) ok = pp.tab.row[j] == pp.tab.row[i] && pp.tab.start[j] + pp.tab.len[j] == pp.tab.start[i];
        P2T_REQUIRE(ok, "p2t_pack_rows: prompt %d starts at token %d of packed row %d behind a gap (prompts lie back to back from token 0)", i,
                    pp.tab.start[i], pp.tab.row[i]);
    }
    P2T_REQUIRE(R <= 65535 - B, "p2t_pack_rows: %d prompts + %d packed rows exceed one launch (grid.y)", B, R);
    const dim3 grid((unsigned)std::max(T, Tpk), (unsigned)(B + R));
    pack_rows_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, index, lens, B, T, H, Tpk, out, out_mask, position_ids, pp.tab);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_kv_store_packed(const p2t_llama_config* c, const p2t_kv_cache* cache, int layer, const void* k, const void* v, int R, int Tpk,
                                   const int32_t* place, int n, p2t_stream stream) {
    P2T_REQUIRE(c && cache && k && v, "p2t_kv_store_packed: null argument");
    P2T_TRY(check_cache(c, cache, "p2t_kv_store_packed"));
    P2T_REQUIRE(c->kv_heads > 0 && layer >= 0 && layer < c->n_layers, "p2t_kv_store_packed: layer %d outside [0, %d)", layer, c->n_layers);
    P2T_REQUIRE(cache->B0 == n, "p2t_kv_store_packed: cache holds %d rows, the packed batch %d prompts", cache->B0, n);
    PackedPrompts pp;
    P2T_TRY(place_table(place, n, R, Tpk, cache->Tp, "p2t_kv_store_packed", &pp));
    P2T_REQUIRE((((uintptr_t)k | (uintptr_t)v | (uintptr_t)cache->k_prompt | (uintptr_t)cache->vt_prompt) & 15) == 0,
                "p2t_kv_store_packed: buffers must be 16-byte aligned");
    P2T_REQUIRE((int64_t)n * c->kv_heads <= 65535, "p2t_kv_store_packed: %d prompts x %d kv heads exceed one launch", n, c->kv_heads);
    return llama_kv_store_packed(c, cache, layer, k, v, Tpk, pp, (hipStream_t)stream);
}

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

extern "C" int p2t_kv_ancestry_update(const p2t_kv_cache* cache, const int64_t* src_rows, uint8_t* ancestry, p2t_stream stream) {
    P2T_REQUIRE(cache && src_rows && cache->step, "p2t_kv_ancestry_update: null argument");
    P2T_TRY(check_ancestry(ancestry, cache->group, 0, "p2t_kv_ancestry_update"));
    P2T_REQUIRE(cache->B0 > 0 && cache->B0 <= 65535 && cache->G > 0 && cache->G % 64 == 0,
                "p2t_kv_ancestry_update: 1 .. 65535 prompts and a capacity that is a positive multiple of 64 (B0 %d, G %d)", cache->B0, cache->G);
    const dim3 grid((unsigned)ceil_div(cache->G, 256), (unsigned)cache->B0);
    kv_ancestry_update_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(ancestry, src_rows, cache->step, cache->group, cache->G);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_kv_quant_store(const void* k, const void* v, int B, int kv_heads, int T, int head_dim, int Tp, void* k_codes, void* vt_codes,
                                  uint8_t* k_scale, uint8_t* v_scale, p2t_stream stream) {
    P2T_REQUIRE(k && v && k_codes && vt_codes && k_scale && v_scale && B > 0 && kv_heads > 0 && T > 0, "p2t_kv_quant_store: null/empty argument");
    P2T_REQUIRE(head_dim > 0 && head_dim % 2 == 0 && head_dim <= 128 && Tp % 64 == 0 && T <= Tp,
                "p2t_kv_quant_store: head_dim %d must be even and <= 128, Tp %d a multiple of 64 that holds T %d", head_dim, Tp, T);
    P2T_REQUIRE((((uintptr_t)k | (uintptr_t)v | (uintptr_t)k_codes | (uintptr_t)vt_codes) & 15) == 0, "p2t_kv_quant_store: buffers must be 16-byte aligned");
    return launch_kv_quant_store(k, v, B * kv_heads, T, head_dim, Tp, (uint8_t*)k_codes, (uint8_t*)vt_codes, k_scale, v_scale, (hipStream_t)stream);
}
