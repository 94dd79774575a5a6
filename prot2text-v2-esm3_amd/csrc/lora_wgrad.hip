// The weight gradients of a LoRA branch as ONE product over the token axis (p2t_hip/lora_linear.py, LoraLinear.backward):
//
//     G[c, j] = sum_m X'[m, c] U[m, j]        dB = dy^T u  (X = dy, U = u),   dA^T = drop(x)^T du  (X = x with the branch's dropout, U = du)
//
// X [M, ld_x] and U [M, ld_u] are the row-major activations as the step holds them (tokens are rows), so the sum runs over
// the STRIDED axis of both operands.  p2t_gemm_nt wants it contiguous: its route is four p2t_transpose copies, a dropped copy
// of x and zeroed token tails.  Here a workgroup owns 128 columns of X and a contiguous range of 64-token tiles; it stages the
// [64 tokens x 128 columns] tile of X (dropout applied on the way: the counter hash of p2t_dropout_rows, never stored) and the
// [64 x R] tile of U in LDS as they lie in memory and feeds v_mfma_f32_32x32x16_bf16 through transposed LDS reads
// (ds_read_b64_tr_b16: both operands want 8 consecutive TOKENS of one column per lane), as attn_bwd_dkv_mfma_kernel does for
// its sums over queries.  X is read once: M C elements of traffic against the 3 M C (+ 2 M C for the dropped copy) of the
// transpose route.
//
// Columns alone give C / 128 workgroups, so the token axis is split as well: every split writes its partial [C, R] sums to an
// f32 workspace [splits, C, R] and a second kernel adds them in split order -- no atomics, the same bits every run.
// fp32 operands (the correctness path) take the same tiling on plain FMAs.
#include "common.h"
#include "epilogue.h"
#include "kernels.h"

namespace p2t {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));
using lds_s4_t = __attribute__((address_space(3))) short4v*;

constexpr int kBC = 128;            // columns of X per workgroup (32 per wave)
constexpr int kTM = 64;             // tokens per tile
constexpr int kMaxR = 64;
constexpr int kWantGroups = 512;    // two workgroups per compute unit of an MI355X (a constant: the sizing runs without a device)
// LDS row strides in bytes, each 64 B past the data: the four token rows a 16-lane group gathers in one transposed read then
// start 16 banks apart, and a 32-lane half covers all 64 banks once
constexpr int kXS = kBC * 2 + 64, kUS = kMaxR * 2 + 64;

// token splits of (C, M): the tiles of 64 tokens each split sums, and how many splits that makes
void wgrad_plan(int64_t C, int64_t M, int64_t* tiles_per_split, int64_t* splits) {
    const int64_t n_tiles = ceil_div(M, kTM), ncb = ceil_div(C, kBC);
    int64_t s = ceil_div(kWantGroups, ncb);
    s = s < 1 ? 1 : (s > n_tiles ? n_tiles : s);
    *tiles_per_split = ceil_div(n_tiles, s);
    *splits = ceil_div(n_tiles, *tiles_per_split);
}

__device__ __forceinline__ unsigned drop_pair(unsigned v, uint64_t seed, int64_t idx, float p, float scale) {
    const float lo = dropout_value(__uint_as_float(v << 16), seed, idx, p, scale);
    const float hi = dropout_value(__uint_as_float(v & 0xFFFF0000u), seed, idx + 1, p, scale);
    return pack_bf16x2(lo, hi);
}

// 8 consecutive bf16 of one row as 4 dwords; elements at or past `n_valid` read as zero.  vec: the row is 16-byte aligned.
__device__ __forceinline__ uint4 load_bf16x8(const bf16_t* p, int n_valid, bool vec) {
    if (n_valid <= 0) return make_uint4(0u, 0u, 0u, 0u);
    if (vec && n_valid >= 8) return *reinterpret_cast<const uint4*>(p);
    const unsigned short* q = reinterpret_cast<const unsigned short*>(p);
    unsigned e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = i < n_valid ? (unsigned)q[i] : 0u;
    return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

// NB: 32-column blocks of U (R <= 32 NB).  grid: (column blocks of X, token splits)
template <int NB, bool DROP>
__global__ void __launch_bounds__(256) lora_wgrad_mfma_kernel(const bf16_t* __restrict__ X, int64_t ld_x, const bf16_t* __restrict__ U, int64_t ld_u,
                                                              float* __restrict__ ws, int64_t M, int C, int R, int tiles_per_split, int x_vec,
                                                              int u_vec, float p, float scale, uint64_t seed) {
    constexpr int X_BYTES = kTM * kXS, UCH = 4 * NB;         // 16-byte chunks of a U row
    __shared__ __attribute__((aligned(16))) char smem[X_BYTES + kTM * kUS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c0 = blockIdx.x * kBC, sp = blockIdx.y;
    const int64_t n_tiles = (M + kTM - 1) / kTM;
    const int64_t t0 = (int64_t)sp * tiles_per_split, t1 = t0 + tiles_per_split < n_tiles ? t0 + tiles_per_split : n_tiles;

    uint4 xr[4], ur[NB];
    auto fetch = [&](int64_t tile) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = tid + 256 * i, row = id >> 4, c = c0 + (id & 15) * 8;
            const int64_t m = tile * kTM + row;
            xr[i] = load_bf16x8(X + m * ld_x + c, m < M ? C - c : 0, x_vec != 0);        // C % 8 == 0: a chunk is whole or absent
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int id = tid + 256 * i, row = id / UCH, j = (id % UCH) * 8;
            const int64_t m = tile * kTM + row;
            ur[i] = load_bf16x8(U + m * ld_u + j, m < M ? R - j : 0, u_vec != 0);
        }
    };
    auto put = [&](int64_t tile) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = tid + 256 * i, row = id >> 4, ch = id & 15;
            uint4 v = xr[i];
            if constexpr (DROP) {
                const int64_t idx = (tile * kTM + row) * (int64_t)C + c0 + ch * 8;       // p2t_dropout_rows' counter: m K + c
                v.x = drop_pair(v.x, seed, idx, p, scale);
                v.y = drop_pair(v.y, seed, idx + 2, p, scale);
                v.z = drop_pair(v.z, seed, idx + 4, p, scale);
                v.w = drop_pair(v.w, seed, idx + 6, p, scale);
            }
            *reinterpret_cast<uint4*>(smem + row * kXS + ch * 16) = v;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int id = tid + 256 * i, row = id / UCH, ch = id % UCH;
            *reinterpret_cast<uint4*>(smem + X_BYTES + row * kUS + ch * 16) = ur[i];
        }
    };

    // transposed reads: lane 4 qq + pp of a 16-lane group addresses tile row (token) 8 hh + 4 r + qq, columns 4 pp .. 4 pp + 3 of the
    // group's 16 columns, and receives, for its own column, the four tokens of read r: two reads = the 8 tokens of an MFMA operand
    const int hh = lane >> 5, g1 = (lane >> 4) & 1, qq = (lane & 15) >> 2, pp = lane & 3;
    const int a_off = (8 * hh + qq) * kXS + (32 * w + 16 * g1 + 4 * pp) * 2;
    const int b_off = X_BYTES + (8 * hh + qq) * kUS + (16 * g1 + 4 * pp) * 2;
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

    if (t0 < t1) fetch(t0);
    for (int64_t t = t0; t < t1; ++t) {
        put(t);
        __syncthreads();
        if (t + 1 < t1) fetch(t + 1);
#pragma unroll
        for (int ks = 0; ks < kTM / 16; ++ks) {
            const short4v alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t)(smem + a_off + (16 * ks) * kXS));
            const short4v ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t)(smem + a_off + (16 * ks + 4) * kXS));
            const short8v a8 = {alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const short4v blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t)(smem + b_off + (16 * ks) * kUS + nb * 64));
                const short4v bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t)(smem + b_off + (16 * ks + 4) * kUS + nb * 64));
                const short8v b8 = {blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a8), __builtin_bit_cast(bf16x8, b8), acc[nb], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // accumulator register r: row (column of X) 8 (r >> 2) + 4 hh + (r & 3) of the wave's 32, column (of U) lane & 31
    float* out = ws + (int64_t)sp * C * R;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int j = 32 * nb + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = c0 + 32 * w + 8 * (r >> 2) + 4 * hh + (r & 3);
            if (c < C && j < R) out[(int64_t)c * R + j] = acc[nb][r];
        }
    }
}

// fp32: the same tiles; thread (tc, tj) owns columns 4 tc .. 4 tc + 3 of X against columns 8 tj .. 8 tj + 7 of U
template <bool DROP>
__global__ void __launch_bounds__(256) lora_wgrad_fma_kernel(const float* __restrict__ X, int64_t ld_x, const float* __restrict__ U, int64_t ld_u,
                                                             float* __restrict__ ws, int64_t M, int C, int R, int tiles_per_split, float p,
                                                             float scale, uint64_t seed) {
    __shared__ __attribute__((aligned(16))) float xs[kTM][kBC];
    __shared__ __attribute__((aligned(16))) float us[kTM][kMaxR];
    const int tid = threadIdx.x, tc = tid & 31, tj = tid >> 5;
    const int c0 = blockIdx.x * kBC, sp = blockIdx.y;
    const int64_t n_tiles = (M + kTM - 1) / kTM;
    const int64_t t0 = (int64_t)sp * tiles_per_split, t1 = t0 + tiles_per_split < n_tiles ? t0 + tiles_per_split : n_tiles;
    float acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.f;
    for (int64_t t = t0; t < t1; ++t) {
        for (int id = tid; id < kTM * kBC; id += 256) {
            const int row = id / kBC, col = id % kBC, c = c0 + col;
            const int64_t m = t * kTM + row;
            float x = 0.f;
            if (m < M && c < C) {
                x = X[m * ld_x + c];
                if constexpr (DROP) x = dropout_value(x, seed, m * (int64_t)C + c, p, scale);
            }
            xs[row][col] = x;
        }
        for (int id = tid; id < kTM * kMaxR; id += 256) {
            const int row = id / kMaxR, j = id % kMaxR;
            const int64_t m = t * kTM + row;
            us[row][j] = (m < M && j < R) ? U[m * ld_u + j] : 0.f;
        }
        __syncthreads();
        if (8 * tj < R) {
#pragma unroll 4
            for (int row = 0; row < kTM; ++row) {
                const float4 x4 = *reinterpret_cast<const float4*>(&xs[row][4 * tc]);
                const float4 u0 = *reinterpret_cast<const float4*>(&us[row][8 * tj]), u1 = *reinterpret_cast<const float4*>(&us[row][8 * tj + 4]);
                const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, uv[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) acc[a][b] = fmaf(xv[a], uv[b], acc[a][b]);
            }
        }
        __syncthreads();
    }
    float* out = ws + (int64_t)sp * C * R;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int c = c0 + 4 * tc + a;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int j = 8 * tj + b;
            if (c < C && j < R) out[(int64_t)c * R + j] = acc[a][b];
        }
    }
}

// G = the partial sums added in split order; stored [C, ld_g], or transposed [R, ld_g]
__global__ void __launch_bounds__(256) lora_wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int C, int R, float* __restrict__ G,
                                                                int64_t ld_g, int transposed) {
    const int64_t n = (int64_t)C * R, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += ws[k * n + i];
    const int64_t c = i / R, j = i - c * R;
    G[transposed ? j * ld_g + c : c * ld_g + j] = s;
}

}  // namespace

}  // namespace p2t

using namespace p2t;

extern "C" size_t p2t_lora_wgrad_workspace_bytes(int64_t C, int64_t R, int64_t M) {
    if (C < 1 || R < 1 || R > kMaxR || M < 1) return 0;
    int64_t tps, splits;
    wgrad_plan(C, M, &tps, &splits);
    return (size_t)splits * (size_t)C * (size_t)R * sizeof(float);
}

extern "C" int p2t_lora_wgrad(const void* X, int64_t ld_x, const void* U, int64_t ld_u, int dtype, float* G, int64_t ld_g, int transposed, int64_t M,
                              int64_t C, int64_t R, float p, uint64_t seed, void* workspace, size_t workspace_bytes, p2t_stream stream) {
    P2T_REQUIRE(X && U && G && workspace, "p2t_lora_wgrad: null pointer");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_lora_wgrad: unsupported dtype %d", dtype);
    P2T_REQUIRE(M >= 1 && M < ((int64_t)1 << 31) && C >= 1 && C < ((int64_t)1 << 31) && R >= 1 && R <= kMaxR,
                "p2t_lora_wgrad: need M >= 1, C >= 1 and 1 <= R <= %d (M %lld, C %lld, R %lld)", kMaxR, (long long)M, (long long)C, (long long)R);
    P2T_REQUIRE(ld_x >= C && ld_u >= R && ld_g >= (transposed ? C : R), "p2t_lora_wgrad: a row stride is shorter than its row");
    P2T_REQUIRE(dtype != P2T_BF16 || (C % 8 == 0 && ld_x % 8 == 0), "p2t_lora_wgrad: bf16 needs C and ld_x multiples of 8 (C %lld, ld_x %lld)",
                (long long)C, (long long)ld_x);
    P2T_REQUIRE(p >= 0.f && p < 1.f, "p2t_lora_wgrad: dropout p out of range");
    int64_t tps, splits;
    wgrad_plan(C, M, &tps, &splits);
    P2T_REQUIRE(workspace_bytes >= (size_t)splits * (size_t)C * (size_t)R * sizeof(float) && splits <= 65535,
                "p2t_lora_wgrad: workspace of %zu bytes is smaller than p2t_lora_wgrad_workspace_bytes", workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(C, kBC), (unsigned)splits);
    const float scale = 1.0f / (1.0f - p);
    float* ws = (float*)workspace;
    if (dtype == P2T_BF16) {
        const int x_vec = (uintptr_t)X % 16 == 0, u_vec = (uintptr_t)U % 16 == 0 && ld_u % 8 == 0;
#define P2T_WGRAD(NB, DROP)                                                                                                              \
    lora_wgrad_mfma_kernel<NB, DROP><<<grid, 256, 0, s>>>((const bf16_t*)X, ld_x, (const bf16_t*)U, ld_u, ws, M, (int)C, (int)R, (int)tps, x_vec, u_vec, \
                                                          p, scale, seed)
        if (R <= 32) { if (p > 0.f) P2T_WGRAD(1, true); else P2T_WGRAD(1, false); }
        else         { if (p > 0.f) P2T_WGRAD(2, true); else P2T_WGRAD(2, false); }
#undef P2T_WGRAD
    } else {
        if (p > 0.f) lora_wgrad_fma_kernel<true><<<grid, 256, 0, s>>>((const float*)X, ld_x, (const float*)U, ld_u, ws, M, (int)C, (int)R, (int)tps, p, scale, seed);
        else lora_wgrad_fma_kernel<false><<<grid, 256, 0, s>>>((const float*)X, ld_x, (const float*)U, ld_u, ws, M, (int)C, (int)R, (int)tps, p, scale, seed);
    }
    P2T_LAUNCH_CHECK();
    lora_wgrad_reduce_kernel<<<(unsigned)ceil_div(C * R, 256), 256, 0, s>>>(ws, (int)splits, (int)C, (int)R, G, ld_g, transposed);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
