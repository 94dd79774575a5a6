// fp8 (OCP e4m3fn) quantisation of GEMM operands for BASELINE.json configs[4] ("fp8 weights, CDNA4 fp8 MFMA").
//
// Scheme: every ROW of a GEMM operand (a token's activations, an output channel's weights) gets
// one power-of-two scale stored as an E8M0 byte  E = 127 + e,  2^e = the smallest power of two with amax / 2^e <= 448
// (the e4m3 maximum), and its elements are stored as e4m3fn( x * 2^-e ), round-to-nearest-even (v_cvt_pk_fp8_f32).
// The scaling itself is exact (power of two), so the only rounding is the e4m3 one, and the numpy oracle reproduces
// bytes and scale bytes bit for bit (oracle/p2t_oracle.py quant_rows_e4m3).  The E8M0 bytes are what the block-scaled
// MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) takes as its scale operands: the hardware applies 2^(Ea-127) * 2^(Ew-127).
//
//   quant_rows_kernel     bf16 / f32 [rows, ld_x] -> fp8 [rows, ld_q] (+ E8M0 [rows]); columns [cols, ld_q) zeroed
//   quant_rows_few_kernel the same for the few rows of a decode step, one block per row
// The norms that write fp8 directly are in norm.hip; the E8M0 / e4m3 helpers they share with this file are in quant_fp8.h.
#include "common.h"
#include "kernels.h"
#include "quant_fp8.h"

namespace p2t {

// v = the 8 elements of row xr at columns c .. c + 7, zeros from cols on
template <typename Tin>
__device__ __forceinline__ void load_block8(const Tin* xr, int c, int cols, float (&v)[8]) {
    if (c + 8 <= cols) {
        if constexpr (sizeof(Tin) == 2) { load8(xr + c, v); } else { float a[4], b[4]; load4(xr + c, a); load4(xr + c + 4, b);
            for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; } }
    } else {
        for (int j = 0; j < 8; ++j) v[j] = c + j < cols ? to_f32(xr[c + j]) : 0.f;
    }
}

// one wave per row, two passes over the row (the second one hits L1 / L2)
template <typename Tin>
__global__ void __launch_bounds__(256) quant_rows_kernel(const Tin* __restrict__ x, int64_t ld_x, int64_t rows, int cols,
                                                         uint8_t* __restrict__ q, int64_t ld_q, uint8_t* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const Tin* xr = x + row * ld_x;
    float amax = 0.f;
    for (int c = lane * 8; c < cols; c += 512) {
        float v[8];
        load_block8(xr, c, cols, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    }
    amax = wave_max(amax);
    const int E = e8m0_of_amax(amax);
    const float inv = pow2_neg(E);
    if (lane == 0) scale[row] = (uint8_t)E;
    uint8_t* qr = q + row * ld_q;
    for (int c = lane * 8; c < ld_q; c += 512) {
        float v[8];
        load_block8(xr, c, cols, v);
        *reinterpret_cast<uint2*>(qr + c) = make_uint2(pack_fp8x4(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv),
                                                       pack_fp8x4(v[4] * inv, v[5] * inv, v[6] * inv, v[7] * inv));
    }
}

int launch_quant_rows(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* q, int64_t ld_q, uint8_t* scale,
                      hipStream_t s) {
    if (rows == 0) return P2T_OK;
    P2T_REQUIRE(ld_q % 8 == 0 && ld_q >= cols && ld_x % 8 == 0, "quant_rows: ld_q and ld_x must be multiples of 8 (ld_q=%lld ld_x=%lld)",
                (long long)ld_q, (long long)ld_x);
    const dim3 grid((unsigned)ceil_div(rows, 4));
    if (dtype == P2T_BF16)
        quant_rows_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)x, ld_x, rows, (int)cols, (uint8_t*)q, ld_q, scale);
    else
        quant_rows_kernel<float><<<grid, 256, 0, s>>>((const float*)x, ld_x, rows, (int)cols, (uint8_t*)q, ld_q, scale);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

// ---- a handful of rows (one decode step of a gemm_fp8 model): one BLOCK per row, the row in registers, every load requested up
// front (the wave-per-row kernels above walk a 14 336-wide row in 28 dependent trips: 12 us; this form: one) ----
// NV chunks of 8 elements per thread: cols <= NV * 2048.  Bit-identical to quant_rows_kernel (a maximum has no order).
template <typename Tin, int NV>
__global__ void __launch_bounds__(256) quant_rows_few_kernel(const Tin* __restrict__ x, int64_t ld_x, int cols, uint8_t* __restrict__ q, int64_t ld_q,
                                                             uint8_t* __restrict__ scale) {
    __shared__ float red[4];
    const Tin* xr = x + (int64_t)blockIdx.x * ld_x;
    float v[NV][8];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) load_block8(xr, (i * 256 + threadIdx.x) * 8, cols, v[i]);
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[i][j]));
    amax = block_max4(amax, red);
    const int E = e8m0_of_amax(amax);
    const float inv = pow2_neg(E);
    if (threadIdx.x == 0) scale[blockIdx.x] = (uint8_t)E;
    uint8_t* qr = q + (int64_t)blockIdx.x * ld_q;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 256 + threadIdx.x) * 8;
        if (c < ld_q)
            *reinterpret_cast<uint2*>(qr + c) = make_uint2(pack_fp8x4(v[i][0] * inv, v[i][1] * inv, v[i][2] * inv, v[i][3] * inv),
                                                           pack_fp8x4(v[i][4] * inv, v[i][5] * inv, v[i][6] * inv, v[i][7] * inv));
    }
}

int launch_quant_rows_few(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* q, int64_t ld_q, uint8_t* scale, hipStream_t s) {
    if (rows == 0) return P2T_OK;
    if (ld_q % 8 || ld_q < cols || ld_x % 8 || ld_q > 8 * 2048) return launch_quant_rows(x, dtype, ld_x, rows, cols, q, ld_q, scale, s);
#define P2T_QF(NV)                                                                                                                 \
    do {                                                                                                                           \
        if (dtype == P2T_BF16) quant_rows_few_kernel<bf16_t, NV><<<(unsigned)rows, 256, 0, s>>>((const bf16_t*)x, ld_x, (int)cols, (uint8_t*)q, ld_q, scale); \
        else quant_rows_few_kernel<float, NV><<<(unsigned)rows, 256, 0, s>>>((const float*)x, ld_x, (int)cols, (uint8_t*)q, ld_q, scale);                   \
    } while (0)
    if (ld_q <= 2048) P2T_QF(1); else if (ld_q <= 4096) P2T_QF(2); else if (ld_q <= 8192) P2T_QF(4); else P2T_QF(8);
#undef P2T_QF
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

// ---- MXFP4 weights (include/p2t_hip.h, "MXFP4 decoder weights"): e2m1 codes + one E8M0 byte per block of 32 columns ----
// e of a block from its absolute maximum: the smallest integer with amax / 2^e <= 6 = 1.5 * 2^2 (the integer rule of e8m0_of_amax):
// amax = (1 + f) 2^ea  ->  e = ea - 2 + (f > 0.5)
__device__ __forceinline__ int mx_e_of_amax(float amax) {
    const unsigned u = __float_as_uint(amax);
    return (int)((u >> 23) & 0xFF) - 127 - 2 + ((u & 0x7FFFFF) > 0x400000 ? 1 : 0);
}
// round-to-nearest onto {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code; v in [0, 6]
__device__ __forceinline__ unsigned mx_code(float v) {
    return (unsigned)(v > 0.25f) + (v >= 0.75f) + (v > 1.25f) + (v >= 1.75f) + (v > 2.5f) + (v >= 3.5f) + (v > 5.0f);
}

// One block per row, one thread per MX block of 32 columns (blocks tid, tid + 256, ..), two passes over the row: block maxima and the
// row maximum first, then the clamped scale bytes and the codes (the second pass hits L1 / L2).
template <typename Tin>
__global__ void __launch_bounds__(256) quant_rows_mxfp4_kernel(const Tin* __restrict__ x, int64_t ld_x, int cols, uint8_t* __restrict__ codes,
                                                               int64_t ld_codes, uint8_t* __restrict__ scales) {
    __shared__ float red[4];
    const int nb = (cols + 127) / 128 * 4;
    const Tin* xr = x + (int64_t)blockIdx.x * ld_x;
    float emax = -INFINITY;                                         // exponents are small integers: exact as floats
    for (int j = threadIdx.x; j < nb; j += 256) {
        float amax = 0.f;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float v[8];
            load_block8(xr, 32 * j + 8 * p, cols, v);
#pragma unroll
            for (int t = 0; t < 8; ++t) amax = fmaxf(amax, fabsf(v[t]));
        }
        if (amax > 0.f) emax = fmaxf(emax, (float)mx_e_of_amax(amax));
    }
    emax = block_max4(emax, red);
    const bool zero_row = !(emax > -INFINITY);
    const int e_floor = zero_row ? 0 : (int)emax - 8;
    for (int j = threadIdx.x; j < nb; j += 256) {
        float v[32];
        float amax = 0.f;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float t8[8];
            load_block8(xr, 32 * j + 8 * p, cols, t8);
#pragma unroll
            for (int t = 0; t < 8; ++t) { v[8 * p + t] = t8[t]; amax = fmaxf(amax, fabsf(t8[t])); }
        }
        int e = amax > 0.f ? max(mx_e_of_amax(amax), e_floor) : e_floor;
        const int E = min(max(e + 127, 1), 253);
        const float inv = pow2_neg(E);
        unsigned wds[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            unsigned wd = 0;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float f = v[8 * p + t];
                wd |= (mx_code(fabsf(f) * inv) | (f < 0.f ? 8u : 0u)) << (4 * t);
            }
            wds[p] = wd;
        }
        *reinterpret_cast<uint4*>(codes + (int64_t)blockIdx.x * ld_codes + 16 * j) = make_uint4(wds[0], wds[1], wds[2], wds[3]);
        scales[(int64_t)blockIdx.x * nb + j] = (uint8_t)E;
    }
}

// out[r, c] = grid[code & 7] * 2^(scale byte - 127), signed: at most two significant bits, exact in bf16.  One thread per 8 columns.
__global__ void __launch_bounds__(256) dequant_rows_mxfp4_kernel(const uint8_t* __restrict__ codes, int64_t ld_codes, const uint8_t* __restrict__ scales,
                                                                 int64_t rows, int cols, bf16_t* __restrict__ out, int64_t ld_out) {
    const int per = (cols + 7) / 8, nb = (cols + 127) / 128 * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows * per; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / per;
        const int c0 = (int)(i - r * per) * 8;
        const unsigned wd = *reinterpret_cast<const unsigned*>(codes + r * ld_codes + c0 / 2);
        const int e = (int)scales[r * nb + c0 / 32] - 127;
        for (int t = 0; t < 8 && c0 + t < cols; ++t) {
            const unsigned cd = (wd >> (4 * t)) & 15u, ex = (cd >> 1) & 3u, mn = cd & 1u;
            const float mag = ex == 0 ? 0.5f * (float)mn : ldexpf(1.0f + 0.5f * (float)mn, (int)ex - 1);
            const float val = ldexpf(mag, e);
            out[r * ld_out + c0 + t] = from_f32<bf16_t>((cd & 8u) ? -val : val);
        }
    }
}

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_quant_rows_mxfp4(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* codes, int64_t ld_codes,
                                    uint8_t* scales, p2t_stream stream) {
    P2T_REQUIRE(x && codes && scales && rows >= 0 && cols > 0 && cols < (1 << 30) && (dtype == P2T_F32 || dtype == P2T_BF16),
                "p2t_quant_rows_mxfp4: bad arguments");
    P2T_REQUIRE(ld_x % 8 == 0 && ld_x >= cols && ld_codes % 16 == 0 && ld_codes >= round_up(cols, 128) / 2,
                "p2t_quant_rows_mxfp4: ld_x must be a multiple of 8, ld_codes a multiple of 16 and >= round_up(cols, 128) / 2 (ld_x=%lld ld_codes=%lld)",
                (long long)ld_x, (long long)ld_codes);
    if (rows == 0) return P2T_OK;
    P2T_REQUIRE(rows < (1ll << 31), "p2t_quant_rows_mxfp4: too many rows");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == P2T_BF16)
        quant_rows_mxfp4_kernel<bf16_t><<<(unsigned)rows, 256, 0, s>>>((const bf16_t*)x, ld_x, (int)cols, (uint8_t*)codes, ld_codes, scales);
    else
        quant_rows_mxfp4_kernel<float><<<(unsigned)rows, 256, 0, s>>>((const float*)x, ld_x, (int)cols, (uint8_t*)codes, ld_codes, scales);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_dequant_rows_mxfp4(const void* codes, int64_t ld_codes, const uint8_t* scales, int64_t rows, int64_t cols, void* out,
                                      int64_t ld_out, p2t_stream stream) {
    P2T_REQUIRE(codes && scales && out && rows >= 0 && cols > 0 && cols < (1 << 30), "p2t_dequant_rows_mxfp4: bad arguments");
    P2T_REQUIRE(ld_codes % 16 == 0 && ld_codes >= round_up(cols, 128) / 2 && ld_out >= cols,
                "p2t_dequant_rows_mxfp4: ld_codes must be a multiple of 16 and >= round_up(cols, 128) / 2, ld_out >= cols");
    if (rows == 0) return P2T_OK;
    const int64_t items = rows * ceil_div(cols, 8), blocks = ceil_div(items, 256);
    dequant_rows_mxfp4_kernel<<<(unsigned)(blocks > 65535 ? 65535 : blocks), 256, 0, (hipStream_t)stream>>>((const uint8_t*)codes, ld_codes, scales, rows,
                                                                                                           (int)cols, (bf16_t*)out, ld_out);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_quant_rows_fp8(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* q, int64_t ld_q,
                                  uint8_t* scale, p2t_stream stream) {
    P2T_REQUIRE(x && q && scale && rows >= 0 && cols > 0 && (dtype == P2T_F32 || dtype == P2T_BF16), "p2t_quant_rows_fp8: bad arguments");
    return launch_quant_rows(x, dtype, ld_x, rows, cols, q, ld_q, scale, (hipStream_t)stream);
}
