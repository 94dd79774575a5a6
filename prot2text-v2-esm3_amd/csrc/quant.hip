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

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_quant_rows_fp8(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* q, int64_t ld_q,
                                  uint8_t* scale, p2t_stream stream) {
    P2T_REQUIRE(x && q && scale && rows >= 0 && cols > 0 && (dtype == P2T_F32 || dtype == P2T_BF16), "p2t_quant_rows_fp8: bad arguments");
    return launch_quant_rows(x, dtype, ld_x, rows, cols, q, ld_q, scale, (hipStream_t)stream);
}
