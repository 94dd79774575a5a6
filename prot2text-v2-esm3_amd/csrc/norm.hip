// Every norm kernel, forward and backward: LayerNorm / RMSNorm / row L2-normalise.  HBM-bound: one wavefront per row, the
// row held in registers (16 B per lane per load), wave-shuffle reductions, no LDS, no block barrier.
//   LayerNorm: HF EsmLayer pre-LN + emb_layer_norm_after (transformers/models/esm/modeling_esm.py:418,429,480,518,529,553)
//   RMSNorm:   HF LlamaRMSNorm (transformers/models/llama/modeling_llama.py:62-67)
//   L2 rows:   torch.nn.functional.normalize (reference models/modeling_esm2llama_instruct.py:67,
//              scripts/train_contrast.py:354,365)
//   norm_kernel              LayerNorm / RMSNorm of the f32 residual stream, stored as f32 / bf16
//   norm_fp8_kernel          the same row written straight as e4m3 + one E8M0 byte (the scheme of quant.hip), the GEMM operand the
//                            next projection reads: no bf16 intermediate, no extra pass
//   rmsnorm_rows_kernel, rmsnorm_fp8_rows_kernel   the two RMSNorm forms for the few rows of a decode step: one block per row
//   rmsnorm_bwd_kernel, layernorm_bwd_kernel       dX with frozen weights (the stage-2 steps through the decoder / the encoder)
// The forward row bodies (load, statistics, one normalised chunk) are written once, in norm_row.h.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "norm_row.h"
#include "quant_fp8.h"

namespace p2t {

// NV = float4 loads per lane; covers cols <= NV*256.
template <int NV, typename Tout, bool RMS>
__global__ void __launch_bounds__(256) norm_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w,
                                                   const float* __restrict__ b, float eps, Tout* __restrict__ y,
                                                   int64_t ld_y, int64_t rows, int cols) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[NV][4];
    float mean, rstd;
    wave_row_stats<NV, RMS>(x + row * ld_x, cols, lane, eps, v, mean, rstd);
    Tout* yr = y + row * ld_y;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < cols) {
            float o[4];
            norm_chunk<RMS>(v[i], mean, rstd, w, b, c, o);
            store4(yr + c, o);
        } else if (c < ld_y) {
            const float z[4] = {0.f, 0.f, 0.f, 0.f};
            store4(yr + c, z);
        }
    }
}

// the same row, output quantised in place
template <int NV, bool RMS>
__global__ void __launch_bounds__(256) norm_fp8_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w,
                                                       const float* __restrict__ b, float eps, uint8_t* __restrict__ q, int64_t ld_q,
                                                       uint8_t* __restrict__ scale, int64_t rows, int cols, float bound_w, float bound_b,
                                                       uint8_t* __restrict__ bound_scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[NV][4];
    float mean, rstd;
    wave_row_stats<NV, RMS>(x + row * ld_x, cols, lane, eps, v, mean, rstd);
    float amax = 0.f, ssq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < cols) {
            norm_chunk<RMS>(v[i], mean, rstd, w, b, c, v[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) { amax = fmaxf(amax, fabsf(v[i][j])); ssq = fmaf(v[i][j], v[i][j], ssq); }
        }
    }
    amax = wave_max(amax);
    if (bound_scale) {           // scale of the NEXT projection's gelu output, from the Cauchy-Schwarz bound of its pre-activation
        ssq = wave_sum(ssq);
        if (lane == 0) bound_scale[row] = (uint8_t)e8m0_of_amax(fmaf(sqrtf(ssq), bound_w, bound_b));
    }
    const int E = e8m0_of_amax(amax);
    const float inv = pow2_neg(E);
    if (lane == 0) scale[row] = (uint8_t)E;
    uint8_t* qr = q + row * ld_q;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < cols) *reinterpret_cast<unsigned*>(qr + c) = pack_fp8x4(v[i][0] * inv, v[i][1] * inv, v[i][2] * inv, v[i][3] * inv);
        else if (c < ld_q) *reinterpret_cast<unsigned*>(qr + c) = 0u;
    }
}

// A handful of rows (one decode step: rows = sequences that generate): one BLOCK per row, the row's and the weight's 16-byte pieces
// all requested before anything is waited for -- one round trip to memory instead of the wave-per-row kernel's two (9.2 -> 4 us
// for 8 x 4096, 65 of them per generated token).  Same arithmetic as norm_kernel<.., RMS> except for the order of the sum.
template <int NV, typename Tout>
__global__ void __launch_bounds__(256) rmsnorm_rows_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w, float eps,
                                                           Tout* __restrict__ y, int64_t ld_y, int cols) {
    __shared__ float red[4];
    float v[NV][4], wv[NV][4];
    const float rstd = block_row_rstd<NV>(x + (int64_t)blockIdx.x * ld_x, w, cols, eps, red, v, wv);
    Tout* yr = y + (int64_t)blockIdx.x * ld_y;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 256 + threadIdx.x) * 4;
        if (c < ld_y) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = c < cols ? wv[i][j] * (v[i][j] * rstd) : 0.f;
            store4(yr + c, o);
        }
    }
}

// RMSNorm of a few rows of the f32 stream written as e4m3 + E8M0 (norm_fp8_kernel<.., RMS>'s arithmetic, another order of the sum)
template <int NV>
__global__ void __launch_bounds__(256) rmsnorm_fp8_rows_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w, float eps,
                                                               uint8_t* __restrict__ q, int64_t ld_q, uint8_t* __restrict__ scale, int cols) {
    __shared__ float red[4];
    float v[NV][4], wv[NV][4];
    const float rstd = block_row_rstd<NV>(x + (int64_t)blockIdx.x * ld_x, w, cols, eps, red, v, wv);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[i][j] = wv[i][j] * (v[i][j] * rstd);
            amax = fmaxf(amax, fabsf(v[i][j]));
        }
    amax = block_max4(amax, red);
    const int E = e8m0_of_amax(amax);
    const float inv = pow2_neg(E);
    if (threadIdx.x == 0) scale[blockIdx.x] = (uint8_t)E;
    uint8_t* qr = q + (int64_t)blockIdx.x * ld_q;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 256 + threadIdx.x) * 4;
        if (c < cols) *reinterpret_cast<unsigned*>(qr + c) = pack_fp8x4(v[i][0] * inv, v[i][1] * inv, v[i][2] * inv, v[i][3] * inv);
        else if (c < ld_q) *reinterpret_cast<unsigned*>(qr + c) = 0u;
    }
}

// calls f(integral_constant<NV>) for the first NV of the list with span <= NV * per_nv; false if there is none
template <int... NVS, typename F>
static bool first_nv(int64_t span, int per_nv, F&& f) {
    return ((span <= (int64_t)NVS * per_nv ? (f(std::integral_constant<int, NVS>{}), true) : false) || ...);
}
// the NV of a wave-per-row kernel (span <= NV * 256) and of a block-per-row one (span <= NV * 1024), plain and fp8 alike
template <typename F> static bool wave_row_nv(int64_t span, F&& f) { return first_nv<1, 2, 4, 8, 10, 16, 32>(span, 256, f); }
template <typename F> static bool block_row_nv(int64_t span, F&& f) { return first_nv<1, 2, 4, 8>(span, 1024, f); }

template <typename Tout, bool RMS>
static int launch_norm_t(const float* x, int64_t ld_x, const float* w, const float* b, float eps, Tout* y, int64_t ld_y,
                         int64_t rows, int64_t cols, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(rows, 4));
    if (!wave_row_nv(ld_y > cols ? ld_y : cols, [&](auto nv) {
            norm_kernel<decltype(nv)::value, Tout, RMS><<<grid, 256, 0, s>>>(x, ld_x, w, b, eps, y, ld_y, rows, (int)cols);
        })) {
        set_error("norm: %lld columns exceed the 8192 supported", (long long)cols);
        return P2T_ERR_UNSUPPORTED;
    }
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

template <bool RMS>
static int launch_norm_fp8_t(const float* x, int64_t ld_x, const float* w, const float* b, float eps, uint8_t* q, int64_t ld_q,
                             uint8_t* scale, int64_t rows, int64_t cols, float bound_w, float bound_b, uint8_t* bound_scale, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(rows, 4));
    if (!wave_row_nv(ld_q > cols ? ld_q : cols, [&](auto nv) {
            norm_fp8_kernel<decltype(nv)::value, RMS><<<grid, 256, 0, s>>>(x, ld_x, w, b, eps, q, ld_q, scale, rows, (int)cols, bound_w, bound_b,
                                                                          bound_scale);
        })) {
        set_error("norm (fp8 output): %lld columns exceed the 8192 supported", (long long)cols);
        return P2T_ERR_UNSUPPORTED;
    }
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

int launch_layernorm(const float* x, int64_t ld_x, const float* w, const float* b, float eps, void* y, int64_t ld_y,
                     int64_t rows, int64_t cols, int out_dtype, hipStream_t s) {
    if (rows == 0) return P2T_OK;
    if (out_dtype == P2T_BF16) return launch_norm_t<bf16_t, false>(x, ld_x, w, b, eps, (bf16_t*)y, ld_y, rows, cols, s);
    return launch_norm_t<float, false>(x, ld_x, w, b, eps, (float*)y, ld_y, rows, cols, s);
}
int launch_rmsnorm(const float* x, int64_t ld_x, const float* w, float eps, void* y, int64_t ld_y, int64_t rows,
                   int64_t cols, int out_dtype, hipStream_t s) {
    if (rows == 0) return P2T_OK;
    if (out_dtype == P2T_BF16) return launch_norm_t<bf16_t, true>(x, ld_x, w, nullptr, eps, (bf16_t*)y, ld_y, rows, cols, s);
    return launch_norm_t<float, true>(x, ld_x, w, nullptr, eps, (float*)y, ld_y, rows, cols, s);
}
int launch_layernorm_fp8(const float* x, int64_t ld_x, const float* w, const float* b, float eps, void* q, int64_t ld_q,
                         uint8_t* scale, int64_t rows, int64_t cols, float bound_w, float bound_b, uint8_t* bound_scale, hipStream_t s) {
    if (rows == 0) return P2T_OK;
    P2T_REQUIRE(cols % 4 == 0 && ld_q % 4 == 0 && ld_q >= cols, "layernorm (fp8 output): cols and ld_q must be multiples of 4");
    return launch_norm_fp8_t<false>(x, ld_x, w, b, eps, (uint8_t*)q, ld_q, scale, rows, cols, bound_w, bound_b, bound_scale, s);
}
int launch_rmsnorm_fp8(const float* x, int64_t ld_x, const float* w, float eps, void* q, int64_t ld_q, uint8_t* scale, int64_t rows,
                       int64_t cols, hipStream_t s) {
    if (rows == 0) return P2T_OK;
    P2T_REQUIRE(cols % 4 == 0 && ld_q % 4 == 0 && ld_q >= cols, "rmsnorm (fp8 output): cols and ld_q must be multiples of 4");
    return launch_norm_fp8_t<true>(x, ld_x, w, nullptr, eps, (uint8_t*)q, ld_q, scale, rows, cols, 0.f, 0.f, nullptr, s);
}

// the decode step's RMSNorms (a few rows): block per row, one round trip; beyond 8192 columns the wave-per-row kernels take the call
int launch_rmsnorm_few_rows(const float* x, int64_t ld_x, const float* w, float eps, void* y, int64_t ld_y, int64_t rows, int64_t cols, int out_dtype,
                            hipStream_t s) {
    if (rows == 0) return P2T_OK;
    if (!block_row_nv(ld_y > cols ? ld_y : cols, [&](auto nv) {
            constexpr int NV = decltype(nv)::value;
            if (out_dtype == P2T_BF16) rmsnorm_rows_kernel<NV, bf16_t><<<(unsigned)rows, 256, 0, s>>>(x, ld_x, w, eps, (bf16_t*)y, ld_y, (int)cols);
            else rmsnorm_rows_kernel<NV, float><<<(unsigned)rows, 256, 0, s>>>(x, ld_x, w, eps, (float*)y, ld_y, (int)cols);
        }))
        return launch_rmsnorm(x, ld_x, w, eps, y, ld_y, rows, cols, out_dtype, s);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
int launch_rmsnorm_fp8_few(const float* x, int64_t ld_x, const float* w, float eps, void* q, int64_t ld_q, uint8_t* scale, int64_t rows, int64_t cols,
                           hipStream_t s) {
    if (rows == 0) return P2T_OK;
    if (cols % 4 || ld_q % 4 || ld_q < cols ||
        !block_row_nv(ld_q, [&](auto nv) {
            rmsnorm_fp8_rows_kernel<decltype(nv)::value><<<(unsigned)rows, 256, 0, s>>>(x, ld_x, w, eps, (uint8_t*)q, ld_q, scale, (int)cols);
        }))
        return launch_rmsnorm_fp8(x, ld_x, w, eps, q, ld_q, scale, rows, cols, s);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

// ---------------------------------------------------------------------------------------------
// RMSNorm backward: y = x * rsqrt(mean(x^2) + eps) * w   ->   g (+)= r * (w dy) - x r^3 mean(w dy x).  One wave per row, two
// passes over the row (the second hits L2).  dy: f32 or `dtype`.
template <typename Tdy>
__global__ void __launch_bounds__(256) rmsnorm_bwd_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w, float eps,
                                                          const Tdy* __restrict__ dy, int64_t ld_dy, float* __restrict__ g, int64_t ld_g,
                                                          int64_t rows, int cols, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * ld_x;
    const Tdy* dr = dy + row * ld_dy;
    float ss = 0.f, dot = 0.f;
    for (int c = lane * 4; c < cols; c += 256) {
        float xv[4], dv[4], wv[4];
        load4(xr + c, xv); load4(dr + c, dv); load4(w + c, wv);
#pragma unroll
        for (int j = 0; j < 4; ++j) { ss = fmaf(xv[j], xv[j], ss); dot = fmaf(dv[j] * wv[j], xv[j], dot); }
    }
    ss = wave_sum(ss);
    dot = wave_sum(dot);
    const float r = rsqrtf(ss / (float)cols + eps);
    const float k = r * r * r * dot / (float)cols;
    float* gr = g + row * ld_g;
    for (int c = lane * 4; c < cols; c += 256) {
        float xv[4], dv[4], wv[4], o[4];
        load4(xr + c, xv); load4(dr + c, dv); load4(w + c, wv);
        if (accumulate) load4(gr + c, o); else o[0] = o[1] = o[2] = o[3] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += r * (dv[j] * wv[j]) - xv[j] * k;
        store4(gr + c, o);
    }
}

// LayerNorm backward: y = (x - mu) r w + b, r = rsqrt(var + eps)  ->  g (+)= r (w dy - mean(w dy) - xhat mean(w dy xhat)),
// xhat = (x - mu) r.  One wave per row (four rows per block); the mean pass, the statistics pass and the write pass re-read the
// row (L2 resident).
template <typename Tdy>
__global__ void __launch_bounds__(256) layernorm_bwd_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w, float eps,
                                                            const Tdy* __restrict__ dy, int64_t ld_dy, float* __restrict__ g, int64_t ld_g,
                                                            int64_t rows, int cols, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * ld_x;
    const Tdy* dr = dy + row * ld_dy;
    const float inv_n = 1.0f / (float)cols;
    float s = 0.f;
    for (int c = lane * 4; c < cols; c += 256) {
        float xv[4];
        load4(xr + c, xv);
        s += (xv[0] + xv[1]) + (xv[2] + xv[3]);
    }
    const float mu = wave_sum(s) * inv_n;
    float var = 0.f, s1 = 0.f, s2 = 0.f;
    for (int c = lane * 4; c < cols; c += 256) {
        float xv[4], dv[4], wv[4];
        load4(xr + c, xv); load4(dr + c, dv); load4(w + c, wv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xc = xv[j] - mu, gw = dv[j] * wv[j];
            var = fmaf(xc, xc, var);
            s1 += gw;
            s2 = fmaf(gw, xc, s2);
        }
    }
    var = wave_sum(var);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    const float r = rsqrtf(var * inv_n + eps);
    const float m1 = s1 * inv_n, k2 = r * r * s2 * inv_n;       // mean(w dy), mean(w dy xhat) / r
    float* gr = g + row * ld_g;
    for (int c = lane * 4; c < cols; c += 256) {
        float xv[4], dv[4], wv[4], o[4];
        load4(xr + c, xv); load4(dr + c, dv); load4(w + c, wv);
        if (accumulate) load4(gr + c, o); else o[0] = o[1] = o[2] = o[3] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += r * (dv[j] * wv[j] - m1 - (xv[j] - mu) * k2);
        store4(gr + c, o);
    }
}

// both backwards take the same arguments and the same grid; dy is f32 or bf16
#define P2T_NORM_BWD(KERNEL)                                                                                                                  \
    do {                                                                                                                                      \
        const dim3 grid((unsigned)ceil_div(rows, 4));                                                                                         \
        if (dy_dtype == P2T_BF16) KERNEL<bf16_t><<<grid, 256, 0, s>>>(x, ld_x, w, eps, (const bf16_t*)dy, ld_dy, g, ld_g, rows, (int)cols, accumulate); \
        else KERNEL<float><<<grid, 256, 0, s>>>(x, ld_x, w, eps, (const float*)dy, ld_dy, g, ld_g, rows, (int)cols, accumulate);              \
        P2T_LAUNCH_CHECK();                                                                                                                   \
        return P2T_OK;                                                                                                                        \
    } while (0)

int launch_rmsnorm_bwd(const float* x, int64_t ld_x, const float* w, float eps, const void* dy, int64_t ld_dy, int dy_dtype, float* g,
                       int64_t ld_g, int64_t rows, int64_t cols, int accumulate, hipStream_t s) {
    P2T_REQUIRE(cols % 4 == 0 && ld_x % 4 == 0 && ld_dy % 4 == 0 && ld_g % 4 == 0, "rmsnorm backward: cols / strides must be multiples of 4");
    P2T_NORM_BWD(rmsnorm_bwd_kernel);
}
static int launch_layernorm_bwd(const float* x, int64_t ld_x, const float* w, float eps, const void* dy, int64_t ld_dy, int dy_dtype, float* g,
                                int64_t ld_g, int64_t rows, int64_t cols, int accumulate, hipStream_t s) {
    P2T_NORM_BWD(layernorm_bwd_kernel);
}
#undef P2T_NORM_BWD

// ---------------------------------------------------------------------------------------------
// y = x / max(||x||, eps), one wave per row, second pass re-reads the row (L1/L2 resident).
template <typename Tin, typename Tout>
__global__ void __launch_bounds__(256) l2norm_kernel(const Tin* __restrict__ x, int64_t ld_x, Tout* __restrict__ y,
                                                     int64_t ld_y, float* __restrict__ inv_norm, int64_t rows, int cols,
                                                     float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const Tin* xr = x + row * ld_x;
    float s = 0.f;
    for (int c = lane * 4; c < cols; c += 256) {
        float v[4];
        load4(xr + c, v);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    s = wave_sum(s);
    const float inv = 1.0f / fmaxf(sqrtf(s), eps);
    if (inv_norm && lane == 0) inv_norm[row] = inv;
    Tout* yr = y + row * ld_y;
    for (int c = lane * 4; c < ld_y; c += 256) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < cols) {
            load4(xr + c, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= inv;
        }
        store4(yr + c, v);
    }
}

// dx = (dy - y (dy . y)) / max(||x||, eps)
__global__ void __launch_bounds__(256) l2norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ dx, int64_t rows, int cols, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * cols;
    const float* gr = dy + row * cols;
    float s = 0.f, d = 0.f;
    for (int c = lane * 4; c < cols; c += 256) {
        float v[4], g[4];
        load4(xr + c, v);
        load4(gr + c, g);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        d += v[0] * g[0] + v[1] * g[1] + v[2] * g[2] + v[3] * g[3];
    }
    s = wave_sum(s);
    d = wave_sum(d);
    const float inv = 1.0f / fmaxf(sqrtf(s), eps);
    const float dot = d * inv;          // dy . y
    for (int c = lane * 4; c < cols; c += 256) {
        float v[4], g[4], o[4];
        load4(xr + c, v);
        load4(gr + c, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (g[j] - v[j] * inv * dot) * inv;
        store4(dx + row * cols + c, o);
    }
}

int launch_l2norm(const void* x, int in_dtype, int64_t ld_x, void* y, int out_dtype, int64_t ld_y, float* inv_norm,
                  int64_t rows, int64_t cols, float eps, hipStream_t s) {
    if (rows == 0) return P2T_OK;
    P2T_REQUIRE(cols % 4 == 0 && ld_x % 4 == 0 && ld_y % 4 == 0, "l2norm: cols/ld must be multiples of 4");
    const dim3 grid((unsigned)ceil_div(rows, 4));
    if (in_dtype == P2T_BF16 && out_dtype == P2T_BF16)
        l2norm_kernel<bf16_t, bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)x, ld_x, (bf16_t*)y, ld_y, inv_norm, rows, (int)cols, eps);
    else if (in_dtype == P2T_F32 && out_dtype == P2T_F32)
        l2norm_kernel<float, float><<<grid, 256, 0, s>>>((const float*)x, ld_x, (float*)y, ld_y, inv_norm, rows, (int)cols, eps);
    else if (in_dtype == P2T_BF16 && out_dtype == P2T_F32)
        l2norm_kernel<bf16_t, float><<<grid, 256, 0, s>>>((const bf16_t*)x, ld_x, (float*)y, ld_y, inv_norm, rows, (int)cols, eps);
    else
        l2norm_kernel<float, bf16_t><<<grid, 256, 0, s>>>((const float*)x, ld_x, (bf16_t*)y, ld_y, inv_norm, rows, (int)cols, eps);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_layernorm(const float* x, int64_t ld_x, const float* w, const float* b, float eps, void* y,
                             int64_t ld_y, int64_t rows, int64_t cols, int out_dtype, p2t_stream stream) {
    P2T_REQUIRE(x && w && b && y && cols > 0 && cols % 4 == 0 && ld_x % 4 == 0 && ld_y % 4 == 0 && ld_y >= cols,
                "p2t_layernorm: bad arguments (cols and strides must be multiples of 4)");
    return launch_layernorm(x, ld_x, w, b, eps, y, ld_y, rows, cols, out_dtype, (hipStream_t)stream);
}
extern "C" int p2t_rmsnorm(const float* x, int64_t ld_x, const float* w, float eps, void* y, int64_t ld_y, int64_t rows,
                           int64_t cols, int out_dtype, p2t_stream stream) {
    P2T_REQUIRE(x && w && y && cols > 0 && cols % 4 == 0 && ld_x % 4 == 0 && ld_y % 4 == 0 && ld_y >= cols,
                "p2t_rmsnorm: bad arguments (cols and strides must be multiples of 4)");
    return launch_rmsnorm(x, ld_x, w, eps, y, ld_y, rows, cols, out_dtype, (hipStream_t)stream);
}

extern "C" int p2t_layernorm_fp8(const float* x, int64_t ld_x, const float* w, const float* b, float eps, void* q, int64_t ld_q,
                                 uint8_t* scale, int64_t rows, int64_t cols, float bound_w, float bound_b, uint8_t* bound_scale,
                                 p2t_stream stream) {
    P2T_REQUIRE(x && w && b && q && scale && rows >= 0 && cols > 0 && bound_w >= 0.f && bound_b >= 0.f, "p2t_layernorm_fp8: bad arguments");
    return launch_layernorm_fp8(x, ld_x, w, b, eps, q, ld_q, scale, rows, cols, bound_w, bound_b, bound_scale, (hipStream_t)stream);
}
extern "C" int p2t_rmsnorm_fp8(const float* x, int64_t ld_x, const float* w, float eps, void* q, int64_t ld_q, uint8_t* scale,
                               int64_t rows, int64_t cols, p2t_stream stream) {
    P2T_REQUIRE(x && w && q && scale && rows >= 0 && cols > 0, "p2t_rmsnorm_fp8: bad arguments");
    return launch_rmsnorm_fp8(x, ld_x, w, eps, q, ld_q, scale, rows, cols, (hipStream_t)stream);
}

extern "C" int p2t_rmsnorm_backward(const float* x, int64_t ld_x, const float* w, float eps, const void* dy, int64_t ld_dy, int dy_dtype, float* dx,
                                    int64_t ld_dx, int64_t rows, int64_t cols, int accumulate, p2t_stream stream) {
    P2T_REQUIRE(x && w && dy && dx && rows >= 0 && cols > 0, "p2t_rmsnorm_backward: bad arguments");
    if (rows == 0) return P2T_OK;
    return launch_rmsnorm_bwd(x, ld_x, w, eps, dy, ld_dy, dy_dtype, dx, ld_dx, rows, cols, accumulate, (hipStream_t)stream);
}
extern "C" int p2t_layernorm_backward(const float* x, int64_t ld_x, const float* w, float eps, const void* dy, int64_t ld_dy, int dy_dtype,
                                      float* dx, int64_t ld_dx, int64_t rows, int64_t cols, int accumulate, p2t_stream stream) {
    P2T_REQUIRE(x && w && dy && dx && rows >= 0 && cols > 0, "p2t_layernorm_backward: bad arguments");
    P2T_REQUIRE(cols % 4 == 0 && ld_x % 4 == 0 && ld_dy % 4 == 0 && ld_dx % 4 == 0 && ld_x >= cols && ld_dy >= cols && ld_dx >= cols,
                "p2t_layernorm_backward: cols / strides must be multiples of 4 and cover cols");
    P2T_REQUIRE(dy_dtype == P2T_F32 || dy_dtype == P2T_BF16, "p2t_layernorm_backward: unsupported dy dtype %d", dy_dtype);
    if (rows == 0) return P2T_OK;
    return launch_layernorm_bwd(x, ld_x, w, eps, dy, ld_dy, dy_dtype, dx, ld_dx, rows, cols, accumulate, (hipStream_t)stream);
}

extern "C" int p2t_l2norm_rows(const float* x, float* y, float* inv_norm, int64_t rows, int64_t cols, float eps,
                               p2t_stream stream) {
    P2T_REQUIRE(x && y && cols > 0, "p2t_l2norm_rows: bad arguments");
    return launch_l2norm(x, P2T_F32, cols, y, P2T_F32, cols, inv_norm, rows, cols, eps, (hipStream_t)stream);
}
extern "C" int p2t_l2norm_rows_backward(const float* x, const float* dy, float* dx, int64_t rows, int64_t cols,
                                        float eps, p2t_stream stream) {
    P2T_REQUIRE(x && dy && dx && cols > 0 && cols % 4 == 0, "p2t_l2norm_rows_backward: bad arguments");
    if (rows == 0) return P2T_OK;
    l2norm_bwd_kernel<<<dim3((unsigned)ceil_div(rows, 4)), 256, 0, (hipStream_t)stream>>>(x, dy, dx, rows, (int)cols, eps);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
