// Optimizer tail of the contrastive step: clip_grad_norm_ + AdamW on the adapter parameters
// (scripts/train_contrast.py:453-465, AdamW(lr=2e-4, eps=1e-6, betas=(0.9,0.999), wd=0.01) :621-626).
// Two launches per tensor, no host sync and no atomics: (1) 256 per-block partial sums of g^2,
// (2) the update kernel, where every block re-adds all partials in a fixed order (deterministic
// total norm), derives the clip coefficient on the device and applies torch's AdamW update.
// The update also refreshes the `shadow` copy (bf16 / GEMM row stride) the next forward reads.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace p2t {

constexpr int kNormBlocks = 256;

__global__ void __launch_bounds__(256) sumsq_partial_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    const int64_t stride = (int64_t)gridDim.x * 256 * 4;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 3 < n) {
            float v[4];
            load4(g + i, v);
            s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) s += g[i + j] * g[i + j];
        }
    }
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template <typename TS>
__global__ void __launch_bounds__(256) adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, TS* __restrict__ shadow, int64_t cols,
                                                    int64_t shadow_ld, const float* __restrict__ partial, int n_partial,
                                                    float decay, float omb1, float beta2, float omb2, float eps, float step,
                                                    float bc2_sqrt, float max_norm, float* __restrict__ grad_norm_out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n_partial; i += 256) s += partial[i];
    s = block_sum<4>(s, red);
    const float total = sqrtf(s);
    if (blockIdx.x == 0 && threadIdx.x == 0 && grad_norm_out) grad_norm_out[0] = total;
    // torch.nn.utils.clip_grad_norm_: coef = max_norm / (total + 1e-6), clamped to 1
    const float coef = fminf(max_norm / (total + 1e-6f), 1.0f);
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float gi = g[i] * coef;
        float pi = p[i] * decay;                                          // param.mul_(1 - lr * wd)
        const float mi = m[i] + (gi - m[i]) * omb1;                       // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = v[i] * beta2 + omb2 * gi * gi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pi -= step * (mi / denom);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (shadow) shadow[(i / cols) * shadow_ld + (i % cols)] = from_f32<TS>(pi);
    }
}

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_clip_adamw_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                                   float* const* exp_avg_sq, const int64_t* numel, void* const* shadow, const int64_t* cols,
                                   const int64_t* shadow_ld, int shadow_dtype, int step, double lr, double beta1, double beta2,
                                   double eps, double weight_decay, double max_norm, float* grad_norm_out, float* scratch,
                                   p2t_stream stream) {
    P2T_REQUIRE(n_tensors > 0 && n_tensors <= 64 && params && grads && exp_avg && exp_avg_sq && numel && scratch && step >= 1,
                "p2t_clip_adamw_step: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    for (int t = 0; t < n_tensors; ++t) {
        sumsq_partial_kernel<<<kNormBlocks, 256, 0, s>>>(grads[t], numel[t], scratch + (int64_t)t * kNormBlocks);
        P2T_LAUNCH_CHECK();
    }
    // scalar prep in double, as torch.optim.AdamW does in Python
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float decay = (float)(1.0 - lr * weight_decay), omb1 = (float)(1.0 - beta1), b2 = (float)beta2;
    const float omb2 = (float)(1.0 - beta2), epsf = (float)eps, stepsz = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float mn = (max_norm > 0.0 && max_norm < 1e30) ? (float)max_norm : INFINITY;
    for (int t = 0; t < n_tensors; ++t) {
        const int64_t n = numel[t];
        int grid = (int)ceil_div(n, 256 * 8);
        grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
        void* sh = shadow ? shadow[t] : nullptr;
        const int64_t c = (sh && cols) ? cols[t] : 1, ld = (sh && shadow_ld) ? shadow_ld[t] : 1;
        float* gn = t == 0 ? grad_norm_out : nullptr;
        if (sh && shadow_dtype == P2T_BF16)
            adamw_kernel<bf16_t><<<grid, 256, 0, s>>>(params[t], grads[t], exp_avg[t], exp_avg_sq[t], n, (bf16_t*)sh, c, ld, scratch,
                                                      n_tensors * kNormBlocks, decay, omb1, b2, omb2, epsf, stepsz, bc2_sqrt, mn, gn);
        else
            adamw_kernel<float><<<grid, 256, 0, s>>>(params[t], grads[t], exp_avg[t], exp_avg_sq[t], n, (float*)sh, c, ld, scratch,
                                                     n_tensors * kNormBlocks, decay, omb1, b2, omb2, epsf, stepsz, bc2_sqrt, mn, gn);
        P2T_LAUNCH_CHECK();
    }
    return P2T_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Flat form (stage 2: 448 LoRA matrices + the adapter in ONE buffer): parameters, gradients and both moments are single f32
// vectors; a host-built segment table says where each trained tensor lives (offsets multiples of 16 elements) and where its
// GEMM-layout shadow goes, a host-built chunk table cuts the segments into pieces of at most kFlatChunk elements.  Two launches
// whatever the number of tensors: (1) kFlatNormBlocks partial sums of g^2 over the whole flat gradient (padding between segments
// is zero), (2) one block per chunk: the partials re-added in a fixed order (bit-identical norm from run to run, no atomics),
// clip coefficient, torch's AdamW, shadow = RNE(scale * p).  HBM-bound: 16 B read + 12 B written per element + the shadow.
namespace p2t {

constexpr int kFlatNormBlocks = P2T_FLAT_NORM_BLOCKS;
constexpr int kFlatUnroll = 4;                                    // float4 per thread per array in flight
constexpr int kFlatChunk = 256 * 4 * kFlatUnroll;
static_assert(kFlatChunk == P2T_FLAT_CHUNK, "chunk size of the header");

__global__ void __launch_bounds__(256) flat_sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partial) {
    __shared__ float red[4];
    float s[kFlatUnroll] = {};
    const int64_t stride = (int64_t)kFlatNormBlocks * 256 * 4;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride * kFlatUnroll) {
        float v[kFlatUnroll][4];
#pragma unroll
        for (int u = 0; u < kFlatUnroll; ++u) {
            if (i + u * stride < n) load4(g + i + u * stride, v[u]);
            else v[u][0] = v[u][1] = v[u][2] = v[u][3] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < kFlatUnroll; ++u) s[u] += v[u][0] * v[u][0] + v[u][1] * v[u][1] + v[u][2] * v[u][2] + v[u][3] * v[u][3];
    }
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < kFlatUnroll; ++u) t += s[u];
    t = block_sum<4>(t, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// j / c and j % c in 32 bits when both fit (the common case), 64-bit otherwise
__device__ __forceinline__ void divmod64(int64_t j, int64_t c, int64_t& q, int64_t& r) {
    if (((uint64_t)j | (uint64_t)c) >> 32 == 0) {
        const uint32_t qq = (uint32_t)j / (uint32_t)c;
        q = qq; r = (uint32_t)j - qq * (uint32_t)c;
    } else {
        q = j / c; r = j - q * c;
    }
}

template <typename TS>
__device__ __forceinline__ void flat_shadow(const p2t_flat_segment& sg, int64_t j, const float (&pv)[4], int cnt, bool vec) {
    TS* sh = (TS*)sg.shadow;
    if (vec && cnt == 4) {                                        // 4 elements of one row: cols % 4 == 0, j % 4 == 0
        int64_t r, c;
        divmod64(j, sg.cols, r, c);
        const float o[4] = {sg.scale * pv[0], sg.scale * pv[1], sg.scale * pv[2], sg.scale * pv[3]};
        store4(sh + r * sg.ld + c, o);
        return;
    }
    for (int q = 0; q < cnt; ++q) {
        int64_t r, c;
        divmod64(j + q, sg.cols, r, c);
        sh[r * sg.ld + c] = from_f32<TS>(sg.scale * pv[q]);
    }
}

__global__ void __launch_bounds__(256) flat_adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, const p2t_flat_segment* __restrict__ segs,
                                                         const p2t_flat_chunk* __restrict__ chunks, const float* __restrict__ partial,
                                                         float decay, float omb1, float beta2, float omb2, float eps, float step,
                                                         float bc2_sqrt, float max_norm, float* __restrict__ grad_norm_out) {
    __shared__ float red[4];
    const p2t_flat_chunk ch = chunks[blockIdx.x];
    const p2t_flat_segment sg = segs[ch.segment];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kFlatNormBlocks / 256; ++k) s += partial[k * 256 + threadIdx.x];
    s = block_sum<4>(s, red);
    const float total = sqrtf(s);
    if (blockIdx.x == 0 && threadIdx.x == 0 && grad_norm_out) grad_norm_out[0] = total;
    const float coef = fminf(max_norm / (total + 1e-6f), 1.0f);   // torch.nn.utils.clip_grad_norm_
    const int esz = sg.shadow_dtype == P2T_BF16 ? 2 : 4;
    const bool vec = sg.shadow && sg.cols % 4 == 0 && sg.ld % 4 == 0 && ((uintptr_t)sg.shadow % (4 * esz)) == 0;
    const int64_t base = ch.start;                                // flat index; ch.start - sg.offset is the index in the tensor
    float pv[kFlatUnroll][4], gv[kFlatUnroll][4], mv[kFlatUnroll][4], vv[kFlatUnroll][4];
    // every float4 lies inside [offset, round_up(offset + numel, 16)): loads need no mask (padding reads as 0), stores do
#pragma unroll
    for (int u = 0; u < kFlatUnroll; ++u) {
        const int idx = (u * 256 + threadIdx.x) * 4;
        if (idx < ch.count) {
            load4(p + base + idx, pv[u]); load4(g + base + idx, gv[u]); load4(m + base + idx, mv[u]); load4(v + base + idx, vv[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < kFlatUnroll; ++u) {
        const int idx = (u * 256 + threadIdx.x) * 4;
        if (idx >= ch.count) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float gi = gv[u][q] * coef;
            float pi = pv[u][q] * decay;                                  // param.mul_(1 - lr * wd)
            const float mi = mv[u][q] + (gi - mv[u][q]) * omb1;           // exp_avg.lerp_(grad, 1 - beta1)
            const float vi = vv[u][q] * beta2 + omb2 * gi * gi;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
            const float denom = sqrtf(vi) / bc2_sqrt + eps;
            pi -= step * (mi / denom);
            pv[u][q] = pi; mv[u][q] = mi; vv[u][q] = vi;
        }
        const int cnt = ch.count - idx < 4 ? ch.count - idx : 4;
        if (cnt == 4) {
            store4(p + base + idx, pv[u]); store4(m + base + idx, mv[u]); store4(v + base + idx, vv[u]);
        } else {
            for (int q = 0; q < cnt; ++q) { p[base + idx + q] = pv[u][q]; m[base + idx + q] = mv[u][q]; v[base + idx + q] = vv[u][q]; }
        }
        if (sg.shadow) {
            const int64_t j = base - sg.offset + idx;
            if (sg.shadow_dtype == P2T_BF16) flat_shadow<bf16_t>(sg, j, pv[u], cnt, vec);
            else flat_shadow<float>(sg, j, pv[u], cnt, vec);
        }
    }
}

}  // namespace p2t

extern "C" int p2t_clip_adamw_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                   const p2t_flat_segment* segments, const p2t_flat_chunk* chunks, int64_t n_chunks, int step,
                                   double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                   float* grad_norm_out, float* scratch, p2t_stream stream) {
    P2T_REQUIRE(params && grads && exp_avg && exp_avg_sq && segments && chunks && scratch, "p2t_clip_adamw_flat: null pointer");
    P2T_REQUIRE(n > 0 && n % 16 == 0 && n_chunks > 0 && n_chunks <= 0x7FFFFFFF && step >= 1,
                "p2t_clip_adamw_flat: bad sizes (n %% 16 == 0, 0 < n_chunks < 2^31, step >= 1)");
    P2T_REQUIRE(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
                "p2t_clip_adamw_flat: flat buffers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    flat_sumsq_kernel<<<kFlatNormBlocks, 256, 0, s>>>(grads, n, scratch);
    P2T_LAUNCH_CHECK();
    // scalar prep in double, as torch.optim.AdamW does in Python
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float decay = (float)(1.0 - lr * weight_decay), omb1 = (float)(1.0 - beta1), b2 = (float)beta2;
    const float omb2 = (float)(1.0 - beta2), epsf = (float)eps, stepsz = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float mn = (max_norm > 0.0 && max_norm < 1e30) ? (float)max_norm : INFINITY;
    flat_adamw_kernel<<<(unsigned)n_chunks, 256, 0, s>>>(params, grads, exp_avg, exp_avg_sq, segments, chunks, scratch, decay, omb1, b2,
                                                         omb2, epsf, stepsz, bc2_sqrt, mn, grad_norm_out);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
