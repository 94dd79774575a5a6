// The row bodies of the forward norm kernels (norm.hip), written once for the form that stores its output and the form
// that quantises it to e4m3: the load of a row into registers, its statistics, and the normalisation of one 4-element chunk.
// The numpy oracle mirrors this arithmetic (order of the sums included) once.
#pragma once
#include "common.h"

namespace p2t {

// ---- one WAVE per row: lane l holds columns (i * 64 + l) * 4 .. + 3 of chunk i; NV chunks cover cols <= NV * 256 ----
// Loads the row into v (zeros beyond cols) and returns its statistics: rstd, and for LayerNorm the mean (0 for RMSNorm).
template <int NV, bool RMS>
__device__ __forceinline__ void wave_row_stats(const float* xr, int cols, int lane, float eps, float (&v)[NV][4], float& mean,
                                               float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        // the fp32 stream is not read again before hundreds of MB of GEMM traffic: a non-temporal load keeps its 168 MB
        // from evicting the next GEMM's operand panels out of the L2s (+0.3 % step, same-box A/B)
        typedef float f4nt __attribute__((ext_vector_type(4)));
        f4nt t = {0.f, 0.f, 0.f, 0.f};           // (only t depends on the branch: with v assigned on both sides NV = 8 took 182 VGPRs)
        if (c < cols) t = __builtin_nontemporal_load(reinterpret_cast<const f4nt*>(xr + c));
        v[i][0] = t[0]; v[i][1] = t[1]; v[i][2] = t[2]; v[i][3] = t[3];
        s += RMS ? (v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3])
                 : (v[i][0] + v[i][1] + v[i][2] + v[i][3]);
    }
    s = wave_sum(s);
    mean = 0.f;
    if (RMS) {
        rstd = rsqrtf(s / (float)cols + eps);
    } else {
        mean = s / (float)cols;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < cols) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = v[i][j] - mean;
                    q += d * d;
                }
            }
        }
        q = wave_sum(q);
        rstd = rsqrtf(q / (float)cols + eps);
    }
}

// o = the normalised chunk at columns c .. c + 3 (o may be v itself)
template <bool RMS>
__device__ __forceinline__ void norm_chunk(const float (&v)[4], float mean, float rstd, const float* w, const float* b,
                                           int c, float (&o)[4]) {
    float wv[4];
    load4(w + c, wv);
    if (RMS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = wv[j] * (v[j] * rstd);
    } else {
        float bv[4];
        load4(b + c, bv);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (v[j] - mean) * rstd * wv[j] + bv[j];
    }
}

// ---- one BLOCK of 256 threads per row (RMSNorm of a few rows): thread t holds columns (i * 256 + t) * 4 .. + 3 of chunk i ----
// The row's and the weight's 16-byte pieces are all requested before anything is waited for; returns rstd (red: 4 floats of LDS).
template <int NV>
__device__ __forceinline__ float block_row_rstd(const float* xr, const float* w, int cols, float eps, float* red,
                                                float (&v)[NV][4], float (&wv)[NV][4]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 256 + threadIdx.x) * 4;
        if (c < cols) { load4(xr + c, v[i]); load4(w + c, wv[i]); }
        else { v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f; wv[i][0] = wv[i][1] = wv[i][2] = wv[i][3] = 0.f; }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) s += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    return rsqrtf(block_sum<4>(s, red) / (float)cols + eps);
}

}  // namespace p2t
