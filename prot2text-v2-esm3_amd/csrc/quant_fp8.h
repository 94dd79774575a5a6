// Device helpers of the row-scaled e4m3 scheme (the scheme itself is described in quant.hip), shared by
// the quantise kernels (quant.hip) and the norms that write fp8 directly (norm.hip).
#pragma once
#include "common.h"

namespace p2t {

// biased E8M0 exponent of the row scale from the row's absolute maximum (bit-exact integer rule, mirrored in numpy):
// amax = (1 + f) 2^ea;  amax / 448 = (1 + f) / 1.75 * 2^(ea - 8)  ->  e = ea - 8 + (f > 0.75)
__device__ __forceinline__ int e8m0_of_amax(float amax) {
    const unsigned u = __float_as_uint(amax);
    const int ea = (int)((u >> 23) & 0xFF) - 127;
    const int e = ea - 8 + ((u & 0x7FFFFF) > 0x600000 ? 1 : 0);
    const int E = e + 127;
    return amax > 0.f ? (E < 1 ? 1 : (E > 254 ? 254 : E)) : 127;
}
__device__ __forceinline__ float pow2_neg(int E) {            // 2^-(E - 127), exact
    return __uint_as_float((unsigned)(254 - E) << 23);
}
__device__ __forceinline__ unsigned pack_fp8x4(float a, float b, float c, float d) {
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
    return (unsigned)r;
}
__device__ __forceinline__ float block_max4(float v, float* red) {            // 4 waves; every thread gets the maximum
    v = wave_max(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

}  // namespace p2t
