// The greedy selectors' argmax (llama_decode.hip: p2t_greedy_select, p2t_greedy_select_rows; lookup.hip: p2t_lookup_verify_rows): torch.argmax
// semantics over the first V columns of a row -- the lowest index among equal maxima -- in one fixed reduction order.
#pragma once
#include "common.h"

namespace p2t {
namespace {

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

}  // namespace
}  // namespace p2t
