// Decoder half of Esm2LlamaInstructForCausalLM.forward (reference
// models/modeling_esm2llama_instruct.py:108-139, 195-215 and HF LlamaForCausalLM's shifted cross-entropy):
//   * positions_where      -- flat positions of the selected elements of an int64 array, in order (the row-major order
//                             torch's boolean-mask indexing uses), plus their count;
//   * scatter_rows         -- inputs_embeds[placeholder_mask] = encoder_hidden_states[encoder_mask];
//   * gather_rows_f32      -- its backward (the two position lists swap roles).
// The shifted cross-entropy of the same forward is in lm_loss.hip.
#include "common.h"
#include "kernels.h"

namespace p2t {

// One block of 1024 threads scans the whole array: thread i owns a contiguous segment, counts its hits, the counts are
// exclusive-scanned through LDS, then each thread walks its segment again and writes the positions.  n is B*T (<= a few
// hundred thousand), so one block is microseconds; the order of `pos` is the order of the array.
__global__ void __launch_bounds__(1024) positions_where_kernel(const int64_t* __restrict__ v, int64_t n, int mode, int64_t match,
                                                               int32_t* __restrict__ pos, int32_t* __restrict__ count) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int64_t seg = (n + 1023) / 1024, lo = tid * seg, hi = lo + seg < n ? lo + seg : n;
    int c = 0;
    for (int64_t i = lo; i < hi; ++i) c += mode == 0 ? (v[i] == match) : (v[i] != 0);
    part[tid] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {          // Hillis-Steele inclusive scan
        const int add = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int r = part[tid] - c;
    for (int64_t i = lo; i < hi; ++i)
        if (mode == 0 ? (v[i] == match) : (v[i] != 0)) pos[r++] = (int32_t)i;
    if (tid == 1023) *count = part[1023];
}

template <typename Tsrc>
__global__ void __launch_bounds__(256) scatter_rows_kernel(float* __restrict__ dst, int64_t ld_dst, const int32_t* __restrict__ dst_pos,
                                                           const Tsrc* __restrict__ src, int64_t ld_src,
                                                           const int32_t* __restrict__ src_pos, const int32_t* __restrict__ n_dst,
                                                           const int32_t* __restrict__ n_src, int H) {
    const int rows = min(*n_dst, *n_src);
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        float* d = dst + (int64_t)dst_pos[r] * ld_dst;
        const Tsrc* s = src + (int64_t)src_pos[r] * ld_src;
        for (int c = threadIdx.x; c < H; c += 256) d[c] = to_f32(s[c]);
    }
}

// dst[dst_pos[r], :H] = src[src_pos[r], :H] for r < min(*n_dst, *n_src), f32 -> f32: the backward of p2t_scatter_rows'
// boolean-mask assignment with the roles of the two position lists swapped (rows of dst not listed stay as they are).
__global__ void __launch_bounds__(256) gather_rows_f32_kernel(float* __restrict__ dst, int64_t ld_dst, const int32_t* __restrict__ dst_pos,
                                                              const float* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ src_pos,
                                                              const int32_t* __restrict__ n_dst, const int32_t* __restrict__ n_src, int H) {
    const int n = min(n_dst[0], n_src[0]);
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        float* d = dst + (int64_t)dst_pos[r] * ld_dst;
        const float* s = src + (int64_t)src_pos[r] * ld_src;
        for (int c = threadIdx.x; c < H; c += 256) d[c] = s[c];
    }
}

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_positions_where(const int64_t* values, int64_t n, int mode, int64_t match, int32_t* pos, int32_t* count,
                                   p2t_stream stream) {
    P2T_REQUIRE(values && pos && count && n > 0 && n < (1ll << 31) && (mode == 0 || mode == 1), "p2t_positions_where: bad arguments");
    positions_where_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(values, n, mode, match, pos, count);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_scatter_rows(float* dst, int64_t ld_dst, const int32_t* dst_pos, const void* src, int64_t ld_src, int src_dtype,
                                const int32_t* src_pos, const int32_t* n_dst, const int32_t* n_src, int64_t max_rows, int H,
                                p2t_stream stream) {
    P2T_REQUIRE(dst && dst_pos && src && src_pos && n_dst && n_src && max_rows > 0 && H > 0 && ld_dst >= H && ld_src >= H,
                "p2t_scatter_rows: bad arguments");
    P2T_REQUIRE(src_dtype == P2T_F32 || src_dtype == P2T_BF16, "p2t_scatter_rows: unsupported dtype %d", src_dtype);
    const unsigned grid = (unsigned)(max_rows < 4096 ? max_rows : 4096);
    if (src_dtype == P2T_BF16)
        scatter_rows_kernel<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>(dst, ld_dst, dst_pos, (const bf16_t*)src, ld_src, src_pos,
                                                                          n_dst, n_src, H);
    else
        scatter_rows_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>(dst, ld_dst, dst_pos, (const float*)src, ld_src, src_pos,
                                                                         n_dst, n_src, H);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_gather_rows_f32(float* dst, int64_t ld_dst, const int32_t* dst_pos, const float* src, int64_t ld_src, const int32_t* src_pos,
                                   const int32_t* n_dst, const int32_t* n_src, int64_t max_rows, int H, p2t_stream stream) {
    P2T_REQUIRE(dst && dst_pos && src && src_pos && n_dst && n_src && max_rows > 0 && H > 0 && ld_dst >= H && ld_src >= H, "p2t_gather_rows_f32: bad arguments");
    const unsigned grid = (unsigned)(max_rows < 4096 ? max_rows : 4096);
    gather_rows_f32_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(dst, ld_dst, dst_pos, src, ld_src, src_pos, n_dst, n_src, H);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
