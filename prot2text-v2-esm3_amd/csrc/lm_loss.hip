// The LM loss: the shifted cross-entropy of Esm2LlamaInstructForCausalLM.forward (HF LlamaForCausalLM's loss; reference
// models/modeling_esm2llama_instruct.py:195-215), mean over (b, t < T-1, labels[b, t+1] counted) of logsumexp(logits[b, t]) -
// logits[b, t, label], forward and backward, in its two forms.  Both live here because they share the rule for which label counts.
//
// Over the full logits [B*T, ld] (p2t_cross_entropy_shifted*, the default stage-2 step):
//   * ce_rows / ce_reduce -- one block per row: row loss and validity, then the token mean, or the sum weighted per target;
//   * ce_bwd_rows         -- (softmax - onehot) / count, or * weights[b, t+1], into d_logits.
// Over the rows that carry a target only (reference scripts/train_instruct.py:192-213
// reads `.loss` alone, never the logits):
//   * lm_target_rows      -- the flat rows (b, t) whose labels[b, t+1] is counted, their labels and their number, on the device;
//   * lm_loss_grad_rows   -- one chunk of logits [R, ld] in place: row loss = logsumexp - target logit, then the row overwritten
//                            by its own gradient (softmax - onehot) * s_r, Liger-style, so no second [R, ld] buffer ever exists;
//   * lm_loss_reduce      -- the row losses summed in a fixed order into the token mean / the weighted sum.
// A row of Llama's vocabulary is 128 256 elements = 256 KB in bf16, four times a CU's LDS: it is NOT staged.  Pass 1 streams it
// once with 16-byte loads keeping a running (max, sum) per thread (online softmax: one read instead of two), pass 2 streams it
// again -- the row was just read by the same workgroup, so it comes from L2 (4 MB per XCD holds 16 such rows, more than the
// workgroups an XCD runs at once) -- and stores 16 bytes per lane.  Vector stores only, no atomics; every reduction has a fixed
// order, so the same input gives the same bits.
#include "common.h"
#include "kernels.h"

namespace p2t {

// the counted label of flat row (b, t): labels[b, t+1] where t + 1 < T, it is not ignore_index and it is an id of the vocabulary;
// -1 without one
__device__ __forceinline__ int64_t counted_label(const int64_t* __restrict__ labels, int64_t row, int T_len, int V, int64_t ignore_index) {
    if ((int)(row % T_len) + 1 >= T_len) return -1;
    const int64_t label = labels[row + 1];
    return (label == ignore_index || label < 0 || label >= V) ? -1 : label;
}

// m = max of the row's V logits, s = sum of exp(x - m): two passes, one block of 256 threads (red: 4 floats of LDS)
template <typename T>
__device__ __forceinline__ void row_max_sumexp(const T* __restrict__ x, int V, float* red, float& m, float& s) {
    m = -INFINITY;
    for (int c = threadIdx.x; c < V; c += 256) m = fmaxf(m, to_f32(x[c]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    s = 0.f;
    for (int c = threadIdx.x; c < V; c += 256) s += expf(to_f32(x[c]) - m);
    s = block_sum<4>(s, red);
}

template <typename T>
__global__ void __launch_bounds__(256) ce_rows_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                      int T_len, int V, int64_t ignore_index, float* __restrict__ row_loss,
                                                      int32_t* __restrict__ row_valid) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x;                     // (b, t)
    const int64_t label = counted_label(labels, row, T_len, V, ignore_index);
    if (label < 0) {
        if (threadIdx.x == 0) { row_loss[row] = 0.f; row_valid[row] = 0; }
        return;
    }
    const T* x = logits + row * ld;
    float m, s;
    row_max_sumexp(x, V, red, m, s);
    if (threadIdx.x == 0) {
        row_loss[row] = logf(s) + m - to_f32(x[label]);
        row_valid[row] = 1;
    }
}

// Over the rows with a counted target: loss = mean of row_loss (no such row: 0 / 0 = NaN, as torch's mean over nothing), or with
// weights the sum of weights[row + 1] * row_loss[row] (the weight sits at the target's label position).  A row without a target
// holds row_loss = +0, which changes no bit of the sum, so both forms skip it.
__global__ void __launch_bounds__(1024) ce_reduce_kernel(const float* __restrict__ row_loss, const int32_t* __restrict__ row_valid,
                                                         const float* __restrict__ weights, int64_t M, float* __restrict__ loss,
                                                         int32_t* __restrict__ count) {
    __shared__ float red[16];
    __shared__ float redc[16];
    float s = 0.f, c = 0.f;
    for (int64_t i = threadIdx.x; i < M; i += 1024)
        if (row_valid[i]) {
            if (weights) s += weights[i + 1] * row_loss[i];
            else s += row_loss[i];
            c += 1.f;
        }
    s = block_sum<16>(s, red);
    c = block_sum<16>(c, redc);
    if (threadIdx.x == 0) {
        *loss = weights ? s : s / c;
        if (count) *count = (int32_t)c;
    }
}

// d loss / d logits: row (b, t) with a counted target y: (softmax(logits) - onehot(y)) / count -- or, with per-target weights,
// weights[b, t+1] (softmax - onehot); every other row and the padding columns: 0.  One block per row.
template <typename T>
__global__ void __launch_bounds__(256) ce_bwd_rows_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int seq, int V,
                                                          int64_t ignore_index, const int32_t* __restrict__ count, T* __restrict__ dl, int64_t ld_d,
                                                          int cols_d, const float* __restrict__ weights) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    T* dr = dl + row * ld_d;
    const int64_t label = counted_label(labels, row, seq, V, ignore_index);
    if (label < 0) {
        for (int c = threadIdx.x; c < cols_d; c += 256) dr[c] = from_f32<T>(0.f);
        return;
    }
    const T* x = logits + row * ld;
    float m, sum;
    row_max_sumexp(x, V, red, m, sum);
    const float wr = weights ? weights[row + 1] : 0.f;
    const float inv = weights ? wr / sum : 1.0f / (sum * (float)count[0]), invc = weights ? wr : 1.0f / (float)count[0];
    for (int c = threadIdx.x; c < cols_d; c += 256) {
        float g = 0.f;
        if (c < V) g = expf(to_f32(x[c]) - m) * inv - (c == (int)label ? invc : 0.f);
        dr[c] = from_f32<T>(g);
    }
}

// weights == nullptr: the token mean (the backward divides by count[0]); else the weighted sum
static int launch_ce_shifted(const void* logits, int64_t ld, int dtype, const int64_t* labels, const float* weights, int B, int T, int V,
                             int64_t ignore_index, float* row_loss, int32_t* row_valid, float* loss, int32_t* count, hipStream_t s) {
    const int64_t M = (int64_t)B * T;
    if (dtype == P2T_BF16)
        ce_rows_kernel<bf16_t><<<(unsigned)M, 256, 0, s>>>((const bf16_t*)logits, ld, labels, T, V, ignore_index, row_loss, row_valid);
    else
        ce_rows_kernel<float><<<(unsigned)M, 256, 0, s>>>((const float*)logits, ld, labels, T, V, ignore_index, row_loss, row_valid);
    P2T_LAUNCH_CHECK();
    ce_reduce_kernel<<<1, 1024, 0, s>>>(row_loss, row_valid, weights, M, loss, count);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
static int launch_ce_shifted_bwd(const void* logits, int64_t ld, int dtype, const int64_t* labels, const float* weights, const int32_t* count, int B,
                                 int T, int V, int64_t ignore_index, void* d_logits, int64_t ld_d, hipStream_t s) {
    const int64_t M = (int64_t)B * T;
    const int cols_d = (int)(round_up(V, 64) < ld_d ? round_up(V, 64) : ld_d);          // the K padding of the LM-head dX GEMM is zeroed
    if (dtype == P2T_BF16)
        ce_bwd_rows_kernel<bf16_t><<<(unsigned)M, 256, 0, s>>>((const bf16_t*)logits, ld, labels, T, V, ignore_index, count, (bf16_t*)d_logits, ld_d,
                                                               cols_d, weights);
    else
        ce_bwd_rows_kernel<float><<<(unsigned)M, 256, 0, s>>>((const float*)logits, ld, labels, T, V, ignore_index, count, (float*)d_logits, ld_d,
                                                              cols_d, weights);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

// ---------------------------------------------------------------------------------------------
// The target-rows form.
// One block of 1024 threads, as positions_where_kernel: thread i owns a contiguous segment of the B*T flat rows, counts its hits,
// the counts are scanned through LDS, and a second walk writes rows / targets below `cap`.  count = {n, n > cap}; the entries
// min(n, cap) .. cap of rows / targets are set to -1.
__global__ void __launch_bounds__(1024) lm_target_rows_kernel(const int64_t* __restrict__ labels, int64_t n_rows, int T_len, int V, int64_t ignore_index,
                                                              int cap, int32_t* __restrict__ rows, int32_t* __restrict__ targets,
                                                              int32_t* __restrict__ count) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int64_t seg = (n_rows + 1023) / 1024, lo = tid * seg, hi = lo + seg < n_rows ? lo + seg : n_rows;
    int c = 0;
    for (int64_t i = lo; i < hi; ++i) c += counted_label(labels, i, T_len, V, ignore_index) >= 0;
    part[tid] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {          // Hillis-Steele inclusive scan
        const int add = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int r = part[tid] - c;
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t label = counted_label(labels, i, T_len, V, ignore_index);
        if (label < 0) continue;
        if (r < cap) { rows[r] = (int32_t)i; targets[r] = (int32_t)label; }
        ++r;
    }
    const int n = part[1023];
    for (int j = (n < cap ? n : cap) + tid; j < cap; j += 1024) { rows[j] = -1; targets[j] = -1; }
    if (tid == 0) { count[0] = n; count[1] = n > cap; }
}

template <typename T> struct RowVec;
template <> struct RowVec<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) { load4(p, v); }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { store4(p, v); }
};
template <> struct RowVec<bf16_t> {
    static constexpr int N = 8;
    static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[8]) { load8(p, v); }
    static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[8]) {
        *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    }
};

// One workgroup of 256 threads per row r of the chunk; the chunk's row r is entry first + r of rows / targets / row_loss.
// ld is a multiple of 64 elements and x is 16-byte aligned (checked by the entry point), so every 16-byte vector lies inside the row.
template <typename T>
__global__ void __launch_bounds__(256) lm_loss_grad_rows_kernel(T* x_all, int64_t ld, int V, const int32_t* __restrict__ rows,
                                                                const int32_t* __restrict__ targets, const int32_t* __restrict__ count, int first,
                                                                const float* __restrict__ weights, int64_t n_weights, float* __restrict__ row_loss,
                                                                int with_grad) {
    constexpr int N = RowVec<T>::N;
    __shared__ float red_m[4];
    __shared__ float red_s[4];
    const int r = first + (int)blockIdx.x;
    T* x = x_all + (int64_t)blockIdx.x * ld;
    const int n = count[0];
    const int target = targets[r];
    const int64_t wrow = (int64_t)rows[r] + 1;          // the weight sits at the target's label position
    const bool live = r < n && target >= 0 && target < V && (!weights || (wrow > 0 && wrow < n_weights));
    const int nvec = (int)(ld / N);
    if (!live) {                                        // wave-uniform: a pad row / a row beyond the count
        if (with_grad) {
            float z[N];
#pragma unroll
            for (int j = 0; j < N; ++j) z[j] = 0.f;
            for (int i = threadIdx.x; i < nvec; i += 256) RowVec<T>::store(x + (int64_t)i * N, z);
        }
        if (threadIdx.x == 0) row_loss[r] = 0.f;
        return;
    }
    // ---- pass 1: running max and sum of exp(x - max) per thread, then merged in a fixed order
    float m = -INFINITY, s = 0.f;
    for (int i = threadIdx.x; i < nvec; i += 256) {
        float v[N];
        RowVec<T>::load(x + (int64_t)i * N, v);
        const int c0 = i * N;
        float vm = -INFINITY;
#pragma unroll
        for (int j = 0; j < N; ++j) vm = fmaxf(vm, c0 + j < V ? v[j] : -INFINITY);       // a select: the pad columns may hold NaN
        if (vm > m) { s *= expf(m - vm); m = vm; }      // (s is 0 while m is -inf: 0 * exp(-inf) = 0)
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) e += c0 + j < V ? expf(v[j] - m) : 0.f;
        if (m > -INFINITY) s += e;
    }
    const float wm = wave_max(m);
    s = wave_sum(m > -INFINITY ? s * expf(m - wm) : 0.f);
    if ((threadIdx.x & 63) == 0) { red_m[threadIdx.x >> 6] = wm; red_s[threadIdx.x >> 6] = s; }
    __syncthreads();
    const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) S += red_m[w] > -INFINITY ? red_s[w] * expf(red_m[w] - M) : 0.f;
    if (threadIdx.x == 0) row_loss[r] = logf(S) + M - to_f32(x[target]);
    if (!with_grad) return;
    __syncthreads();                                    // x[target] is read above before any lane overwrites it
    // ---- pass 2: the row becomes its own gradient
    const float s_r = weights ? weights[wrow] : 1.0f / (float)n;
    const float inv = 1.0f / S;
    for (int i = threadIdx.x; i < nvec; i += 256) {
        float v[N], g[N];
        RowVec<T>::load(x + (int64_t)i * N, v);
        const int c0 = i * N;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int c = c0 + j;
            g[j] = c < V ? (expf(v[j] - M) * inv - (c == target ? 1.f : 0.f)) * s_r : 0.f;
        }
        RowVec<T>::store(x + (int64_t)i * N, g);
    }
}

// loss = sum over the listed rows of row_loss (/ n: the token mean, NaN without a target as p2t_cross_entropy_shifted), or of
// weights[row + 1] * row_loss; NaN when the list overflowed its capacity.
__global__ void __launch_bounds__(1024) lm_loss_reduce_kernel(const float* __restrict__ row_loss, const int32_t* __restrict__ rows,
                                                              const int32_t* __restrict__ count, int cap, const float* __restrict__ weights,
                                                              int64_t n_weights, float* __restrict__ loss) {
    __shared__ float red[16];
    const int n = count[0], m = n < cap ? n : cap;
    float s = 0.f;
    for (int i = threadIdx.x; i < m; i += 1024) {
        if (weights) {
            const int64_t wrow = (int64_t)rows[i] + 1;
            s += (wrow > 0 && wrow < n_weights) ? weights[wrow] * row_loss[i] : 0.f;
        } else {
            s += row_loss[i];
        }
    }
    s = block_sum<16>(s, red);
    if (threadIdx.x == 0) *loss = count[1] ? __builtin_nanf("") : (weights ? s : s / (float)n);
}

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_cross_entropy_shifted(const void* logits, int64_t ld, int dtype, const int64_t* labels, int B, int T, int V,
                                         int64_t ignore_index, float* row_loss, int32_t* row_valid, float* loss, int32_t* count,
                                         p2t_stream stream) {
    P2T_REQUIRE(logits && labels && row_loss && row_valid && loss && B > 0 && T > 0 && V > 0 && ld >= V,
                "p2t_cross_entropy_shifted: bad arguments");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_cross_entropy_shifted: unsupported dtype %d", dtype);
    return launch_ce_shifted(logits, ld, dtype, labels, nullptr, B, T, V, ignore_index, row_loss, row_valid, loss, count, (hipStream_t)stream);
}

extern "C" int p2t_cross_entropy_shifted_weighted(const void* logits, int64_t ld, int dtype, const int64_t* labels, const float* weights, int B, int T,
                                                  int V, int64_t ignore_index, float* row_loss, int32_t* row_valid, float* loss, int32_t* count,
                                                  p2t_stream stream) {
    P2T_REQUIRE(logits && labels && weights && row_loss && row_valid && loss && B > 0 && T > 0 && V > 0 && ld >= V,
                "p2t_cross_entropy_shifted_weighted: bad arguments");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_cross_entropy_shifted_weighted: unsupported dtype %d", dtype);
    return launch_ce_shifted(logits, ld, dtype, labels, weights, B, T, V, ignore_index, row_loss, row_valid, loss, count, (hipStream_t)stream);
}

extern "C" int p2t_cross_entropy_shifted_backward(const void* logits, int64_t ld, int dtype, const int64_t* labels, int B, int T, int V,
                                                  int64_t ignore_index, const int32_t* count, void* d_logits, int64_t ld_d, p2t_stream stream) {
    P2T_REQUIRE(logits && labels && count && d_logits && B > 0 && T > 0 && V > 0 && ld >= V && ld_d >= V, "p2t_cross_entropy_shifted_backward: bad arguments");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_cross_entropy_shifted_backward: unsupported dtype %d", dtype);
    return launch_ce_shifted_bwd(logits, ld, dtype, labels, nullptr, count, B, T, V, ignore_index, d_logits, ld_d, (hipStream_t)stream);
}

extern "C" int p2t_cross_entropy_shifted_weighted_backward(const void* logits, int64_t ld, int dtype, const int64_t* labels, const float* weights,
                                                           int B, int T, int V, int64_t ignore_index, void* d_logits, int64_t ld_d, p2t_stream stream) {
    P2T_REQUIRE(logits && labels && weights && d_logits && B > 0 && T > 0 && V > 0 && ld >= V && ld_d >= V,
                "p2t_cross_entropy_shifted_weighted_backward: bad arguments");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_cross_entropy_shifted_weighted_backward: unsupported dtype %d", dtype);
    return launch_ce_shifted_bwd(logits, ld, dtype, labels, weights, nullptr, B, T, V, ignore_index, d_logits, ld_d, (hipStream_t)stream);
}

extern "C" int p2t_lm_target_rows(const int64_t* labels, int B, int T, int V, int64_t ignore_index, int cap, int32_t* rows, int32_t* targets,
                                  int32_t* count, p2t_stream stream) {
    P2T_REQUIRE(labels && rows && targets && count && B > 0 && T > 0 && V > 0 && cap > 0 && (int64_t)B * T < (1ll << 31),
                "p2t_lm_target_rows: bad arguments");
    lm_target_rows_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(labels, (int64_t)B * T, T, V, ignore_index, cap, rows, targets, count);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_lm_loss_grad_rows(void* logits, int64_t ld, int dtype, int R, int V, const int32_t* rows, const int32_t* targets,
                                     const int32_t* count, int first, int cap, const float* weights, int64_t n_weights, float* row_loss,
                                     int with_grad, p2t_stream stream) {
    P2T_REQUIRE(logits && rows && targets && count && row_loss && R > 0 && V > 0 && first >= 0 && cap > 0 && (int64_t)first + R <= cap,
                "p2t_lm_loss_grad_rows: bad arguments");
    P2T_REQUIRE(ld >= V && ld % 64 == 0 && ld < (1ll << 31) && ((uintptr_t)logits & 15) == 0,
                "p2t_lm_loss_grad_rows: ld = %lld must be a multiple of 64 that holds V = %d, rows 16-byte aligned", (long long)ld, V);
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_lm_loss_grad_rows: unsupported dtype %d", dtype);
    P2T_REQUIRE(!weights || n_weights > 0, "p2t_lm_loss_grad_rows: weights need their element count");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == P2T_BF16)
        lm_loss_grad_rows_kernel<bf16_t><<<(unsigned)R, 256, 0, s>>>((bf16_t*)logits, ld, V, rows, targets, count, first, weights, n_weights, row_loss,
                                                                    with_grad);
    else
        lm_loss_grad_rows_kernel<float><<<(unsigned)R, 256, 0, s>>>((float*)logits, ld, V, rows, targets, count, first, weights, n_weights, row_loss,
                                                                   with_grad);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_lm_loss_reduce(const float* row_loss, const int32_t* rows, const int32_t* count, int cap, const float* weights,
                                  int64_t n_weights, float* loss, p2t_stream stream) {
    P2T_REQUIRE(row_loss && rows && count && loss && cap > 0, "p2t_lm_loss_reduce: bad arguments");
    P2T_REQUIRE(!weights || n_weights > 0, "p2t_lm_loss_reduce: weights need their element count");
    lm_loss_reduce_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(row_loss, rows, count, cap, weights, n_weights, loss);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
