// Stage-2 step through the ESM2 encoder with LoRA branches (scripts/train_instruct.py:155-183 with ESM2 module names; the reference
// runs the encoder under autograd, models/modeling_esm2llama_instruct.py:174-193).  p2t_hip/encoder_train.py drives the encoder
// layer by layer through the C ABI; the pieces the decoder's per-layer step does not already have live here:
//   p2t_esm2_embed          the token-dropout-scaled embedding rows of p2t_esm2_forward, f32 (the frozen start of the tape)
//   p2t_layernorm_backward  dX of torch.nn.LayerNorm with frozen weight / bias (per-layer norms and emb_layer_norm_after)
//   p2t_gelu_rows           gelu_erf of a pre-activation Z that a LoRA branch was added to (the fused P2T_EPI_GELU cannot see
//                           the branch), and its backward dZ = dY * gelu_erf'(Z)
#include "common.h"
#include "kernels.h"

namespace p2t {

// y = (x - mu) r w + b, r = rsqrt(var + eps)  ->  g (+)= r (w dy - mean(w dy) - xhat mean(w dy xhat)), xhat = (x - mu) r.
// One wave per row (four rows per block); the mean pass, the statistics pass and the write pass re-read the row (L2 resident).
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

// out[m, c] = gelu_erf(z[m, c])                 (dy == nullptr)
//           = dy[m, c] * gelu_erf'(z[m, c])     (backward)
// for c < N; columns N .. n_out - 1 are written as zeros (the K padding of the consumer GEMM).
template <typename Tz, typename Td, typename To>
__global__ void __launch_bounds__(256) gelu_rows_kernel(const Tz* __restrict__ z, int64_t ld_z, const Td* __restrict__ dy, int64_t ld_dy,
                                                        To* __restrict__ out, int64_t ld_out, int64_t M, int N, int n_out) {
    const int64_t n = M * (int64_t)n_out, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t m = i / n_out;
        const int c = (int)(i - m * n_out);
        float v = 0.f;
        if (c < N) {
            const float zv = to_f32(z[m * ld_z + c]);
            v = dy ? to_f32(dy[m * ld_dy + c]) * gelu_erf_grad(zv) : gelu_erf_for<To>(zv);
        }
        out[m * ld_out + c] = from_f32<To>(v);
    }
}

template <typename Tz, typename Td, typename To>
static void launch_gelu_rows_t(const void* z, int64_t ld_z, const void* dy, int64_t ld_dy, void* out, int64_t ld_out, int64_t M, int N, int n_out,
                               hipStream_t s) {
    const int64_t n = M * (int64_t)n_out;
    const unsigned grid = (unsigned)(ceil_div(n, 256) < 8192 ? ceil_div(n, 256) : 8192);
    gelu_rows_kernel<Tz, Td, To><<<grid, 256, 0, s>>>((const Tz*)z, ld_z, (const Td*)dy, ld_dy, (To*)out, ld_out, M, N, n_out);
}

}  // namespace p2t

using namespace p2t;

extern "C" int p2t_esm2_embed(const int64_t* ids, const int64_t* mask, const void* table, int dtype, const float* emb_scale, int B, int T, int H,
                              int vocab, int mask_id, int token_dropout, float* x, p2t_stream stream) {
    P2T_REQUIRE(ids && mask && table && emb_scale && x && B > 0 && T > 0 && H > 0 && H % 4 == 0 && vocab > 0,
                "p2t_esm2_embed: bad arguments (hidden must be a multiple of 4)");
    P2T_REQUIRE(dtype == P2T_F32 || dtype == P2T_BF16, "p2t_esm2_embed: unsupported dtype %d", dtype);
    return launch_esm_embed(ids, mask, table, dtype, emb_scale, T, H, vocab, mask_id, token_dropout, x, (int64_t)B * T, (hipStream_t)stream);
}

extern "C" int p2t_layernorm_backward(const float* x, int64_t ld_x, const float* w, float eps, const void* dy, int64_t ld_dy, int dy_dtype,
                                      float* dx, int64_t ld_dx, int64_t rows, int64_t cols, int accumulate, p2t_stream stream) {
    P2T_REQUIRE(x && w && dy && dx && rows >= 0 && cols > 0, "p2t_layernorm_backward: bad arguments");
    P2T_REQUIRE(cols % 4 == 0 && ld_x % 4 == 0 && ld_dy % 4 == 0 && ld_dx % 4 == 0 && ld_x >= cols && ld_dy >= cols && ld_dx >= cols,
                "p2t_layernorm_backward: cols / strides must be multiples of 4 and cover cols");
    P2T_REQUIRE(dy_dtype == P2T_F32 || dy_dtype == P2T_BF16, "p2t_layernorm_backward: unsupported dy dtype %d", dy_dtype);
    if (rows == 0) return P2T_OK;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(rows, 4));
    if (dy_dtype == P2T_BF16)
        layernorm_bwd_kernel<bf16_t><<<grid, 256, 0, s>>>(x, ld_x, w, eps, (const bf16_t*)dy, ld_dy, dx, ld_dx, rows, (int)cols, accumulate);
    else
        layernorm_bwd_kernel<float><<<grid, 256, 0, s>>>(x, ld_x, w, eps, (const float*)dy, ld_dy, dx, ld_dx, rows, (int)cols, accumulate);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}

extern "C" int p2t_gelu_rows(const void* z, int z_dtype, int64_t ld_z, const void* dy, int dy_dtype, int64_t ld_dy, void* out, int out_dtype,
                             int64_t ld_out, int64_t M, int64_t N, p2t_stream stream) {
    P2T_REQUIRE(z && out && M >= 0 && N > 0 && ld_z >= N && ld_out >= N && (!dy || ld_dy >= N), "p2t_gelu_rows: bad arguments");
    auto ok = [](int t) { return t == P2T_F32 || t == P2T_BF16; };
    P2T_REQUIRE(ok(z_dtype) && ok(out_dtype) && (!dy || ok(dy_dtype)), "p2t_gelu_rows: unsupported dtypes");
    if (M == 0) return P2T_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_out = round_up(N, 64) < ld_out ? round_up(N, 64) : ld_out;
    const int zb = z_dtype == P2T_BF16, ob = out_dtype == P2T_BF16, db = dy && dy_dtype == P2T_BF16;
    const int key = zb * 4 + db * 2 + ob;
#define P2T_GELU(TZ, TD, TO) launch_gelu_rows_t<TZ, TD, TO>(z, ld_z, dy, ld_dy, out, ld_out, M, (int)N, (int)n_out, s)
    switch (key) {
        case 0: P2T_GELU(float, float, float); break;
        case 1: P2T_GELU(float, float, bf16_t); break;
        case 2: P2T_GELU(float, bf16_t, float); break;
        case 3: P2T_GELU(float, bf16_t, bf16_t); break;
        case 4: P2T_GELU(bf16_t, float, float); break;
        case 5: P2T_GELU(bf16_t, float, bf16_t); break;
        case 6: P2T_GELU(bf16_t, bf16_t, float); break;
        default: P2T_GELU(bf16_t, bf16_t, bf16_t); break;
    }
#undef P2T_GELU
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
