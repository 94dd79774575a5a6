// Row-wise activations between the GEMMs that cannot ride in a GEMM epilogue, forward and backward:
//   swiglu_gu     SwiGLU on the interleaved gate / up pre-activations (the decoder's training forward keeps them for the backward)
//   gelu_rows     gelu_erf of a pre-activation Z that a LoRA branch was added to (the fused P2T_EPI_GELU cannot see the branch), and
//                 its backward dZ = dY * gelu_erf'(Z)
//   dropout_rows  the LoRA branch's input dropout; the mask is regenerated from the seed, never stored
#include "common.h"
#include "epilogue.h"
#include "kernels.h"

namespace p2t {

// ---------------------------------------------------------------------------------------------
// SwiGLU on the interleaved pre-activations the gate/up GEMM writes with a plain store: 64-column block jb of gu holds
// gate[32 jb .. +31] then up[32 jb .. +31] (the row order of gu_w, include/p2t_hip.h p2t_llama_layer).
//   forward : act[m, f] = silu(g) * u
//   backward: d_gu = (d_act * u * sigma(g) (1 + g (1 - sigma(g))),  d_act * silu(g))   in the same interleaved layout
template <typename T, bool BWD>
__global__ void __launch_bounds__(256) swiglu_gu_kernel(const T* __restrict__ gu, int64_t ld_gu, const T* __restrict__ d_act, int64_t ld_da,
                                                        T* __restrict__ out, int64_t ld_out, int64_t M, int F, int Fo) {
    // Fo: columns written per row of `out` in the forward (F rounded up to the next GEMM's K padding: zeros beyond F)
    const int per = (BWD ? F : Fo) / 4;
    const int64_t n4 = M * (int64_t)per, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const int64_t m = i / per;
        const int f = (int)(i - m * per) * 4;
        if (!BWD && f >= F) {
            const float z[4] = {0.f, 0.f, 0.f, 0.f};
            store4(out + m * ld_out + f, z);
            continue;
        }
        const int col = (f >> 5) * 64 + (f & 31);
        float g[4], u[4];
        load4(gu + m * ld_gu + col, g);
        load4(gu + m * ld_gu + col + 32, u);
        if (!BWD) {
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = silu_for<T>(g[j]) * u[j];
            store4(out + m * ld_out + f, a);
        } else {
            float da[4], dg[4], du[4];
            load4(d_act + m * ld_da + f, da);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float sg = 1.0f / (1.0f + expf(-g[j]));
                dg[j] = da[j] * u[j] * (sg * (1.0f + g[j] * (1.0f - sg)));
                du[j] = da[j] * (g[j] * sg);
            }
            store4(out + m * ld_out + col, dg);
            store4(out + m * ld_out + col + 32, du);
        }
    }
}

template <bool BWD>
static int launch_swiglu_gu(const void* gu, int64_t ld_gu, const void* d_act, int64_t ld_da, void* out, int64_t ld_out, int64_t M, int64_t F,
                            int dtype, hipStream_t s) {
    P2T_REQUIRE(F % 32 == 0 && ld_gu % 4 == 0 && ld_out % 4 == 0, "swiglu: F must be a multiple of 32");
    const int64_t Fo = BWD ? F : (round_up(F, 64) < ld_out ? round_up(F, 64) : ld_out);
    const int64_t n4 = M * (Fo / 4);
    const unsigned grid = (unsigned)(ceil_div(n4, 256) < 4096 ? ceil_div(n4, 256) : 4096);
    if (dtype == P2T_BF16)
        swiglu_gu_kernel<bf16_t, BWD><<<grid, 256, 0, s>>>((const bf16_t*)gu, ld_gu, (const bf16_t*)d_act, ld_da, (bf16_t*)out, ld_out, M, (int)F, (int)Fo);
    else
        swiglu_gu_kernel<float, BWD><<<grid, 256, 0, s>>>((const float*)gu, ld_gu, (const float*)d_act, ld_da, (float*)out, ld_out, M, (int)F, (int)Fo);
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
int launch_swiglu_from_gu(const void* gu, int64_t ld_gu, void* act, int64_t ld_act, int64_t M, int64_t F, int dtype, hipStream_t s) {
    return launch_swiglu_gu<false>(gu, ld_gu, nullptr, 0, act, ld_act, M, F, dtype, s);
}
int launch_swiglu_gu_bwd(const void* gu, int64_t ld_gu, const void* d_act, int64_t ld_da, void* d_gu, int64_t ld_dgu, int64_t M, int64_t F, int dtype,
                         hipStream_t s) {
    return launch_swiglu_gu<true>(gu, ld_gu, d_act, ld_da, d_gu, ld_dgu, M, F, dtype, s);
}

// ---------------------------------------------------------------------------------------------
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

extern "C" int p2t_swiglu_gu(const void* gu, int64_t ld_gu, const void* d_act, int64_t ld_da, void* out, int64_t ld_out, int64_t M, int64_t F, int dtype,
                             p2t_stream stream) {
    P2T_REQUIRE(gu && out && M >= 0 && F > 0 && (dtype == P2T_F32 || dtype == P2T_BF16), "p2t_swiglu_gu: bad arguments");
    if (M == 0) return P2T_OK;
    if (d_act) return launch_swiglu_gu<true>(gu, ld_gu, d_act, ld_da, out, ld_out, M, F, dtype, (hipStream_t)stream);
    return launch_swiglu_gu<false>(gu, ld_gu, nullptr, 0, out, ld_out, M, F, dtype, (hipStream_t)stream);
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

// dst (+)= keep(seed, m * K + c) ? src / (1 - p) : 0: the LoRA branch's input dropout (peft lora_dropout, train_instruct.py:158) and,
// with the same seed, its backward (the mask is regenerated, never stored).
template <typename Ts, typename Td>
__global__ void __launch_bounds__(256) dropout_rows_kernel(const Ts* __restrict__ src, int64_t ld_src, Td* __restrict__ dst, int64_t ld_dst, int64_t M,
                                                           int K, float p, float scale, uint64_t seed, int accumulate) {
    const int64_t n = M * (int64_t)K, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t m = i / K;
        const int c = (int)(i - m * K);
        const float x = dropout_value(to_f32(src[m * ld_src + c]), seed, i, p, scale);
        Td* d = dst + m * ld_dst + c;
        *d = from_f32<Td>(accumulate ? to_f32(*d) + x : x);
    }
}

extern "C" int p2t_dropout_rows(const void* src, int src_dtype, int64_t ld_src, void* dst, int dst_dtype, int64_t ld_dst, int64_t M, int64_t K, float p,
                                uint64_t seed, int accumulate, p2t_stream stream) {
    P2T_REQUIRE(src && dst && M >= 0 && K > 0 && ld_src >= K && ld_dst >= K && p >= 0.f && p < 1.f, "p2t_dropout_rows: bad arguments");
    if (M == 0) return P2T_OK;
    const float scale = 1.0f / (1.0f - p);
    const int64_t n = M * K;
    const unsigned grid = (unsigned)(ceil_div(n, 256) < 8192 ? ceil_div(n, 256) : 8192);
    hipStream_t s = (hipStream_t)stream;
#define P2T_DROP(TS, TD) dropout_rows_kernel<TS, TD><<<grid, 256, 0, s>>>((const TS*)src, ld_src, (TD*)dst, ld_dst, M, (int)K, p, scale, seed, accumulate)
    if (src_dtype == P2T_BF16 && dst_dtype == P2T_BF16) P2T_DROP(bf16_t, bf16_t);
    else if (src_dtype == P2T_F32 && dst_dtype == P2T_BF16) P2T_DROP(float, bf16_t);
    else if (src_dtype == P2T_BF16 && dst_dtype == P2T_F32) P2T_DROP(bf16_t, float);
    else if (src_dtype == P2T_F32 && dst_dtype == P2T_F32) P2T_DROP(float, float);
    else { set_error("p2t_dropout_rows: unsupported dtypes %d -> %d", src_dtype, dst_dtype); return P2T_ERR_ARG; }
#undef P2T_DROP
    P2T_LAUNCH_CHECK();
    return P2T_OK;
}
