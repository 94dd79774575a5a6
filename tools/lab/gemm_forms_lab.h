// LAB BUILD ONLY (-DP2T_LAB, `make lab` in csrc/ -> tools/build/libp2t_lab.so): the launch-form zoo of rounds 1-2, kept for
// A/B measurements (tools/microbench.py, tools/ab.sh) and for the fuzz tests that force one kernel form on shapes the default
// policy would give to another (tests/test_gpu_lab_forms.py runs them against this build through P2T_HIP_LIB).  The product
// library (libp2t_hip.so) contains none of this: its p2t_set_gemm_policy accepts 0 and 9 only.
//
// Included in csrc/gemm_mfma.hip after the default launch policy, inside namespace p2t.  A forced form is a rewrite of the
// default plan, made from the same facts and helpers (persist_fits, persist8, persist4, plan_per_tile, ...), never a second copy
// of the default decision.  Forced forms (policy):
//   128 / 256 = tile height of the per-tile kernels; 1 = the eight-wave per-tile kernel at the default height, no split-K;
//   2 = the per-tile part of the default policy without the four-wave forms; 3 = eight-wave persistent kernel with the split-K
//   fix-up whenever possible; 4 = persistent, never the fix-up; 5 = persistent, partial round as 128-row halves; 6 = 64-deep
//   single-barrier skeleton (gemm_fp8.hip's, on bf16 operands); 7 = four-wave kernel, one tile per block; 8 = four-wave
//   persistent kernel with split-K pairs whenever possible; 10 = four-wave persistent, a partial last round as whole tiles;
//   12 = 10 with the other generated instruction order of the K loop (tools/gen_w4_schedule.py, SCHED 0).
// 3 / 4 / 5 / 8 / 10 / 12 on a shape the persistent kernels do not take run as 2; 6 / 7 on an epilogue or shape without that
// form run the default policy with 2's per-tile part; 8 / 10 / 12 on an epilogue without the four-wave form run the eight-wave
// persistent kernel (8: the default tail, 10 / 12: no 128-row halves).  1000 + n: the policy counts n compute units.
#pragma once

static std::atomic<int> g_cu_override{0};
void set_cu_override(int n) { g_cu_override.store(n, std::memory_order_relaxed); }
static int lab_cu_override() { return g_cu_override.load(std::memory_order_relaxed); }

// the epilogue code / output type under which launch_gemm_bf16_k64 (gemm_fp8.hip) takes Epi; -1: it has no such form
extern int launch_gemm_bf16_k64(const void*, int64_t, const void*, int64_t, int64_t, int, int, int, int, int, const EpiParams&, hipStream_t);
template <typename Epi>
constexpr int kK64Code = std::is_same<Epi, EpiResid>::value                                                    ? P2T_EPI_RESID
                         : std::is_same<Epi, EpiGelu<bf16_t>>::value || std::is_same<Epi, EpiGelu<float>>::value   ? P2T_EPI_GELU
                         : std::is_same<Epi, EpiStore<bf16_t>>::value || std::is_same<Epi, EpiStore<float>>::value ? P2T_EPI_STORE
                                                                                                                   : -1;
template <typename Epi>
constexpr int kK64Out = std::is_same<Epi, EpiResid>::value || std::is_same<Epi, EpiStore<float>>::value || std::is_same<Epi, EpiGelu<float>>::value
                            ? P2T_F32 : P2T_BF16;

template <typename Epi>
static GemmPlan plan_lab(const GemmFacts& f, int policy) {
    constexpr EpiTraits t = kEpiTraits<Epi>;
    switch (policy) {
        case 1: return per_tile8(f, small_tiles_pay(f));
        case 128: case 256: return per_tile8(f, policy == 128);
        case 2: return plan_per_tile(f, t, true);
        case 6:
            if (kK64Code<Epi> >= 0) return {GEMM_K64, f.items, f.items};
            break;
        case 7:
            if (kW4TileCode<Epi> >= 0 && f.K % 128 == 0 && f.K >= 256 && f.stride32) return {GEMM_W4_TILE, f.items, f.items};
            break;
        default:            // 3, 4, 5, 8, 10, 12: persistent forms
            if (!persist_fits(f)) return plan_per_tile(f, t, true);
            if ((policy == 8 || policy == 10 || policy == 12) && t.w4 && f.stride32)
                return persist4(f, policy == 8 && f.ns >= 16, policy == 12 ? 0 : 1);
            return persist8(f, policy == 3 || ((policy == 8 || policy == 10 || policy == 12) && pairs_pay(f)), policy == 5 || policy == 8);
    }
    return persist_pays(f, t) ? plan_persist(f, t, false) : plan_per_tile(f, t, true);     // 6 / 7 without that form
}
