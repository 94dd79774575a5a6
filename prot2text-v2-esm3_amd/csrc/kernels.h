// Internal launchers shared between translation units (not part of the C ABI).
#pragma once
#include "common.h"

namespace p2t {

struct EpiParams;

size_t colsum_scratch_bytes(int64_t cols);
int launch_colsum(const void* x, int dtype, int64_t rows, int64_t cols, int64_t ld, float* out, int accumulate, float* scratch,
                  hipStream_t s);

int launch_layernorm(const float* x, int64_t ld_x, const float* w, const float* b, float eps, void* y, int64_t ld_y,
                     int64_t rows, int64_t cols, int out_dtype, hipStream_t s);
int launch_rmsnorm(const float* x, int64_t ld_x, const float* w, float eps, void* y, int64_t ld_y, int64_t rows,
                   int64_t cols, int out_dtype, hipStream_t s);
int launch_rmsnorm_few_rows(const float* x, int64_t ld_x, const float* w, float eps, void* y, int64_t ld_y, int64_t rows, int64_t cols,
                            int out_dtype, hipStream_t s);     // decode step: block per row (norm.hip)
int launch_l2norm(const void* x, int in_dtype, int64_t ld_x, void* y, int out_dtype, int64_t ld_y, float* inv_norm,
                  int64_t rows, int64_t cols, float eps, hipStream_t s);
// g (+)= dX of RMSNorm with a frozen weight; dy: f32 or bf16 (norm.hip)
int launch_rmsnorm_bwd(const float* x, int64_t ld_x, const float* w, float eps, const void* dy, int64_t ld_dy, int dy_dtype, float* g,
                       int64_t ld_g, int64_t rows, int64_t cols, int accumulate, hipStream_t s);

int launch_mask_prepare(const int64_t* ids, const int64_t* mask, int B, int T, int mask_id, int token_dropout,
                        uint8_t* key_mask, int32_t* kv_info, float* emb_scale, hipStream_t s);
int launch_esm_embed(const int64_t* ids, const int64_t* mask, const void* table, int dtype, const float* emb_scale, int T,
                     int H, int vocab, int mask_id, int token_dropout, float* x, int64_t M, hipStream_t s);
int launch_llama_embed(const int64_t* ids, const void* table, int dtype, int H, int vocab, float* x, int64_t M, hipStream_t s);
int launch_inv_freq(float* inv_freq, int half, float theta, int llama3, float factor, float low_ff, float high_ff,
                    float orig_max_pos, hipStream_t s);
int launch_rope_table(const float* inv_freq, int T, int half, float* cs, hipStream_t s);
// docs (optional): i32 [2][B][T] from launch_doc_prepare (packed rows): the rotation of token t uses position t - docs[0][b][t].
// perm128: qkv comes from p2t_llama_layer.qkv_w at head_dim 128, whose rows are permuted per head for the fused rotary epilogue
int launch_qkv_post(const void* qkv, int64_t ldq, const float* cs, void* q, void* k, void* v, int B, int T, int nh, int nkv,
                    int d, int dp, float q_scale, int dtype, hipStream_t s, const int32_t* docs = nullptr, int perm128 = 0);
// packed rows (include/p2t_hip.h, p2t_doc_prepare): position_ids (i64 or i32) + mask -> docs i32 [2][B][T] (document start, end)
// and flags |= 1 (malformed) / 2 (not an arange); flags must be zeroed first
int launch_doc_prepare(const void* pos, int pos_i64, const int64_t* mask, int B, int T, int32_t* docs, int32_t* flags, hipStream_t s);

int launch_qk_norm_rope(const void* qkv, int64_t ldq, const float* cs, const float* q_norm_w, const float* k_norm_w, float eps, void* q,
                        void* k, void* v, int B, int T, int nh, int nkv, int d, int dp, float q_scale, int dtype, hipStream_t s,
                        const int32_t* docs = nullptr);

int launch_gemm_simple(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int N, int K, int n_cover, int dtype,
                       int out_dtype, int epilogue, const EpiParams& ep, hipStream_t s);
int launch_gemm_mfma(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int N, int K, int n_cover,
                     int out_dtype, int epilogue, const EpiParams& ep, void* fix_ws, size_t fix_bytes, unsigned fix_epoch,
                     hipStream_t s);
// fp8 path (quant.hip, the fp8-writing norms of norm.hip, gemm_fp8.hip)
int launch_quant_rows(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* q, int64_t ld_q, uint8_t* scale,
                      hipStream_t s);
int launch_layernorm_fp8(const float* x, int64_t ld_x, const float* w, const float* b, float eps, void* q, int64_t ld_q,
                         uint8_t* scale, int64_t rows, int64_t cols, float bound_w, float bound_b, uint8_t* bound_scale, hipStream_t s);
int launch_rmsnorm_fp8(const float* x, int64_t ld_x, const float* w, float eps, void* q, int64_t ld_q, uint8_t* scale, int64_t rows,
                       int64_t cols, hipStream_t s);
// the decode step's forms for a few rows (block per row, one round trip; quant.hip, norm.hip)
int launch_quant_rows_few(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* q, int64_t ld_q, uint8_t* scale, hipStream_t s);
int launch_rmsnorm_fp8_few(const float* x, int64_t ld_x, const float* w, float eps, void* q, int64_t ld_q, uint8_t* scale, int64_t rows, int64_t cols,
                           hipStream_t s);
int launch_gemm_fp8(const void* A, int64_t lda, const uint8_t* a_scale, const void* W, int64_t ldw, const uint8_t* w_scale, int64_t M, int N,
                    int K, int n_cover, int out_dtype, int epilogue, const EpiParams& ep, int tile, hipStream_t s);
// ---- GEMM launch plans: the launch policy of gemm_mfma.hip / gemm_fp8.hip as pure host code (no HIP call), apart from the
// launch itself, so that it can be queried (lab build: p2t_lab_gemm_plan) and tested without a GPU
enum GemmForm : int {
    GEMM_NONE = 0,      // no form of this path takes the call (fp8 tile 4 on a shape the four-wave kernel does not take)
    GEMM_TILE128,       // gemm_nt_mfma_kernel, one 128 x 256 tile per block
    GEMM_TILE256,       // gemm_nt_mfma_kernel, one 256 x 256 tile per block
    GEMM_SPLITK,        // gemm_nt_mfma_tail_kernel: n_full whole tiles, then n_tail tiles as split-K pairs on two blocks each
    GEMM_PERSIST,       // gemm_nt_mfma_persist_kernel: n_full tiles walked by one block per CU, then n_tail split-K pairs / 128-row halves
    GEMM_W4_TILE,       // gemm_w4.hip, one tile per block
    GEMM_W4_PERSIST,    // gemm_w4.hip persistent: n_full tiles, then n_tail split-K pairs in the same stream
    GEMM_W4_PAIRS,      // gemm_w4.hip: every one of the n_tail tiles as a split-K pair
    GEMM_K64,           // lab: bf16 operands through gemm_fp8.hip's 64-deep skeleton
    FP8_TILE128,        // gemm_nt_fp8_kernel, 128-row tiles
    FP8_TILE256,        // gemm_nt_fp8_kernel, 256-row tiles
    FP8_W4,             // gemm_fp8_w4.hip persistent
    FP8_ABLATION,       // lab: gemm_nt_fp8_kernel with K-loop ablation `variant` (results are garbage)
    FP8_STAMPS,         // lab: gemm_fp8_w4.hip with per-workgroup stamps, variant `variant`
};
struct GemmPlan {
    int form = GEMM_NONE;
    int64_t grid = 0;             // workgroups
    int64_t n_full = 0;           // tiles run whole (the persistent forms: walked by the grid)
    int64_t n_tail = 0;           // tiles run as split-K pairs (or 128-row halves: half_tail)
    int half_tail = 0;
    int variant = 0;              // GEMM_W4_PERSIST: instruction order of the K loop (1 = the product's); FP8_ABLATION / FP8_STAMPS: which
};
// the facts of one call that the launch policy reads
struct GemmFacts {
    int64_t M, lda, ldw;
    int N, K, n_cover, cus;
    size_t fix_bytes;             // usable split-K fix-up workspace (0: none)
    int ns;                       // 32-deep K stages
    int64_t tn, items, rem;       // 256-column tile columns; 256 x 256 tiles; tiles of a partial last round on `cus` CUs
    bool whole_tiles;             // no edge tiles
    bool stride32;                // the four-wave kernels' 32-bit lane offsets reach every row
};
GemmFacts gemm_facts(int64_t M, int N, int K, int n_cover, int64_t lda, int64_t ldw, int cus, size_t fix_bytes);
bool small_tiles_pay(const GemmFacts& f);      // 128-row tiles fill the chip better than 256-row ones
GemmPlan plan_gemm_mfma(const GemmFacts& f, int epilogue, int out_dtype, int policy);   // policy: p2t_set_gemm_policy
GemmPlan plan_gemm_fp8(const GemmFacts& f, int epilogue, int out_dtype, int tile, bool no_w4);
bool fp8_w4_fits(int64_t M, int N, int K, int n_cover, int64_t lda, int64_t ldw, int grid);    // gemm_fp8_w4.hip takes the shape

unsigned* fault_word_ptr();            // the GPU's sticky fault word (misc.hip); nullptr if the symbol cannot be resolved
int get_gemm_policy();
void set_gemm_policy(int policy);       // launch-form override of the MFMA GEMM (tests / experiments), 0 = default
size_t gemm_fix_workspace_bytes();       // split-K tail fix-up workspace (flags + slabs); header must be zeroed once per
size_t gemm_fix_header_bytes();          // sequence of launches that use distinct epochs
// GemmArgs::use_mfma (bf16 / fp32 operands; fp8 has one path).  AUTO (or any other value): the MFMA kernel where the call is eligible
// (bf16, K % 64 == 0, 16-byte rows), else the fp32-FMA kernel; SIMPLE: the fp32-FMA kernel; MFMA: P2T_ERR_UNSUPPORTED if not eligible
enum : int { GEMM_KERNEL_AUTO = -1, GEMM_KERNEL_SIMPLE = 0, GEMM_KERNEL_MFMA = 1 };
// full dispatcher behind p2t_gemm_nt (gemm.hip): out[M, N] = epilogue(A[M, K] . W[N, K]^T).  The constructor names what every
// call says; everything else is set by member name where it is not the default.
struct GemmArgs {
    const void* A; int64_t lda; const void* W; int64_t ldw; const float* bias = nullptr; void* out; int64_t ldc; void* z = nullptr;
    int64_t M; int64_t N; int64_t K; int dtype; int out_dtype; int epilogue; int accumulate = 0; int use_mfma = GEMM_KERNEL_AUTO;
    int n_zero = -1;            // -1: default (next multiple of 64, clipped to ldc)
    float drop_p = 0.f; uint64_t drop_seed = 0;
    int tile = 0;               // fp8 only: 0 auto, 4 four-wave kernel, 128 / 256 rows of the per-tile kernel (bf16: p2t_set_gemm_policy)
    GemmArgs(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K, int dtype, void* out, int64_t ldc,
             int out_dtype, int epilogue)
        : A(A), lda(lda), W(W), ldw(ldw), out(out), ldc(ldc), M(M), N(N), K(K), dtype(dtype), out_dtype(out_dtype), epilogue(epilogue) {}
    // P2T_EPI_QKV_ROPE only (head_dim 64 or 128): rotary table [T, head_dim], outputs [B, heads, T, head_dim]
    const float* cs = nullptr; void* q = nullptr; void* k = nullptr; void* v = nullptr;
    int seq = 0, nh = 0, nkv = 0; float q_scale = 1.f; int head_dim = 64;
    // optional split-K tail fix-up (MFMA kernel, 256-row tiles): workspace + an epoch unique since its header was zeroed
    void* fix_ws = nullptr; size_t fix_bytes = 0; unsigned fix_epoch = 0;
    // dtype == P2T_FP8: A and W are e4m3 bytes (row strides in bytes), one E8M0 scale byte per row of each
    const uint8_t* a_scale = nullptr; const uint8_t* w_scale = nullptr;
    const uint8_t* out_row_scale = nullptr;        // P2T_EPI_GELU_FP8: E8M0 byte of every output row
};
int gemm_nt(const GemmArgs& a, hipStream_t s);
// the fp8 form: A [M, K] and W [N, K] are e4m3 bytes with one E8M0 scale byte per row, W rows packed at stride K
static inline GemmArgs gemm_args_fp8(const void* A, int64_t lda, const uint8_t* a_scale, const void* W, const uint8_t* w_scale, int64_t M, int64_t N,
                                     int64_t K, void* out, int64_t ldc, int out_dtype, int epilogue) {
    GemmArgs g(A, lda, W, K, M, N, K, P2T_FP8, out, ldc, out_dtype, epilogue);
    g.use_mfma = GEMM_KERNEL_MFMA; g.a_scale = a_scale; g.w_scale = w_scale;
    return g;
}
// The A operand of a projection: rows of the model dtype at stride ld (scale == nullptr), or (gemm_fp8) e4m3 bytes at stride ld
// with one E8M0 scale byte per row.  Either way its rows are zero padded to ld, which is also the weight's row stride and the
// GEMM's K (the width rounded up to 64 elements, or to 128 bytes).
struct Operand { void* p; int64_t ld; uint8_t* scale; };

// out[M, N] = epilogue(a . W[N, a.ld]^T); ws: the weight's row scales, read by the fp8 form only
static inline GemmArgs projection(const Operand& a, const void* W, const uint8_t* ws, int64_t M, int64_t N, int dt, void* out, int64_t ldc, int out_dtype, int epi) {
    return a.scale ? gemm_args_fp8(a.p, a.ld, a.scale, W, ws, M, N, a.ld, out, ldc, out_dtype, epi)
                   : GemmArgs(a.p, a.ld, W, a.ld, M, N, a.ld, dt, out, ldc, out_dtype, epi);
}
// hand the call the split-K fix-up workspace `ws` (gemm_fix_workspace_bytes()); `epoch` counts the calls since its header was zeroed
static inline void with_fix(GemmArgs& g, void* ws, unsigned& epoch) { g.fix_ws = ws; g.fix_bytes = gemm_fix_workspace_bytes(); g.fix_epoch = ++epoch; }
// weight-streaming GEMM for M <= 64 rows (gemm_skinny.hip): bf16, epilogues STORE / STORE_F32 / RESID / SWIGLU, no bias;
// P2T_ERR_UNSUPPORTED for anything else
// epilogue arguments of launch_gemm_skinny_qkv_rope: rotation at position prompt_len[row / group] + step[row * step_stride] and the cache
// append (step_stride 0: the shared lock-step counter, 1: every row's own).  q_tokens > 1 (several tokens per cache row, per-row counters):
// GEMM row m is token m % q_tokens of cache row m / q_tokens -- its counter is step[m / q_tokens] + m % q_tokens, its q goes to row m of q
struct SkinnyRope {
    const float* inv_freq = nullptr; const int32_t* prompt_len = nullptr; const int32_t* step = nullptr;
    int group = 1, nh = 0, nkv = 0, d = 0, G = 0; float q_scale = 1.f; int step_stride = 0;
    int q_tokens = 1;
    void* q = nullptr;       // bf16 [M, nh, d]
    void* k = nullptr;       // bf16 [M, nkv, G, d]   (one layer of p2t_kv_cache.k_gen)
    void* vt = nullptr;      // bf16 [M, nkv, d, G]   (one layer of p2t_kv_cache.vt_gen)
};
int launch_gemm_skinny_qkv_rope(const void* x, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K, const SkinnyRope& ra,
                                hipStream_t s, int pre);
// pre: W is the pre-shuffled stream copy written by launch_preshuffle (ldw unused)
int launch_gemm_skinny(const void* x, int64_t lda, const void* W, int64_t ldw, void* out, int64_t ldc, int64_t M, int64_t N, int64_t K, int dtype,
                       int out_dtype, int epilogue, hipStream_t s, int pre = 0);
int launch_preshuffle(const void* W, int64_t ldw, int64_t N, int64_t K, void* out, hipStream_t s);
// e4m3 operands + one E8M0 scale byte per row (gemm_fp8 models): K % 128 == 0; ra: the QKV + rotation + cache-append form
int launch_gemm_skinny_fp8(const void* x, int64_t lda, const uint8_t* xs, const void* W, int64_t ldw, const uint8_t* ws, void* out, int64_t ldc, int64_t M,
                           int64_t N, int64_t K, int out_dtype, int epilogue, const SkinnyRope* ra, hipStream_t s, int pre);
int launch_preshuffle_fp8(const void* W, int64_t ldw, int64_t N, int64_t K, void* out, hipStream_t s);
// MXFP4 weights (e2m1 codes [N, ldw bytes] + E8M0 block scales [N, K / 32]) against the same e4m3 rows; pre: the interleaved stream
// copy of launch_preshuffle_mxfp4 (ldw, wbs unused)
int launch_gemm_skinny_mxfp4(const void* x, int64_t lda, const uint8_t* xs, const void* W, int64_t ldw, const uint8_t* wbs, void* out, int64_t ldc,
                             int64_t M, int64_t N, int64_t K, int out_dtype, int epilogue, const SkinnyRope* ra, hipStream_t s, int pre);
int launch_preshuffle_mxfp4(const void* codes, int64_t ldw, const uint8_t* bs, int64_t N, int64_t K, void* out, hipStream_t s);

int launch_attn_simple(const void* q, const void* k, const void* v, const uint8_t* key_mask, const int32_t* kv_info, void* out,
                       int64_t ld_out, int B, int T, int nh, int nkv, int d, int dp, float scale, int causal, int dtype,
                       float* lse, hipStream_t s, const int32_t* docs = nullptr);
int launch_attn_mfma(const void* q, const void* k, const void* v, const uint8_t* key_mask, const int32_t* kv_info, void* out,
                     int64_t ld_out, int B, int T, int nh, int nkv, int d, int dp, float scale, int causal, int log2_scores, float* lse, hipStream_t s,
                     const int32_t* docs = nullptr);
// hand-placed form for head_dim padded to 64 with log2-scores q (attn_fwd64.hip; tools/gen_attn_fwd64.py writes its loop)
bool attn_fwd64_eligible(int64_t ld_out, int T, int nh, int nkv, int d, int dp, int log2_scores);
int launch_attn_fwd64(const void* q, const void* k, const void* v, const uint8_t* key_mask, const int32_t* kv_info, void* out, int64_t ld_out,
                      int B, int T, int nh, int nkv, int d, int causal, float* lse, hipStream_t s);
// log2_scores: q was stored pre-multiplied by scale * log2(e) (kLog2e below), so q k^T is already the base-2 exponent: `scale` is
// ignored and p = exp2(s - m).  The towers do this for bf16 models (one multiply + add less per score in the MFMA kernel).
int attention(const void* q, const void* k, const void* v, const uint8_t* key_mask, const int32_t* kv_info, void* out,
              int64_t ld_out, int B, int T, int nh, int nkv, int d, int dp, float scale, int causal, int dtype, int use_mfma,
              int log2_scores, hipStream_t s, float* lse = nullptr, const int32_t* docs = nullptr);
// lse (optional, f32 [B, nh, T]): natural-log sum-exp of the effective logits (scale * q.k, or ln 2 * q.k with log2_scores) of
// every query row, +inf for a row without a visible key -- what the attention backward (llama_train.hip) rebuilds P from.
// docs (optional, causal only): i32 [2][B][T] from launch_doc_prepare.  Query t sees keys docs[0][b][t] <= key <= t; both rows are
// non-decreasing in t, so the first query of a tile holds its smallest start and the last key of a tile its largest end: the
// kernels start the key loop at the tile's first start (64-key blocks wholly before it are skipped, not masked) and end the
// query loop of a key tile at its last end.  Never the hand-placed kernel.
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// stage-2 training through the frozen decoder (llama_train.hip): the per-layer activations the backward reads again
struct LlamaTapeLayer {
    float* x_in; float* x_mid;          // residual stream before the layer / after its attention branch, f32 [M, H]
    void* q; void* k; void* v;          // rotated (and, for bf16 models, pre-scaled) heads, `dtype` [B, heads, T, dp]
    float* lse;                         // f32 [B, nh, T], see attention()
    void* ao;                           // attention output, `dtype` [M, QO]
    void* gu;                           // gate / up pre-activations, `dtype` [M, 2F] in the interleaved order of gu_w
};
struct LlamaTape {
    static constexpr int kMaxLayers = 128;
    int n_layers; bool overflow;
    float* x_last;                      // input of the final RMSNorm, f32 [M, H]
    LlamaTapeLayer layer[kMaxLayers];
};
size_t llama_tape_plan(const p2t_llama_config* c, int B, int T, void* base, size_t bytes, LlamaTape* tape);
// docs (optional, packed rows): i32 [2][B][T] from launch_doc_prepare -- positional rotary and document-confined attention
// Where the prompts of a packed prompt batch lie (include/p2t_hip.h, p2t_pack_rows): prompt i = tokens start[i] .. start[i] + len[i] - 1
// of packed row row[i].  It travels by value in the launch arguments (like kv_cache.hip's SlotTable): a host array in, no copy, no
// allocation.  `longest`: the largest len, the grid's extent.  Filled and checked by place_table (kv_cache.hip).
constexpr int kPackedPromptsMax = 256;
struct PlaceTable { int32_t row[kPackedPromptsMax]; int32_t start[kPackedPromptsMax]; int32_t len[kPackedPromptsMax]; };
struct PackedPrompts { int n; int longest; PlaceTable tab; };
// place: HOST i32 [n][3] = (row, start, len) -> pp, after every refusal: 1 <= n <= kPackedPromptsMax (beyond: P2T_ERR_UNSUPPORTED), rows in
// [0, R), starts >= 0, len >= 1, start + len <= Tpk, len <= Tp (Tp 0: no cache to hold them), no two prompts overlapping in a row
int place_table(const int32_t* place, int n, int R, int Tpk, int Tp, const char* who, PackedPrompts* pp);
// docs with kv (the packed prefill): `packed` says where each prompt lies, and every layer's keys / values go through llama_kv_store_packed
int llama_forward_impl(const p2t_llama_config* c, const p2t_llama_weights* w, const int64_t* ids, const float* inputs_embeds, const int64_t* mask,
                       int B, int T, int k, float* out, void* workspace, size_t workspace_bytes, p2t_stream stream, const LlamaTape* tape,
                       const p2t_kv_cache* kv = nullptr, const int32_t* docs = nullptr, const PackedPrompts* packed = nullptr);
// generation prefill (kv_cache.hip): layer l's rotated keys / values ([B, kv_heads, T, dp]) -> the prompt segment of the cache
int llama_kv_store(const p2t_llama_config* c, const p2t_kv_cache* kc, int layer, const void* k, const void* v, int B, int T, hipStream_t s);
// the same from packed rows ([R, kv_heads, Tpk, dp]): prompt i's keys -> row i of the prompt segment, positions 0 .. len[i] - 1; ONE launch
int llama_kv_store_packed(const p2t_llama_config* c, const p2t_kv_cache* kc, int layer, const void* k, const void* v, int Tpk, const PackedPrompts& pp,
                          hipStream_t s);
// last_hidden[i] = x[row[i], start[i] + len[i] - 1] (f32 rows of H): the packed form of the prefill's gather (kv_cache.hip)
int launch_gather_last_packed(const float* x, int Tpk, int H, const PackedPrompts& pp, float* out, hipStream_t s);
// every refusal of a cache descriptor against the model's head shape and dtype (kv_cache.hip).  `who`: the entry point's name
int check_cache(const p2t_llama_config* c, const p2t_kv_cache* kc, const char* who);
// every refusal of a beam group under an ancestry table (kv_cache.hip): a null table, fewer than 2 or more than 16 rows per prompt, more
// than 16 query heads per kv head (heads_per_kv 0: not the caller's concern)
int check_ancestry(const void* ancestry, int group, int heads_per_kv, const char* who);
// attention of one query token per row over layer `layer` of the cache (attn_decode.hip): q [BB, heads, dp] -> out [BB, ld_out], both the
// model dtype; c gives heads / kv_heads / head_dim / dtype.  use_mfma (bf16): 0 = the lane-per-key kernel, the one f32 runs;
// step_stride: 0 = the cache's shared counter, 1 = kc->step[row]
int launch_attn_decode(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp, int round_p,
                       int use_mfma, int step_stride, hipStream_t s);
// the same over a beam group whose generated keys stay where they were written: key i of row r's history is in physical row
// ancestry[r][i] of r's prompt (u8 [BB][kc->G], kv_cache.hip).  The shared counter; group 2 .. 16, at most 16 query heads per kv head
int launch_attn_decode_beams(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp,
                             int round_p, int use_mfma, const uint8_t* ancestry, hipStream_t s);
// the same for q_tokens query tokens per row (group 1, kc->step = the rows' own counters): q [BB * q_tokens, heads, dp], row r * q_tokens + j
// is token j of cache row r and sees the generated keys 0 .. kc->step[r] + j.  At most 16 query heads per kv head (check_multi)
int launch_attn_decode_multi(const p2t_llama_config* c, const void* q, void* out, int64_t ld_out, const p2t_kv_cache* kc, int layer, float c_exp,
                             int round_p, int use_mfma, int q_tokens, hipStream_t s);
int check_multi(int q_tokens, int heads_per_kv, const char* who);
// SwiGLU on the interleaved gate / up pre-activations gu [M, 2F], forward and backward (activations.hip)
int launch_swiglu_from_gu(const void* gu, int64_t ld_gu, void* act, int64_t ld_act, int64_t M, int64_t F, int dtype, hipStream_t s);
int launch_swiglu_gu_bwd(const void* gu, int64_t ld_gu, const void* d_act, int64_t ld_da, void* d_gu, int64_t ld_dgu, int64_t M, int64_t F, int dtype,
                         hipStream_t s);
// (misc.hip) dst[m, c] = (Tdst)src[m, c] for c < cols, 0 for cols <= c < ld_dst  (a GEMM operand with its K padding)
int launch_cast_rows(const void* src, int src_dtype, int64_t ld_src, void* dst, int dst_dtype, int64_t ld_dst, int64_t rows, int64_t cols, hipStream_t s);

// lm_loss.hip (the shifted cross-entropy over the full logits and over the target rows only, forward and backward) shares its label
// rule and its row max / sum-exp between its own kernels and nothing between translation units: its seven entry points are
// declared in include/p2t_hip.h alone

// adapter tail helpers (adapter.hip)
int launch_adapter_dz2(const void* g2, const void* z2, const float* inv_norm, const float* dy, void* dz2, int64_t ld, int64_t M,
                       int D, int dtype, float drop_p, uint64_t drop_seed, hipStream_t s);

// bump allocator over a caller-provided workspace
struct Arena {
    char* base; size_t size; size_t off = 0; bool overflow = false;
    Arena(void* b, size_t n) : base((char*)b), size(n) {}
    void* take(size_t bytes) {
        const size_t a = (off + 255) & ~(size_t)255;
        if (a + bytes > size) { overflow = true; off = a + bytes; return base; }
        off = a + bytes;
        return base + a;
    }
};

static inline int head_dim_padded(int d) { return d <= 32 ? 32 : (d <= 64 ? 64 : 128); }

}  // namespace p2t
