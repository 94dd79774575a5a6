/* libp2t_hip -- C ABI of the MI355X-native contrastive-alignment hot path of Prot2Text-V2.
 *
 * The reference (RockingMat/Prot2Text-V2-esm3) is pure Python: it has no FFI, the hot path is
 * reached through nn.Module calls.  This header is the drop-in boundary a maintainer binds with
 * ctypes (INTEGRATION.md shows the stub); every entry point names the reference call it replaces:
 *
 *   p2t_esm2_forward          Esm2LlamaInstructForCausalLM.forward(return_encoder_outputs=True)
 *                             models/modeling_esm2llama_instruct.py:175-189 -> HF EsmModel.forward
 *   p2t_adapter_forward       ModalityAdapter.forward, models/modeling_esm2llama_instruct.py:60-68
 *   p2t_adapter_backward      autograd of the same (loss.backward(), scripts/train_contrast.py:448)
 *   p2t_llama_hidden_forward  llm_decoder.model(..., output_hidden_states=True).hidden_states[k]
 *                             scripts/train_contrast.py:292-304 -> HF LlamaModel.forward
 *   p2t_readout / _backward   readout_embeddings, scripts/train_contrast.py:198-248
 *   p2t_l2norm_rows           torch.nn.functional.normalize(p=2, dim=-1), train_contrast.py:354,365
 *   p2t_infonce_forward/_backward  SegmentedBatchInfoNCELoss / BatchInfoNCELoss, train_contrast.py:72-114
 *   p2t_clip_adamw_step       clip_grad_norm_ + AdamW.step, train_contrast.py:453-465,621-626
 *   p2t_clip_adamw_flat       the same over one flat buffer with a segment table, train_instruct.py:431-447
 *
 * Conventions: plain pointers and sizes, no framework types.  All pointers are DEVICE pointers
 * unless named host_*.  Every call only ENQUEUES work on `stream` (a hipStream_t passed as void*),
 * never allocates, never synchronises; buffers are owned by the caller (PyTorch's allocator in the
 * Python host).  Return value: P2T_OK or a negative code, text via p2t_last_error().
 * The library is re-entrant per stream.  Global state: the thread-local error string; the measurement hooks
 * (p2t_prof_*, mutex-guarded, off by default); the GEMM launch-form override (p2t_set_gemm_policy, one atomic word,
 * default 0); one sticky fault word per GPU in device memory (p2t_fault_status).  No environment variable is read.
 */
#ifndef P2T_HIP_H
#define P2T_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2T_VERSION 103

enum { P2T_OK = 0, P2T_ERR_ARG = -1, P2T_ERR_HIP = -2, P2T_ERR_UNSUPPORTED = -3 };
enum { P2T_F32 = 0, P2T_BF16 = 1,                         /* storage dtype of weights / activations */
       P2T_FP8 = 2 };                                      /* GEMM operands only: OCP e4m3fn bytes + one E8M0 scale byte per row */
enum { P2T_READOUT_LAST = 0, P2T_READOUT_MEAN = 1, P2T_READOUT_STD = 2, P2T_READOUT_MIX = 3 };
enum {                                                     /* GEMM epilogues (p2t_gemm_nt) */
    P2T_EPI_STORE = 0,      /* C = acc + bias                                   */
    P2T_EPI_GELU = 1,       /* C = gelu_erf(acc + bias); optional Z = acc + bias */
    P2T_EPI_RESID = 2,      /* R(f32, in place) += acc + bias                   */
    P2T_EPI_SWIGLU = 3,     /* C[m, f] = silu(gate) * up, gate/up interleaved by 32 rows of W */
    P2T_EPI_STORE_F32 = 4,  /* C(f32) = acc (+ C if accumulate)                  */
    P2T_EPI_GELU_BWD = 5,   /* C = acc * gelu_erf'(Z), Z read from z (adapter backward) */
    P2T_EPI_QKV_ROPE = 6,   /* internal to the towers: bias + q-scale + rotary + head split, head_dim 64 */
    P2T_EPI_GELU_FP8 = 7    /* p2t_gemm_nt_fp8 only: C(e4m3 bytes) = gelu_erf(acc + bias) * 2^-(row_scale[m] - 127) */
};

typedef void* p2t_stream;

int p2t_version(void);
const char* p2t_last_error(void);
/* sizeof() of the ABI structs, for bindings to self-check: 0 esm2_config, 1 esm2_layer, 2 esm2_weights,
 * 3 llama_config, 4 llama_layer, 5 llama_weights, 6 adapter_config, 7 adapter_weights, 8 adapter_saved, 9 llama_layer_t,
 * 10 kv_cache, 11 llama_layer_stream, 12 flat_segment, 13 flat_chunk, 14 beam_state, 15 llama_layer_mxfp4, 16 lm_head_q. */
size_t p2t_struct_size(int which);

/* ---------------------------------------------------------------- measurement hooks (bench.py) */
/* When enabled, every bf16 MFMA GEMM (class 0), MFMA attention (class 1) and fp8 MFMA GEMM (class 2; only reported
 * when n_classes >= 3) launch is bracketed by HIP events on its
 * own launch stream.  p2t_prof_collect synchronises those events (the only host sync in the library) and returns,
 * per class, the summed kernel time in ms, the launch count and the algorithmic FLOPs (GEMM: 2 M N K; attention:
 * 4 B nh T^2 d, halved when causal); it then resets the record list. */
int p2t_prof_enable(int on);
int p2t_prof_collect(double* ms, int64_t* launches, double* flops, int n_classes);
/* Launch-form override of the MFMA GEMMs (process-wide, one atomic word): 0 = the measured default policy; 9 = the same
 * policy without the four-wave kernels (bf16 and fp8) -- the eight-wave forms the bit-identity tests compare against
 * (tests/test_gpu_fullsize.py).  Results are identical up to the fp32 summation order.  Any other value is refused by
 * the product library: the launch-form zoo of the development rounds (forced tile heights, forced split-K, the other
 * generated instruction order ...) is compiled into the LAB build only (csrc/Makefile `make lab`, -DP2T_LAB,
 * tools/lab/gemm_forms_lab.h -> tools/build/libp2t_lab.so), which tools/ and tests/test_gpu_lab_forms.py load
 * through P2T_HIP_LIB. */
int p2t_set_gemm_policy(int policy);
int p2t_is_lab_build(void);     /* 1: lab build, 0: product library */

/* ---------------------------------------------------------------- runtime guards of the epoch loop */
/* The reference's train_epoch / eval_epoch keep `ddp_loss = [sum of batch losses, batches seen]` and `ddp_gradnorm =
 * [sum of gradient norms, optimizer steps]` (scripts/train_contrast.py:410-413,443-444,461-462,493-512) and look at
 * every batch loss on the host (`loss.item()`, the "impossible batch loss" print of :431-434, the epoch NaN abort of
 * :476-480).  p2t_epoch_accumulate keeps the same four sums on the device -- sums f32[4] = {loss sum, batches,
 * gradient-norm sum, optimizer steps}; grad_norm may be NULL when no optimizer step ran after this batch -- and the
 * guards as flags i32[4] = {number of impossible losses so far (NaN, inf or <= 0: the condition of :433), batch index
 * of the first one (caller initialises to -1), OR of the GPU's sticky fault word, bit pattern of the first impossible
 * loss}: one launch per batch, no host synchronisation; the host reads `flags` every N batches and at the epoch end.
 *
 * Fault word: one word per GPU, bit 0 = a split-K consumer of an MFMA GEMM gave up waiting for its producer (bounded
 * spin, never expected: csrc/gemm_mfma.hip TILE_CONSUME, csrc/gemm_w4.hip).  While it is set every such consumer
 * writes NaN tiles, so the loss of the step is NaN as well.  Sticky: only p2t_fault_status(clear = 1) resets it.
 * p2t_fault_status copies it to the host (SYNCHRONOUS hipMemcpy: for epoch boundaries and tests);
 * p2t_fault_inject sets it from a stream (tests of the guard). */
int p2t_epoch_accumulate(const float* loss, const float* grad_norm, int batch_idx, float* sums, int32_t* flags,
                         p2t_stream stream);
int p2t_fault_status(unsigned* host_out, int clear);
int p2t_fault_inject(unsigned value, p2t_stream stream);

/* ---------------------------------------------------------------- synthetic data (bench / tests) */
/* dst[i] = (int(hash24(i)) - 2^23) * scale23 + offset ; see p2t_hip/synth.py (bit-identical). */
int p2t_fill_hash(void* dst, int64_t n, uint64_t add, uint64_t xorv, float scale23, float offset,
                  int dtype, p2t_stream stream);
int p2t_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, p2t_stream stream);
/* x[i] *= scalar[0], scalar on the device (chain-rule scaling of a gradient without a host sync). */
int p2t_scale_by_device_scalar(float* x, int64_t n, const float* scalar, p2t_stream stream);
/* dst[c, r] = src[r, c]  (row strides in elements) */
int p2t_transpose(const void* src, int64_t rows, int64_t cols, int64_t ld_src, void* dst, int64_t ld_dst,
                  int dtype, p2t_stream stream);

/* ---------------------------------------------------------------- building blocks */
/* C[M,N] = A[M,K] * W[N,K]^T with a fused epilogue.  A, W: `dtype`, K-contiguous, row strides
 * lda/ldw (elements, multiples of 8).  For dtype BF16 with K % 64 == 0 the MFMA kernel runs
 * (v_mfma_f32_16x16x32_bf16, 256x256x64 LDS tiles); otherwise the fp32-FMA kernel.  bias: f32 [N] or NULL.
 * out: `out_dtype` [M, ldc]; columns N..min(ldc, N rounded up to 64)-1 are written as zeros (they are the zero
 * K-padding of the next GEMM).  z (GELU only, may be NULL): pre-activation, out_dtype, same stride.  EPI_RESID: out is f32 and accumulated in place.  EPI_SWIGLU: N is the
 * interleaved gate/up row count (a multiple of 64), out has N/2 columns.  use_mfma: -1 auto, 0 force FMA kernel, 1 require MFMA.
 * fix_ws (optional, p2t_gemm_fix_workspace_bytes() bytes): lets the MFMA kernel run the tiles of a last partial
 * "round" of the 256 CUs as two concurrent K halves (split-K fix-up).  Its first 2048 bytes (the tiles' flag words)
 * must have been zeroed (once) before a sequence of calls that pass strictly increasing fix_epoch values >= 1.
 * A consumer that gives up waiting sets the GPU's fault word (see p2t_fault_status) and poisons its tile with NaN. */
int p2t_gemm_nt(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out, int64_t ldc,
                void* z, int64_t M, int64_t N, int64_t K, int dtype, int out_dtype, int epilogue, int accumulate,
                int use_mfma, void* fix_ws, size_t fix_ws_bytes, unsigned fix_epoch, p2t_stream stream);
size_t p2t_gemm_fix_workspace_bytes(void);
/* ---- fp8 GEMM operands (BASELINE.json configs[4]: "fp8 weights, CDNA4 fp8 MFMA") ----
 * Row-wise quantisation: x `dtype` (F32 / BF16) [rows, ld_x] -> q: OCP e4m3fn bytes [rows, ld_q] (columns cols..ld_q-1 zero;
 * ld_q a multiple of 8, of 128 when q feeds p2t_gemm_nt_fp8) and scale: one E8M0 byte per row, E = 127 + e with 2^e the
 * smallest power of two such that amax(row) / 2^e <= 448; q = e4m3_rne(x * 2^-e).  An all-zero row gets E = 127. */
int p2t_quant_rows_fp8(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* q, int64_t ld_q,
                       uint8_t* scale, p2t_stream stream);
/* torch.nn.LayerNorm / LlamaRMSNorm of the f32 stream written directly in that format (no bf16 intermediate).
 * bound_scale (LayerNorm only, may be NULL): E8M0 byte per row of the smallest power of two >= (||y_row||_2 * bound_w +
 * bound_b) / 448, y the normalised row -- with bound_w >= max_n ||W_n||_2 and bound_b >= max_n |bias_n| of the projection
 * that consumes y, a valid scale for every element of gelu(y W^T + bias) (Cauchy-Schwarz; |gelu(z)| <= |z|): the row scale
 * P2T_EPI_GELU_FP8 needs BEFORE its GEMM runs. */
int p2t_layernorm_fp8(const float* x, int64_t ld_x, const float* w, const float* b, float eps, void* q, int64_t ld_q,
                      uint8_t* scale, int64_t rows, int64_t cols, float bound_w, float bound_b, uint8_t* bound_scale,
                      p2t_stream stream);
int p2t_rmsnorm_fp8(const float* x, int64_t ld_x, const float* w, float eps, void* q, int64_t ld_q, uint8_t* scale,
                    int64_t rows, int64_t cols, p2t_stream stream);
/* C[M,N] = (A8 * 2^(a_scale-127))[M,K] * (W8 * 2^(w_scale-127))[N,K]^T on v_mfma_scale_f32_16x16x128_f8f6f4 (both scales
 * applied by the instruction), fp32 accumulate, the epilogues of p2t_gemm_nt (all but GELU_BWD).  A8 / W8: e4m3 bytes,
 * row strides lda / ldw in BYTES (multiples of 16), K % 128 == 0 with the padding zeroed; a_scale [M], w_scale [N] E8M0
 * bytes.  tile: 0 auto (the persistent four-wave kernel when the shape has no edge tiles, K % 256 == 0 and at least one tile per
 * CU; else the per-tile kernel), 4 = four-wave kernel required, 128 / 256 = per-tile kernel of that tile height; any other
 * tile is P2T_ERR_ARG (the lab build adds its ablation / stamp forms).  P2T_EPI_GELU_FP8: out is e4m3 bytes [M, ldc bytes] (columns N up to
 * the next multiple of 128 zeroed), out_row_scale the E8M0 byte of every output row (an input: see p2t_layernorm_fp8). */
int p2t_gemm_nt_fp8(const void* A, int64_t lda, const uint8_t* a_scale, const void* W, int64_t ldw, const uint8_t* w_scale,
                    const float* bias, void* out, int64_t ldc, void* z, int64_t M, int64_t N, int64_t K, int out_dtype,
                    int epilogue, int accumulate, int tile, const uint8_t* out_row_scale, p2t_stream stream);

/* The QKV projection as the towers launch it for head_dim 64 / 128 (P2T_EPI_QKV_ROPE): acc + bias, query * q_scale
 * BEFORE the rotation (HF EsmSelfAttention.forward, modeling_esm.py:345,362-378: q_scale = head_dim^-1/2 and SDPA scale 1;
 * Llama: q_scale 1, no bias, modeling_llama.py:254-259), rotate-half rotary with the table built from inv_freq
 * (f32 [head_dim/2]; cos_sin_scratch f32 [seq * head_dim]), head split.  A `dtype` [M = B * seq, lda]; W `dtype`
 * [(nh + 2 nkv) * head_dim, ldw], rows q heads | k heads | v heads, for head_dim 128 in the packed per-head row order of
 * p2t_llama_layer; bias f32 or NULL.  Outputs `dtype`: q [B, nh, seq, head_dim], k and v [B, nkv, seq, head_dim].
 * Exposed so that the fused epilogue can be checked on its own against the reference arithmetic. */
int p2t_gemm_qkv_rope(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int64_t M, int64_t K,
                      int dtype, const float* inv_freq, float* cos_sin_scratch, void* q, void* k, void* v, int seq, int nh,
                      int nkv, int head_dim, float q_scale, int use_mfma, void* fix_ws, size_t fix_ws_bytes,
                      unsigned fix_epoch, p2t_stream stream);

/* torch.nn.LayerNorm over the last dim: x f32 [rows, ld_x] -> y `out_dtype` [rows, ld_y]; pad zeroed. */
int p2t_layernorm(const float* x, int64_t ld_x, const float* w, const float* b, float eps, void* y, int64_t ld_y,
                  int64_t rows, int64_t cols, int out_dtype, p2t_stream stream);
/* LlamaRMSNorm (fp32 variance, weight last). */
int p2t_rmsnorm(const float* x, int64_t ld_x, const float* w, float eps, void* y, int64_t ld_y, int64_t rows,
                int64_t cols, int out_dtype, p2t_stream stream);

/* mask int64 [B, T] -> key_mask u8 [B, T]; kv_info i32 [2B]: [b] = 1 + last valid key, [B + b] = 1 if the mask
 * is a plain prefix (the right-padded batch contract); emb_scale f32 [2B] (optional, ESM token-dropout rescale:
 * numerator, denominator; needs ids). */
int p2t_mask_prepare(const int64_t* ids, const int64_t* mask, int B, int T, int mask_id, int token_dropout,
                     uint8_t* key_mask, int32_t* kv_info, float* emb_scale, p2t_stream stream);
/* Head split + query scale + rotary.  qkv `dtype` [B*T, ldq] rows = [q heads | k heads | v heads];
 * inv_freq f32 [d/2]; cos_sin_scratch f32 [T * d].  Outputs q [B, nh, T, dp], k and v [B, nkv, T, dp], head dim
 * zero-padded to dp in {32, 64, 128}.  (For head_dim 64 the towers fuse this pass into the QKV GEMM epilogue.) */
int p2t_qkv_post(const void* qkv, int64_t ldq, const float* inv_freq, float* cos_sin_scratch, void* q, void* k,
                 void* v, int B, int T, int nh, int nkv, int d, int dp, float q_scale, int dtype, p2t_stream stream);

/* Attention.  q [B, nh, T, dp], k and v [B, nkv, T, dp], all `dtype`, row-major (the MFMA kernel transposes V with
 * ds_read_b64_tr_b16).  key_mask u8 [B, T] (1 = valid), kv_info i32 [2B] from p2t_mask_prepare.
 * softmax(scale * q k^T + mask) v -> out [B*T, ld_out] `dtype`, head h in columns h*d..h*d+d-1; columns nh*d up to the
 * next multiple of 64 (the o-proj K padding) zeroed.  causal: also require key <= query.
 * log2_scores != 0: q was stored pre-multiplied by scale * log2(e) (what the towers do for bf16 models, through the q_scale
 * of p2t_gemm_qkv_rope / p2t_qkv_post: q is rounded to bf16 once either way), so q k^T is the base-2 exponent itself:
 * `scale` is ignored, the result is softmax_2(q k^T + mask) v = the same attention, one multiply-add less per score.
 * use_mfma: -1 auto / 1 require = the MFMA kernels (bf16): the hand-placed kernel (csrc/attn_fwd64.hip) where dp == 64,
 * d % 8 == 0 and log2_scores, else the general one (csrc/attn_mfma.hip); 2 = the general MFMA kernel everywhere;
 * 3 = require the hand-placed one; 0 = the exact fp32-softmax kernel. */
int p2t_attention(const void* q, const void* k, const void* v, const uint8_t* key_mask, const int32_t* kv_info,
                  void* out, int64_t ld_out, int B, int T, int nh, int nkv, int d, int dp, float scale, int causal,
                  int dtype, int use_mfma, int log2_scores, float* lse, p2t_stream stream);
/* lse (may be NULL): f32 [B, nh, T], the natural-log sum-exp of every query row's effective logits (scale * q k^T, or
 * ln 2 * q k^T with log2_scores), +inf for a row without a visible key -- what p2t_attention_backward rebuilds P from.
 *
 * Backward of the attention above (exact-fp32 arithmetic on `dtype` operands; stage-2 training, see
 * p2t_llama_train_backward): with P = exp(logits - lse), D = rowsum(dO o O), dS = P o (dO v^T - D):
 * dq [B, nh, T, dp] = c dS k, dk [B, nkv, T, dp] = c dS^T q, dv = P^T dO (f32; c = scale, or ln 2 with log2_scores;
 * GQA: the query heads of a group accumulate into their shared key / value head; padded head dims written as 0).
 * o / d_o: the attention output and its gradient in the [B*T, ld] layout of p2t_attention's `out`.
 * D_scratch: f32 [B, nh, T].  use_mfma: -1 auto = the MFMA kernels (csrc/attn_bwd_mfma.hip: bf16, log2_scores, head_dim
 * 64 / 128; seven MFMA products per tile pair, no float atomics) where they apply, else the exact kernels; 0 = exact; 1 = require. */
int p2t_attention_backward(const void* q, const void* k, const void* v, const void* o, int64_t ld_o, const void* d_o,
                           int64_t ld_do, const float* lse, const uint8_t* key_mask, const int32_t* kv_info, float* dq,
                           float* dk, float* dv, float* D_scratch, int B, int T, int nh, int nkv, int d, int dp,
                           float scale, int causal, int dtype, int log2_scores, int use_mfma, p2t_stream stream);

/* ---------------------------------------------------------------- ESM2 encoder */
typedef struct {
    int32_t n_layers, hidden, ffn, heads, head_dim, vocab;
    int32_t pad_id, mask_id, token_dropout, emb_layer_norm_before;
    float layer_norm_eps, rope_theta;
    int32_t dtype;                       /* P2T_F32 | P2T_BF16: activations, attention, vectors */
    int32_t gemm_fp8;                    /* 1: the four projections run on the fp8 MFMA kernel (needs dtype BF16): the
                                            matrices are e4m3 bytes with one E8M0 scale per row, see p2t_esm2_layer */
} p2t_esm2_config;

/* Packed per-layer weights (device).  Matrices are `dtype`, row-major [N][ld], ld = K rounded up
 * to 64, zero padded.  qkv_w rows: query (H), key (H), value (H).  Vectors are f32. */
typedef struct {
    const void* qkv_w;  const float* qkv_b;
    const void* o_w;    const float* o_b;
    const float* ln1_w; const float* ln1_b;          /* attention.LayerNorm */
    const void* fc1_w;  const float* fc1_b;          /* intermediate.dense  */
    const void* fc2_w;  const float* fc2_b;          /* output.dense        */
    const float* ln2_w; const float* ln2_b;          /* layer LayerNorm     */
    /* gemm_fp8 only: the four matrices above are then e4m3 bytes, row-major [N][ld], ld = K rounded up to 128 (zero
     * padded), quantised with p2t_quant_rows_fp8, and these are their E8M0 row scales [N] */
    const uint8_t* qkv_ws; const uint8_t* o_ws; const uint8_t* fc1_ws; const uint8_t* fc2_ws;
    /* gemm_fp8, optional (0 = quantise the GELU output in a separate pass): upper bounds of max_n ||fc1_w[n]||_2 (of the
     * weights the GEMM multiplies with, i.e. after quantisation) and of max_n |fc1_b[n]|; with them the FFN-up GEMM writes
     * its GELU output directly as e4m3 under the per-token bound scale of p2t_layernorm_fp8 */
    float fc1_wnorm_bound, fc1_babs_bound;
} p2t_esm2_layer;

typedef struct {
    const void* word_emb;                            /* [vocab][hidden] dtype, unpadded */
    const float* emb_ln_w; const float* emb_ln_b;    /* only if emb_layer_norm_before */
    const p2t_esm2_layer* layers;                    /* HOST array of n_layers structs */
    const float* final_ln_w; const float* final_ln_b;
    const float* inv_freq;                           /* rotary_embeddings.inv_freq f32 [head_dim/2] (a checkpoint
                                                        buffer in HF); NULL = 1/theta^(2j/d) computed on device */
} p2t_esm2_weights;

size_t p2t_esm2_workspace_bytes(const p2t_esm2_config* cfg, int B, int T);
/* ids, mask: int64 [B, T] (right-padded batch contract, dataset/dataloader.py:113-123).
 * out: last_hidden_state, `dtype` [B*T, ld_out] (ld_out >= hidden; pad columns zeroed). */
int p2t_esm2_forward(const p2t_esm2_config* cfg, const p2t_esm2_weights* w, const int64_t* ids,
                     const int64_t* mask, int B, int T, void* out, int64_t ld_out, void* workspace,
                     size_t workspace_bytes, p2t_stream stream);

/* ---------------------------------------------------------------- Llama text tower */
typedef struct {
    int32_t n_layers, hidden, ffn, heads, kv_heads, head_dim, vocab;
    float rms_norm_eps, rope_theta;
    int32_t rope_llama3;                 /* 0 default, 1 llama3 scaling */
    float rope_factor, rope_low_freq_factor, rope_high_freq_factor;
    int32_t rope_original_max_pos;
    int32_t dtype;
    int32_t gemm_fp8;                    /* as p2t_esm2_config.gemm_fp8 */
} p2t_llama_config;

/* qkv_w rows: q (heads*d), k (kv*d), v (kv*d); for head_dim 128 the 128 rows of EVERY head are stored in the order
 * 0..31, 64..95, 32..63, 96..127 (the rotary partners j, j+64 then sit 32 rows apart inside a 64-row block, which is what
 * the fused QKV + RoPE epilogue pairs up); natural order for every other head_dim.  gu_w: gate/up interleaved in blocks of 32 rows
 * (rows 64j..64j+31 = gate features 32j.., rows 64j+32..64j+63 = up features 32j..).  No biases. */
typedef struct {
    const void* qkv_w; const void* o_w; const void* gu_w; const void* down_w;
    const float* ln1_w;                              /* input_layernorm */
    const float* ln2_w;                              /* post_attention_layernorm */
    const uint8_t* qkv_ws; const uint8_t* o_ws; const uint8_t* gu_ws; const uint8_t* down_ws;   /* gemm_fp8: E8M0 row scales */
    /* Qwen3 (both or neither): self_attn.q_norm / k_norm weights, f32 [head_dim] -- RMSNorm over head_dim of every query /
     * key head after the projection and before the rotation (HF Qwen3Attention.forward).  qkv_w rows are then in natural order. */
    const float* q_norm_w; const float* k_norm_w;
} p2t_llama_layer;

typedef struct {
    const void* embed;                               /* [vocab][hidden] dtype */
    const p2t_llama_layer* layers;                   /* HOST array, at least the first k layers */
    const float* final_norm_w;
    const float* inv_freq;                           /* f32 [head_dim/2] or NULL = computed from the config */
} p2t_llama_weights;

size_t p2t_llama_workspace_bytes(const p2t_llama_config* cfg, int B, int T);
/* hidden_states[k]: residual stream after k layers (k < n_layers) or the post-norm output (k == n_layers).
 * out: f32 [B*T, hidden]. */
int p2t_llama_hidden_forward(const p2t_llama_config* cfg, const p2t_llama_weights* w, const int64_t* ids,
                             const int64_t* mask, int B, int T, int k, float* out, void* workspace,
                             size_t workspace_bytes, p2t_stream stream);

/* Same tower from caller-supplied layer-0 inputs (f32 [B*T, hidden]) instead of token ids: the decoder half of
 * Esm2LlamaInstructForCausalLM.forward, models/modeling_esm2llama_instruct.py:204-215 (`inputs_embeds=...`). */
int p2t_llama_hidden_forward_embeds(const p2t_llama_config* cfg, const p2t_llama_weights* w, const float* inputs_embeds,
                                    const int64_t* mask, int B, int T, int k, float* out, void* workspace,
                                    size_t workspace_bytes, p2t_stream stream);
/* llama_decoder.get_input_embeddings()(input_ids), models/modeling_esm2llama_instruct.py:134: f32 [n_tokens, hidden]. */
int p2t_llama_embed_tokens(const p2t_llama_config* cfg, const p2t_llama_weights* w, const int64_t* ids, int64_t n_tokens,
                           float* out, p2t_stream stream);

/* ---------------------------------------------------------------- decoder inputs + LM loss (SFT forward) */
/* Flat positions, in array order, of the elements with value == match (mode 0) or value != 0 (mode 1): the order in
 * which torch's boolean-mask indexing enumerates them (`input_ids == placeholder_id`, `encoder_attention_mask.bool()`,
 * models/modeling_esm2llama_instruct.py:136-137).  pos: int32 [n] (capacity), count: int32 [1]; both on the device. */
int p2t_positions_where(const int64_t* values, int64_t n, int mode, int64_t match, int32_t* pos, int32_t* count,
                        p2t_stream stream);
/* dst[dst_pos[r], :H] = src[src_pos[r], :H] for r < min(*n_dst, *n_src)  (`inputs_embeds[placeholder_mask] =
 * encoder_hidden_states[encoder_mask]`, :138).  dst f32, src `src_dtype`; counts are read on the device (no host sync;
 * the caller compares them afterwards to raise torch's shape-mismatch error). */
int p2t_scatter_rows(float* dst, int64_t ld_dst, const int32_t* dst_pos, const void* src, int64_t ld_src, int src_dtype,
                     const int32_t* src_pos, const int32_t* n_dst, const int32_t* n_src, int64_t max_rows, int H,
                     p2t_stream stream);
/* HF causal-LM loss (transformers loss_utils.ForCausalLMLoss as called by LlamaForCausalLM.forward with labels): logits
 * `dtype` [B*T, ld >= V]; position (b, t) predicts labels[b, t+1]; targets equal to ignore_index (and out-of-range ones)
 * are skipped; loss = mean over the rest in f32 (NaN when there is none).  row_loss f32 [B*T], row_valid int32 [B*T]
 * are outputs as well (deterministic two-stage reduction); count may be NULL. */
int p2t_cross_entropy_shifted(const void* logits, int64_t ld, int dtype, const int64_t* labels, int B, int T, int V,
                              int64_t ignore_index, float* row_loss, int32_t* row_valid, float* loss, int32_t* count,
                              p2t_stream stream);

/* ---------------------------------------------------------------- stage-2 training through the frozen decoder */
/* The reference's stage-2 step is `loss = model(**batch).loss; loss.backward()` (scripts/train_instruct.py:192-213) on
 * Esm2LlamaInstructForCausalLM.forward (models/modeling_esm2llama_instruct.py:195-215).  With the decoder frozen the
 * backward is a chain of dX operations from the LM loss to `inputs_embeds`, whose placeholder rows are the adapter's
 * outputs (:138) -- the adapter is then differentiated by p2t_adapter_backward.  No LoRA matrices yet.
 *
 * d loss / d logits of p2t_cross_entropy_shifted (count: its device-side counter): rows with a counted target get
 * (softmax - onehot) / count, all others 0; d_logits `dtype` [B*T, ld_d >= V], columns V .. next multiple of 64 zeroed
 * (the K padding of the LM-head dX GEMM). */
int p2t_cross_entropy_shifted_backward(const void* logits, int64_t ld, int dtype, const int64_t* labels, int B, int T,
                                       int V, int64_t ignore_index, const int32_t* count, void* d_logits, int64_t ld_d,
                                       p2t_stream stream);
/* LlamaRMSNorm backward (modeling_llama.py:62-67): dx (+)= r (w dy) - x r^3 mean(w dy x), r = rsqrt(mean(x^2) + eps);
 * x, dx f32, dy `dy_dtype` (F32 / BF16); accumulate != 0 adds into dx (the residual-stream gradient). */
int p2t_rmsnorm_backward(const float* x, int64_t ld_x, const float* w, float eps, const void* dy, int64_t ld_dy,
                         int dy_dtype, float* dx, int64_t ld_dx, int64_t rows, int64_t cols, int accumulate,
                         p2t_stream stream);
/* Pieces of the stage-2 step exposed one by one, for the LoRA form of that step (scripts/train_instruct.py:146-183; p2t_hip/
 * decoder_train.py drives them per layer -- the low-rank branches sit BETWEEN the fused blocks of p2t_llama_train_forward):
 * SwiGLU on the interleaved gate / up pre-activations of p2t_llama_layer.gu_w (64-column block j = gate[32 j..] | up[32 j..]):
 * d_act == NULL: out[m, f] = silu(g) u (out `dtype` [M, ld_out >= F], zeros up to the next multiple of 64);
 * else the backward: out = d_gu in the same interleaved layout [M, 2F] from d_act [M, ld_da]. */
int p2t_swiglu_gu(const void* gu, int64_t ld_gu, const void* d_act, int64_t ld_da, void* out, int64_t ld_out, int64_t M, int64_t F,
                  int dtype, p2t_stream stream);
/* Backward of the head split + rotation (+ q_scale folded into q) of p2t_qkv_post: dq [B, nh, T, dp], dk, dv [B, nkv, T, dp] f32
 * -> d_qkv `dtype` [B*T, ld], rows = [q heads | k heads | v heads] in the natural order of q_proj / k_proj / v_proj.
 * cos_sin_scratch f32 [T * d]. */
int p2t_rope_backward_pack(const float* dq, const float* dk, const float* dv, const float* inv_freq, float* cos_sin_scratch,
                           void* d_qkv, int64_t ld, int B, int T, int nh, int nkv, int d, int dp, float q_scale, int dtype,
                           p2t_stream stream);
/* dst[m, c] (+)= keep(seed, m K + c) ? src[m, c] / (1 - p) : 0, c < K (F32 / BF16 either side): the input dropout of a LoRA
 * branch (`lora_dropout`) and, called again with the same seed on the gradient, its backward -- the mask is the counter-hash
 * of (seed, element), regenerated, never stored.  p == 0: a (converting, optionally accumulating) copy. */
int p2t_dropout_rows(const void* src, int src_dtype, int64_t ld_src, void* dst, int dst_dtype, int64_t ld_dst, int64_t M,
                     int64_t K, float p, uint64_t seed, int accumulate, p2t_stream stream);
/* G[c, j] = sum over m < M of X'[m, c] U[m, j], c < C, j < R: the weight gradients of a LoRA branch y = W x + (alpha / r) B (A drop(x))
 * (reference scripts/train_instruct.py:146-183, LoraConfig(r, lora_alpha, lora_dropout); p2t_hip/lora_linear.py LoraLinear.backward:
 * dB = dy^T u with X = dy, U = u = drop(x) A^T; dA = du^T drop(x) with X = x, U = du = dy (s B), stored transposed), summed over
 * the token axis as the activations lie in memory -- no transposed copies, no dropped copy of x.  X [M, ld_x], U [M, ld_u]:
 * `dtype` (F32 | BF16), row-major, tokens are rows.  X' = X for p == 0, else p2t_dropout_rows' keep(seed, m C + c) ? X / (1 - p)
 * : 0 rounded to `dtype`, computed on the fly.  G: f32, [C, ld_g] for transposed == 0, [R, ld_g] (G[j, c]) otherwise; exactly
 * C R elements are written.  BF16: MFMA with fp32 accumulation, C % 8 == 0 and ld_x % 8 == 0; F32: FMA, any C.  M >= 1,
 * 1 <= R <= 64.  The token axis is split over workgroups; partial sums go to `workspace` (f32 [splits, C, R], at least
 * p2t_lora_wgrad_workspace_bytes(C, R, M) bytes: splits C R 4; 0 for arguments out of range) and are added in split order:
 * no atomics, the same bits every run.  Anything else: P2T_ERR_ARG before any GPU call. */
size_t p2t_lora_wgrad_workspace_bytes(int64_t C, int64_t R, int64_t M);
int p2t_lora_wgrad(const void* X, int64_t ld_x, const void* U, int64_t ld_u, int dtype, float* G, int64_t ld_g, int transposed,
                   int64_t M, int64_t C, int64_t R, float p, uint64_t seed, void* workspace, size_t workspace_bytes,
                   p2t_stream stream);
/* dst[dst_pos[r], :H] = src[src_pos[r], :H], r < min(*n_dst, *n_src), f32: the backward of p2t_scatter_rows (the
 * gradient of `inputs_embeds[placeholder_mask] = encoder_hidden_states[encoder_mask]` with respect to the encoder
 * states: call it with the two position lists swapped; rows not listed keep their contents -- zero dst first). */
int p2t_gather_rows_f32(float* dst, int64_t ld_dst, const int32_t* dst_pos, const float* src, int64_t ld_src,
                        const int32_t* src_pos, const int32_t* n_dst, const int32_t* n_src, int64_t max_rows, int H,
                        p2t_stream stream);
/* ---- LM loss over the target rows only (p2t_hip/lm_head.py; the reference's stage-2 loops read `.loss` alone, scripts/
 * train_instruct.py:192-213, 313-349).  The three calls share one row list; none reads anything on the host.
 *
 * The rows (b, t), as flat indices b T + t in array order, whose labels[b, t+1] is a counted target by p2t_cross_entropy_shifted's
 * rule (t + 1 < T, label != ignore_index, 0 <= label < V): rows int32 [cap], targets int32 [cap] (those labels), count int32 [2] =
 * {n, overflow}.  n is the number of such rows whatever cap is; overflow = 1 when n > cap, and then only the first cap are
 * listed.  Entries min(n, cap) .. cap of rows and targets are -1.  B T < 2^31. */
int p2t_lm_target_rows(const int64_t* labels, int B, int T, int V, int64_t ignore_index, int cap, int32_t* rows, int32_t* targets,
                       int32_t* count, p2t_stream stream);
/* One chunk of LM-head logits, `dtype` (F32 | BF16) [R, ld], IN PLACE; ld a multiple of 64 with ld >= V, 16-byte aligned.  Row r
 * of the chunk is entry first + r of the list (first + R <= cap).  For an entry below count[0] with a target y:
 *   row_loss[first + r] = logsumexp(x[:V]) - x[y]                    (from the stored values, as p2t_cross_entropy_shifted reads them)
 *   x[c] <- (exp(x[c] - logsumexp) - [c == y]) s_r  for c < V, 0 for V <= c < ld (whatever those columns held)
 * with s_r = 1 / count[0] (weights == NULL: the token mean) or weights[rows[.] + 1] (f32 [n_weights] = [B T], aligned with the
 * labels as in p2t_cross_entropy_shifted_weighted).  Every other row (at or beyond count[0], target -1) becomes all 0 with
 * row_loss 0.  with_grad == 0: row_loss only, the logits are left as they are.  One workgroup per row, two streaming passes,
 * fixed-order reductions: the same bits every run. */
int p2t_lm_loss_grad_rows(void* logits, int64_t ld, int dtype, int R, int V, const int32_t* rows, const int32_t* targets,
                          const int32_t* count, int first, int cap, const float* weights, int64_t n_weights, float* row_loss,
                          int with_grad, p2t_stream stream);
/* loss f32 [1] = sum of row_loss over the first min(count[0], cap) entries / count[0] (NaN when count[0] == 0, as
 * p2t_cross_entropy_shifted), or with weights the sum of weights[rows[i] + 1] row_loss[i]; NaN when count[1] (overflow) is set --
 * a capacity that was too small must not train silently on a subset.  One workgroup, fixed order. */
int p2t_lm_loss_reduce(const float* row_loss, const int32_t* rows, const int32_t* count, int cap, const float* weights,
                       int64_t n_weights, float* loss, p2t_stream stream);
/* Transposed decoder weights for the dX GEMMs, `dtype`, one struct per layer (HOST array): each matrix is the forward
 * weight transposed -- [forward K rows][row stride = forward N rounded up to 64, zero padded] -- built once (the decoder is
 * frozen).  qkv_wT from the NATURAL row order q_proj | k_proj | v_proj (not the packed order of p2t_llama_layer.qkv_w);
 * gu_wT from the interleaved gate / up order of p2t_llama_layer.gu_w. */
typedef struct p2t_llama_layer_t {
    const void* qkv_wT;     /* [hidden, >= (heads + 2 kv_heads) head_dim] */
    const void* o_wT;       /* [heads head_dim, >= hidden] */
    const void* gu_wT;      /* [hidden, >= 2 ffn] */
    const void* down_wT;    /* [ffn, >= hidden] */
} p2t_llama_layer_t;
/* Bytes of the activation "tape" one training forward writes and the backward reads (all n_layers: residual streams
 * before / inside every layer, rotated heads, attention outputs and log-sum-exps, gate / up pre-activations -- about
 * 170 KB per token and layer for Llama-3.1-8B: sized for 288 GB of HBM, nothing is recomputed), and of the transient
 * workspace both calls share. */
size_t p2t_llama_tape_bytes(const p2t_llama_config* cfg, int B, int T);
size_t p2t_llama_train_workspace_bytes(const p2t_llama_config* cfg, int B, int T);
/* p2t_llama_hidden_forward_embeds(k = n_layers) that also fills the tape.  out: f32 [B*T, hidden], post final RMSNorm. */
int p2t_llama_train_forward(const p2t_llama_config* cfg, const p2t_llama_weights* w, const float* inputs_embeds,
                            const int64_t* mask, int B, int T, float* out, void* tape, size_t tape_bytes, void* workspace,
                            size_t workspace_bytes, p2t_stream stream);
/* d_out: f32 [B*T, hidden] = d loss / d (post-norm hidden states), e.g. d_logits . lm_head.  d_inputs_embeds: f32
 * [B*T, hidden], overwritten.  The fp32 residual-stream gradient is accumulated in place in d_inputs_embeds; GEMM
 * operands are `dtype`; dtype BF16 uses the MFMA GEMMs, F32 the exact kernels (parity mode). */
int p2t_llama_train_backward(const p2t_llama_config* cfg, const p2t_llama_weights* w, const p2t_llama_layer_t* wT,
                             const int64_t* mask, int B, int T, const float* d_out, const void* tape, size_t tape_bytes,
                             float* d_inputs_embeds, void* workspace, size_t workspace_bytes, p2t_stream stream);


/* ---------------------------------------------------------------- packed rows (stage 2 on padding-free batches) */
/* A packed row is a right-padded row (attention mask 1...1 0...0) whose position_ids are runs 0, 1, 2, ...: every position 0
 * under the mask starts a new DOCUMENT (transformers' DataCollatorWithFlattening convention).  Token t of the document that
 * starts at s = t - position_ids[t] attends to the keys s <= k <= t, and its rotary angle uses position_ids[t] instead of t.
 * The shifted LM loss never scores a target that starts a document (the caller sets those labels to the ignore index).
 * A packed batch made from the samples of a padded batch gives the same loss and gradients as that batch (RoPE is relative:
 * dropping the left-pad offset only changes rounding).
 *
 * p2t_doc_prepare: position_ids [B, T] (int64 if pos_i64, else int32) and mask int64 [B, T] -> docs int32 [2][B][T]:
 * docs[0][b][t] = the document start of token t, docs[1][b][t] = its end (exclusive); a padding token t is a document of its
 * own (t, t + 1).  Both rows are non-decreasing in t, so a tile's smallest start is that of its first query and its largest
 * end that of its last key: these are the loop bounds of the attention kernels below.  Every start lies in [0, t] and every
 * end in [t + 1, T] whatever the input.  flags int32 [1] (device, zeroed here): bit 0 = malformed (mask not a prefix, or
 * position_ids under the mask not runs from 0), bit 1 = position_ids is not arange(T) in every row (bit 1 clear: the batch
 * is an ordinary one, run it without documents).  A caller must not pass docs with bit 0 set. */
int p2t_doc_prepare(const void* position_ids, int pos_i64, const int64_t* mask, int B, int T, int32_t* docs, int32_t* flags,
                    p2t_stream stream);
/* p2t_qkv_post with the rotation of token t at position t - docs[0][b][t]. */
int p2t_qkv_post_docs(const void* qkv, int64_t ldq, const float* inv_freq, float* cos_sin_scratch, const int32_t* docs, void* q,
                      void* k, void* v, int B, int T, int nh, int nkv, int d, int dp, float q_scale, int dtype, p2t_stream stream);
/* p2t_rope_backward_pack with the same positions. */
int p2t_rope_backward_pack_docs(const float* dq, const float* dk, const float* dv, const float* inv_freq, float* cos_sin_scratch,
                                const int32_t* docs, void* d_qkv, int64_t ld, int B, int T, int nh, int nkv, int d, int dp,
                                float q_scale, int dtype, p2t_stream stream);
/* Causal attention confined to documents (p2t_attention with causal = 1 and key >= docs[0][b][query]); lse keeps its meaning.
 * The MFMA kernel's key loop of a 128-query tile starts at the 64-key block holding the tile's first start: whole blocks before
 * it are skipped, only the blocks that straddle a boundary are masked per element.  use_mfma as p2t_attention, except that
 * the hand-placed kernel (3) has no documents. */
int p2t_attention_docs(const void* q, const void* k, const void* v, const uint8_t* key_mask, const int32_t* kv_info,
                       const int32_t* docs, void* out, int64_t ld_out, int B, int T, int nh, int nkv, int d, int dp, float scale,
                       int dtype, int use_mfma, int log2_scores, float* lse, p2t_stream stream);
/* Its backward (p2t_attention_backward, causal): the dk / dv kernels end the query loop of a key tile at the tile's last
 * document end.  GQA sums stay atomic-free. */
int p2t_attention_backward_docs(const void* q, const void* k, const void* v, const void* o, int64_t ld_o, const void* d_o,
                                int64_t ld_do, const float* lse, const uint8_t* key_mask, const int32_t* kv_info,
                                const int32_t* docs, float* dq, float* dk, float* dv, float* D_scratch, int B, int T, int nh,
                                int nkv, int d, int dp, float scale, int dtype, int log2_scores, int use_mfma, p2t_stream stream);
/* p2t_llama_train_forward / _backward on packed rows (docs from p2t_doc_prepare, caller-owned; the tape and workspace sizes
 * are those of the unpacked calls).  The QKV projection is stored and rotated by p2t_qkv_post's positional form instead of
 * the fused rotary epilogue. */
int p2t_llama_train_forward_docs(const p2t_llama_config* cfg, const p2t_llama_weights* w, const float* inputs_embeds,
                                 const int64_t* mask, const int32_t* docs, int B, int T, float* out, void* tape, size_t tape_bytes,
                                 void* workspace, size_t workspace_bytes, p2t_stream stream);
int p2t_llama_train_backward_docs(const p2t_llama_config* cfg, const p2t_llama_weights* w, const p2t_llama_layer_t* wT,
                                  const int64_t* mask, const int32_t* docs, int B, int T, const float* d_out, const void* tape,
                                  size_t tape_bytes, float* d_inputs_embeds, void* workspace, size_t workspace_bytes,
                                  p2t_stream stream);
/* Per-target loss weights: p2t_cross_entropy_shifted with loss = sum of weights[b, t+1] * ce(b, t) over the counted targets
 * (weights f32 [B, T], aligned with labels; count still counts the targets), and its backward
 * d_logits[b, t] = weights[b, t+1] (softmax - onehot).  Per-document weights 1 / (n_docs * n_supervised(doc)) give the mean of
 * the per-sample losses: the reference's batch_size_per_device = 1 recipe on packed rows. */
int p2t_cross_entropy_shifted_weighted(const void* logits, int64_t ld, int dtype, const int64_t* labels, const float* weights,
                                       int B, int T, int V, int64_t ignore_index, float* row_loss, int32_t* row_valid, float* loss,
                                       int32_t* count, p2t_stream stream);
int p2t_cross_entropy_shifted_weighted_backward(const void* logits, int64_t ld, int dtype, const int64_t* labels,
                                                const float* weights, int B, int T, int V, int64_t ignore_index, void* d_logits,
                                                int64_t ld_d, p2t_stream stream);
/* ---------------------------------------------------------------- ModalityAdapter */
typedef struct {
    int32_t input_dim, intermediate_dim, output_dim;
    float dropout_p;                     /* 0 in eval */
    uint64_t dropout_seed;
    int32_t dtype;
} p2t_adapter_config;

typedef struct {                          /* matrices `dtype` [N][ld = K up to 64]; biases f32 */
    const void* fc1_w; const float* fc1_b; const void* fc2_w; const float* fc2_b;
} p2t_adapter_weights;

/* Activation buffers (caller-allocated, M = rows): z1,h1 [M, ld(intermediate)], z2,g2 [M, ld(output)] `dtype`,
 * ld(n) = n rounded up to 64; inv_norm f32 [M].  h1 and g2 are always required (they are the forward's
 * intermediates); z1, z2, inv_norm may be NULL for inference and are required by p2t_adapter_backward. */
typedef struct { void* z1; void* h1; void* z2; void* g2; float* inv_norm; } p2t_adapter_saved;

/* x `dtype` [M, ld_x] -> y `dtype` [M, ld(output_dim)], rows L2-normalised. */
int p2t_adapter_forward(const p2t_adapter_config* cfg, const p2t_adapter_weights* w, const void* x, int64_t ld_x,
                        int64_t M, void* y, const p2t_adapter_saved* save, p2t_stream stream);
size_t p2t_adapter_backward_workspace_bytes(const p2t_adapter_config* cfg, int64_t M);
/* dy f32 [M, output_dim] -> f32 gradients (accumulated if accumulate != 0): d_fc1_w [I, input_dim],
 * d_fc1_b [I], d_fc2_w [O, I], d_fc2_b [O] (unpadded, contiguous). */
int p2t_adapter_backward(const p2t_adapter_config* cfg, const p2t_adapter_weights* w, const void* x, int64_t ld_x,
                         int64_t M, const p2t_adapter_saved* saved, const float* dy, float* d_fc1_w, float* d_fc1_b,
                         float* d_fc2_w, float* d_fc2_b, int accumulate, void* workspace, size_t workspace_bytes,
                         p2t_stream stream);

/* The same backward carried to the adapter's input (stage 2 with LoRA on the encoder): d_x f32 [M, ld_dx] (+)= d loss / d x
 * (accumulate != 0 adds), with both dropout masks and the L2-normalisation exactly as p2t_adapter_backward applies them.
 * fc1_w / fc2_w as p2t_adapter_forward reads them; saved->z1, z2, g2 and inv_norm are required. */
size_t p2t_adapter_backward_dx_workspace_bytes(const p2t_adapter_config* cfg, int64_t M);
int p2t_adapter_backward_dx(const p2t_adapter_config* cfg, const p2t_adapter_weights* w, int64_t M, const p2t_adapter_saved* saved,
                            const float* dy, float* d_x, int64_t ld_dx, int accumulate, void* workspace, size_t workspace_bytes,
                            p2t_stream stream);

/* ---------------------------------------------------------------- stage 2 through the ESM2 encoder (LoRA on its projections) */
/* The embedding rows of p2t_esm2_forward (token dropout: <mask> rows zeroed, rows scaled by emb_scale of p2t_mask_prepare,
 * then multiplied by the attention mask): x f32 [B*T, H]. */
int p2t_esm2_embed(const int64_t* ids, const int64_t* mask, const void* table, int dtype, const float* emb_scale, int B, int T, int H,
                   int vocab, int mask_id, int token_dropout, float* x, p2t_stream stream);
/* torch.nn.LayerNorm backward with frozen weight and bias (modeling_esm.py:420-439, 517-521, 552-553): with xhat = (x - mu) r,
 * r = rsqrt(var + eps), dx (+)= r (w dy - mean(w dy) - xhat mean(w dy xhat)).  x, dx f32, dy `dy_dtype` (F32 / BF16); cols and the
 * strides multiples of 4; accumulate != 0 adds into dx (the residual-stream gradient). */
int p2t_layernorm_backward(const float* x, int64_t ld_x, const float* w, float eps, const void* dy, int64_t ld_dy, int dy_dtype,
                           float* dx, int64_t ld_dx, int64_t rows, int64_t cols, int accumulate, p2t_stream stream);
/* GELU (erf) on a pre-activation the caller has assembled (a frozen GEMM plus a LoRA branch, which P2T_EPI_GELU cannot see):
 * dy == NULL: out = gelu_erf(z); else out = dy * gelu_erf'(z).  [M, N] at the given strides, each of z / dy / out F32 or BF16;
 * columns N up to min(ld_out, N rounded up to 64) - 1 of out are written as zeros (the K padding of the next GEMM). */
int p2t_gelu_rows(const void* z, int z_dtype, int64_t ld_z, const void* dy, int dy_dtype, int64_t ld_dy, void* out, int out_dtype,
                  int64_t ld_out, int64_t M, int64_t N, p2t_stream stream);

/* ---------------------------------------------------------------- readout / normalise / loss */
/* emb [B, T, ld] (`dtype`, or f32), mask int64 [B, T] (NULL = all ones) -> out f32 [B, D] (mean/std/last)
 * or [B, 2D] (mix).  D and ld must be multiples of 4 (vector loads). */
int p2t_readout(const void* emb, int dtype, int64_t ld, const int64_t* mask, int B, int T, int D, int mode,
                float* out, p2t_stream stream);
/* d_out f32 [B, D or 2D] -> d_emb f32 [B, T, D]. */
int p2t_readout_backward(const void* emb, int dtype, int64_t ld, const int64_t* mask, int B, int T, int D, int mode,
                         const float* pooled, const float* d_out, float* d_emb, p2t_stream stream);
/* y = x / max(||x||, eps) per row; inv_norm (optional) f32 [rows]. */
int p2t_l2norm_rows(const float* x, float* y, float* inv_norm, int64_t rows, int64_t cols, float eps,
                    p2t_stream stream);
int p2t_l2norm_rows_backward(const float* x, const float* dy, float* dx, int64_t rows, int64_t cols, float eps,
                             p2t_stream stream);
/* Row-wise InfoNCE of `seg` [S, D] against `batch` [N, D] (both f32, L2-normalised), labels i32 [S]:
 * loss_out[0] (+)= weight * mean_i( logsumexp_j(l_ij) - l_i,label_i ), l = seg batch^T / temperature.
 * logits f32 [S, N] and row_loss f32 [S] are outputs / scratch (required). */
int p2t_infonce_forward(const float* seg, const float* batch, const int32_t* labels, int S, int N, int D,
                        float temperature, float weight, int accumulate, float* loss_out, float* logits,
                        float* row_loss, p2t_stream stream);
/* d_seg f32 [S, D] = weight * d loss / d seg, from the logits the forward wrote. */
int p2t_infonce_backward(const float* batch, const int32_t* labels, const float* logits, int S, int N, int D,
                         float temperature, float weight, float* d_seg, p2t_stream stream);

/* Optional column (text -> protein) term -- not in the reference loop, which is row-only (train_contrast.py:94-114);
 * its arithmetic is the reference's own BatchInfoNCELoss with the arguments swapped (:72-91), i.e.
 * F.cross_entropy(logits^T, arange).  p_all, t_all: f32 [N, D], the L2-normalised protein / text embeddings of the GLOBAL
 * batch (all-gathered), positives on the diagonal.  col_lse[j] = logsumexp_i(l_ij) for every column j (output, f32 [N]);
 * loss_out[0] (+)= weight * mean of (col_lse_j - l_jj) over `count` columns: j = cols[i] (i32 [count], device) when cols is
 * given, else j = first .. first+count-1 (this rank's / this segment's own columns).
 * scratch_logits f32 [N, N], scratch_col_loss f32 [N]. */
int p2t_infonce_col_forward(const float* p_all, const float* t_all, int N, int D, float temperature, const int32_t* cols,
                            int first, int count, float weight, int accumulate, float* loss_out, float* col_lse,
                            float* scratch_logits, float* scratch_col_loss, p2t_stream stream);
/* Gradient of sum_j (col_lse_j - l_jj) with respect to the S protein rows whose row logits [S, N] the row forward wrote:
 * d_seg[i] (+)= scale / temperature * sum_j (exp(l_ij - col_lse_j) - [j == labels_i]) t_all[j]. */
int p2t_infonce_col_backward(const float* t_all, const int32_t* labels, const float* logits, const float* col_lse, int S,
                             int N, int D, float temperature, float scale, int accumulate, float* d_seg, p2t_stream stream);

/* ---------------------------------------------------------------- generation: KV cache, prefill, decode steps */
/* What `llama_decoder.generate(inputs_embeds=..., attention_mask=..., **kwargs)` runs under
 * Esm2LlamaInstructForCausalLM.generate (models/modeling_esm2llama_instruct.py:217-251): HF GenerationMixin over the cached
 * LlamaAttention path.  Here: the prompt rows are compacted (valid tokens first: positions 0..len-1 = HF's
 * cumsum(attention_mask) - 1 on the tokens under the mask), one prefill writes the PROMPT segment of the cache, and every
 * decode step appends one token per row to the GENERATED segment.  BB = B0 * group rows generate in lock-step (group = beams
 * per prompt; the beams of a prompt share its prompt segment).  All buffers are the caller's; capacities Tp and G are
 * multiples of 64; dp = head_dim rounded up to 32 / 64 / 128.  Keys are stored after the rotation, values transposed. */
typedef struct {
    void* k_prompt;  void* vt_prompt;   /* `dtype` [n_layers][B0][kv_heads][Tp][dp]  /  [n_layers][B0][kv_heads][dp][Tp] */
    void* k_gen;     void* vt_gen;      /* `dtype` [n_layers][BB][kv_heads][G][dp]   /  [n_layers][BB][kv_heads][dp][G]  */
    const int32_t* prompt_len;          /* device i32 [B0]: valid prompt tokens per row (p2t_compact_rows' lens) */
    int32_t* step;                      /* device i32 [1]: generated tokens already in the cache; a decode step appends at
                                           index step[0], attends to prompt_len + step[0] + 1 keys and increments it last */
    int32_t B0, group, Tp, G;
    /* fp8 prompt segment (bf16 models; opt-in): both NULL = the layouts above.  Both set: k_prompt / vt_prompt hold e4m3 (OCP e4m3fn)
     * BYTES in the same index order -- K codes [n_layers][B0][kv_heads][Tp][dp], V codes [n_layers][B0][kv_heads][dp][Tp] -- and these are
     * one E8M0 scale byte per key for K and one for V, [n_layers][B0][kv_heads][Tp] each.  The scale of a key is chosen over that
     * key's dp features of one kv head by p2t_quant_rows_fp8's rule (the smallest 2^e with amax / 2^e <= 448; byte 127 for an all-zero
     * key; bytes 1 .. 254) and the codes are e4m3_round(x / 2^e), round to nearest even: what p2t_quant_rows_fp8 gives on the same bf16
     * row.  Keys are quantised after the rotation; columns head_dim .. dp are zero codes.  The generated segment stays `dtype`.
     * One set without the other: P2T_ERR_ARG; set on a model that is not bf16: P2T_ERR_UNSUPPORTED. */
    uint8_t* k_prompt_scale;  uint8_t* v_prompt_scale;
} p2t_kv_cache;

/* Stable partition of every row by its mask: out[b, r] = x[b, t_r] for the r-th token with mask != 0, rows >= lens[b] zero;
 * out_mask[b, r] = r < lens[b].  x, out: f32 [B, T, H] (H % 4 == 0, out != x); scratch: i32 [B * T]. */
int p2t_compact_rows(const float* x, const int64_t* mask, int B, int T, int H, float* out, int64_t* out_mask, int32_t* lens,
                     int32_t* scratch, p2t_stream stream);
size_t p2t_llama_prefill_workspace_bytes(const p2t_llama_config* cfg, int B, int T);
/* All layers over the compacted prompts (mask: prefix masks, as p2t_compact_rows writes them; cache->prompt_len = its lens),
 * every layer's rotated keys / values into the prompt segment; last_hidden f32 [B, hidden] = the post-final-RMSNorm state of
 * each row's LAST valid token (the LM head of the first generated token reads it). */
int p2t_llama_prefill(const p2t_llama_config* cfg, const p2t_llama_weights* w, const float* inputs_embeds, const int64_t* mask,
                      int B, int T, const p2t_kv_cache* cache, float* last_hidden, void* workspace, size_t workspace_bytes,
                      p2t_stream stream);
/* ---- padding-free prefill of ragged prompts (opt-in).  p2t_llama_prefill runs every layer over B x longest tokens; a PACKED prompt
 * batch holds the same prompts back to back in R rows of Tpk tokens, f32 [R, Tpk, hidden]: prompt i occupies tokens start_i ..
 * start_i + len_i - 1 of row row_i in p2t_compact_rows' token order (the r-th token under its mask is position r), position_ids restart
 * at 0 per prompt, the row's mask is a prefix and the tail is padding (one-token documents of p2t_doc_prepare).  Attention and rotation
 * are confined per prompt by docs (the packed rows of stage 2 above); every layer's keys and values are scattered into each prompt's
 * OWN row of the cache's prompt segment, so nothing behind the prefill changes.  The placement `place` is a HOST array i32 [n][3] =
 * (row, start, len), planned from the lengths (generation.plan_prompt_rows) and carried by value in the launch arguments: at most 256
 * prompts per call (beyond: P2T_ERR_UNSUPPORTED).  Every entry point checks it before its launch: rows in [0, R), start >= 0, len >= 1,
 * start + len <= Tpk, no two prompts overlapping in a row. */
/* The first half of p2t_compact_rows alone: index[b * T + t] = r for the r-th token of row b with mask != 0, -1 off the mask; lens[b] =
 * their number.  mask i64 [B, T]; index i32 [B * T], lens i32 [B] (device). */
int p2t_prompt_index(const int64_t* mask, int B, int T, int32_t* index, int32_t* lens, p2t_stream stream);
/* x f32 [B, T, H] (H % 4 == 0, 16-byte aligned) + p2t_prompt_index's index and lens + the placement of its B prompts -> out f32 [R, Tpk,
 * H] (zero off the prompts), out_mask i64 [R, Tpk] (1 under a prompt), position_ids i32 [R, Tpk] (r under a prompt, 0 elsewhere).  One
 * launch, one pass from the original rows with 16-byte loads and stores, every output element written once; no compacted copy in
 * between.  The prompts of a row must lie back to back from token 0 (P2T_ERR_ARG otherwise): the mask is then the prefix that
 * p2t_doc_prepare wants, and docs comes from it.  place[i][2] is lens[i] as the host read it. */
int p2t_pack_rows(const float* x, const int32_t* index, const int32_t* lens, int B, int T, int H, const int32_t* place, int R, int Tpk,
                  float* out, int64_t* out_mask, int32_t* position_ids, p2t_stream stream);
/* ONE layer's rotated keys and values from packed rows into the prompt segment, ONE launch for every prompt: k, v `dtype` [R][kv_heads][Tpk][dp] -> layer `layer` of the cache, K rows [i][kvh][0 .. len_i)[dp],
 * V transposed [i][kvh][dp][0 .. len_i).  grid (64-key tiles of the longest prompt, prompts x kv heads); a tile's source starts at any
 * token of the packed row (a token is dp elements: 16-byte pieces stay aligned), its destination is tile-aligned.  fp32, bf16, and --
 * cache with the scale arrays set -- the fp8 prompt segment: p2t_kv_quant_store's arithmetic on each key, codes and both scale arrays
 * bit-equal to what it writes for the same keys laid out one prompt per row.  Positions >= len_i of a cache row, other layers and
 * other prompts' rows are not written.  cache->B0 == n, len_i <= cache->Tp, buffers 16-byte aligned. */
int p2t_kv_store_packed(const p2t_llama_config* cfg, const p2t_kv_cache* cache, int layer, const void* k, const void* v, int R, int Tpk,
                        const int32_t* place, int n, p2t_stream stream);
size_t p2t_llama_prefill_packed_workspace_bytes(const p2t_llama_config* cfg, int R, int Tpk);
/* p2t_llama_prefill on a packed prompt batch: inputs_embeds / mask as p2t_pack_rows writes them, docs i32 [2][R][Tpk] from
 * p2t_doc_prepare on its position_ids (flags bit 0 clear), cache->B0 == n and cache->prompt_len = the lengths.  last_hidden f32 [n,
 * hidden]: the post-final-RMSNorm state of token start_i + len_i - 1 of row row_i.  The QKV projection is stored and rotated by
 * p2t_qkv_post's positional form (as the packed rows of stage 2), so a model whose padded prefill rotates in the GEMM epilogue
 * differs from it by rounding.  gemm_fp8 models: P2T_ERR_UNSUPPORTED (the packed prefill runs the model-dtype GEMMs).  Every refusal
 * comes before the first launch.
 * FINITE PADDING: the tokens of a packed row that no prompt covers must hold finite embeddings (p2t_pack_rows writes zeros).  A prompt
 * is isolated from what else lies in its row by masks: the attention sets the probability of a key outside the document to an exact
 * zero, and the bf16 kernel then multiplies that zero with the V rows of the whole 64-key tile -- 0 x finite = 0, but 0 x NaN = NaN.
 * Known limit, measured: NaN embeddings behind the last prompt turn every first-token logit of a bf16 model into NaN (the fp32
 * kernels gave the clean run's bits with the same NaN tail); finite junk there changes no bit in either dtype.  The padded
 * prefill's padding tokens are under the same contract. */
int p2t_llama_prefill_packed(const p2t_llama_config* cfg, const p2t_llama_weights* w, const float* inputs_embeds, const int64_t* mask,
                             const int32_t* docs, int R, int Tpk, int n, const int32_t* place, const p2t_kv_cache* cache,
                             float* last_hidden, void* workspace, size_t workspace_bytes, p2t_stream stream);
size_t p2t_llama_decode_workspace_bytes(const p2t_llama_config* cfg, int BB, int Tp, int G);
/* Optional second copies of the four projection weights of a layer in the STREAM order of the decode GEMM (p2t_preshuffle_w;
 * bf16 models; built once per generate-capable model: 288 GB of HBM hold both layouts of an 8-B decoder many times over).
 * w_stream: HOST array of n_layers entries or NULL (the step then streams p2t_llama_layer's own matrices, 64-byte pieces of 16
 * rows per load instead of whole lines: 8-30 % slower per GEMM).  gemm_fp8 models: the p2t_preshuffle_w_fp8 copies of the e4m3
 * matrices (their row scales stay p2t_llama_layer's *_ws). */
typedef struct { const void* qkv_w; const void* o_w; const void* gu_w; const void* down_w; } p2t_llama_layer_stream;
/* One token per row: x f32 [BB, hidden] (the embedding of the token chosen last) through all layers at position
 * prompt_len[row / group] + step[0], its keys / values appended at index step[0], final RMSNorm, LM head
 * (lm_head `dtype` [vocab, ld_head], ld_head >= hidden rounded up to 64, pad zero) -> logits `dtype` [BB, ld_logits]
 * (HF keeps the logits in the model dtype and up-casts the last position to f32: generation/utils.py `_sample`); step[0] += 1.
 * lm_head_preshuffled: lm_head is the p2t_preshuffle_w copy (ld_head ignored).
 * Every length is read on the device: the call can be captured into a HIP graph and replayed. */
enum { P2T_DECODE_NO_ROPE_FUSION = 1 };     /* flags: run the QKV projection and the rotation + cache append as two launches even where the
                                               fused epilogue applies (bf16, head_dim 64 / 128, no q/k norm): the same arithmetic, bit for bit */
int p2t_llama_decode_step(const p2t_llama_config* cfg, const p2t_llama_weights* w, const p2t_llama_layer_stream* w_stream,
                          const void* lm_head, int64_t ld_head, int lm_head_preshuffled, const p2t_kv_cache* cache,
                          const float* x, void* logits, int64_t ld_logits, int flags, void* workspace, size_t workspace_bytes,
                          p2t_stream stream);
/* Greedy choice with HF's finished-row rule: next[r] = finished[r] ? pad_id : argmax(logits[r, :V]) (lowest index among equal
 * maxima, torch.argmax), out_tokens[r, step[0]] = next[r], finished[r] |= next[r] in eos_ids.  eos_ids i64 [n_eos], finished
 * i32 [BB], next_tokens i64 [BB], out_tokens i64 [BB, ld_tokens >= G]: all on the device. */
int p2t_greedy_select(const void* logits, int dtype, int64_t ld, int V, int BB, const int64_t* eos_ids, int n_eos,
                      int64_t pad_id, int32_t* finished, int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens,
                      const int32_t* step, int G, p2t_stream stream);
/* Choice by sampling, with p2t_greedy_select's arguments and bookkeeping (a finished row emits pad_id, out_tokens[r, clamp(step[0],
 * 0, G - 1)] = next[r], finished[r] |= next[r] in eos_ids; the token is always in [0, V)): HF's TemperatureLogitsWarper ->
 * TopKLogitsWarper -> TopPLogitsWarper and one multinomial draw per row, all in f32 on the stored logits of columns [0, V)
 * (columns V .. ld are never read).  temperature > 0; top_k: 0 = off, else 1 .. 1024; top_p: >= 1 = off, else in (0, 1).
 * Supported: top_k on (top_p on or off), and both off; top_p on without top_k needs a sort of the whole vocabulary:
 * P2T_ERR_UNSUPPORTED.  Per row r:
 *   x_c = float(logit_c) / temperature (a division).  kth = the min(top_k, V)-th largest x; every c with x_c >= kth survives,
 *   ties at kth included.  The survivor table holds 2048: beyond that, all x_c > kth and the ties at kth in ascending column order
 *   until it is full, and bit 0 of *flags is set (>= 1025 exact ties).  Ranks: value descending, column ascending among equal
 *   values.  e_j = exp(x_j - x_0); rank j is kept iff sum_{i >= j} e_i > (1 - top_p) sum_i e_i, rank 0 always (min_tokens_to_keep
 *   1).  Draw: h = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ (uint64)(row0 + r)) ^ (uint64)(int64)step[0]) (mix64: the
 *   splitmix64 finaliser of p2t_fill_hash), hash24 = h >> 40, u = (hash24 + 0.5) * 2^-24 rounded to f32; the token is the kept
 *   rank with the smallest j such that sum_{i <= j} e_i > u * (sum of the kept e_i), the last kept rank if rounding leaves none.
 *   Both filters off: the same rule over all V columns in ascending column order.
 * p2t_hip.synth.sample_uniform(seed, row, step) restates the chain.  Rows r of a call draw as global rows row0 + r, and step[0] is
 * the draw's counter: a replayed graph draws fresh numbers.  scores (or NULL): f32 [BB, ld_scores >= V], x_c on the kept columns and
 * -inf elsewhere (HF's processed scores), finished rows included.  flags: one device word, OR-ed into.  No float atomics, fixed
 * reduction orders: the same inputs give the same bits.  Rows holding +inf or NaN in [0, V), or -inf everywhere, are unspecified
 * (the token still lies in [0, V)).  Does not allocate, copy or synchronise: it can be captured into a HIP graph. */
int p2t_sample_select(const void* logits, int dtype, int64_t ld, int V, int BB, const int64_t* eos_ids, int n_eos,
                      int64_t pad_id, int32_t* finished, int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens,
                      const int32_t* step, int G, float temperature, int top_k, float top_p, uint64_t seed, int64_t row0,
                      float* scores, int64_t ld_scores, int32_t* flags, p2t_stream stream);
/* Logits processors in front of p2t_greedy_select / p2t_sample_select: HF's RepetitionPenaltyLogitsProcessor ->
 * NoRepeatNGramLogitsProcessor -> NoBadWordsLogitsProcessor (SuppressTokensLogitsProcessor as words of one token) ->
 * MinNewTokensLengthLogitsProcessor (transformers 5.15, the order of generation/utils.py `_get_logits_processor`), for prompts given as
 * embeddings: HF's input_ids then hold the generated tokens only, and so does the history here.  logits: `dtype` (F32 | BF16)
 * [BB, ld >= V], never written (HF up-casts the last position to f32 before any processor runs); out: f32 [BB, ld_out >= V], which the
 * selectors then read with dtype F32; it must not overlap logits.  Columns V .. ld are never read, columns V .. ld_out never written.
 * Per row r, with cur = clamp(step[0], 0, G) and the history h = out_tokens[r, 0 .. cur) (i64 [BB, ld_tokens >= G]: the columns the
 * selectors wrote, the pad tokens of a finished row included -- harmless, a finished row emits pad whatever its scores are); every
 * value an f32, every stage strictly after the one before, so a later -inf wins; a history or word token outside [0, V) is compared
 * like any other and never written to:
 *   1. y_c = float(logit_c) for c < V.
 *   2. repetition_penalty != 1: for every history token t, y_t = x_t < 0 ? x_t * penalty : x_t / penalty (one IEEE multiplication or
 *      division), x_t the STORED logit: duplicates in the history write the same bits.
 *   3. n = no_repeat_ngram_size > 0 and cur >= n: for every i in [0, cur - n] with h[i .. i + n - 2] equal to the last n - 1 history tokens
 *      h[cur - n + 1 .. cur), y[h[i + n - 1]] = -inf.  n = 1: every history token.
 *   4. word w = word_ids[word_offsets[w] .. word_offsets[w + 1]) of length L (word_ids i64 [n_word_ids], word_offsets i32 [n_words + 1],
 *      ascending; a word whose offsets leave [0, n_word_ids] or are not ascending is skipped): L = 1: y[word] = -inf, always.  L > 1:
 *      applied once cur >= L (HF skips a word "longer than the context", although its L - 1 leading tokens would fit): if they equal the
 *      last L - 1 history tokens, y[last token of w] = -inf.  HF drops a word equal to [eos]; that is the caller's to do.
 *   5. cur < min_new_tokens: y[e] = -inf for each of the n_eos ids (no eos ids: nothing, HF does not install the processor).
 * HF's NoBadWordsLogitsProcessor adds a bias row (0 or -inf) and so turns a stored -0.0 into +0.0; here every column no stage names
 * keeps its stored bits.  One 1024-thread block per row, barriers between the stages, no atomics: the same inputs give the same bits.
 * Does not allocate, copy or synchronise: it can be captured into a HIP graph. */
int p2t_logits_process(const void* logits, int dtype, int64_t ld, int V, int BB, const int64_t* out_tokens, int64_t ld_tokens,
                       const int32_t* step, int G, float* out, int64_t ld_out, float repetition_penalty, int no_repeat_ngram_size,
                       int min_new_tokens, const int64_t* eos_ids, int n_eos, const int64_t* word_ids, const int32_t* word_offsets,
                       int n_words, int n_word_ids, p2t_stream stream);
/* Choice by beam search: one step of transformers' `_beam_search` (5.x, generation/utils.py) with an empty id prompt
 * (decoder_prompt_len 0, max_length = max_new_tokens), for B0 prompts of nb = num_beams rows each (row b nb + j = beam j of prompt b).
 * State, all on the device and the caller's.  Tables and per-beam vectors have TWO halves: a step at cur = step[0] reads half cur & 1
 * and writes half (cur + 1) & 1 (rows move between beams, so they are never updated in place); a fresh state lies in half 0. */
typedef struct {
    int64_t* run_seq;        /* i64 [2][B0][nb][G]  running sequences; columns the search has not reached hold the caller's fill (pad_id) */
    int32_t* run_idx;        /* i32 [2][B0][nb][G]  the global row (b nb + beam) every token of them was continued from; fill -1 */
    float* run_scores;       /* f32 [2][B0][nb]     running scores; fresh: 0 for beam 0, -1e9 for the others */
    int64_t* fin_seq;        /* i64 [2][B0][nb][G]  finished hypotheses, best first */
    int32_t* fin_idx;        /* i32 [2][B0][nb][G]  their beam indices */
    float* fin_scores;       /* f32 [2][B0][nb]     their length-normalised scores; fresh: -1e9 */
    int32_t* is_finished;    /* i32 [2][B0][nb]     1 where a slot holds a finished hypothesis; fresh: 0 */
    int32_t* heuristic_open; /* i32 [B0]            1 while a running beam of the prompt can still beat its worst finished one; fresh: 1 */
    int32_t* done;           /* i32 [2]             {1 once the search has stopped, the number of steps it took}; fresh: 0, 0.  The final
                                                    tables lie in half done[1] & 1 */
    int32_t* sync;           /* i32 [1 + B0]        ticket and per-prompt flags of the stop condition; zeroed once by the caller */
    float* workspace;        /* p2t_beam_workspace_bytes(B0, nb) bytes, carries the candidates from the first launch to the second */
} p2t_beam_state;
size_t p2t_beam_workspace_bytes(int B0, int num_beams);
/* logits: `dtype` (F32 | BF16) [B0 nb, ld >= V], the rows' next-token logits (columns V .. ld are never read).  With cur = step[0],
 * keep = max(2, 1 + n_eos) nb, and every value an f32:
 *   1. per row r: mx = the largest stored logit; S = sum over c < V of expf(x_c - mx), added in a fixed order (1024 threads take the
 *      columns in 16-byte pieces, each adds its own in ascending order; 64 lanes by a butterfly; 16 waves in order); lse = logf(S);
 *      lp_c = (x_c - mx) - lse  (two subtractions, in this order).  scores (or NULL): f32 [B0 nb, ld_scores >= V] = lp, which is what HF
 *      returns as the step's `scores` under beam search.
 *   2. per prompt, candidates (beam j, column c) with acc = lp_c + run_scores[j] (one addition).  The keep best by acc, ranked by
 *      (acc descending, beam ascending, then inside a beam stored logit descending, column ascending): x -> acc is monotone, so this
 *      is the rank key (acc descending, flat index j V + c ascending) wherever two different logits of a beam do not round to the
 *      same acc.  Candidate k of the ranked list: token t_k, beam j_k, acc a_k.
 *   3. hit_k = (cur + 1 >= max_length) or t_k in eos_ids.  live_k = a_k + (hit_k ? -1e9 : -0).  The nb best by (live descending, k
 *      ascending) go on: running row i <- row j_k of half cur & 1 with t_k at column cur, run_idx[.., cur] = b nb + j_k, run_scores[i]
 *      = live_k; next_tokens[b nb + i] = t_k and src_rows[b nb + i] = b nb + j_k (what p2t_kv_reorder takes).
 *   4. just_k = hit_k and k < nb.  fin_k = a_k / float(pow(double(cur + 1), double(length_penalty)))  (an IEEE f32 division), then
 *      fin_k += (all nb slots finished before the step and early_stopping == 1) ? -1e9 : -0; += heuristic_open ? -0 : -1e9;
 *      += just_k ? -0 : -1e9, in this order.  The nb old finished slots followed by the keep candidates are ranked by (score
 *      descending, position ascending); the nb best become the finished slots (sequence, beam indices, score, flag = old flag or
 *      just_k).
 *   5. heuristic_open &= any over finished slots i of run_scores[0] / float(pow(double(len), double(length_penalty))) > (is_finished[i] ?
 *      min over all nb slots of fin_scores : -1e9), len = max_length if early_stopping == 2 ("never") and length_penalty > 0, else cur + 1.
 *   6. the search goes on iff any prompt is open, and not (every slot of every prompt finished and early_stopping == 1), and not every
 *      candidate k of every prompt a hit; otherwise, or when cur + 1 >= max_length, done = {1, cur + 1}.
 * Once done[0] is set (or with cur outside [0, max_length)) a call leaves the state untouched, writes pad_id to next_tokens and the
 * identity to src_rows: replayed steps past the end are harmless.  Supported: 1 <= nb <= 16, keep <= 64, V >= keep, B0 nb V < 2^31;
 * otherwise P2T_ERR_UNSUPPORTED.  Malformed arguments (null pointers, ld < V, non-positive counts, G not a multiple of 64, max_length
 * > G, NaN penalty, early_stopping outside 0 .. 2): P2T_ERR_ARG before any GPU call.  G is the row length of the tables.  Rows holding
 * +inf or NaN in [0, V) are unspecified (every index stays in range).  Two launches, no float atomics, fixed reduction orders: the same
 * inputs give the same bits.  Does not allocate, copy or synchronise: it can be captured into a HIP graph. */
int p2t_beam_select(const void* logits, int dtype, int64_t ld, int B0, int num_beams, int V, const int64_t* eos_ids, int n_eos,
                    int64_t pad_id, float length_penalty, int early_stopping, int max_length, int G, const int32_t* step,
                    const p2t_beam_state* state, int64_t* next_tokens, int64_t* src_rows, float* scores, int64_t ld_scores,
                    p2t_stream stream);
/* Logits processors under beam search: HF's `_beam_search` (transformers 5.15, generation/utils.py) takes log_softmax of the step's
 * logits, runs the processors on THOSE rows with the beam's running sequence as the history, returns the processed rows as the step's
 * `scores` and adds the running scores without renormalising.  This call writes the processed rows; p2t_beam_select_logprobs ranks
 * them.  logits: `dtype` (F32 | BF16) [B0 nb, ld >= V], never written; lp: f32 [B0 nb, ld_lp >= V], must not overlap logits (columns
 * V .. ld are never read, columns V .. ld_lp never written).  Of the state only run_seq and done are read.  The processor settings are
 * p2t_logits_process's.  With cur = step[0]: done[0] != 0 or cur outside [0, max_length): nothing is written.  Otherwise per row r,
 * every value an f32, every stage strictly after the one before:
 *   1. mx, S, lse and lp_c = (x_c - mx) - lse for c < V: step 1 of p2t_beam_select, the same fixed summation order, so the row has the
 *      bits p2t_beam_select writes to its `scores`.
 *   2. - 5.  stages 2 - 5 of p2t_logits_process on that row with the history h = run_seq[cur & 1][r][0 .. cur) (the half is chosen on
 *      the device from step[0]); for prompts given as embeddings that is the generated tokens only.  The penalty's x_t is
 *      (float(logit_t) - mx) - lse, recomputed from the stored logit: y_t = x_t < 0 ? x_t * penalty : x_t / penalty (log-probabilities
 *      are <= 0, so in practice the product), duplicates in the history write the same bits.  A history or word token outside [0, V) is
 *      compared like any other and never written to.
 * Malformed arguments (null pointers, ld < V, ld_lp < V, non-positive counts, G not a multiple of 64, max_length outside 1 .. G, a
 * penalty that is not positive and finite, negative sizes, counts without their arrays): P2T_ERR_ARG before any GPU call; nb > 16 or
 * B0 nb V >= 2^31: P2T_ERR_UNSUPPORTED.  One 1024-thread block per row, barriers between the stages, no atomics: the same inputs give
 * the same bits.  Rows holding +inf or NaN in [0, V) are unspecified (every index stays in range).  Does not allocate, copy or
 * synchronise: it can be captured into a HIP graph. */
int p2t_beam_logprobs_process(const void* logits, int dtype, int64_t ld, int B0, int num_beams, int V, const int32_t* step, int G,
                              int max_length, const p2t_beam_state* state, float repetition_penalty, int no_repeat_ngram_size,
                              int min_new_tokens, const int64_t* eos_ids, int n_eos, const int64_t* word_ids, const int32_t* word_offsets,
                              int n_words, int n_word_ids, float* lp, int64_t ld_lp, p2t_stream stream);
/* p2t_beam_select for rows that ALREADY hold log-probabilities (processed ones: p2t_beam_logprobs_process): lp f32 [B0 nb, ld >= V],
 * never written; state, halves, workspace (p2t_beam_workspace_bytes), `done` behaviour, supported range and argument checks are
 * p2t_beam_select's.  With cur = step[0], keep = max(2, 1 + n_eos) nb, and every value an f32:
 *   2. per prompt, candidates (beam j, column c) with acc = lp_c + run_scores[j] (one addition), lp_c READ from the row.  A processed
 *      row is not a monotone image of the logits, so the rows themselves are ranked: inside a beam by (lp descending, column ascending),
 *      of which the first keep are the beam's candidates; the prompt's keep best of those by (acc descending, beam ascending, then
 *      rank inside the beam ascending).  Candidate k of the ranked list: token t_k, beam j_k, acc a_k.
 *   3. - 6.  steps 3 - 6 of p2t_beam_select on that list, unchanged.
 * Rows may hold -inf (banned columns): they rank like any value, ties by column ascending, whatever their number.  A prompt with fewer
 * than nb finite candidates gets -inf running scores, as in HF; no NaN arises from them (-inf + -1e9 and -inf / len_pow are -inf).
 * Rows holding +inf or NaN in [0, V) are unspecified (every index stays in range).  Two launches, no float atomics: the same inputs
 * give the same bits.  Does not allocate, copy or synchronise: it can be captured into a HIP graph. */
int p2t_beam_select_logprobs(const float* lp, int64_t ld, int B0, int num_beams, int V, const int64_t* eos_ids, int n_eos, int64_t pad_id,
                             float length_penalty, int early_stopping, int max_length, int G, const int32_t* step,
                             const p2t_beam_state* state, int64_t* next_tokens, int64_t* src_rows, p2t_stream stream);
/* Choice by beam sampling: one step of `_beam_search` with do_sample=True (HF's beam-search multinomial sampling), with
 * p2t_beam_select's arguments, state (the same p2t_beam_state, halves and `done`; the workspace holds
 * p2t_beam_sample_workspace_bytes(B0, nb) bytes) and bookkeeping, and the sampler's temperature / top_k / top_p / seed.  HF draws keep
 * continuations per prompt without replacement from softmax(processed log-probabilities + running scores) over nb V candidates
 * (`_get_top_k_continuations`); a draw without replacement is the descending order of score + Gumbel noise, and the noise here is a
 * counter hash per candidate.  With cur = step[0], keep = max(2, 1 + n_eos) nb, and every value an f32:
 *   1. per row: mx, S, lse, lp_c = (x_c - mx) - lse: step 1 of p2t_beam_select, the same fixed summation order.
 *   2. the warpers in HF's order, on the log-probabilities.  y_c = lp_c / temperature (an IEEE division).  top_k: the survivors are the
 *      columns whose STORED logit is >= the min(top_k, V)-th largest stored logit, ties included; x -> y is monotone, so this is HF's
 *      set wherever two different logits do not round to one y.  The table holds 2048: beyond that, all logits above the threshold and
 *      the ties in ascending column order until it is full, and bit 0 of *flags is set.  Ranks: (stored logit descending, column
 *      ascending).  top_p: e_j = expf(y_j - y_0); rank j is kept iff sum_{i >= j} e_i > (1 - top_p) sum_i e_i (ranks added in
 *      ascending order), rank 0 always.  Both filters off: every column is kept.  scores (or NULL): f32 [B0 nb, ld_scores >= V], y_c on
 *      the kept columns and -inf elsewhere: HF's processed scores of the step.
 *   3. a kept candidate (beam j, column c) of prompt b: acc = y_c + run_scores[j] (one addition);
 *      h = mix64(mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ (uint64)(prompt0 + b)) ^ (uint64)(int64)cur) ^ (uint64)(j V + c));
 *      u = (2 (h >> 41) + 1) * 2^-24 (an odd 24-bit integer times 2^-24: exact, strictly inside (0, 1));  g = -logf(-logf(u));
 *      key = acc + g (one addition).  p2t_hip.synth.beam_sample_uniform(seed, prompt, step, flat_index) restates u.
 *   4. the prompt's kept candidates are ranked by (key descending, flat index j V + c ascending); the first keep of them IN THAT ORDER
 *      are HF's keep draws in draw order.  Candidate k of the list: token t_k, beam j_k and a_k = acc, the UNPERTURBED score (HF
 *      gathers the accumulated log-probabilities at the drawn indices).
 *   5. steps 3 - 6 of p2t_beam_select on that list, unchanged: hits and live, the nb best live rows by (live descending, k ascending),
 *      just_k = hit_k and k < nb, the length-normalised merge into the finished slots, the open / closed heuristic, the stop condition,
 *      `done`, pad_id and the identity once stopped (the state is then left alone).
 *   6. bit 1 of *flags is set when a prompt has fewer than keep kept candidates over all its beams, or when a_(keep-1) is not within 100
 *      of the prompt's best acc (max over its beams of y_0 + run_scores[j]): HF's f32 softmax gives such a candidate probability 0
 *      and torch.multinomial fails there.  The results are then unspecified, but every index stays in range and the tables hold no NaN
 *      (-inf scores are possible).
 * temperature > 0 and finite; top_k 0 (off) or 1 .. 1024; top_p >= 1 (off) or in (0, 1); flags: one device word, OR-ed into -- else
 * P2T_ERR_ARG, like p2t_beam_select's malformed arguments, before any GPU call.  top_p on without top_k, and anything outside
 * p2t_beam_select's range (nb <= 16, keep <= 64, V >= keep, B0 nb V < 2^31): P2T_ERR_UNSUPPORTED.  step[0] is the draw's counter: a
 * replayed graph draws fresh numbers.  Rows holding +inf or NaN in [0, V) are unspecified (every index stays in range).  Two launches,
 * no float atomics, fixed reduction orders: the same inputs give the same bits.  Does not allocate, copy or synchronise: it can be
 * captured into a HIP graph. */
size_t p2t_beam_sample_workspace_bytes(int B0, int num_beams);
int p2t_beam_sample_select(const void* logits, int dtype, int64_t ld, int B0, int num_beams, int V, const int64_t* eos_ids, int n_eos,
                           int64_t pad_id, float length_penalty, int early_stopping, int max_length, int G, const int32_t* step,
                           const p2t_beam_state* state, int64_t* next_tokens, int64_t* src_rows, float* scores, int64_t ld_scores,
                           float temperature, int top_k, float top_p, uint64_t seed, int64_t prompt0, int32_t* flags,
                           p2t_stream stream);
/* The decode step's projections on their own: out[M, N] = A[M, K] . W[N, K]^T for M <= 64 rows of bf16 -- a weight stream (every
 * byte of W read once, 8 waves split K per 16 output features, partial sums added in wave order; HBM-bound, not MFMA-bound).
 * K % 32 == 0, lda / ldw multiples of 8, no bias.  epilogue: P2T_EPI_STORE (out_dtype P2T_BF16 or P2T_F32), P2T_EPI_STORE_F32,
 * P2T_EPI_RESID (out f32, += ), P2T_EPI_SWIGLU (W = the gate/up interleave of p2t_llama_layer.gu_w with N = 2 F rows, out bf16
 * [M, F]).  w_preshuffled: W is the p2t_preshuffle_w copy (ldw ignored).  Anything else: P2T_ERR_UNSUPPORTED. */
int p2t_gemm_nt_skinny(const void* A, int64_t lda, const void* W, int64_t ldw, int w_preshuffled, void* out, int64_t ldc, int64_t M,
                       int64_t N, int64_t K, int out_dtype, int epilogue, p2t_stream stream);
/* W bf16 [N, ldw] -> the stream order the decode GEMM reads with whole-line loads: out[((t * K/32 + s) * 64 + lane) * 8 + e] =
 * W[16 t + lane % 16][32 s + 8 (lane / 16) + e], rows N .. next multiple of 16 as zeros; out: bf16 [round_up(N, 16) * K].
 * K % 32 == 0.  Pass the result to p2t_gemm_nt_skinny with w_preshuffled = 1 (same N, K). */
int p2t_preshuffle_w(const void* W, int64_t ldw, int64_t N, int64_t K, void* out, p2t_stream stream);
/* The same stream on e4m3 operands (gemm_fp8 models, section "fp8 GEMMs" of DESIGN.md): A / W e4m3 bytes [rows, K rounded up to 128, zero
 * padded], one E8M0 scale byte per row each (p2t_quant_rows_fp8 / p2t_rmsnorm_fp8 write both for A); v_mfma_scale_f32_16x16x128_f8f6f4.
 * lda / ldw multiples of 16.  p2t_preshuffle_w_fp8: out[(((t * K/128 + s) * 2 + h) * 64 + lane) * 16 + b] = W[16 t + lane % 16][128 s + 64 h
 * + 16 (lane / 16) + b]; out: bytes [round_up(N, 16) * K]. */
int p2t_gemm_nt_skinny_fp8(const void* A, int64_t lda, const uint8_t* a_scale, const void* W, int64_t ldw, const uint8_t* w_scale,
                           int w_preshuffled, void* out, int64_t ldc, int64_t M, int64_t N, int64_t K, int out_dtype, int epilogue,
                           p2t_stream stream);
int p2t_preshuffle_w_fp8(const void* W, int64_t ldw, int64_t N, int64_t K, void* out, p2t_stream stream);

/* ---------------------------------------------------------------- MXFP4 decoder weights (decode step only; DESIGN.md sections 9, 11)
 * Storage (OCP MXFP4): e2m1 codes, two per byte -- the even column in the low nibble -- row-major [N][ld_codes >= Kq / 2] bytes, and one
 * E8M0 scale byte per block of 32 consecutive K columns, dense [N][Kq / 32].  Kq = K rounded up to 128; columns >= K count as zeros.
 * A code is sign (bit 3) | magnitude index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}; the value is that times 2^(scale byte - 127).
 *
 * Scale rule (this project's fp8 rule, not OCP's floor rule: nothing saturates).  For block j of a row, e_j = the smallest integer with
 * amax_j / 2^e_j <= 6; E_row = max_j e_j; then the CLAMP e_j <- max(e_j, E_row - 8).  A zero block gets E_row - 8, an all-zero row the
 * byte 127 everywhere.  The stored byte is 127 + e_j.  (Inputs are finite and, where non-zero, normal f32 magnitudes.)
 * Codes: round-to-nearest onto the grid times 2^e_j, ties to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2,
 * 3.5 -> 4, 5 -> 4); the sign bit is the input's sign (so the sign of a value that rounds to zero is unspecified for a reader).
 *
 * Why the clamp: with it every value of a row is a multiple of 2^(E_row - 9) below 2^(E_row + 3), i.e. e4m3-representable under the
 * ONE row scale p2t_quant_rows_fp8 picks -- p2t_quant_rows_fp8(dequantised row) returns the row bit for bit.  That is what lets the
 * prefill, the cache-less forward and decode beyond 64 rows run the e4m3 kernels on the SAME weights W~ the decode step streams in
 * 4.25 bits.  Without the clamp a block 2^-9 or more below the row maximum falls under the e4m3 grid of the row scale and is rounded.
 * Re-quantising W~ gives W~ back (values; a block whose maximum rounded down to 3 * 2^e may re-quantise at e - 1 to the same values).
 * |w - w~| <= 2^e_j per element (half the widest grid step, 2 * 2^e_j between 4 and 6).
 *
 * p2t_quant_rows_mxfp4: x F32 / BF16 [rows, ld_x] (ld_x % 8 == 0) -> codes [rows, ld_codes] (ld_codes % 16 == 0; bytes [0, Kq / 2) of
 * every row written, nothing behind them) + scales [rows, Kq / 32].  One block per row, two passes.
 * p2t_dequant_rows_mxfp4: -> out bf16 [rows, ld_out], columns [0, cols): exact (two significant bits).
 * p2t_preshuffle_w_mxfp4: the stream copy of the decode GEMM, ONE buffer of round_up(N, 16) / 16 * (K / 128) chunks of 1088 bytes,
 * chunk (t, s) = what one MFMA consumes: byte 16 lane + b = codes[16 t + lane % 16][64 s + 16 (lane / 16) + b] (1024 bytes), then byte
 * 1024 + lane = scales[16 t + lane % 16][4 s + lane / 16] (64 bytes); rows >= N: zero codes, byte 127.  K % 128 == 0 (K = Kq here).
 * p2t_gemm_nt_skinny_mxfp4: p2t_gemm_nt_skinny_fp8 with W in this format -- A e4m3 [M <= 64, lda] + a_scale as there, W codes [N, ldw
 * bytes] + w_block_scale [N, K / 32], or w_preshuffled: W = the stream copy (ldw, w_block_scale ignored).  K % 128 == 0, K >= 128,
 * lda % 16 == 0, ldw % 16 == 0, ldw >= K / 2; same epilogues.  v_mfma_scale_f32_16x16x128_f8f6f4 with an fp4 A operand: lane (r, g)
 * takes the code bytes of the K columns 128 s + 32 g .. + 31, one MX block per lane and step (its scale byte is that lane's scale
 * operand); the e4m3 operand keeps the fp8 form's lane map.  Anything else: P2T_ERR_UNSUPPORTED. */
int p2t_quant_rows_mxfp4(const void* x, int dtype, int64_t ld_x, int64_t rows, int64_t cols, void* codes, int64_t ld_codes,
                         uint8_t* scales, p2t_stream stream);
int p2t_dequant_rows_mxfp4(const void* codes, int64_t ld_codes, const uint8_t* scales, int64_t rows, int64_t cols, void* out,
                           int64_t ld_out, p2t_stream stream);
int p2t_preshuffle_w_mxfp4(const void* codes, int64_t ld_codes, const uint8_t* scales, int64_t N, int64_t K, void* out,
                           p2t_stream stream);
int p2t_gemm_nt_skinny_mxfp4(const void* A, int64_t lda, const uint8_t* a_scale, const void* W, int64_t ldw,
                             const uint8_t* w_block_scale, int w_preshuffled, void* out, int64_t ldc, int64_t M, int64_t N, int64_t K,
                             int out_dtype, int epilogue, p2t_stream stream);
/* The four projections of a layer in that format, in the row order and K padding of p2t_llama_layer's matrices (K = hidden / heads *
 * head_dim / ffn rounded up to 128; codes with ld = K / 2).  stream_order != 0: the *_w are p2t_preshuffle_w_mxfp4 copies and the *_bs
 * are ignored (the same value in every layer). */
typedef struct {
    const void* qkv_w; const void* o_w; const void* gu_w; const void* down_w;
    const uint8_t* qkv_bs; const uint8_t* o_bs; const uint8_t* gu_bs; const uint8_t* down_bs;
    int32_t stream_order; int32_t reserved;
} p2t_llama_layer_mxfp4;
/* p2t_llama_decode_step for a gemm_fp8 configuration (bf16 activations) with at most 64 rows, whose four projections per layer stream
 * `layers` (HOST array of n_layers entries) instead of the e4m3 matrices of `w`; norms, row quantisers, attention, the fused rotation
 * epilogue (or the two-launch path where it does not apply) and the bf16 LM head are that function's.  `w` is the gemm_fp8 weight set
 * whose e4m3 matrices hold the same W~ (the prefill reads those). */
int p2t_llama_decode_step_mxfp4(const p2t_llama_config* cfg, const p2t_llama_weights* w, const p2t_llama_layer_mxfp4* layers,
                                const void* lm_head, int64_t ld_head, int lm_head_preshuffled, const p2t_kv_cache* cache,
                                const float* x, void* logits, int64_t ld_logits, int flags, void* workspace, size_t workspace_bytes,
                                p2t_stream stream);
/* ---- The quantised LM head (generate(lm_head_dtype="fp8" | "mxfp4"); bf16 models).  The head W [vocab, hidden] as
 *   P2T_LM_HEAD_E4M3:  e4m3 codes [vocab, ld >= Kq] + one E8M0 byte per vocabulary row `scales` [vocab]: p2t_quant_rows_fp8 of the head;
 *   P2T_LM_HEAD_MXFP4: e2m1 codes [vocab, ld >= Kq / 2 bytes] + one E8M0 byte per 32 columns `scales` [vocab, Kq / 32]: p2t_quant_rows_mxfp4
 * (Kq = hidden rounded up to 128, pad zero, ld % 16 == 0, codes 16-byte aligned).  stream_order != 0: `codes` is the p2t_preshuffle_w_fp8 /
 * p2t_preshuffle_w_mxfp4 copy (ld ignored; the MXFP4 copy carries its block scales: scales may be NULL; the e4m3 copy keeps `scales`).
 * A stream copy serves at most 64 rows.  More than 64 rows run the general fp8 GEMM on ROW-MAJOR e4m3 codes at ld = Kq: the e4m3 head's
 * own, or, for an MXFP4 head, codes_e4m3 / scales_e4m3 = p2t_quant_rows_fp8 of the dequantised head (exact: "MXFP4 decoder weights" above);
 * both NULL otherwise. */
enum { P2T_LM_HEAD_E4M3 = 1, P2T_LM_HEAD_MXFP4 = 2 };
typedef struct {
    int32_t format; int32_t stream_order;
    const void* codes; const uint8_t* scales; int64_t ld;
    const void* codes_e4m3; const uint8_t* scales_e4m3;
} p2t_lm_head_q;
size_t p2t_lm_head_q_workspace_bytes(int64_t M, int64_t hidden);
/* logits bf16 [M, ld_logits] = head(rmsnorm(x) * norm_w): x f32 [M, ld_x] (the residual stream; ld_x % 8 == 0, hidden % 8 == 0) is
 * normalised and written as e4m3 rows [M, Kq] + one E8M0 byte per row by the rule of the fp8 step's projections (p2t_rmsnorm_fp8), then
 * multiplied with the head: v_mfma_scale_f32_16x16x128_f8f6f4, f32 accumulation, one rounding to bf16; up to 64 rows on the weight
 * stream of p2t_gemm_nt_skinny_fp8 / _mxfp4 (columns vocab .. ld_logits are not written), beyond that on p2t_gemm_nt_fp8's kernels.
 * norm_w == NULL: x holds rows that are normalised already (p2t_llama_prefill's last_hidden) and is quantised by p2t_quant_rows_fp8's
 * rule.  act_codes [M, Kq] / act_scales [M] (optional, both or neither, 16-byte aligned): receive the e4m3 rows the GEMM read (tests);
 * NULL: they live in `workspace` (p2t_lm_head_q_workspace_bytes).  out_dtype: P2T_BF16 (anything else: P2T_ERR_UNSUPPORTED, as are a stream
 * copy with M > 64, an MXFP4 head with M > 64 and no e4m3 copy, an e4m3 head with M > 64 and ld != Kq, and M > 64 with vocab % 16 != 0:
 * p2t_gemm_nt's own condition).  Enqueues only: capturable. */
int p2t_lm_head_logits_q(const float* x, int64_t ld_x, const float* norm_w, float eps, const p2t_lm_head_q* head, int64_t M,
                         int64_t hidden, int64_t vocab, void* logits, int64_t ld_logits, int out_dtype, uint8_t* act_codes,
                         uint8_t* act_scales, void* workspace, size_t workspace_bytes, p2t_stream stream);
/* p2t_llama_decode_step and p2t_llama_decode_step_mxfp4 behind one door: w_stream or mx_layers (either may be NULL; both set:
 * P2T_ERR_ARG; mx_layers under p2t_llama_decode_step_mxfp4's conditions), and head_q: NULL = that step, launch for launch; set = the
 * final RMSNorm and the LM head run as p2t_lm_head_logits_q on the residual stream (lm_head / ld_head / lm_head_preshuffled are then
 * ignored and may be NULL / 0) and the workspace holds p2t_llama_decode_workspace_bytes + p2t_lm_head_q_workspace_bytes(BB, hidden). */
int p2t_llama_decode_step_q(const p2t_llama_config* cfg, const p2t_llama_weights* w, const p2t_llama_layer_stream* w_stream,
                            const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                            const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x, void* logits, int64_t ld_logits,
                            int flags, void* workspace, size_t workspace_bytes, p2t_stream stream);
/* The decode step's attention on its own (exposed so that it can be checked against the plain arithmetic): ONE query token per
 * row, q `dtype` [BB, nh, dp], over prompt_len[row / group] keys of the prompt segment and step[0] + 1 keys of the generated
 * segment (the layouts of ONE layer of p2t_kv_cache), GQA; softmax((scale) q k^T) v with f32 statistics -- log2_scores: q holds
 * scale * log2(e) already (as the towers store it for bf16 models) and `scale` is ignored.  out `dtype` [BB, ld_out >= nh *
 * head_dim].  One block per (row, kv head) streams all its keys; its waves are merged in LDS in wave order (no atomics).  use_mfma: -1 / 1
 * = the matrix-pipe kernel for bf16 (what the decode step runs), 0 = the lane-per-key kernel (every dtype; f32 always). */
int p2t_attention_decode(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                         const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp,
                         int G, float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out, p2t_stream stream);
/* p2t_attention_decode over an fp8 prompt segment (p2t_kv_cache with the two scale arrays set; ONE layer's buffers): k_prompt /
 * vt_prompt are e4m3 bytes, k_prompt_scale / v_prompt_scale their E8M0 bytes per key [B0][kv_heads][Tp] (16-byte aligned, like the
 * code buffers); the generated segment is bf16.  bf16 only (another dtype, or use_mfma = 0: P2T_ERR_UNSUPPORTED): the matrix-pipe
 * kernel, whose prompt tiles widen the codes to bf16 exactly (e4m3 is a subset of bf16), multiply a key's f32 score by its K scale
 * and its probability by its V scale after the row sum took the unscaled one -- powers of two, so the result is the bf16 kernel's
 * arithmetic on the dequantised operands, with its rounding points.  Keys behind prompt_len are never read into a result. */
int p2t_attention_decode_prompt_fp8(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                                    const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim,
                                    int Tp, int G, float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                                    const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, p2t_stream stream);
/* The prefill's store into an fp8 prompt segment, ONE layer: k, v bf16 [B][kv_heads][T][dp] (keys after the rotation) -> K codes
 * [B][kv_heads][Tp][dp], V codes transposed [B][kv_heads][dp][Tp] and the two scale arrays [B][kv_heads][Tp] (p2t_kv_cache's format),
 * in one launch: one block per (64-key tile, row x kv head), the maximum over a key's features reduced inside a lane group (no
 * atomics), V transposed through LDS.  Positions < T only: every byte behind them keeps its value.  T <= Tp, Tp % 64 == 0. */
int p2t_kv_quant_store(const void* k, const void* v, int B, int kv_heads, int T, int head_dim, int Tp, void* k_codes, void* vt_codes,
                       uint8_t* k_scale, uint8_t* v_scale, p2t_stream stream);
/* ---- continuous batching: rows that carry their OWN step counters (group == 1).  A finished row's slot is loaded with the next
 * prompt while the other rows go on; every length lives on the device, so a captured step graph keeps replaying across refills.
 * p2t_kv_cache keeps its layout: the counters travel beside it (row_step, device i32 [BB]) and cache->step is neither read nor
 * written by these entry points (it may be NULL). */
/* p2t_llama_decode_step_q with per-row counters: row r runs at position prompt_len[r] + row_step[r], its keys / values are appended at
 * index clamp(row_step[r], 0, G - 1), its attention covers prompt_len[r] + row_step[r] + 1 keys, and last of all row_step[r] += 1 where
 * frozen[r] == 0 (frozen: device i32 [BB], or NULL = no row is frozen).  A frozen row still runs (launch shapes are fixed): it
 * re-appends at its own index and does not advance -- harmless, and safe for a slot that was never loaded (prompt_len 0, row_step 0,
 * frozen: it attends to the one key it just wrote).  Every model and weight form of p2t_llama_decode_step_q; group != 1:
 * P2T_ERR_UNSUPPORTED.  Equal counters and frozen == NULL: the logits and cache contents of p2t_llama_decode_step_q, bit for bit.
 * Enqueues only: capturable. */
int p2t_llama_decode_step_rows(const p2t_llama_config* cfg, const p2t_llama_weights* w, const p2t_llama_layer_stream* w_stream,
                               const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                               const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x, void* logits, int64_t ld_logits,
                               int flags, void* workspace, size_t workspace_bytes, int32_t* row_step, const int32_t* frozen,
                               p2t_stream stream);
/* p2t_greedy_select over per-row counters: logits row i (of n) belongs to engine row r = row_map[i] (device i32 [n]; NULL: r = i and
 * n == BB; an r outside [0, BB) touches nothing).  finished[r] != 0: next_tokens[r] = pad_id and NOTHING is written to out_tokens (the
 * row's counter no longer moves: the token at it is its last one).  Otherwise next_tokens[r] = out_tokens[r, clamp(row_step[r], 0,
 * G - 1)] = argmax(logits[i, :V]) (lowest index among equal maxima), then finished[r] |= 1 if that token is in eos_ids and
 * finished[r] |= 2 if row_step[r] + 1 >= row_limit[r] (device i32 [BB], 1 .. G: the row's own max_new_tokens).  row_step is not
 * written.  Enqueues only: capturable. */
int p2t_greedy_select_rows(const void* logits, int dtype, int64_t ld, int V, int n, const int64_t* eos_ids, int n_eos, int64_t pad_id,
                           int32_t* finished, int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, const int32_t* row_step,
                           const int32_t* row_limit, const int32_t* row_map, int BB, int G, p2t_stream stream);
/* p2t_sample_select with p2t_greedy_select_rows' row model: its arguments without `step` and `row0`, n logits rows, and per engine row
 * the counter row_step (i32 [BB]), the limit row_limit (i32 [BB], 1 .. G) and the draw key row_key (i64 [BB], any value), all on the
 * device; row_map: device i32 [n], or NULL = r = i and n == BB (n <= BB either way).  Logits row i belongs to engine row r = row_map[i];
 * an r outside [0, BB) touches nothing.
 *   finished[r] != 0: next_tokens[r] = pad_id, and NOTHING is written to out_tokens, to finished or to scores row i; the block returns
 *   before it reads logits row i (which may hold anything).  This differs from the lock-step kernels, which do the whole row's work
 *   for a finished row and write its scores.
 *   Otherwise temperature, top-k, survivor table, ranks, top-p cut and inverse CDF are p2t_sample_select's, the same arithmetic in the
 *   same fixed reduction orders, on logits row i, with the draw u = uniform(seed, (uint64)row_key[r], row_step[r]): p2t_sample_select's
 *   chain with row_key[r] in the place of row0 + r and row_step[r] (unclamped) in the place of step[0];
 *   p2t_hip.synth.sample_uniform(seed, key, step).  The token goes to out_tokens[r, clamp(row_step[r], 0, G - 1)] and next_tokens[r];
 *   then finished[r] |= 1 if it is in eos_ids and finished[r] |= 2 if row_step[r] + 1 >= row_limit[r].  row_step is not written.
 * A row's token so depends on (seed, its key, its counter, its logits) and on nothing else: not on i, r, n or BB.  Equal counters s,
 * row_map NULL, no finished row, row_key[r] = row0 + r: p2t_sample_select's tokens, eos bits and scores at step[0] = s, bit for bit.
 * scores (or NULL): f32 [n, ld_scores >= V], row i as p2t_sample_select writes it.  flags: as there (bit 0: table full).  top_p on
 * without top_k: P2T_ERR_UNSUPPORTED.  Every written column and every LDS index is clamped in the kernel.  Enqueues only: capturable. */
int p2t_sample_select_rows(const void* logits, int dtype, int64_t ld, int V, int n, const int64_t* eos_ids, int n_eos, int64_t pad_id,
                           int32_t* finished, int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, const int32_t* row_step,
                           const int32_t* row_limit, const int32_t* row_map, const int64_t* row_key, int BB, int G, float temperature,
                           int top_k, float top_p, uint64_t seed, float* scores, int64_t ld_scores, int32_t* flags, p2t_stream stream);
/* p2t_logits_process with the same row model, in front of p2t_greedy_select_rows / p2t_sample_select_rows: logits row i (of n) belongs
 * to engine row r = row_map[i] (NULL: r = i, n == BB; an r outside [0, BB) touches nothing).  Its history is out_tokens[r, 0 .. cur) with
 * cur = clamp(row_step[r], 0, G) -- the row's OWN tokens, whatever the other rows' counters are -- and stage 5 compares that same cur
 * with min_new_tokens.  The output row is row i of out (f32 [n, ld_out >= V]).  finished: device i32 [BB] or NULL; a row with
 * finished[r] != 0 is skipped: nothing is read, and output row i keeps its bytes (the per-row selectors do not read it).  Stages 1 - 5,
 * their order and their bits are p2t_logits_process's: equal counters s, row_map NULL and no finished row give its rows at step[0] = s,
 * bit for bit.  Enqueues only: capturable. */
int p2t_logits_process_rows(const void* logits, int dtype, int64_t ld, int V, int n, const int64_t* out_tokens, int64_t ld_tokens,
                            const int32_t* row_step, const int32_t* row_map, const int32_t* finished, int BB, int G, float* out,
                            int64_t ld_out, float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens, const int64_t* eos_ids,
                            int n_eos, const int64_t* word_ids, const int32_t* word_offsets, int n_words, int n_word_ids, p2t_stream stream);
/* Loads k freshly prefilled prompts into slots of a running engine.  p2t_llama_prefill wants cache->B0 == B, so the k prompts are
 * prefilled into `staging` (a p2t_kv_cache with B0 = k, the same Tp and the same prompt-segment format; its generated segment is not
 * touched); this call copies staging row i's prompt segment -- K, transposed V and, when set, both scale arrays, ALL Tp entries of every
 * layer, so nothing of the previous occupant stays -- into slot slots[i] of `cache` in ONE launch of 16-byte loads and stores, and sets
 * cache->prompt_len[slot] = staging->prompt_len[i], row_step[slot] = 0, finished[slot] = 0, row_limit[slot] = limits[i].  slots, limits:
 * HOST i32 [k] (they travel in the launch's arguments).  Refused before the launch: a slot outside [0, cache->B0) or named twice, a
 * limit outside 1 .. cache->G, k != staging->B0, different Tp, scale arrays on one cache only, buffers that are not 16-byte aligned
 * (P2T_ERR_ARG); more than 256 slots per call (P2T_ERR_UNSUPPORTED).  No allocation, copy or synchronisation; meant to run between
 * graph replays, not inside a capture. */
int p2t_kv_slot_load(const p2t_llama_config* cfg, const p2t_kv_cache* staging, const p2t_kv_cache* cache, const int32_t* slots,
                     const int32_t* limits, int k, int32_t* row_step, int32_t* finished, int32_t* row_limit, p2t_stream stream);
/* p2t_attention_decode (k_prompt_scale == v_prompt_scale == NULL) / p2t_attention_decode_prompt_fp8 (both set) with one counter per row:
 * row r attends to prompt_len[r] keys of the prompt segment and row_step[r] + 1 of the generated one (group == 1, BB = B0). */
int p2t_attention_decode_rows(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                              const int32_t* prompt_len, const int32_t* row_step, int B0, int nh, int nkv, int head_dim, int Tp, int G,
                              float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                              const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, p2t_stream stream);
/* Beam re-ordering of the generated segment: row r of (k_dst, vt_dst) = row src_row[r] of the cache's generated segment, the
 * first step[0] tokens of every layer / head (k_dst, vt_dst: second buffers of the same shape; the caller swaps). */
int p2t_kv_reorder(const p2t_llama_config* cfg, const p2t_kv_cache* cache, const int64_t* src_row, void* k_dst, void* vt_dst,
                   p2t_stream stream);
/* ---- beam search without the cache copy (opt-in): the generated keys / values stay in the physical row that wrote them, and an
 * ANCESTRY TABLE beside the cache (as row_step is; p2t_kv_cache keeps its layout) says where a beam's history lies: ancestry, device
 * u8 [B0 * group][cache->G], ancestry[r][i] = the index inside r's prompt (0 .. group - 1) of the physical row whose generated segment
 * holds key i of beam row r's history.  Zero-initialised; columns > step[0] are never read. */
/* The table's update, in p2t_kv_reorder's place in the step (before the step that appends at index step[0]): with s = clamp(step[0],
 * 0, G - 1) read on the device, new[r][i] = old[src_rows[r]][i] for i < s, new[r][s] = r % group, columns > s untouched; in place, as
 * if all reads preceded all writes (one thread per (prompt, column) reads the prompt's group bytes, then writes them).  src_rows: what
 * p2t_beam_select* writes (global row indices inside the row's own prompt); a source outside the row's prompt is clamped into it.
 * Null arguments, group < 2: P2T_ERR_ARG; group > 16: P2T_ERR_UNSUPPORTED; before any launch.  One launch, capturable. */
int p2t_kv_ancestry_update(const p2t_kv_cache* cache, const int64_t* src_rows, uint8_t* ancestry, p2t_stream stream);
/* p2t_attention_decode / p2t_attention_decode_prompt_fp8 (the scale arrays both set, or both NULL) for a beam group under an ancestry
 * table: row r attends to prompt_len[r / group] prompt keys and to the step[0] + 1 generated keys (p, i) -- key i of physical row p of
 * r's prompt -- with ancestry[r][i] == p % group.  The matrix-pipe kernel runs one block per (prompt, kv head) and chunk of 16 / (nh /
 * nkv) beams: its 16 head slots are (beam, head) pairs, the prompt segment is streamed once for all of them, the generated tiles of
 * the group's physical rows are streamed with the table as one more condition of the score select (a slot with no visible key in a
 * tile keeps its running statistics as they were).  use_mfma = 0 / f32: the lane-per-key kernel, one block per (row, kv head), the
 * same rule.  ancestry == NULL, group < 2: P2T_ERR_ARG; group > 16 or nh / nkv > 16: P2T_ERR_UNSUPPORTED. */
int p2t_attention_decode_beams(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                               const int32_t* prompt_len, const int32_t* step, int B0, int group, int nh, int nkv, int head_dim, int Tp,
                               int G, float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                               const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, const uint8_t* ancestry, p2t_stream stream);
/* p2t_llama_decode_step_q whose attention is p2t_attention_decode_beams': every other launch is that step's, for every weight form and
 * head.  Row r appends at index step[0] of ITS OWN physical row, as ever; the caller has run p2t_kv_ancestry_update for this step.
 * ancestry == NULL, cache->group < 2: P2T_ERR_ARG; group > 16 or heads / kv_heads > 16: P2T_ERR_UNSUPPORTED; all before any launch. */
int p2t_llama_decode_step_beams(const p2t_llama_config* cfg, const p2t_llama_weights* w, const p2t_llama_layer_stream* w_stream,
                                const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                                const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x, void* logits, int64_t ld_logits,
                                int flags, void* workspace, size_t workspace_bytes, const uint8_t* ancestry, p2t_stream stream);
/* ---- prompt-lookup decoding (opt-in; greedy; group == 1, per-row counters): a step carries Q = k + 1 tokens per row -- the token chosen
 * last and a draft of up to k tokens found in the row's own generated text -- and keeps the longest prefix of the draft the model agrees
 * with plus the model's own next token: greedy decoding's tokens in fewer steps.  History of row r: h[0 .. s] = out_tokens[r, 0 .. s],
 * s = row_step[r]; h[s] is the token chosen last, not yet in the cache.  A rejected draft token's cache entry is simply stale: nothing
 * reads past a row's counter plus the step's own tokens, and the next step overwrites it. */
/* The draft (HF PromptLookupCandidateGenerator.get_candidates): for m = min(max_ngram, s) down to 1, the EARLIEST i <= s - m with
 * h[i .. i + m) == h[s - m + 1 .. s]; the draft is h[i + m .. min(i + m + num_tokens, s + 1)), c tokens (no match at any m: c = 0).
 * step_tokens (i64 [BB, num_tokens + 1]) row r = (h[s], the draft, pad_id behind it), draft_len[r] (i32 [BB]) = c.  finished[r] != 0:
 * all pad_id, c = 0.  One block per row; 1 <= num_tokens <= 7, 1 <= max_ngram <= 4 (P2T_ERR_ARG).  One launch, capturable. */
int p2t_lookup_draft_rows(const int64_t* out_tokens, int64_t ld_tokens, const int32_t* row_step, const int32_t* finished, int BB, int G,
                          int num_tokens, int max_ngram, int64_t pad_id, int64_t* step_tokens, int32_t* draft_len, p2t_stream stream);
/* p2t_attention_decode_rows for q_tokens query tokens per row: q and out have B0 * q_tokens rows, row r * q_tokens + j is token j of cache
 * row r and attends to prompt_len[r] prompt keys and the generated keys 0 .. row_step[r] + j (this step's tokens 0 .. j among them: causal).
 * bf16 on the matrix pipe (use_mfma != 0; the fp8 prompt segment with both scale arrays set): one block per (row, kv head) and chunk of
 * 16 / (nh / nkv) queries, whose 16 head slots are (query, head) pairs -- the row's keys are streamed once per chunk; use_mfma = 0 / f32:
 * the lane-per-key kernel over B0 * q_tokens virtual rows.  Either way row r * q_tokens + j holds the bits p2t_attention_decode_rows
 * computes on the same cache with row r's counter at row_step[r] + j.  Cache entries behind row_step[r] + q_tokens - 1 are never read into a
 * result.  q_tokens outside 1 .. 64: P2T_ERR_ARG; nh / nkv > 16: P2T_ERR_UNSUPPORTED. */
int p2t_attention_decode_multi(const void* q, const void* k_prompt, const void* vt_prompt, const void* k_gen, const void* vt_gen,
                               const int32_t* prompt_len, const int32_t* row_step, int B0, int nh, int nkv, int head_dim, int Tp, int G,
                               float scale, int log2_scores, int dtype, int use_mfma, void* out, int64_t ld_out,
                               const uint8_t* k_prompt_scale, const uint8_t* v_prompt_scale, int q_tokens, p2t_stream stream);
/* p2t_llama_decode_step_rows for q_tokens tokens per row: x f32 [B0 * q_tokens, hidden] and logits [B0 * q_tokens, ld_logits], row
 * r * q_tokens + j = token j of cache row r.  Token j runs at position prompt_len[r] + row_step[r] + j, its key and value are appended at
 * index clamp(row_step[r] + j, 0, G - 1), its attention is p2t_attention_decode_multi's, and its logits row predicts token row_step[r] +
 * j + 1.  The launches are those of a step of B0 * q_tokens rows but the attention's; row_step is READ ONLY (p2t_lookup_verify_rows
 * advances it) and there is no `frozen`: a finished row re-appends behind its counter, where nothing is read.  The workspace is that of
 * B0 * q_tokens rows: p2t_llama_decode_workspace_bytes(cfg, B0 * q_tokens, Tp, G) (+ p2t_lm_head_q_workspace_bytes(B0 * q_tokens, hidden)
 * with head_q).  Every model and weight form of p2t_llama_decode_step_rows.  B0 * q_tokens > 64, group != 1, heads / kv_heads > 16:
 * P2T_ERR_UNSUPPORTED; q_tokens outside 1 .. 64: P2T_ERR_ARG; all before the first enqueue.  Enqueues only: capturable. */
int p2t_llama_decode_step_multi(const p2t_llama_config* cfg, const p2t_llama_weights* w, const p2t_llama_layer_stream* w_stream,
                                const p2t_llama_layer_mxfp4* mx_layers, const void* lm_head, int64_t ld_head, int lm_head_preshuffled,
                                const p2t_lm_head_q* head_q, const p2t_kv_cache* cache, const float* x, void* logits, int64_t ld_logits,
                                int flags, void* workspace, size_t workspace_bytes, const int32_t* row_step, int q_tokens, p2t_stream stream);
/* The verification behind such a step: g_j = argmax(logits[r * q_tokens + j, :V]) (lowest index among equal maxima, one block per logits
 * row into choice, i32 [BB * q_tokens] scratch), then one thread per row: a = the largest value <= draft_len[r] with g_(j-1) ==
 * step_tokens[r, j] for 1 <= j <= a (and s + j < row_limit[r]: a token behind the limit decides nothing); the new tokens g_0 .. g_a, cut behind the first one in eos_ids and at the row's limit, go to
 * out_tokens[r, s + 1 ..]; row_step[r] = s + their number, next_tokens[r] = the last of them, finished[r] |= 1 (eos) | 2 (the token at
 * index row_limit[r] - 1 was written), p2t_greedy_select_rows' bits.  finished[r] != 0 on entry: next_tokens[r] = pad_id and nothing else is
 * written.  stats (i32 [BB, 3]) += (1, draft_len[r], a) for a live row (a: before the eos / limit cut).  No float atomics; every index is clamped; nothing
 * is written outside out_tokens[r, 0 .. G).  2 <= q_tokens <= 8 (P2T_ERR_ARG).  Two launches, capturable. */
int p2t_lookup_verify_rows(const void* logits, int dtype, int64_t ld, int V, int BB, int q_tokens, const int64_t* step_tokens,
                           const int32_t* draft_len, const int64_t* eos_ids, int n_eos, int64_t pad_id, int32_t* finished,
                           int64_t* next_tokens, int64_t* out_tokens, int64_t ld_tokens, int32_t* row_step, const int32_t* row_limit, int G,
                           int32_t* stats, int32_t* choice, p2t_stream stream);

/* ---------------------------------------------------------------- optimizer tail */
/* One clip_grad_norm_(max_norm) + AdamW step over n_tensors (<= 64) f32 parameter tensors (HOST arrays of
 * device pointers).  shadow[i] (optional, may be NULL per tensor) receives the updated parameter in
 * `shadow_dtype` as a matrix with cols[i] columns and row stride shadow_ld[i] (the GEMM-layout copy the
 * next forward reads).  max_norm <= 0 or >= 1e30 = no clipping.  grad_norm_out f32 [1] (device): total norm
 * before clipping.  scratch: f32 [256 * n_tensors]. */
int p2t_clip_adamw_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* numel, void* const* shadow, const int64_t* cols,
                        const int64_t* shadow_ld, int shadow_dtype, int step, double lr, double beta1, double beta2,
                        double eps, double weight_decay, double max_norm, float* grad_norm_out, float* scratch,
                        p2t_stream stream);

/* Flat form of the same step (stage 2: hundreds of tensors in one buffer).  params / grads / exp_avg / exp_avg_sq: f32 [n] device
 * vectors, 16-byte aligned, n % 16 == 0.  segments (device): one p2t_flat_segment per trained tensor, offsets multiples of 16
 * elements, no overlap; elements between segments are padding (their gradient must be 0, they are never written).  chunks (device):
 * n_chunks pieces (segment, flat start, count <= P2T_FLAT_CHUNK) that tile every segment exactly; one block each, so no element
 * searches for its segment.  A segment's shadow (optional) receives RNE(scale * p) for element j at
 * shadow[(j / cols) * ld + j % cols] (rows * cols == numel); padding rows / columns of the shadow are never written.
 * Two launches whatever the number of segments: partial sums of g^2 (P2T_FLAT_NORM_BLOCKS of them, into scratch f32
 * [P2T_FLAT_NORM_BLOCKS]), then clip_grad_norm_(max_norm) + torch's AdamW, every block re-adding the partials in one fixed order
 * (bit-identical norm, no atomics).  max_norm <= 0 or >= 1e30 = no clipping; grad_norm_out f32 [1] (device, optional): total
 * norm before clipping. */
#define P2T_FLAT_NORM_BLOCKS 1024
#define P2T_FLAT_CHUNK 4096
typedef struct {
    int64_t offset;                      /* first element in the flat buffers (multiple of 16) */
    int64_t numel;
    void* shadow;                        /* NULL: no shadow */
    int64_t rows, cols, ld;              /* shadow matrix [rows, cols] at row stride ld (elements) */
    float scale;                         /* shadow = RNE(scale * p) */
    int32_t shadow_dtype;                /* P2T_F32 | P2T_BF16 */
} p2t_flat_segment;
typedef struct {
    int64_t start;                       /* flat index of the chunk's first element */
    int32_t segment;                     /* index into the segment table */
    int32_t count;                       /* elements, 1 .. P2T_FLAT_CHUNK */
} p2t_flat_chunk;
int p2t_clip_adamw_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                        const p2t_flat_segment* segments, const p2t_flat_chunk* chunks, int64_t n_chunks, int step,
                        double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                        float* grad_norm_out, float* scratch, p2t_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* P2T_HIP_H */
