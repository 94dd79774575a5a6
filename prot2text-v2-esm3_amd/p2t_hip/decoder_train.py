"""Stage-2 step of the decoder with LoRA adapters and / or per-head q / k RMSNorm:

    reference  scripts/train_instruct.py:146-183   LoraConfig(r, lora_alpha = 2 r, lora_dropout = 0.1, bias = "none") on the seven
                                                   decoder projections, modules_to_save = adapter.fc1 / fc2
               scripts/train_instruct.py:192-213   loss = model(**batch).loss; loss.backward()
               models/esmc_config.py:9             the fork's text tower is a Qwen3 (per-head q_norm / k_norm)

`p2t_llama_train_forward / _backward` (csrc/llama_train.hip) run the FROZEN decoder as fused blocks and hand back only the
gradient at its inputs.  A LoRA branch sits between those blocks (y = W x + (alpha / r) B (A drop(x)) ahead of the rotation / the
SwiGLU), and so does Qwen3's q / k norm, so this module drives the same HIP kernels one by one through the C ABI (the row-wise ones:
csrc/norm.hip, csrc/activations.hip, csrc/misc.hip; the loss: csrc/lm_loss.hip), per layer:
p2t_rmsnorm, p2t_gemm_nt (frozen weights: MFMA where K allows; low-rank products: the same entry point), p2t_qkv_post,
p2t_attention (+ log-sum-exps), p2t_swiglu_gu, and backwards p2t_gemm_nt on transposed weights, p2t_attention_backward,
p2t_rope_backward_pack, p2t_rmsnorm_backward, p2t_transpose (the token axis made contiguous for dA / dB), p2t_dropout_rows (the
branch's input dropout: a counter-hash mask regenerated in the backward, never stored; the branch is p2t_hip/lora_linear.py's, shared
with the encoder step).  torch allocates, slices, concatenates and
wires autograd; no torch op computes on the path.

Each layer is written once (`_layer_forward`).  The full-tape step keeps every layer's record; under gradient checkpointing
(`lora_lm_loss(checkpoint=True)`, reference models/modeling_esm2llama_instruct.py:253-268) the tape keeps each layer's fp32 input alone,
the backward runs the same body again up to `gu`, and dA / dB come from p2t_lora_wgrad (the token axis summed in place, no transposes).

Parity: tests/golden/sft_lora_tiny.npz = torch autograd through the REFERENCE class with every target wrapped by a hand-written
LoRA linear (tests/golden/make_golden.py run_sft_lora) and, for Qwen3, through HF Qwen3ForCausalLM.  `peft` is not importable in
this image: the arithmetic is LoRA's published one, parity against peft's own code is UNPINNED (as is the checkpoint key layout
`peft_state_dict` writes; p2t_hip/lora.py reads the same restated layout).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import lm_head, ops
from ._lib import call
from .lora_linear import DECODER_TARGETS, LoraLinear, LoraPairs, scaled_grads, tape_bytes
from .ops import ptr, round_up, stream

TARGETS = DECODER_TARGETS


class DecoderLora(LoraPairs):
    """The trainable A [r, in] / B [out, r] pairs of `LoraConfig(r, lora_alpha, lora_dropout, target_modules)` on a LlamaDecoder."""

    TOWER, TARGETS, SEED_OFFSET = "decoder", TARGETS, 0
    WEIGHT = "layers.{i}.{t}.weight"                    # in decoder.model
    MODULE = "llama_decoder.model.layers.{i}.{t}"

    def __init__(self, decoder, r: int, lora_alpha: Optional[float] = None, lora_dropout: float = 0.1, target_modules: Sequence[str] = TARGETS, seed: int = 0):
        super().__init__(decoder.model, decoder.spec.num_hidden_layers, r, lora_alpha, lora_dropout, target_modules, seed)


class _Lin(LoraLinear):
    """One decoder projection built on its own, outside a pass (tests, tools): its own parameter dict, dropout None = `lora.p`, and
    the pair's values as the tuple `lora` = (A, B, r, alpha / r, p, mask seed), None without a pair.  The step itself uses LoraLinear."""

    def __init__(self, decoder, lora: Optional[DecoderLora], i: int, target: str, dt, dropout: Optional[float] = None):
        p = (lora.p if dropout is None else float(dropout)) if lora is not None else 0.0
        super().__init__(decoder.model, dict(decoder.model.named_parameters()), f"layers.{i}.{target}", lora, i, target, dt, p)
        self.lora = (*self.ab, self.r, self.s, self.p, self.seed) if self.ab is not None else None


def _interleave(g: torch.Tensor, u: torch.Tensor, F: int) -> torch.Tensor:
    """[M, F] gate, up -> [M, 2F] in the 32-column gate / up blocks of p2t_llama_layer.gu_w (a copy, no arithmetic)."""
    M = g.shape[0]
    return torch.stack([g[:, :F].reshape(M, F // 32, 32), u[:, :F].reshape(M, F // 32, 32)], 2).reshape(M, 2 * F).contiguous()


def _deinterleave(d_gu: torch.Tensor, F: int):
    M = d_gu.shape[0]
    v = d_gu[:, :2 * F].reshape(M, F // 32, 2, 32)
    return v[:, :, 0].reshape(M, F).contiguous(), v[:, :, 1].reshape(M, F).contiguous()


def _layer_forward(st: dict, i: int, lin: dict, x: torch.Tensor, keep: bool, stop: bool = False):
    """Layer i of the decoder on the fp32 residual stream x [M, H] -> (the layer's record, the stream after it).  The ONE body of
    the layer: the forward pass runs it (keep: the record holds what the backward reads, x itself as `x_in`; else only `lin`), and
    the checkpointed backward runs it again from the kept `x_in` with stop = True, which ends at `gu` -- the stream then is
    `x_mid`, and the down projection with its residual add is not redone."""
    s, dt, P = st["spec"], st["dt"], st["P"]
    B, T, H = st["shape"]
    M = B * T
    nh, nkv, d, F = s.num_attention_heads, s.num_key_value_heads, s.head_dim, s.intermediate_size
    f32v = lambda n: P[n].detach().float().contiguous()
    docs = st["docs"]
    p = f"layers.{i}."
    rec = dict(lin=lin, x_in=x if keep else None)
    if keep:
        x = x.clone()                                   # the record keeps the layer's input; the stream goes on in a copy
    h = ops.rmsnorm(x, f32v(p + "input_layernorm.weight"), s.rms_norm_eps, out_dtype=dt)
    parts = []
    for t in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"):
        y, u = lin[t].forward(h)
        rec["u_" + t] = u
        parts.append(y)
    if s.qk_norm:                                       # Qwen3Attention.forward: RMSNorm over head_dim of every head, before the rotation
        rec["q_raw"], rec["k_raw"] = parts[0], parts[1]
        parts[0] = ops.rmsnorm(parts[0].view(M * nh, d), f32v(p + "self_attn.q_norm.weight"), s.rms_norm_eps, ld_out=d).view(M, nh * d)
        parts[1] = ops.rmsnorm(parts[1].view(M * nkv, d), f32v(p + "self_attn.k_norm.weight"), s.rms_norm_eps, ld_out=d).view(M, nkv * d)
    qkv = ops.cast(torch.cat(parts, 1), dt) if dt != torch.float32 else torch.cat(parts, 1)
    if qkv.shape[1] % 8:
        qkv = torch.nn.functional.pad(qkv, (0, 8 - qkv.shape[1] % 8))
    q4, k4, v4 = ops.qkv_post(qkv.contiguous(), st["inv_freq"], B, T, nh, nkv, d, st["q_fold"], docs=docs)
    lse = torch.empty((B, nh, T), dtype=torch.float32, device=x.device)
    ao = ops.attention(q4, k4, v4, st["key_mask"], st["kv_info"], d, 1.0 if st["l2s"] else st["scale"], True, log2_scores=st["l2s"], lse=lse,
                       docs=docs)                       # [M, QO]
    rec.update(q=q4, k=k4, v=v4, lse=lse, ao=ao)
    _, rec["u_self_attn.o_proj"] = lin["self_attn.o_proj"].forward(ao, resid=x)
    rec["x_mid"] = (x if stop else x.clone()) if keep else None
    h2 = ops.rmsnorm(x, f32v(p + "post_attention_layernorm.weight"), s.rms_norm_eps, out_dtype=dt)
    g, rec["u_mlp.gate_proj"] = lin["mlp.gate_proj"].forward(h2)
    up, rec["u_mlp.up_proj"] = lin["mlp.up_proj"].forward(h2)
    gu = _interleave(g, up, F)
    gu = ops.cast(gu, dt) if dt != torch.float32 else gu
    rec["gu"] = gu if keep else None
    if stop:
        return rec, x
    act = torch.empty((M, round_up(F, 64)), dtype=dt, device=x.device)
    call("p2t_swiglu_gu", ptr(gu), gu.stride(0), None, 0, ptr(act), act.stride(0), M, F, ops.dt_of(dt), stream())
    _, rec["u_mlp.down_proj"] = lin["mlp.down_proj"].forward(act, resid=x)
    return rec, x


class DecoderLoraLossFn(torch.autograd.Function):
    """LM loss of the decoder as a function of `inputs_embeds` and the LoRA parameters (frozen base weights)."""

    @staticmethod
    def forward(ctx, inputs_embeds, decoder, lora, attention_mask, labels, opts, *params):
        s, m = decoder.spec, decoder.model
        dt = m.dtype
        B, T, H = inputs_embeds.shape
        M = B * T
        d, F, L = s.head_dim, s.intermediate_size, s.num_hidden_layers
        if F % 32:
            raise ValueError("Llama intermediate_size must be a multiple of 32")
        dev = m.embed_tokens.weight.device
        P = dict(m.named_parameters())
        mask = attention_mask.to(device=dev, dtype=torch.int64).contiguous()
        key_mask, kv_info, _ = ops.mask_prepare(mask)
        docs, weights = opts.get("docs"), opts.get("loss_weights")      # packed rows (ops.doc_prepare) / per-target loss weights
        inv_freq = m._inv_freq().to(dev)
        l2s = dt == torch.bfloat16                       # as the towers: q carries scale * log2 e, the logits are ln 2 * q.k
        scale = float(d) ** -0.5
        q_fold = scale * 1.4426950408889634 if l2s else 1.0
        x = inputs_embeds.detach().to(device=dev, dtype=torch.float32).reshape(M, H).contiguous().clone()
        tape = []
        keep = opts["keep_tape"]                        # False: forward-only loss, no layer's activations are kept
        ckpt = keep and bool(opts.get("checkpoint"))    # the tape holds every layer's input alone; the backward redoes the layer
        st = dict(decoder=decoder, spec=s, dt=dt, P=P, tape=tape, checkpoint=ckpt, key_mask=key_mask, kv_info=kv_info, docs=docs, weights=weights,
                  inv_freq=inv_freq, l2s=l2s, scale=scale, q_fold=q_fold, shape=(B, T, H), params=params, in_dtype=inputs_embeds.dtype)
        for i in range(L):
            p = f"layers.{i}."
            lin = {t: LoraLinear(m, P, p + t, lora, i, t, dt, opts["dropout"]) for t in TARGETS}
            if ckpt:
                tape.append(dict(lin=lin, x_in=x.clone()))
            rec, x = _layer_forward(st, i, lin, x, keep and not ckpt)
            if keep and not ckpt:
                tape.append(rec)
        lab = labels.to(dev).to(torch.int64).contiguous()
        fused = opts.get("fused")                       # LlamaDecoder.fused_lm_loss(): the target rows only, no logits (p2t_hip/lm_head.py)
        if fused is not None:
            loss, head = lm_head.lm_head_loss(decoder, x, lab, weights=weights, chunk_rows=fused["chunk_rows"], targets=fused.get("targets"),
                                                   with_grad=keep)
            logits = None
        else:
            loss, logits, head = lm_head.head_loss(decoder, x, lab, weights=weights)
        st.update(head=head, fused=fused is not None, device=x.device)
        ctx.state = st
        if keep:
            decoder.last_tape_bytes = tape_bytes(tape, (*lm_head.head_saved_tensors(head), lab, key_mask, kv_info, docs, weights))
        if logits is not None:
            ctx.mark_non_differentiable(logits)
        return loss[0], logits

    @staticmethod
    def backward(ctx, g_loss, _g_logits):
        st = ctx.state
        dec = st["decoder"]
        s, m = dec.spec, dec.model
        dt = m.dtype
        B, T, H = st["shape"]
        M = B * T
        nh, nkv, d, F = s.num_attention_heads, s.num_key_value_heads, s.head_dim, s.intermediate_size
        dp = ops.head_dim_padded(d)
        dev = st["device"]
        P = st["P"]
        f32v = lambda n: P[n].detach().float().contiguous()
        # the head's gradient at the input of the final RMSNorm, unscaled: g_loss multiplies the whole chain at its end
        g = lm_head.lm_head_backward(dec, st["head"], None) if st["fused"] else lm_head.head_backward(dec, st["head"])
        st["head"] = None

        def rms_bwd(x, w, dy, out, acc, rows=M, cols=H):
            call("p2t_rmsnorm_backward", ptr(x), x.stride(0), ptr(w), float(s.rms_norm_eps), ptr(dy), dy.stride(0), 0 if dy.dtype == torch.float32 else 1,
                 ptr(out), out.stride(0), rows, cols, int(acc), stream())
        grads: dict = {}
        c_s = 0.6931471805599453 if st["l2s"] else st["scale"]
        to_dt = lambda t: ops.cast(t, dt) if t.dtype != dt else t
        ta = st["checkpoint"]                           # ... and dA / dB by p2t_lora_wgrad, straight over the token axis
        for i in range(len(st["tape"]) - 1, -1, -1):
            rec = st["tape"][i]
            lin = rec["lin"]
            if ta:                                      # checkpointed: the layer's records again, from its input, up to gu
                rec, _ = _layer_forward(st, i, lin, rec["x_in"], True, stop=True)
            p = f"layers.{i}."
            # ---- MLP branch: x2 = x1 + down(silu(g) u)
            g16 = to_dt(g)
            act = torch.empty((M, round_up(F, 64)), dtype=dt, device=dev)
            call("p2t_swiglu_gu", ptr(rec["gu"]), rec["gu"].stride(0), None, 0, ptr(act), act.stride(0), M, F, ops.dt_of(dt), stream())
            u_down = rec["u_mlp.down_proj"] if "u_mlp.down_proj" in rec else lin["mlp.down_proj"].branch_input(act)
            d_act = lin["mlp.down_proj"].backward(g16, act, u_down, None, False, False, grads, token_axis=ta)                  # [M, Fp]
            d_gu = torch.empty((M, 2 * F), dtype=dt, device=dev)
            call("p2t_swiglu_gu", ptr(rec["gu"]), rec["gu"].stride(0), ptr(d_act), d_act.stride(0), ptr(d_gu), d_gu.stride(0), M, F, ops.dt_of(dt), stream())
            d_gate, d_up = _deinterleave(d_gu, F)
            h2 = ops.rmsnorm(rec["x_mid"], f32v(p + "post_attention_layernorm.weight"), s.rms_norm_eps, out_dtype=dt)
            d_h2 = lin["mlp.gate_proj"].backward(d_gate, h2, rec["u_mlp.gate_proj"], None, True, False, grads, token_axis=ta)
            lin["mlp.up_proj"].backward(d_up, h2, rec["u_mlp.up_proj"], d_h2, True, True, grads, token_axis=ta)
            rms_bwd(rec["x_mid"], f32v(p + "post_attention_layernorm.weight"), d_h2, g, 1)
            # ---- attention branch: x1 = x + o(attn(...))
            g16 = to_dt(g)
            d_ao = lin["self_attn.o_proj"].backward(g16, rec["ao"], rec["u_self_attn.o_proj"], None, False, False, grads, token_axis=ta)       # [M, QO]
            dq, dk, dv = ops.attention_backward(rec["q"], rec["k"], rec["v"], rec["ao"], d_ao, rec["lse"], st["key_mask"], st["kv_info"], d, c_s, True,
                                                log2_scores=st["l2s"], docs=st["docs"])
            NQ = (nh + 2 * nkv) * d
            d_qkv = torch.zeros((M, round_up(NQ, 64)), dtype=dt, device=dev)
            cs = torch.empty((T, d), dtype=torch.float32, device=dev)
            if st["docs"] is not None:
                call("p2t_rope_backward_pack_docs", ptr(dq), ptr(dk), ptr(dv), ptr(st["inv_freq"]), ptr(cs), ptr(st["docs"]), ptr(d_qkv), d_qkv.stride(0),
                     B, T, nh, nkv, d, dp, float(st["q_fold"]), ops.dt_of(dt), stream())
            else:
                call("p2t_rope_backward_pack", ptr(dq), ptr(dk), ptr(dv), ptr(st["inv_freq"]), ptr(cs), ptr(d_qkv), d_qkv.stride(0), B, T, nh, nkv, d, dp,
                     float(st["q_fold"]), ops.dt_of(dt), stream())
            d_q, d_k, d_v = d_qkv[:, :nh * d], d_qkv[:, nh * d:(nh + nkv) * d], d_qkv[:, (nh + nkv) * d:NQ]
            if s.qk_norm:
                def norm_bwd(raw, w, dy, heads):
                    dyc = dy.contiguous().view(M * heads, d)
                    out = torch.empty((M * heads, d), dtype=torch.float32, device=dev)
                    rms_bwd(raw.view(M * heads, d), f32v(w), dyc, out, 0, rows=M * heads, cols=d)
                    return to_dt(out.view(M, heads * d))
                d_q = norm_bwd(rec["q_raw"], p + "self_attn.q_norm.weight", d_q, nh)
                d_k = norm_bwd(rec["k_raw"], p + "self_attn.k_norm.weight", d_k, nkv)
            h1 = ops.rmsnorm(rec["x_in"], f32v(p + "input_layernorm.weight"), s.rms_norm_eps, out_dtype=dt)
            pad8 = lambda t: t if (t.stride(0) % 8 == 0 and t.stride(1) == 1) else torch.nn.functional.pad(t, (0, (-t.shape[1]) % 8)).contiguous()
            d_h1 = lin["self_attn.q_proj"].backward(pad8(d_q), h1, rec["u_self_attn.q_proj"], None, True, False, grads, token_axis=ta)
            lin["self_attn.k_proj"].backward(pad8(d_k), h1, rec["u_self_attn.k_proj"], d_h1, True, True, grads, token_axis=ta)
            lin["self_attn.v_proj"].backward(pad8(d_v), h1, rec["u_self_attn.v_proj"], d_h1, True, True, grads, token_axis=ta)
            rms_bwd(rec["x_in"], f32v(p + "input_layernorm.weight"), d_h1, g, 1)
            st["tape"][i] = None                        # free the layer's activations
        gl = g_loss.float().reshape(1).contiguous()
        call("p2t_scale_by_device_scalar", ptr(g), g.numel(), ptr(gl), stream())
        out_params = scaled_grads(st["params"], grads, gl)
        ctx.state = None
        return (g.view(B, T, H).to(st["in_dtype"]), None, None, None, None, None, *out_params)


def lora_lm_loss(decoder, lora: Optional[DecoderLora], inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, labels: torch.Tensor,
                 dropout: Optional[float] = None, docs: Optional[torch.Tensor] = None, loss_weights: Optional[torch.Tensor] = None,
                 checkpoint: bool = False, fused: Optional[dict] = None):
    """(loss, logits) of `llama_decoder(inputs_embeds=..., attention_mask=..., labels=...)` with the LoRA branches in the graph.
    dropout: None = the branches' own `lora.p` (every mode, as before); a value overrides it for this call and leaves the mask counter
    where it is -- 0.0 is peft's eval mode (InstructTrainer.evaluate).  Without gradients to compute, no activation tape is kept.
    docs: packed rows (ops.doc_prepare: positional rotary + document-confined attention; the caller has set the labels of document
    starts to -100); loss_weights: f32 [B, T] per-target weights (ops.cross_entropy_shifted) instead of the token mean.
    checkpoint: gradient checkpointing -- the tape keeps each layer's fp32 input alone and the backward redoes the layer from it
    (same kernels, same dropout seeds: the loss and every gradient but dA / dB are bit-identical to checkpoint = False; dA / dB come
    from p2t_lora_wgrad, a differently ordered fp32 sum).  `decoder.last_tape_bytes`: the bytes of the tensors kept for the backward.
    fused: dict(chunk_rows=..., targets=lm_head.select_targets(...) or absent) -- the LM loss over the target rows only
    (LlamaDecoder.fused_lm_loss; p2t_hip/lm_head.py): logits is then None, and the head keeps no [M, vocab] tensor."""
    params = tuple(lora.parameters()) if lora is not None else ()
    if lora is not None and dropout is None:
        if lora.training:
            lora.step_count += 1                        # a fresh dropout mask per step
        dropout = lora.p                                # in every mode (peft's eval mode would be 0.0)
    keep = torch.is_grad_enabled() and (inputs_embeds.requires_grad or any(q.requires_grad for q in params))
    opts = dict(dropout=float(dropout or 0.0), keep_tape=keep, docs=docs, loss_weights=loss_weights, checkpoint=bool(checkpoint), fused=fused)
    loss, logits = DecoderLoraLossFn.apply(inputs_embeds, decoder, lora, attention_mask, labels, opts, *params)
    return loss, (logits[..., : decoder.spec.vocab_size] if logits is not None else None)
