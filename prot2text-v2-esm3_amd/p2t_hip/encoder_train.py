"""Stage-2 step through the ESM2 encoder with LoRA adapters on its projections (the protein half of the stage-2 recipe):

    reference  scripts/train_instruct.py:155-183                   LoraConfig(target_modules = [...]) -- peft matches every module
                                                                   whose name equals a target or ends in "." + target
               models/modeling_esm2llama_instruct.py:174-193       the ESM2 encoder runs under autograd (no no_grad, no detach), so
                                                                   LoRA pairs on its modules are trained by loss.backward()

`p2t_esm2_forward` runs the FROZEN encoder as fused blocks and keeps no tape.  With a LoRA branch y = W x + b + s B (A drop(x)) on
`attention.self.{query,key,value}`, `attention.output.dense`, `intermediate.dense` or `output.dense`, this module drives the C ABI
layer by layer instead, as p2t_hip/decoder_train.py does for the decoder and with the same LoRA branch (p2t_hip/lora_linear.py; HF
EsmLayer, transformers/models/esm/modeling_esm.py):

    h  = LayerNorm(x)                   p2t_layernorm                 backward p2t_layernorm_backward
    q, k, v = W h + b (+ branch)        p2t_gemm_nt (+ low-rank)      dX GEMMs on W^T, dA / dB
    rotate-half rotary, q * d^-1/2      p2t_qkv_post                  p2t_rope_backward_pack
    attention (bidirectional, lse)      p2t_attention                 p2t_attention_backward (causal = 0)
    x += o(attn) + b (+ branch)         p2t_gemm_nt (RESID)
    h2 = LayerNorm(x)
    Z = fc1 h2 + b (+ branch), gelu(Z)  P2T_EPI_GELU (no branch) or   P2T_EPI_GELU_BWD on the fc2 dX GEMM, or p2t_gelu_rows
                                        p2t_gemm_nt + p2t_gelu_rows   (backward) when fc2 carries a branch
    x += fc2 gelu(Z) + b (+ branch)
    out = emb_layer_norm_after(x)

The tape keeps x at the layer's input and after the attention (fp32), q / k / v, the log-sum-exps, the attention output, Z and the
branches' u = drop(x) A^T; the backward stops at layer 0's input (the embeddings are frozen).  Dropout masks are the counter hash of
p2t_dropout_rows, regenerated in the backward.  torch allocates, slices and wires autograd; no torch op computes on the path.
Under gradient checkpointing (`encoder_lora_forward(checkpoint=True)`) the tape keeps each layer's fp32 input alone; the backward runs the
layer's one body (`_layer_forward`) again up to Z and takes dA / dB from p2t_lora_wgrad.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _lib, ops
from ._lib import call
from .lora_linear import ENCODER_TARGETS, LoraLinear, LoraPairs, resolve_targets, scaled_grads, tape_bytes  # noqa: F401 (resolve_targets: re-exported)
from .ops import ptr, round_up, stream

TARGETS = ENCODER_TARGETS


class EncoderLora(LoraPairs):
    """The trainable A [r, in] / B [out, r] pairs of a LoraConfig on the ESM2 encoder's linears."""

    TOWER, TARGETS, SEED_OFFSET = "ESM2 encoder", TARGETS, 64
    WEIGHT = "encoder.layer.{i}.{t}.weight"             # in the encoder
    MODULE = "esm_encoder.encoder.layer.{i}.{t}"

    def __init__(self, encoder, r: int, lora_alpha: Optional[float] = None, lora_dropout: float = 0.1, target_modules: Sequence[str] = TARGETS,
                 seed: int = 0):
        super().__init__(encoder, encoder.spec.num_hidden_layers, r, lora_alpha, lora_dropout, target_modules, seed)


def _gelu_rows(z: torch.Tensor, dy: Optional[torch.Tensor], n: int, out_dtype) -> torch.Tensor:
    M = z.shape[0]
    out = torch.empty((M, round_up(n, 64)), dtype=out_dtype, device=z.device)
    call("p2t_gelu_rows", ptr(z), ops.dt_of(z), z.stride(0), ptr(dy), ops.dt_of(dy) if dy is not None else 0, dy.stride(0) if dy is not None else 0,
         ptr(out), ops.dt_of(out), out.stride(0), M, n, stream())
    return out


def _layer_forward(st: dict, i: int, lin: dict, x: torch.Tensor, keep: bool, stop: bool = False, with_lse: bool = False):
    """Layer i of the encoder on the fp32 residual stream x [M, H] -> (the layer's record, the stream after it).  The ONE body of
    the layer: the forward pass runs it (keep: the record holds what the backward reads, x itself as `x_in`; else only `lin`), and
    the checkpointed backward runs it again from the kept `x_in` with stop = True, which ends at Z -- the stream then is `x_mid`,
    and the output projection with its residual add is not redone (only u = drop(gelu(Z)) A^T of its branch is).  with_lse: the attention writes its log-sum-exps although the
    record is not kept -- the checkpointed forward asks for it, so that it launches the attention form the recompute will launch."""
    s, dt, P = st["spec"], st["dt"], st["P"]
    B, T = st["shape"]
    M, H, F = B * T, s.hidden_size, s.intermediate_size
    nh, d, eps = s.num_attention_heads, s.head_dim, s.layer_norm_eps
    f32v = lambda n: P[n].detach().float().contiguous()
    p = f"encoder.layer.{i}."
    rec = dict(lin=lin, x_in=x if keep else None)
    if keep:
        x = x.clone()                                   # the record keeps the layer's input; the stream goes on in a copy
    h = ops.layernorm(x, f32v(p + "attention.LayerNorm.weight"), f32v(p + "attention.LayerNorm.bias"), eps, out_dtype=dt)
    parts = []
    for t in TARGETS[:3]:
        y, rec["u_" + t] = lin[t].forward(h, keep_u=keep)
        parts.append(y)
    qkv = torch.cat([y[:, :H] for y in parts], 1)
    qkv = ops.cast(qkv, dt) if dt != torch.float32 else qkv
    q4, k4, v4 = ops.qkv_post(qkv, st["inv_freq"], B, T, nh, nh, d, st["q_fold"])
    lse = torch.empty((B, nh, T), dtype=torch.float32, device=x.device) if keep or with_lse else None
    ao = ops.attention(q4, k4, v4, st["key_mask"], st["kv_info"], d, 1.0, False, log2_scores=st["l2s"], lse=lse)
    if keep:
        rec.update(q=q4, k=k4, v=v4, lse=lse, ao=ao)
    _, rec["u_attention.output.dense"] = lin["attention.output.dense"].forward(ao, resid=x, keep_u=keep)
    rec["x_mid"] = (x if stop else x.clone()) if keep else None
    h2 = ops.layernorm(x, f32v(p + "LayerNorm.weight"), f32v(p + "LayerNorm.bias"), eps, out_dtype=dt)
    fc1 = lin["intermediate.dense"]
    if fc1.ab is None:                                  # the fused bias + GELU epilogue, keeping Z
        z = torch.empty((M, round_up(F, 64)), dtype=dt, device=x.device)
        act = ops.gemm_nt(h2, fc1.w, fc1.bias, n=F, k=H, epilogue=_lib.EPI_GELU, out_dtype=dt, z=z)
    else:                                               # the branch lands BEFORE the GELU: Z assembled in fp32, then p2t_gelu_rows
        zf, rec["u_intermediate.dense"] = fc1.forward(h2, keep_u=keep)
        act = None if stop and lin["output.dense"].ab is None else _gelu_rows(zf, None, F, dt)
        z = ops.cast(zf, dt) if dt != torch.float32 else zf
    rec["z"] = z if keep else None
    if stop:                                            # the output projection is not redone; its branch's u is, from the forward's own
        rec["u_output.dense"] = lin["output.dense"].branch_input(act)      # activation (gelu of the fp32 Z, not of the kept, rounded one)
        return rec, x
    _, rec["u_output.dense"] = lin["output.dense"].forward(act, resid=x, keep_u=keep)
    return rec, x


class EncoderLoraFn(torch.autograd.Function):
    """last_hidden_state of the ESM2 encoder ([B, T, Hp] in the model dtype, zero padded as `EsmEncoder.encode` returns it) as a
    function of the LoRA parameters (frozen base weights and embeddings)."""

    @staticmethod
    def forward(ctx, input_ids, attention_mask, encoder, lora, opts, *params):
        s, dt = encoder.spec, encoder.dtype
        B, T = input_ids.shape
        M, H, F = B * T, s.hidden_size, s.intermediate_size
        d, L = s.head_dim, s.num_hidden_layers
        Hp = round_up(H, 64)
        if H % 8 or F % 8:
            raise ValueError("the encoder LoRA step needs hidden_size and intermediate_size multiples of 8")
        P = dict(encoder.named_parameters())
        dev = P["embeddings.word_embeddings.weight"].device
        f32v = lambda n: P[n].detach().float().contiguous()
        ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
        mask = attention_mask.to(device=dev, dtype=torch.int64).contiguous()
        key_mask, kv_info, emb_scale = ops.mask_prepare(mask, ids, s.mask_token_id, s.token_dropout)
        x = torch.empty((M, H), dtype=torch.float32, device=dev)
        call("p2t_esm2_embed", ptr(ids), ptr(mask), ptr(P["embeddings.word_embeddings.weight"]), ops.dt_of(dt), ptr(emb_scale), B, T, H, s.vocab_size,
             s.mask_token_id, int(s.token_dropout), ptr(x), stream())
        inv_freq = encoder.rotary_embeddings.inv_freq.detach().float().contiguous()
        l2s = dt == torch.bfloat16                      # as p2t_esm2_forward: q carries d^-1/2 * log2 e, the logits are ln 2 * q.k
        q_fold = (1.4426950408889634 if l2s else 1.0) / math.sqrt(d)
        eps = s.layer_norm_eps
        keep = opts["keep_tape"]
        ckpt = keep and bool(opts.get("checkpoint"))    # the tape holds every layer's input alone; the backward redoes the layer
        tape = []
        st = dict(encoder=encoder, spec=s, dt=dt, P=P, tape=tape, checkpoint=ckpt, key_mask=key_mask, kv_info=kv_info, inv_freq=inv_freq, l2s=l2s,
                  q_fold=q_fold, shape=(B, T), params=params)
        for i in range(L):
            p = f"encoder.layer.{i}."
            lin = {t: LoraLinear(encoder, P, p + t, lora, i, t, dt, opts["dropout"]) for t in TARGETS}
            if ckpt:
                tape.append(dict(lin=lin, x_in=x.clone()))
            rec, x = _layer_forward(st, i, lin, x, keep and not ckpt, with_lse=ckpt)
            if keep and not ckpt:
                tape.append(rec)
        out = ops.layernorm(x, f32v("encoder.emb_layer_norm_after.weight"), f32v("encoder.emb_layer_norm_after.bias"), eps, out_dtype=dt, ld_out=Hp)
        st["x_last"] = x
        ctx.state = st if keep else None
        if keep:
            encoder.last_tape_bytes = tape_bytes(tape, (x, key_mask, kv_info))
        return out.view(B, T, Hp)

    @staticmethod
    def backward(ctx, d_out):
        st = ctx.state
        enc = st["encoder"]
        s, dt = enc.spec, enc.dtype
        B, T = st["shape"]
        M, H, F = B * T, s.hidden_size, s.intermediate_size
        nh, d = s.num_attention_heads, s.head_dim
        dp = ops.head_dim_padded(d)
        eps = s.layer_norm_eps
        P = st["P"]
        dev = st["x_last"].device
        f32v = lambda n: P[n].detach().float().contiguous()
        to_dt = lambda t: ops.cast(t, dt) if t.dtype != dt else t
        c_s = 0.6931471805599453 if st["l2s"] else 1.0

        def ln_bwd(x, name, dy, out, acc):
            call("p2t_layernorm_backward", ptr(x), x.stride(0), ptr(f32v(name)), float(eps), ptr(dy), dy.stride(0), ops.dt_of(dy), ptr(out), out.stride(0),
                 M, H, int(acc), stream())

        dy = d_out.reshape(M, -1)
        if dy.dtype not in (torch.float32, torch.bfloat16) or dy.stride(1) != 1 or dy.stride(0) % 4:
            dy = dy.float().contiguous()
        g = torch.empty((M, H), dtype=torch.float32, device=dev)
        ln_bwd(st["x_last"], "encoder.emb_layer_norm_after.weight", dy, g, 0)
        grads: dict = {}
        ta = st["checkpoint"]                           # checkpointed: every layer redone from its input; dA / dB by p2t_lora_wgrad
        for i in range(len(st["tape"]) - 1, -1, -1):
            rec = st["tape"][i]
            lin = rec["lin"]
            if ta:
                rec, _ = _layer_forward(st, i, lin, rec["x_in"], True, stop=True)
            p = f"encoder.layer.{i}."
            # ---- FFN: x2 = x1 + fc2(gelu(Z)) + b
            g16 = to_dt(g)
            z, fc2 = rec["z"], lin["output.dense"]
            if fc2.ab is None:                          # dZ = (dy W2) * gelu'(Z) in the dX GEMM's epilogue
                dz = ops.gemm_nt(g16, fc2.transposed(), None, n=F, k=H, epilogue=_lib.EPI_GELU_BWD, out_dtype=dt, z=z)
            else:                                       # gelu(Z) recomputed: the branch's dA needs fc2's input
                act = _gelu_rows(z, None, F, dt)
                d_act = fc2.backward(g16, act, rec["u_output.dense"], None, True, False, grads, token_axis=ta)
                dz = _gelu_rows(z, d_act, F, dt)
            h2 = ops.layernorm(rec["x_mid"], f32v(p + "LayerNorm.weight"), f32v(p + "LayerNorm.bias"), eps, out_dtype=dt)
            d_h2 = lin["intermediate.dense"].backward(dz, h2, rec["u_intermediate.dense"] if "u_intermediate.dense" in rec else None, None, True, False, grads, token_axis=ta)
            ln_bwd(rec["x_mid"], p + "LayerNorm.weight", d_h2, g, 1)
            # ---- attention: x1 = x + o(attn(rope(q), rope(k), v)) + b
            g16 = to_dt(g)
            d_ao = lin["attention.output.dense"].backward(g16, rec["ao"], rec["u_attention.output.dense"], None, False, False, grads, token_axis=ta)
            dq, dk, dv = ops.attention_backward(rec["q"], rec["k"], rec["v"], rec["ao"], d_ao, rec["lse"], st["key_mask"], st["kv_info"], d, c_s, False,
                                                log2_scores=st["l2s"])
            d_qkv = torch.zeros((M, round_up(3 * H, 64)), dtype=dt, device=dev)
            cs = torch.empty((T, d), dtype=torch.float32, device=dev)
            call("p2t_rope_backward_pack", ptr(dq), ptr(dk), ptr(dv), ptr(st["inv_freq"]), ptr(cs), ptr(d_qkv), d_qkv.stride(0), B, T, nh, nh, d, dp,
                 float(st["q_fold"]), ops.dt_of(dt), stream())
            h1 = ops.layernorm(rec["x_in"], f32v(p + "attention.LayerNorm.weight"), f32v(p + "attention.LayerNorm.bias"), eps, out_dtype=dt)
            d_h1 = None
            for j, t in enumerate(TARGETS[:3]):
                d_h1 = lin[t].backward(d_qkv[:, j * H:(j + 1) * H], h1, rec["u_" + t], d_h1, True, j > 0, grads, token_axis=ta)
            ln_bwd(rec["x_in"], p + "attention.LayerNorm.weight", d_h1, g, 1)
            st["tape"][i] = None
        out_params = scaled_grads(st["params"], grads)
        ctx.state = None
        return (None, None, None, None, None, *out_params)


def encoder_lora_forward(encoder, lora: EncoderLora, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor],
                         dropout: Optional[float] = None, checkpoint: bool = False) -> torch.Tensor:
    """last_hidden_state [B, T, Hp] of the encoder with the LoRA branches in the graph (what `EsmEncoder.encode` returns otherwise).
    dropout: None = `lora.p` in train mode (one mask step per call), 0 in eval mode (peft's nn.Dropout, no mask step -- what
    InstructTrainer.evaluate sets); a value overrides both and leaves the mask counter where it is.  Without gradients to compute, no activation tape is kept.
    checkpoint: gradient checkpointing -- the tape keeps each layer's fp32 input alone and the backward redoes the layer from it (same
    kernels, same dropout seeds; dA / dB then come from p2t_lora_wgrad, a differently ordered fp32 sum, every other value is
    bit-identical).  `encoder.last_tape_bytes`: the bytes of the tensors kept for the backward."""
    if input_ids is None or input_ids.dim() != 2:
        raise ValueError("protein_input_ids must be a [batch, seq_len] tensor of token ids")
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    if tuple(attention_mask.shape) != tuple(input_ids.shape):
        raise ValueError(f"protein_attention_mask shape {tuple(attention_mask.shape)} != input ids {tuple(input_ids.shape)}")
    if encoder.gemm_fp8:
        raise ValueError("stage-2 training runs the encoder GEMMs in the model dtype (set_gemm_dtype('model'))")
    params = tuple(lora.parameters())
    if dropout is None:
        if lora.training:
            lora.step_count += 1                        # a fresh dropout mask per step
        dropout = lora.p if lora.training else 0.0
    keep = torch.is_grad_enabled() and any(q.requires_grad for q in params)
    opts = dict(dropout=float(dropout), keep_tape=keep, checkpoint=bool(checkpoint))
    return EncoderLoraFn.apply(input_ids, attention_mask, encoder, lora, opts, *params)
