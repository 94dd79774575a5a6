"""fp64 reference of the stage-2 per-layer step (p2t_hip/decoder_train.py), plain torch on the CPU.

`step(...)` is the LM loss of a Llama / Qwen3 decoder fed `inputs_embeds`, with LoRA branches y = W x + s B (A drop(x)) on the seven
projections, differentiated by torch autograd in fp64: (loss, d inputs_embeds, {key: dA}, {key: dB}).  It restates HF
LlamaDecoderLayer / Qwen3DecoderLayer (pre-norm residual blocks, GQA attention with rotary, SwiGLU MLP, final RMSNorm, LM head,
the shifted cross-entropy of ForCausalLMLoss) without the library, so that it can also express what HF cannot:

* packed rows: `docs` = per-token document starts [B, T]; attention is confined to each document (a block-diagonal causal mask)
  and the rotary position is the position inside the document;
* per-target loss weights (loss = sum of weight * token loss, the weight sitting at the label position);
* LoRA dropout through an explicit keep-mask per projection (the kernel's own mask, read back by the GPU tests);
* round=True: a bf16 rounding wherever decoder_train.py materialises a bf16 tensor, in the forward (the value) or in the backward
  (the gradient), as `R` / `G` mark them in `step`.  Roundings inside a kernel (the bf16 P of the MFMA attention) are not mirrored:
  what remains between the bf16 HIP step and this reference is kernel-internal arithmetic only.

The angle of the rotary is fp32(t * inv_freq) with an fp32 inv_freq, as the kernels' table and HF's rotary embedding compute it;
everything after it is fp64.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

TARGETS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


def bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 through fp32 (what a kernel's fp32 result stored as bf16 is), back in the input dtype."""
    return x.float().bfloat16().to(x.dtype)


class _RoundValue(torch.autograd.Function):
    """forward: bf16(x); backward: the gradient as it is (the kernels differentiate at the rounded value they stored)."""

    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """forward: x as it is; backward: bf16(gradient) (a gradient the backward materialises in bf16)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


def inv_freq_of(head_dim: int, theta: float, rope_type: str = "default", factor: float = 8.0, low_ff: float = 1.0, high_ff: float = 4.0,
                original_max_pos: int = 8192) -> torch.Tensor:
    """fp32 inv_freq of HF's default / llama3 rotary (modeling_rope_utils), the table the decoder hands its kernels."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float) / head_dim))
    if rope_type == "llama3":
        low_wl, high_wl = original_max_pos / low_ff, original_max_pos / high_ff
        wavelen = 2 * math.pi / inv
        inv_l = torch.where(wavelen > low_wl, inv / factor, inv)
        smooth = (original_max_pos / wavelen - low_ff) / (high_ff - low_ff)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        medium = ~(wavelen < high_wl) * ~(wavelen > low_wl)
        inv = torch.where(medium, smoothed, inv_l)
    return inv.float()


def rope_cos_sin(inv_freq: torch.Tensor, pos: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos, sin [..., d/2] in fp64 of the fp32 angle fp32(pos) * inv_freq."""
    ang = pos.to(torch.float32)[..., None] * inv_freq.to(torch.float32)
    ang = ang.double()
    return torch.cos(ang), torch.sin(ang)


def rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """HF rotate_half form: x [..., d] = (x1, x2) -> (x1 c - x2 s, x2 c + x1 s)."""
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    return w * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps))


def positions_of(docs: Optional[torch.Tensor], B: int, T: int) -> torch.Tensor:
    t = torch.arange(T).expand(B, T)
    return t if docs is None else t - docs


def allowed(mask: torch.Tensor, docs: Optional[torch.Tensor]) -> torch.Tensor:
    """[B, T(query), T(key)]: causal, key under the mask, and (packed rows) query and key in the same document."""
    B, T = mask.shape
    i = torch.arange(T)
    ok = (i[None, :, None] >= i[None, None, :]) & (mask[:, None, :] != 0)
    if docs is not None:
        ok = ok & (docs[:, :, None] == docs[:, None, :])
    return ok


def step(embeds: torch.Tensor, weights: Dict[str, torch.Tensor], cfg: dict, mask: torch.Tensor, labels: torch.Tensor, *,
         lora: Optional[Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]]] = None, lora_scale: float = 1.0,
         keep: Optional[Dict[Tuple[int, str], torch.Tensor]] = None, p: float = 0.0, docs: Optional[torch.Tensor] = None,
         loss_weights: Optional[torch.Tensor] = None, round: bool = False):
    """embeds [B, T, H]; weights: HF parameter names of LlamaForCausalLM without the "model." prefix ("layers.0.self_attn.q_proj.weight",
    ..., "norm.weight", "lm_head.weight"); cfg: n_layers, heads, kv_heads, head_dim, eps, inv_freq (fp32), qk_norm, vocab;
    lora {(layer, target): (A [r, in], B [out, r])} with scale s = alpha / r; keep {(layer, target): bool [B*T, in]} the dropout
    keep-mask of that projection's input (None: no dropout); docs: [B, T] document starts of packed rows (None: an ordinary batch);
    loss_weights [B, T] (None: the token mean).  Returns (loss, d embeds, {key: dA}, {key: dB}) in fp64."""
    f64 = torch.float64
    R = _RoundValue.apply if round else (lambda t: t)
    G = _RoundGrad.apply if round else (lambda t: t)
    B, T, H = embeds.shape
    M = B * T
    nh, nkv, d, L = cfg["heads"], cfg["kv_heads"], cfg["head_dim"], cfg["n_layers"]
    eps, V = cfg["eps"], cfg["vocab"]
    W = {k: v.detach().to(f64) for k, v in weights.items()}
    x0 = embeds.detach().to(f64).reshape(M, H).clone().requires_grad_(True)
    leaves = {}
    ab = {}
    for key, (a, b) in (lora or {}).items():
        a, b = a.detach().to(f64).requires_grad_(True), b.detach().to(f64).requires_grad_(True)
        leaves[key] = (a, b)
        ab[key] = (R(a), R(b * lora_scale))            # a16, bs16 = bf16(s B)
    fold = d ** -0.5 * LOG2E                            # the bf16 step folds scale * log2 e into q and takes ln 2 * q.k; the same in fp64
    cos, sin = rope_cos_sin(cfg["inv_freq"], positions_of(docs, B, T))                  # [B, T, d/2]
    cos, sin = cos[:, None], sin[:, None]
    ok = allowed(mask, docs)[:, None]                                                    # [B, 1, T, T]
    seen = ok.any(-1, keepdim=True)                     # a padding token of a packed row sees no key: its output is 0

    def proj(x, i, t, dx_bf16):
        """y = W x + s B (A drop(x)); dx_bf16: this projection's dX is a bf16 tensor (o_proj / down_proj): the W GEMM's dX is rounded,
        then the branch's share is accumulated into it (p2t_dropout_rows accumulate=1), rounded again."""
        w = W[f"layers.{i}.{t}.weight"]
        key = (i, t)
        if key not in ab:
            return (G(x) if dx_bf16 else x) @ w.T
        if dx_bf16:
            x = G(x)
        y = (G(x) if dx_bf16 else x) @ w.T
        a16, bs16 = ab[key]
        xd = x
        if keep is not None and key in keep and p > 0:
            xd = R(x * keep[key].to(f64) * float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)))
        u = G(R(xd @ a16.T))                                                             # u stored bf16; du = bf16(dy (s B))
        return y + u @ bs16.T

    x = x0
    for i in range(L):
        pre = f"layers.{i}."
        h = R(rmsnorm(x, W[pre + "input_layernorm.weight"], eps))
        q, k, v = (proj(h, i, f"self_attn.{n}_proj", False) for n in "qkv")
        if cfg.get("qk_norm"):
            q = rmsnorm(G(q).view(M, nh, d), W[pre + "self_attn.q_norm.weight"], eps).reshape(M, nh * d)
            k = rmsnorm(G(k).view(M, nkv, d), W[pre + "self_attn.k_norm.weight"], eps).reshape(M, nkv * d)
        qkv = G(R(torch.cat([q, k, v], 1)))                                              # qkv bf16; d_qkv bf16 (p2t_rope_backward_pack)
        q, k, v = qkv[:, :nh * d], qkv[:, nh * d:(nh + nkv) * d], qkv[:, (nh + nkv) * d:]
        q = q.view(B, T, nh, d).transpose(1, 2)
        k = k.view(B, T, nkv, d).transpose(1, 2)
        v = v.reshape(B, T, nkv, d).transpose(1, 2)
        q = R(rotate(q * fold, cos, sin))
        k = R(rotate(k, cos, sin))
        rep = nh // nkv
        k, v = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
        s = (q @ k.transpose(-1, -2)) * LN2
        s = s.masked_fill(~ok, float("-inf")).masked_fill(~seen, 0.0)
        ao = R(((torch.softmax(s, -1) * seen) @ v).transpose(1, 2).reshape(M, nh * d))
        x = x + G(proj(ao, i, "self_attn.o_proj", True))
        h2 = R(rmsnorm(x, W[pre + "post_attention_layernorm.weight"], eps))
        g = G(R(proj(h2, i, "mlp.gate_proj", False)))
        up = G(R(proj(h2, i, "mlp.up_proj", False)))
        act = R(g * torch.sigmoid(g) * up)
        x = x + G(proj(act, i, "mlp.down_proj", True))
    hN = R(rmsnorm(x, W["norm.weight"], eps))
    logits = G(R(hN @ W["lm_head.weight"].T)).view(B, T, V)
    lab = labels.to(torch.int64)
    tgt = torch.full_like(lab, -100)
    tgt[:, :-1] = lab[:, 1:]
    valid = (tgt >= 0) & (tgt < V)
    lp = torch.log_softmax(logits, -1)
    tok = -lp.gather(-1, tgt.clamp(0, V - 1)[..., None])[..., 0]
    if loss_weights is None:
        loss = tok[valid].sum() / valid.sum()
    else:
        w = torch.zeros_like(tok)
        w[:, :-1] = loss_weights.to(f64)[:, 1:]
        loss = (tok * w)[valid].sum()
    keys = list(leaves)
    grads = torch.autograd.grad(loss, [x0] + [leaves[q][0] for q in keys] + [leaves[q][1] for q in keys], allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g
    dA = {q: z(grads[1 + j], leaves[q][0]) for j, q in enumerate(keys)}
    dB = {q: z(grads[1 + len(keys) + j], leaves[q][1]) for j, q in enumerate(keys)}
    return loss.detach(), grads[0].view(B, T, H), dA, dB
