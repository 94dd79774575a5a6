"""fp64 reference of the stage-2 step with LoRA on the ESM2 encoder (p2t_hip/encoder_train.py), plain torch on the CPU.

`encoder(...)` restates HF EsmModel(add_pooling_layer=False).forward (transformers/models/esm/modeling_esm.py) for rotary ESM2
checkpoints -- token-dropout embeddings, pre-LN layers with q * d^-1/2 before the rotate-half rotary, bidirectional attention over
right-padded keys, erf GELU, the final emb_layer_norm_after -- with LoRA branches y = W x + b + s B (A drop(x)) on any of the six
linears of a layer.  `adapter` is ModalityAdapter.forward in eval mode.  `full_step` chains encoder -> adapter -> the placeholder
scatter -> the decoder step of tests/stage2_reference.py and returns the loss and every gradient the stage-2 step trains.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

import stage2_reference as S

ENC_TARGETS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "intermediate.dense", "output.dense")
f64 = torch.float64


def layer_norm(x, w, b, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps)


def encoder(W: Dict[str, torch.Tensor], cfg: dict, ids: torch.Tensor, mask: torch.Tensor, lora: Optional[dict] = None, scale: float = 1.0,
            keep: Optional[dict] = None, p: float = 0.0) -> torch.Tensor:
    """W: the encoder's parameters (EsmEncoder.named_parameters() names) in fp64; cfg: n_layers, heads, head_dim, eps, mask_id,
    token_dropout, inv_freq (fp32); lora {(layer, target): (A, B)} (autograd leaves or not); keep {(layer, target): bool [B*T, in]}
    dropout keep-masks with probability p.  -> last_hidden_state [B, T, H]."""
    B, T = ids.shape
    H = W["embeddings.word_embeddings.weight"].shape[1]
    M, nh, d = B * T, cfg["heads"], cfg["head_dim"]
    eps = cfg["eps"]
    e = W["embeddings.word_embeddings.weight"][ids]
    if cfg["token_dropout"]:
        is_mask = ids == cfg["mask_id"]
        e = e.masked_fill(is_mask[..., None], 0.0)
        ratio = is_mask.sum(-1).to(f64) / mask.sum(-1).to(f64)
        e = e * (1.0 - 0.15 * 0.8) / (1.0 - ratio)[:, None, None]
    x = (e * mask[..., None].to(f64)).reshape(M, H)
    cos, sin = S.rope_cos_sin(cfg["inv_freq"], torch.arange(T))                       # [T, d/2]
    ok = (mask[:, None, None, :] != 0)                                                   # [B, 1, 1, T(key)]

    def lin(v, i, t):
        pre = f"encoder.layer.{i}.{t}."
        y = v @ W[pre + "weight"].T + W[pre + "bias"]
        if lora and (i, t) in lora:
            a, b = lora[(i, t)]
            vd = v
            if keep is not None and (i, t) in keep and p > 0:
                vd = v * keep[(i, t)].to(f64) * float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
            y = y + scale * ((vd @ a.to(f64).T) @ b.to(f64).T)
        return y

    for i in range(cfg["n_layers"]):
        pre = f"encoder.layer.{i}."
        h = layer_norm(x, W[pre + "attention.LayerNorm.weight"], W[pre + "attention.LayerNorm.bias"], eps)
        q, k, v = (lin(h, i, f"attention.self.{n}").view(B, T, nh, d).transpose(1, 2) for n in ("query", "key", "value"))
        q = S.rotate(q * d ** -0.5, cos, sin)
        k = S.rotate(k, cos, sin)
        s = (q @ k.transpose(-1, -2)).masked_fill(~ok, float("-inf"))
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(M, nh * d)
        x = x + lin(o, i, "attention.output.dense")
        h2 = layer_norm(x, W[pre + "LayerNorm.weight"], W[pre + "LayerNorm.bias"], eps)
        x = x + lin(torch.nn.functional.gelu(lin(h2, i, "intermediate.dense")), i, "output.dense")
    return layer_norm(x, W["encoder.emb_layer_norm_after.weight"], W["encoder.emb_layer_norm_after.bias"], eps).view(B, T, H)


def adapter(Wa: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """normalize(gelu(fc2(gelu(fc1(x))))) (eval mode)."""
    g = torch.nn.functional.gelu
    y = g(g(x @ Wa["fc1.weight"].T + Wa["fc1.bias"]) @ Wa["fc2.weight"].T + Wa["fc2.bias"])
    return torch.nn.functional.normalize(y, p=2, dim=-1)


def model_weights(model):
    """(encoder W, adapter W, decoder W for stage2_reference.step, encoder cfg, decoder cfg) of an Esm2LlamaInstructForCausalLM, fp64 on the CPU."""
    cpu = lambda t: t.detach().to("cpu", f64)
    enc = model.esm_encoder
    We = {n: cpu(q) for n, q in enc.named_parameters() if not n.startswith("lora.")}
    Wa = {n: cpu(q) for n, q in model.adapter.named_parameters()}
    dec = model.llama_decoder
    Wd = {n[len("model."):] if n.startswith("model.") else n: cpu(q) for n, q in dec.named_parameters() if not n.startswith("lora.")}
    if "lm_head.weight" not in Wd:
        Wd["lm_head.weight"] = Wd["embed_tokens.weight"]
    es, ls = enc.spec, dec.spec
    ecfg = dict(n_layers=es.num_hidden_layers, heads=es.num_attention_heads, head_dim=es.head_dim, eps=es.layer_norm_eps, mask_id=es.mask_token_id,
                token_dropout=bool(es.token_dropout), inv_freq=enc.rotary_embeddings.inv_freq.detach().float().cpu())
    dcfg = dict(n_layers=ls.num_hidden_layers, heads=ls.num_attention_heads, kv_heads=ls.num_key_value_heads, head_dim=ls.head_dim,
                eps=ls.rms_norm_eps, inv_freq=dec.model._inv_freq().detach().float().cpu(), qk_norm=ls.qk_norm, vocab=ls.vocab_size)
    return We, Wa, Wd, ecfg, dcfg


def spec_weights(esm, llama, ad, seed: int = 0):
    """model_weights of the synthetic model of `seed` (Esm2LlamaInstructForCausalLM.from_specs / make_golden.build_reference_model),
    materialised on the host without building it."""
    from p2t_hip import specs
    def mat(tensors, prefix):
        return {n[len(prefix):]: torch.from_numpy(v).to(f64) for n, v in specs.materialize(tensors, seed).items()}
    We = mat(specs.esm_tensors(esm, "esm_encoder."), "esm_encoder.")
    Wa = mat(specs.adapter_tensors(ad, "adapter."), "adapter.")
    Wd = {n[len("model."):] if n.startswith("model.") else n: t for n, t in mat(specs.llama_tensors(llama, "llama_decoder."), "llama_decoder.").items()}
    if "lm_head.weight" not in Wd:
        Wd["lm_head.weight"] = Wd["embed_tokens.weight"]
    d = esm.head_dim
    ecfg = dict(n_layers=esm.num_hidden_layers, heads=esm.num_attention_heads, head_dim=d, eps=esm.layer_norm_eps, mask_id=esm.mask_token_id,
                token_dropout=bool(esm.token_dropout), inv_freq=1.0 / (esm.rope_theta ** (torch.arange(0, d, 2, dtype=torch.float) / d)))
    dcfg = dict(n_layers=llama.num_hidden_layers, heads=llama.num_attention_heads, kv_heads=llama.num_key_value_heads, head_dim=llama.head_dim,
                eps=llama.rms_norm_eps, qk_norm=llama.qk_norm, vocab=llama.vocab_size,
                inv_freq=S.inv_freq_of(llama.head_dim, llama.rope_theta, llama.rope_type, llama.rope_factor, llama.rope_low_freq_factor,
                                       llama.rope_high_freq_factor, llama.rope_original_max_position_embeddings))
    return We, Wa, Wd, ecfg, dcfg


def full_step(model, pid, pmask, ids, mask, labels, placeholder_id: int, enc_lora: Optional[dict], dec_lora: Optional[dict], scale: float,
              weights=None):
    """Loss and gradients of the stage-2 step in fp64: (loss, {(i, t): dA}, {(i, t): dB} of the encoder, the same of the decoder,
    {adapter parameter name: gradient}).  weights: spec_weights(...) instead of reading `model`'s parameters."""
    We, Wa, Wd, ecfg, dcfg = model_weights(model) if weights is None else weights
    Wa = {n: t.clone().requires_grad_(True) for n, t in Wa.items()}
    leaves = {k: (a.detach().to(f64).clone().requires_grad_(True), b.detach().to(f64).clone().requires_grad_(True)) for k, (a, b) in (enc_lora or {}).items()}
    h = encoder(We, ecfg, pid, pmask, leaves, scale)
    y = adapter(Wa, h)
    emb = Wd["embed_tokens.weight"][ids].clone()
    sel = ids == placeholder_id
    emb[sel] = y[pmask.bool()]
    loss, d_emb, dA_dec, dB_dec = S.step(emb.detach(), Wd, dcfg, mask, labels, lora=dec_lora, lora_scale=scale)
    keys = list(leaves)
    flat = [leaves[k][0] for k in keys] + [leaves[k][1] for k in keys] + list(Wa.values())
    g = torch.autograd.grad(emb, flat, d_emb, allow_unused=True)
    z = lambda gg, t: torch.zeros_like(t) if gg is None else gg
    n = len(keys)
    dA = {k: z(g[j], leaves[k][0]) for j, k in enumerate(keys)}
    dB = {k: z(g[n + j], leaves[k][1]) for j, k in enumerate(keys)}
    dAd = {n_: z(g[2 * n + j], t) for j, (n_, t) in enumerate(Wa.items())}
    return loss, dA, dB, dA_dec, dB_dec, dAd


# ---- tests/golden/sft_esm_lora_tiny.npz (make_golden_esm_lora.py: torch autograd through the reference class)
def load_golden():
    import json
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sft_esm_lora_tiny.npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(bytes(g.pop("meta_json")).decode())
    return g


def golden_pairs(g, case: str):
    """({(layer, target): (A, B)} of the encoder, the same of the decoder) of a golden case, fp32 CPU tensors."""
    from p2t_hip import specs, synth
    meta = g["meta"]
    m = meta["cases"][case]
    esm, llama = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**meta["llama"])
    r = meta["r"]
    shapes = {"attention.self.query": (esm.hidden_size, esm.hidden_size), "attention.self.key": (esm.hidden_size, esm.hidden_size),
              "attention.self.value": (esm.hidden_size, esm.hidden_size), "attention.output.dense": (esm.hidden_size, esm.hidden_size),
              "intermediate.dense": (esm.intermediate_size, esm.hidden_size), "output.dense": (esm.hidden_size, esm.intermediate_size)}
    H, F, d = llama.hidden_size, llama.intermediate_size, llama.head_dim
    nq, nkv = llama.num_attention_heads * d, llama.num_key_value_heads * d
    shapes.update({"self_attn.q_proj": (nq, H), "self_attn.k_proj": (nkv, H), "self_attn.v_proj": (nkv, H), "self_attn.o_proj": (H, nq),
                   "mlp.gate_proj": (F, H), "mlp.up_proj": (F, H), "mlp.down_proj": (H, F)})
    out = []
    for targets, n_layers, tag in ((m["enc_targets"], esm.num_hidden_layers, meta["enc_lora_tag"]), (m["dec_targets"], llama.num_hidden_layers, "")):
        pairs = {}
        for i in range(n_layers):
            for t in targets:
                o, k = shapes[t]
                pairs[(i, t)] = (torch.from_numpy(synth.uniform_f32(meta["lora_seed"], f"lora.{i}.{tag}{t}.A", (r, k), 0.25)),
                                 torch.from_numpy(synth.uniform_f32(meta["lora_seed"], f"lora.{i}.{tag}{t}.B", (o, r), 0.25)))
        out.append(pairs)
    return out[0], out[1]
