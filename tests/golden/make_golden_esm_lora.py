"""Golden vectors of the stage-2 step with LoRA on the ESM2 encoder, produced by torch autograd through the REFERENCE class
(models/modeling_esm2llama_instruct.py, HF EsmModel + LlamaForCausalLM, the ModalityAdapter), imported as make_golden.py imports it.

Every targeted linear of the encoder (and, in the mixed cases, of the decoder) is wrapped by make_golden._LoraLinear -- peft's
LoRA arithmetic y = W x + (alpha / r) B (A x), r = 4, alpha = 8, lora_dropout 0 -- and the modality adapter is trainable
(modules_to_save).  fp32 autograd, as the reference runs (its additive attention masks assume fp32).  The encoder runs under autograd, as in the reference (:174-193).  Cases:

    enc_d16      ESM head_dim 16, the six encoder linears, no decoder LoRA
    enc_d16_td   the same with <mask> tokens in two proteins (token dropout's rescale)
    mix_d16      ESM head_dim 16: query, value, output.dense + the seven decoder projections
    mix_d64      ESM head_dim 64: the six encoder linears + v_proj, up_proj

The proteins are unequal and right-padded (make_golden.sft_batch).  Recorded: the loss, dA / dB of every wrapped (layer, target)
of both towers and the adapter's four gradients.  CPU; writes tests/golden/sft_esm_lora_tiny.npz.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import LORA_TARGETS, _LoraLinear, build_reference_model, load_reference, lora_init, sft_batch  # noqa: E402
from p2t_hip import specs  # noqa: E402

ENC_TARGETS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "intermediate.dense", "output.dense")
LLAMA = specs.LlamaSpec(num_hidden_layers=2, hidden_size=64, intermediate_size=160, num_attention_heads=4, num_key_value_heads=2, vocab_size=512)
ESM16 = specs.EsmSpec(num_hidden_layers=2, hidden_size=64, intermediate_size=128, num_attention_heads=4)
ESM64 = specs.EsmSpec(num_hidden_layers=2, hidden_size=128, intermediate_size=256, num_attention_heads=2)
CASES = {
    "enc_d16": (ESM16, ENC_TARGETS, (), False),
    "enc_d16_td": (ESM16, ENC_TARGETS, (), True),
    "mix_d16": (ESM16, ("attention.self.query", "attention.self.value", "output.dense"), LORA_TARGETS, False),
    "mix_d64": (ESM64, ENC_TARGETS, ("self_attn.v_proj", "mlp.up_proj"), False),
}
R, ALPHA, LORA_SEED, PLACEHOLDER = 4, 8.0, 5, 511
MASKED = ((0, 3), (1, 2))                               # (row, column) of the proteins that get <mask> in the *_td cases


def _wrap(module, name, layer, tag, wrapped):
    parent_name, leaf = name.rsplit(".", 1)
    parent = module
    for p in parent_name.split("."):
        parent = getattr(parent, p)
    base = getattr(parent, leaf)
    a, b = lora_init(LORA_SEED, layer, tag, R, base.out_features, base.in_features)
    w = _LoraLinear(base, R, ALPHA, a, b)
    setattr(parent, leaf, w)
    wrapped[(layer, name)] = w


def run(ref):
    lens = [10, 6, 3]
    pid0, pmask, ids, mask, labels = sft_batch(3, lens, 18, 9, PLACEHOLDER, 510, 500, 7)
    t = torch.from_numpy
    out, metas = {}, {}
    for name, (esm, enc_t, dec_t, masked) in CASES.items():
        model = build_reference_model(ref, esm, LLAMA, specs.AdapterSpec(esm.hidden_size, 96, LLAMA.hidden_size, 0.3), 0)
        model.config.placeholder_id = PLACEHOLDER
        model.adapter.requires_grad_(True)
        enc, dec = {}, {}
        for i, layer in enumerate(model.esm_encoder.encoder.layer):
            for tg in enc_t:
                _wrap(layer, tg, i, "esm." + tg, enc)
        for i, layer in enumerate(model.llama_decoder.model.layers):
            for tg in dec_t:
                _wrap(layer, tg, i, tg, dec)
        pid = pid0.copy()
        if masked:
            for r_, c in MASKED:
                pid[r_, c] = esm.mask_token_id
        res = model(input_ids=t(ids), attention_mask=t(mask), labels=t(labels), protein_input_ids=t(pid), protein_attention_mask=t(pmask))
        res.loss.backward()
        out[f"{name}.loss"] = np.float32(res.loss.item())
        out[f"{name}.protein_input_ids"] = pid
        for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
            out[f"{name}.grad.{n}"] = dict(model.adapter.named_parameters())[n].grad.numpy().astype(np.float32)
        for tower, wrapped in (("enc", enc), ("dec", dec)):
            for (i, tg), w in wrapped.items():
                out[f"{name}.{tower}.{i}.{tg}.dA"] = w.lora_A.grad.numpy().astype(np.float32)
                out[f"{name}.{tower}.{i}.{tg}.dB"] = w.lora_B.grad.numpy().astype(np.float32)
        metas[name] = dict(esm=specs.spec_dict(esm), enc_targets=list(enc_t), dec_targets=list(dec_t), masked=masked)
        gmax = max(float(w.lora_A.grad.norm()) for w in enc.values())
        print(f"sft_esm_lora {name}: loss {float(res.loss):.6f} max |enc dA| {gmax:.3e} |g fc1.w| {float(model.adapter.fc1.weight.grad.norm()):.4e}")
    meta = dict(cases=metas, llama=specs.spec_dict(LLAMA), adapter_hidden=96, placeholder_id=PLACEHOLDER, lens=lens, r=R, alpha=ALPHA,
                lora_seed=LORA_SEED, enc_lora_tag="esm.")
    path = os.path.join(HERE, "sft_esm_lora_tiny.npz")
    np.savez_compressed(path, protein_attention_mask=pmask, input_ids=ids, attention_mask=mask, labels=labels,
                        meta_json=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **out)
    print(f"wrote {path}")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    run(load_reference())
