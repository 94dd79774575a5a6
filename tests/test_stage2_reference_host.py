"""The fp64 reference of the stage-2 step (tests/stage2_reference.py) against transformers, on the CPU:

* round=False equals HF LlamaForCausalLM / Qwen3ForCausalLM in fp64 with the LoRA merged into the weights (W + s B A): loss and
  d inputs_embeds, and dA = s B^T dW', dB = s dW' A^T from the merged weight's gradient;
* its packed form (documents in one row) equals the same documents run as separate rows, to 1e-12;
* round=True stays near round=False and moves every quantity off it (the roundings are live)."""
import math

import pytest
import torch

import stage2_reference as S

transformers = pytest.importorskip("transformers")


def _case(kind, seed=0):
    torch.manual_seed(seed)
    if kind == "llama":
        cfg = dict(n_layers=2, heads=4, kv_heads=2, head_dim=32, hidden=96, ffn=160, vocab=200, eps=1e-5, qk_norm=False,
                   theta=500000.0, rope_type="llama3")
    else:
        cfg = dict(n_layers=2, heads=4, kv_heads=2, head_dim=32, hidden=64, ffn=96, vocab=200, eps=1e-6, qk_norm=True, theta=10000.0,
                   rope_type="default")
    d, H, F = cfg["head_dim"], cfg["hidden"], cfg["ffn"]
    # llama3 scaling at a short original context, so that all three wavelength bands occur at head_dim 32
    cfg["inv_freq"] = S.inv_freq_of(d, cfg["theta"], cfg["rope_type"], 8.0, 1.0, 4.0, 64)
    W = {}
    for i in range(cfg["n_layers"]):
        p = f"layers.{i}."
        shapes = {"self_attn.q_proj": (cfg["heads"] * d, H), "self_attn.k_proj": (cfg["kv_heads"] * d, H), "self_attn.v_proj": (cfg["kv_heads"] * d, H),
                  "self_attn.o_proj": (H, cfg["heads"] * d), "mlp.gate_proj": (F, H), "mlp.up_proj": (F, H), "mlp.down_proj": (H, F)}
        for t, sh in shapes.items():
            W[p + t + ".weight"] = torch.randn(sh, dtype=torch.float64) / math.sqrt(sh[1])
        W[p + "input_layernorm.weight"] = 1 + 0.1 * torch.randn(H, dtype=torch.float64)
        W[p + "post_attention_layernorm.weight"] = 1 + 0.1 * torch.randn(H, dtype=torch.float64)
        if cfg["qk_norm"]:
            W[p + "self_attn.q_norm.weight"] = 1 + 0.1 * torch.randn(d, dtype=torch.float64)
            W[p + "self_attn.k_norm.weight"] = 1 + 0.1 * torch.randn(d, dtype=torch.float64)
    W["norm.weight"] = 1 + 0.1 * torch.randn(H, dtype=torch.float64)
    W["lm_head.weight"] = torch.randn((cfg["vocab"], H), dtype=torch.float64) / math.sqrt(H)
    r, s = 4, 2.0
    lora = {}
    for i in range(cfg["n_layers"]):
        for t in S.TARGETS:
            out_f, in_f = W[f"layers.{i}.{t}.weight"].shape
            lora[(i, t)] = (torch.randn((r, in_f), dtype=torch.float64) / math.sqrt(in_f), 0.2 * torch.randn((out_f, r), dtype=torch.float64))
    return cfg, W, lora, s


def _hf(kind, cfg, W, lora, s):
    common = dict(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], intermediate_size=cfg["ffn"], num_hidden_layers=cfg["n_layers"],
                  num_attention_heads=cfg["heads"], num_key_value_heads=cfg["kv_heads"], head_dim=cfg["head_dim"], rms_norm_eps=cfg["eps"],
                  tie_word_embeddings=False, attention_bias=False)
    if kind == "llama":
        c = transformers.LlamaConfig(**common, mlp_bias=False, rope_parameters=dict(rope_type="llama3", rope_theta=cfg["theta"], factor=8.0,
                                     low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=64))
        model = transformers.LlamaForCausalLM(c)
    else:
        c = transformers.Qwen3Config(**common, rope_parameters=dict(rope_type="default", rope_theta=cfg["theta"]))
        model = transformers.Qwen3ForCausalLM(c)
    model.config._attn_implementation = "eager"
    model = model.double().eval()
    merged = {}
    sd = {}
    for name, w in W.items():
        key = name if name == "lm_head.weight" else "model." + name
        if name.endswith("_proj.weight"):
            i, t = int(name.split(".")[1]), name.split(".", 2)[2][: -len(".weight")]
            a, b = lora[(i, t)]
            w = (w + s * b @ a).clone().requires_grad_(True)
            merged[(i, t)] = w
        sd[key] = w
    missing = model.load_state_dict({k: v.detach() for k, v in sd.items()}, strict=False)
    assert not [k for k in missing.missing_keys if "rotary" not in k and "embed_tokens" not in k], missing.missing_keys
    # the merged weights as leaves, so that their gradients come back
    for (i, t), w in merged.items():
        mod = model.get_submodule(f"model.layers.{i}.{t}")
        del mod.weight
        mod.weight = w
    return model, merged


def _batch(B, T, H, lens, seed=1, V=200):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn((B, T, H), generator=g, dtype=torch.float64)
    mask = torch.zeros((B, T), dtype=torch.int64)
    labels = torch.full((B, T), -100, dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
        labels[b, 1:n] = torch.randint(0, V, (n - 1,), generator=g)
    return emb, mask, labels


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_reference_equals_transformers_with_the_lora_merged(kind):
    cfg, W, lora, s = _case(kind)
    emb, mask, labels = _batch(3, 24, cfg["hidden"], [24, 17, 5])
    loss, d_emb, dA, dB = S.step(emb, W, cfg, mask, labels, lora=lora, lora_scale=s)
    model, merged = _hf(kind, cfg, W, lora, s)
    e = emb.clone().requires_grad_(True)
    logits = model(inputs_embeds=e, attention_mask=mask).logits             # (HF's own loss upcasts to fp32: ForCausalLMLoss in fp64 here)
    hf_loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, cfg["vocab"]), labels[:, 1:].reshape(-1), ignore_index=-100)
    keys = list(merged)
    gs = torch.autograd.grad(hf_loss, [e] + [merged[k] for k in keys])
    # (HF's rotary cos / sin are fp32 values of the fp32 angle, the reference's fp64 ones: ~1e-7 between the two)
    hf = float(hf_loss.detach())
    assert abs(float(loss) - hf) < 1e-7 * hf
    rel = lambda a, b: float((a - b).norm() / b.norm())
    valid = mask.bool()                                                  # HF's rows of padding see other keys; both give them 0
    assert rel(d_emb[valid], gs[0][valid]) < 1e-6
    assert float(d_emb[~valid].abs().max()) == 0.0
    for j, k in enumerate(keys):
        a, b = lora[k]
        gw = gs[1 + j]
        assert rel(dA[k], s * b.T @ gw) < 1e-6, k
        assert rel(dB[k], s * gw @ a.T) < 1e-6, k


@pytest.mark.parametrize("kind", ["llama", "qwen3"])
def test_packed_reference_equals_separate_rows(kind):
    cfg, W, lora, s = _case(kind, seed=2)
    lens = [1, 7, 12, 3]
    T = sum(lens) + 2                                                    # two padding tokens at the end of the packed row
    H = cfg["hidden"]
    g = torch.Generator().manual_seed(5)
    emb = torch.randn((1, T, H), generator=g, dtype=torch.float64)
    labels = torch.randint(0, cfg["vocab"], (1, T), generator=g)
    mask = torch.zeros((1, T), dtype=torch.int64)
    mask[0, :sum(lens)] = 1
    docs = torch.zeros((1, T), dtype=torch.int64)
    starts = []
    t = 0
    for n in lens:
        docs[0, t:t + n] = t
        starts.append(t)
        labels[0, t] = -100                                              # a document start is never a target
        t += n
    docs[0, t:] = torch.arange(t, T)                                     # padding: a document of its own (position 0)
    labels[0, t:] = -100
    wts = torch.rand((1, T), generator=g, dtype=torch.float64).float()
    loss, d_emb, dA, dB = S.step(emb, W, cfg, mask, labels, lora=lora, lora_scale=s, docs=docs, loss_weights=wts)
    # the same documents as separate rows, right-padded to the longest
    Tm = max(lens)
    eb = torch.zeros((len(lens), Tm, H), dtype=torch.float64)
    mb = torch.zeros((len(lens), Tm), dtype=torch.int64)
    lb = torch.full((len(lens), Tm), -100, dtype=torch.int64)
    wb = torch.zeros((len(lens), Tm), dtype=torch.float32)
    for j, (st, n) in enumerate(zip(starts, lens)):
        eb[j, :n], mb[j, :n], lb[j, :n], wb[j, :n] = emb[0, st:st + n], 1, labels[0, st:st + n], wts[0, st:st + n]
    loss2, d2, dA2, dB2 = S.step(eb, W, cfg, mb, lb, lora=lora, lora_scale=s, loss_weights=wb)
    assert abs(float(loss) - float(loss2)) < 1e-12 * abs(float(loss2))
    for j, (st, n) in enumerate(zip(starts, lens)):
        assert float((d_emb[0, st:st + n] - d2[j, :n]).abs().max()) < 1e-12 * float(d2.abs().max())
    assert float(d_emb[0, sum(lens):].abs().max()) == 0.0
    for k in dA:
        assert float((dA[k] - dA2[k]).abs().max()) <= 1e-12 * float(dA2[k].abs().max()), k
        assert float((dB[k] - dB2[k]).abs().max()) <= 1e-12 * float(dB2[k].abs().max()), k


def test_rounding_is_live_and_small():
    cfg, W, lora, s = _case("llama", seed=3)
    W = {k: S.bf16(v) for k, v in W.items()}
    emb, mask, labels = _batch(2, 16, cfg["hidden"], [16, 9], seed=4)
    keep = {(i, t): torch.rand((32, W[f"layers.{i}.{t}.weight"].shape[1])) > 0.1 for i in range(2) for t in S.TARGETS}
    a = S.step(emb, W, cfg, mask, labels, lora=lora, lora_scale=s, keep=keep, p=0.1)
    b = S.step(emb, W, cfg, mask, labels, lora=lora, lora_scale=s, keep=keep, p=0.1, round=True)
    assert 0 < abs(float(a[0]) - float(b[0])) < 1e-2 * float(a[0])
    e = float((a[1] - b[1]).norm() / a[1].norm())
    assert 1e-5 < e < 5e-2
    for k in a[2]:
        assert 1e-5 < float((a[2][k] - b[2][k]).norm() / a[2][k].norm()) < 1e-1, k
    # a keep-mask of zeros on one projection removes that branch's dA
    keep0 = dict(keep)
    keep0[(1, "mlp.up_proj")] = torch.zeros_like(keep[(1, "mlp.up_proj")])
    c = S.step(emb, W, cfg, mask, labels, lora=lora, lora_scale=s, keep=keep0, p=0.1)
    assert float(c[2][(1, "mlp.up_proj")].abs().max()) == 0.0
