"""CPU: target resolution of `add_lora` with ESM2 module names (peft's suffix rule), the encoder LoRA's peft keys and init, the new
entry points' exports and argument checks, and the fp64 restatement of tests/esm_lora_reference.py against torch's own modules.
Nothing is launched on a GPU."""
import ctypes

import pytest
import torch

import esm_lora_reference as R
from p2t_hip import _lib, specs
from p2t_hip.decoder_train import TARGETS as DEC
from p2t_hip.encoder_train import TARGETS as ENC, EncoderLora, resolve_targets


def test_suffix_rule_selects_encoder_modules():
    assert resolve_targets(["dense"]) == ((), ("attention.output.dense", "intermediate.dense", "output.dense"))
    assert resolve_targets(["output.dense"]) == ((), ("attention.output.dense", "output.dense"))
    assert resolve_targets(["query"]) == ((), ("attention.self.query",))
    assert resolve_targets(list(DEC)) == (DEC, ())                    # the default: decoder only, in the given order
    dec, enc = resolve_targets(["self_attn.q_proj", "value", "mlp.down_proj", "dense", "attention.output.dense"])
    assert dec == ("self_attn.q_proj", "mlp.down_proj")
    assert enc == ("attention.self.value", "attention.output.dense", "intermediate.dense", "output.dense")


@pytest.mark.parametrize("bad", [["layernorm_qkv.1"], ["self_attn.q_proj", "out_proj"], ["ffn.1"], ["attention.self"], ["LayerNorm"]])
def test_names_that_match_nothing_raise(bad):
    with pytest.raises(ValueError, match="unsupported LoRA targets"):
        resolve_targets(bad)


class _Enc(torch.nn.Module):
    """The parameter names EncoderLora reads, on the CPU (no engine)."""

    def __init__(self, s):
        super().__init__()
        self.spec = s
        P = {"embeddings.word_embeddings.weight": (s.vocab_size, s.hidden_size)}
        for i in range(s.num_hidden_layers):
            for t, shp in (("attention.self.query", (s.hidden_size, s.hidden_size)), ("attention.self.key", (s.hidden_size, s.hidden_size)),
                           ("attention.self.value", (s.hidden_size, s.hidden_size)), ("attention.output.dense", (s.hidden_size, s.hidden_size)),
                           ("intermediate.dense", (s.intermediate_size, s.hidden_size)), ("output.dense", (s.hidden_size, s.intermediate_size))):
                P[f"encoder.layer.{i}.{t}.weight"] = shp
        for n, shp in P.items():
            self.register_parameter(n.replace(".", "_"), torch.nn.Parameter(torch.zeros(shp), requires_grad=False))
        self._names = list(P)

    def named_parameters(self, *a, **k):
        return [(n, getattr(self, n.replace(".", "_"))) for n in self._names]


def test_encoder_lora_init_and_peft_keys():
    s = specs.EsmSpec(num_hidden_layers=2, hidden_size=64, intermediate_size=128, num_attention_heads=4)
    lo = EncoderLora(_Enc(s), 4, None, 0.1, ("attention.self.query", "intermediate.dense", "output.dense"), seed=3)
    assert lo.alpha == 8.0 and lo.scale == 2.0 and lo.p == 0.1
    a, b = lo.get(1, "output.dense")
    assert tuple(a.shape) == (4, 128) and tuple(b.shape) == (64, 4) and float(b.abs().sum()) == 0.0
    assert float(a.abs().max()) <= 1.0 / 128 ** 0.5 and float(a.abs().max()) > 0
    keys = list(lo.peft_state_dict())
    assert keys[0] == "base_model.model.esm_encoder.encoder.layer.0.attention.self.query.lora_A.weight"
    assert "base_model.model.esm_encoder.encoder.layer.1.intermediate.dense.lora_B.weight" in keys
    assert len(keys) == 2 * 2 * 3
    assert lo.get(0, "attention.self.key") is None
    with pytest.raises(ValueError):
        EncoderLora(_Enc(s), 4, target_modules=("self_attn.q_proj",))


def test_adapter_config_lists_encoder_targets():
    from p2t_hip.instruct import adapter_config
    s = specs.EsmSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=4)
    lo = EncoderLora(_Enc(s), 8, 16.0, 0.05, ENC)
    cfg = adapter_config(lo)
    assert cfg["target_modules"] == list(ENC) and cfg["r"] == 8 and cfg["lora_alpha"] == 16.0 and cfg["lora_dropout"] == 0.05


def test_new_entry_points_exported_and_checked():
    for n in ("p2t_layernorm_backward", "p2t_gelu_rows", "p2t_esm2_embed", "p2t_adapter_backward_dx", "p2t_adapter_backward_dx_workspace_bytes"):
        assert hasattr(_lib.lib, n) and n in _lib.SIGNATURES
    with pytest.raises(ValueError, match="multiples of 4"):
        _lib.call("p2t_layernorm_backward", 1, 6, 1, 1e-5, 1, 6, 0, 1, 6, 2, 6, 0, None)
    with pytest.raises(ValueError, match="bad arguments"):
        _lib.call("p2t_gelu_rows", None, 0, 8, None, 0, 0, None, 0, 8, 4, 8, None)
    cfg = _lib.AdapterConfigC(input_dim=64, intermediate_dim=96, output_dim=64, dropout_p=0.0, dropout_seed=0, dtype=0)
    assert _lib.call("p2t_adapter_backward_dx_workspace_bytes", ctypes.byref(cfg), 10) > 0
    with pytest.raises(ValueError, match="null argument"):
        _lib.call("p2t_adapter_backward_dx", ctypes.byref(cfg), None, 10, None, None, None, 64, 0, None, 0, None)


def test_fp64_encoder_restatement_matches_torch_modules():
    """The restated EsmLayer arithmetic (rotary on q * d^-1/2, key-padding softmax, erf GELU, LayerNorms) against the same layer
    assembled from torch.nn modules, with a LoRA branch on every linear; autograd gradients of A / B agree to fp64 rounding."""
    torch.manual_seed(0)
    B, T, H, F, nh, L = 2, 7, 32, 48, 2, 2
    d = H // nh
    W = {"embeddings.word_embeddings.weight": torch.randn(33, H, dtype=torch.float64)}
    for i in range(L):
        for t, (o, k) in zip(R.ENC_TARGETS, [(H, H)] * 4 + [(F, H), (H, F)]):
            W[f"encoder.layer.{i}.{t}.weight"] = torch.randn(o, k, dtype=torch.float64) / k ** 0.5
            W[f"encoder.layer.{i}.{t}.bias"] = torch.randn(o, dtype=torch.float64) * 0.1
        for n in ("attention.LayerNorm", "LayerNorm"):
            W[f"encoder.layer.{i}.{n}.weight"] = 1 + 0.1 * torch.randn(H, dtype=torch.float64)
            W[f"encoder.layer.{i}.{n}.bias"] = 0.1 * torch.randn(H, dtype=torch.float64)
    W["encoder.emb_layer_norm_after.weight"] = torch.ones(H, dtype=torch.float64)
    W["encoder.emb_layer_norm_after.bias"] = torch.zeros(H, dtype=torch.float64)
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float) / d))
    cfg = dict(n_layers=L, heads=nh, head_dim=d, eps=1e-5, mask_id=32, token_dropout=True, inv_freq=inv)
    ids = torch.randint(4, 24, (B, T))
    ids[0, 2] = 32
    mask = torch.ones((B, T), dtype=torch.int64)
    mask[1, 4:] = 0
    lora = {(i, t): (torch.randn(3, W[f"encoder.layer.{i}.{t}.weight"].shape[1], dtype=torch.float64, requires_grad=True),
                     torch.randn(W[f"encoder.layer.{i}.{t}.weight"].shape[0], 3, dtype=torch.float64, requires_grad=True))
            for i in range(L) for t in R.ENC_TARGETS}
    out = R.encoder(W, cfg, ids, mask, lora, 0.5)

    # the same forward from torch modules: nn.LayerNorm, F.scaled_dot_product_attention, nn.GELU
    e = W["embeddings.word_embeddings.weight"][ids].masked_fill((ids == 32)[..., None], 0.0)
    e = e * 0.88 / (1 - (ids == 32).sum(-1, keepdim=True).double() / mask.sum(-1, keepdim=True).double())[..., None]
    x = e * mask[..., None]
    pos = torch.arange(T).float()[:, None] * inv
    emb = torch.cat([pos, pos], -1).double()
    rot = lambda v: v * emb.cos() + torch.cat([-v[..., d // 2:], v[..., :d // 2]], -1) * emb.sin()

    def lin(v, i, t):
        a, b = lora[(i, t)]
        return torch.nn.functional.linear(v, W[f"encoder.layer.{i}.{t}.weight"], W[f"encoder.layer.{i}.{t}.bias"]) + 0.5 * (v @ a.T) @ b.T

    for i in range(L):
        p = f"encoder.layer.{i}."
        h = torch.nn.functional.layer_norm(x, (H,), W[p + "attention.LayerNorm.weight"], W[p + "attention.LayerNorm.bias"], 1e-5)
        q, k, v = (lin(h, i, f"attention.self.{n}").view(B, T, nh, d).transpose(1, 2) for n in ("query", "key", "value"))
        o = torch.nn.functional.scaled_dot_product_attention(rot(q * d ** -0.5), rot(k), v, attn_mask=mask[:, None, None, :].bool(), scale=1.0)
        x = x + lin(o.transpose(1, 2).reshape(B, T, H), i, "attention.output.dense")
        h2 = torch.nn.functional.layer_norm(x, (H,), W[p + "LayerNorm.weight"], W[p + "LayerNorm.bias"], 1e-5)
        x = x + lin(torch.nn.GELU()(lin(h2, i, "intermediate.dense")), i, "output.dense")
    want = torch.nn.functional.layer_norm(x, (H,), None, None, 1e-5)
    assert float((out - want).abs().max()) < 1e-10
    leaves = [q for ab in lora.values() for q in ab]
    r = torch.randn_like(out)
    g1 = torch.autograd.grad((out * r).sum(), leaves)
    g2 = torch.autograd.grad((want * r).sum(), leaves)
    assert max(float((a - b).abs().max()) for a, b in zip(g1, g2)) < 1e-9


@pytest.mark.parametrize("case", ["enc_d16", "enc_d16_td", "mix_d16", "mix_d64"])
def test_fp64_restatement_reproduces_reference_class_golden(case):
    """The restatement the GPU tests compare against, against torch autograd through the REFERENCE class (HF EsmModel /
    LlamaForCausalLM / ModalityAdapter with LoRA-wrapped linears, tests/golden/make_golden_esm_lora.py): loss and every gradient.
    The golden is fp32 autograd (the reference's own precision), so 1e-6 holds for the loss only; the gradients, carried back through
    two decoder layers, the adapter and two encoder layers in fp32, sit at a few 1e-6 -- TOL = 1e-5 (observed <= 2.7e-6, loss 1.8e-7)."""
    g = R.load_golden()
    meta, m = g["meta"], g["meta"]["cases"][case]
    esm, llama = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**meta["llama"])
    ad = specs.AdapterSpec(esm.hidden_size, meta["adapter_hidden"], llama.hidden_size, 0.3)
    enc, dec = R.golden_pairs(g, case)
    t = lambda k: torch.from_numpy(g[k].copy())
    loss, dA, dB, dAd, dBd, dAdp = R.full_step(None, t(f"{case}.protein_input_ids"), t("protein_attention_mask"), t("input_ids"), t("attention_mask"),
                                                t("labels"), meta["placeholder_id"], enc, dec or None, meta["alpha"] / meta["r"],
                                                weights=R.spec_weights(esm, llama, ad, 0))
    TOL = 1e-5
    rel = lambda a, b: float((a.double() - torch.from_numpy(b).double()).norm() / torch.from_numpy(b).double().norm())
    assert abs(float(loss) - float(g[f"{case}.loss"])) <= 1e-6 * float(g[f"{case}.loss"])
    for (i, tg) in enc:
        assert rel(dA[(i, tg)], g[f"{case}.enc.{i}.{tg}.dA"]) <= TOL and rel(dB[(i, tg)], g[f"{case}.enc.{i}.{tg}.dB"]) <= TOL, (i, tg)
    for (i, tg) in dec:
        assert rel(dAd[(i, tg)], g[f"{case}.dec.{i}.{tg}.dA"]) <= TOL and rel(dBd[(i, tg)], g[f"{case}.dec.{i}.{tg}.dB"]) <= TOL, (i, tg)
    for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        assert rel(dAdp[n], g[f"{case}.grad.{n}"]) <= TOL, n
