"""The stage-2 per-layer step (p2t_hip.decoder_train.lora_lm_loss) against the fp64 reference of tests/stage2_reference.py, at
head_dim 64 / 128 (Llama geometry with llama3 rotary, GQA) and Qwen3 (head_dim 128 with the q / k head norm), on padded and packed
batches, with and without LoRA dropout:

* fp32 HIP (FMA GEMMs, exact attention) against the unrounded reference: loss 1e-5, every gradient group 1e-4;
* bf16 HIP (MFMA GEMMs and attention) against the ROUNDING-MATCHED reference (a bf16 rounding wherever the step materialises a bf16
  tensor): what is left is kernel-internal arithmetic, held to 3e-3 (loss) / 3e-2 (groups) through observe(); the same run against
  the unrounded reference is reported as `...unmatched...` -- the ratio of the two splits the bf16 error into the step's own
  roundings and the kernels';
* bf16 with every B = 0 against the fused frozen-decoder chain (p2t_llama_train_forward / _backward), padded and packed.

The dropout keep-mask of every projection is the kernel's own: p2t_dropout_rows on a ones matrix with the projection's seed."""
import numpy as np
import pytest
import torch

import stage2_reference as S
from gpu_util import build_model, dev, observe, rel
from p2t_hip import _lib, ops, specs, synth
from p2t_hip._lib import call
from p2t_hip.decoder_train import TARGETS, _Lin, lora_lm_loss
from p2t_hip.ops import ptr, stream

pytestmark = pytest.mark.gpu

GEOM = {
    "llama_d128": dict(num_hidden_layers=2, hidden_size=1024, intermediate_size=2848, num_attention_heads=8, num_key_value_heads=2, vocab_size=4096,
                       head_dim=128, rope_type="llama3", rope_theta=500000.0, rope_factor=8.0),
    "llama_d64": dict(num_hidden_layers=2, hidden_size=512, intermediate_size=1376, num_attention_heads=8, num_key_value_heads=2, vocab_size=4096,
                      head_dim=64, rope_type="default", rope_theta=10000.0),
    "qwen3_d128": dict(num_hidden_layers=2, hidden_size=1024, intermediate_size=2848, num_attention_heads=8, num_key_value_heads=4, vocab_size=4096,
                       head_dim=128, rope_type="default", rope_theta=1000000.0, rms_norm_eps=1e-6, qk_norm=True),
}
PADDED_LENS = [200, 1, 137]                             # B = 3, ragged, one single-token description
PACKED_ROWS = ([1, 63, 65, 129, 254], [300, 129, 1, 63])  # T = 512: a full row and a row with 19 padding tokens


def _decoder(geom, dtype, seed=3):
    esm = specs.EsmSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2)
    ls = specs.LlamaSpec(**GEOM[geom])
    model = build_model(esm, ls, specs.AdapterSpec(64, 64, ls.hidden_size, 0.0), dtype, seed)
    model.requires_grad_(False)
    return model, model.llama_decoder


def _add_lora(model, init, p, r=16):
    lora = model.add_lora(r, lora_dropout=p)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for i in range(model.llama_decoder.spec.num_hidden_layers):
            for t in TARGETS:
                a, b = lora.get(i, t)
                if init == "uniform0.25":                # the goldens' scale (tests/golden/sft_lora_tiny.npz): the branch dominates q / k
                    a.copy_(torch.from_numpy(synth.uniform_f32(5, f"lora.{i}.{t}.A", tuple(a.shape), 0.25)))
                    b.copy_(torch.from_numpy(synth.uniform_f32(5, f"lora.{i}.{t}.B", tuple(b.shape), 0.25)))
                elif init == "zero_b":
                    b.zero_()
                else:                                    # peft's kaiming A (DecoderLora's own init) and a trained-looking B
                    b.copy_(torch.randn(tuple(b.shape), generator=g) * 0.02)
    return lora


def _batch(kind, V, seed=0):
    """(ids [B, T], mask, labels, docs-starts or None, position_ids or None, loss_weights or None) on the host."""
    g = torch.Generator().manual_seed(seed)
    if kind == "padded":
        T = max(PADDED_LENS) + 3
        B = len(PADDED_LENS)
        ids = torch.randint(0, V, (B, T), generator=g)
        mask = torch.zeros((B, T), dtype=torch.int64)
        labels = torch.full((B, T), -100, dtype=torch.int64)
        for b, n in enumerate(PADDED_LENS):
            mask[b, :n] = 1
            labels[b, max(1, n // 3):n] = ids[b, max(1, n // 3):n]
        return ids, mask, labels, None, None
    T = 512
    B = len(PACKED_ROWS)
    ids = torch.randint(0, V, (B, T), generator=g)
    mask = torch.zeros((B, T), dtype=torch.int64)
    pos = torch.zeros((B, T), dtype=torch.int64)
    labels = torch.full((B, T), -100, dtype=torch.int64)
    w = torch.zeros((B, T), dtype=torch.float32)
    n_docs = sum(len(r) for r in PACKED_ROWS)
    for b, lens in enumerate(PACKED_ROWS):
        t = 0
        for n in lens:
            mask[b, t:t + n] = 1
            pos[b, t:t + n] = torch.arange(n)
            s0 = t + max(1, n // 4)
            labels[b, s0:t + n] = ids[b, s0:t + n]       # a document start is never a target
            sup = t + n - s0
            if sup:
                w[b, s0:t + n] = 1.0 / (n_docs * sup)     # "sample" weighting (p2t_hip.data.pack_instruct_batch)
            t += n
    return ids, mask, labels, pos, w


def _run(model, dec, lora, kind, p):
    V = dec.spec.vocab_size
    ids, mask, labels, pos, w = _batch(kind, V)
    B, T = ids.shape
    emb = dec.model.embed_tokens.weight.detach().float()[ids.to(dev())].contiguous().requires_grad_(True)
    docs = ops.doc_prepare(pos.to(dev()), mask.to(dev())) if pos is not None else None
    wd = w.to(dev()).contiguous() if w is not None else None
    if lora is not None:
        lora.zero_grad(set_to_none=True)
    loss, _ = lora_lm_loss(dec, lora, emb, mask.to(dev()), labels.to(dev()), docs=docs, loss_weights=wd)
    loss.backward()
    keep = None
    if lora is not None and p > 0:                       # the kernel's own keep-mask of every projection input, for this step's seeds
        keep = {}
        for i in range(dec.spec.num_hidden_layers):
            for t in TARGETS:
                lin = _Lin(dec, lora, i, t, dec.model.dtype)
                seed, K = lin.seed, lin.K
                ones = torch.ones((B * T, K), dtype=torch.float32, device=dev())
                out = torch.empty_like(ones)
                call("p2t_dropout_rows", ptr(ones), _lib.F32, K, ptr(out), _lib.F32, K, B * T, K, float(p), int(seed), 0, stream())
                keep[(i, t)] = (out != 0).cpu()
    hip = dict(loss=float(loss.detach()), d_emb=emb.grad.detach().double().cpu())
    if lora is not None:
        hip["dA"] = {(i, t): lora.get(i, t)[0].grad.detach().double().cpu() for i in range(dec.spec.num_hidden_layers) for t in TARGETS}
        hip["dB"] = {(i, t): lora.get(i, t)[1].grad.detach().double().cpu() for i in range(dec.spec.num_hidden_layers) for t in TARGETS}
    starts = None if docs is None else docs[0].long().cpu()
    return hip, dict(embeds=emb.detach().cpu(), mask=mask, labels=labels, docs=starts, loss_weights=w, keep=keep)


def _reference(dec, lora, inp, p, round_):
    s = dec.spec
    W = {n: q.detach().cpu() for n, q in dec.model.named_parameters() if n != "embed_tokens.weight"}
    W["lm_head.weight"] = dec.lm_head.weight.detach().cpu()
    cfg = dict(n_layers=s.num_hidden_layers, heads=s.num_attention_heads, kv_heads=s.num_key_value_heads, head_dim=s.head_dim, eps=s.rms_norm_eps,
               inv_freq=dec.model._inv_freq().cpu(), qk_norm=s.qk_norm, vocab=s.vocab_size)
    ab = None
    if lora is not None:
        ab = {(i, t): tuple(x.detach().cpu() for x in lora.get(i, t)) for i in range(s.num_hidden_layers) for t in TARGETS}
    loss, d_emb, dA, dB = S.step(inp["embeds"], W, cfg, inp["mask"], inp["labels"], lora=ab, lora_scale=lora.scale if lora is not None else 1.0,
                                 keep=inp["keep"], p=p, docs=inp["docs"], loss_weights=inp["loss_weights"], round=round_)
    return dict(loss=float(loss), d_emb=d_emb, dA=dA, dB=dB)


def _errors(hip, ref, L):
    out = {"loss": abs(hip["loss"] - ref["loss"]) / abs(ref["loss"]), "d_emb": rel(hip["d_emb"].numpy(), ref["d_emb"].numpy())}
    for which in ("dA", "dB"):
        if which not in hip:
            continue
        for t in TARGETS:
            kind = t.split(".")[1]
            got = np.concatenate([hip[which][(i, t)].numpy().ravel() for i in range(L)])
            want = np.concatenate([ref[which][(i, t)].numpy().ravel() for i in range(L)])
            out[f"{which}.{kind}"] = rel(got, want)
    return out


CASES = [("llama_d128", "padded", "kaiming", 0.1), ("llama_d128", "packed", "kaiming", 0.0),
         ("llama_d64", "padded", "kaiming", 0.0), ("llama_d64", "packed", "kaiming", 0.1), ("qwen3_d128", "padded", "kaiming", 0.1),
         ("qwen3_d128", "packed", "kaiming", 0.0)]


@pytest.mark.parametrize("geom,kind,init,p", CASES)
def test_fp32_step_matches_the_fp64_reference(geom, kind, init, p):
    torch.manual_seed(0)
    model, dec = _decoder(geom, torch.float32)
    lora = _add_lora(model, init, p)
    hip, inp = _run(model, dec, lora, kind, p)
    ref = _reference(dec, lora, inp, p, False)
    err = _errors(hip, ref, dec.spec.num_hidden_layers)
    assert err["loss"] < 1e-5, err
    for k, e in err.items():
        assert e < 1e-4, (k, e, err)


@pytest.mark.parametrize("geom,kind,init,p", CASES)
def test_bf16_step_matches_the_rounding_matched_reference(geom, kind, init, p):
    torch.manual_seed(0)
    model, dec = _decoder(geom, torch.bfloat16)
    lora = _add_lora(model, init, p)
    hip, inp = _run(model, dec, lora, kind, p)
    L = dec.spec.num_hidden_layers
    matched = _errors(hip, _reference(dec, lora, inp, p, True), L)
    unmatched = _errors(hip, _reference(dec, lora, inp, p, False), L)
    tag = f"stage2_matched[{geom},{kind},{init},p{p}]"
    for k in matched:
        observe(f"{tag}.bf16_unmatched.{k}", unmatched[k], 1.0)           # reported: the bf16 step against exact arithmetic
    for k, e in matched.items():
        observe(f"{tag}.bf16_matched.{k}", e, 3e-3 if k == "loss" else 3e-2)


@pytest.mark.parametrize("geom", ["llama_d64", "llama_d128"])
@pytest.mark.parametrize("kind", ["padded", "packed"])
def test_bf16_lora_with_zero_b_is_the_fused_frozen_chain(geom, kind):
    """B = 0: the per-layer LoRA step and the fused frozen-decoder chain (two drivers of the same kernels) give the same loss and
    gradient at inputs_embeds -- the gradient the modality adapter trains on."""
    model, dec = _decoder(geom, torch.bfloat16)
    V = dec.spec.vocab_size
    ids, mask, labels, pos, w = _batch(kind, V)
    kw = dict(attention_mask=mask.to(dev()), labels=labels.to(dev()))
    if pos is not None:
        kw.update(position_ids=pos.to(dev()), loss_weights=w.to(dev()))
    base = dec.model.embed_tokens.weight.detach().float()[ids.to(dev())].contiguous()
    e1 = base.clone().requires_grad_(True)
    fused = dec(inputs_embeds=e1, **kw)
    fused.loss.backward()
    _add_lora(model, "zero_b", 0.0)
    e2 = base.clone().requires_grad_(True)
    per_layer = dec(inputs_embeds=e2, **kw)
    per_layer.loss.backward()
    tag = f"stage2_zero_b[{geom},{kind}]"
    observe(f"{tag}.bf16.loss", abs(float(per_layer.loss.detach()) - float(fused.loss.detach())) / abs(float(fused.loss.detach())), 2e-2)
    observe(f"{tag}.bf16.d_emb", rel(e2.grad.cpu().numpy(), e1.grad.cpu().numpy()), 2e-2)


def _kappa(dec, lora, inp, seed=1):
    """Relative change of d inputs_embeds in the fp64 reference per relative perturbation 1e-6 of inputs_embeds: the problem's own
    amplification of an input error, free of any kernel."""
    g = torch.Generator().manual_seed(seed)
    base = _reference(dec, lora, inp, 0.0, False)["d_emb"]
    e = inp["embeds"].double()
    moved = dict(inp, embeds=e * (1 + 1e-6 * torch.randn(e.shape, generator=g, dtype=torch.float64)))
    return rel(_reference(dec, lora, moved, 0.0, False)["d_emb"].numpy(), base.numpy()) / 1e-6


def test_golden_scale_lora_error_is_conditioning():
    """The LoRA scale of tests/golden/sft_lora_tiny.npz (A, B ~ uniform(0.25): the branch dominates q and k) at head_dim 128: the
    bf16 step's large error there (sft_lora[d128].bf16.*) is the problem's conditioning, not a defect of the step.  Evidence, all
    on one model and batch: the fp32 HIP step against fp64 is ~100x further off than at peft's scale (the kernels are exact fp32
    there; what grows is the amplification), and the fp64 reference's own sensitivity to a 1e-6 input perturbation grows by as much."""
    model, dec = _decoder("llama_d128", torch.float32)
    out = {}
    for init in ("kaiming", "uniform0.25"):
        lora = _add_lora(model, init, 0.0)
        hip, inp = _run(model, dec, lora, "packed", 0.0)
        err = _errors(hip, _reference(dec, lora, inp, 0.0, False), dec.spec.num_hidden_layers)
        out[init] = (max(err.values()), _kappa(dec, lora, inp))
        observe(f"stage2_conditioning[{init}].fp32.worst_group", out[init][0], 1e-3)
        observe(f"stage2_conditioning[{init}].kappa_d_emb", out[init][1], 1e6)
    (e_k, k_k), (e_u, k_u) = out["kaiming"], out["uniform0.25"]
    assert e_k < 1e-4, out                               # peft's scale: fp32 meets the tight bound
    assert k_u > 10 * k_k, out                           # the golden scale amplifies input errors an order of magnitude more
    assert e_u / e_k < 10 * k_u / k_k, out               # ... which accounts for the fp32 step's larger error there
    # the bf16 step at the golden scale, reported: matched (kernel-internal roundings, amplified) and unmatched
    model, dec = _decoder("llama_d128", torch.bfloat16)
    lora = _add_lora(model, "uniform0.25", 0.0)
    hip, inp = _run(model, dec, lora, "packed", 0.0)
    L = dec.spec.num_hidden_layers
    matched = _errors(hip, _reference(dec, lora, inp, 0.0, True), L)
    unmatched = _errors(hip, _reference(dec, lora, inp, 0.0, False), L)
    for k in matched:
        observe(f"stage2_conditioning[uniform0.25].bf16_matched.{k}", matched[k], 1.0)
        observe(f"stage2_conditioning[uniform0.25].bf16_unmatched.{k}", unmatched[k], 1.5)
