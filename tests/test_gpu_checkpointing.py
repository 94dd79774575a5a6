"""Gradient checkpointing in the stage-2 LoRA steps (p2t_hip/decoder_train.py, p2t_hip/encoder_train.py): with
`gradient_checkpointing_enable()` the tape keeps each layer's fp32 input alone and the backward redoes the layer from it.

The recompute runs the same kernels on the same inputs in the same order with the same dropout seeds, so the loss, the gradient at
`inputs_embeds` and the adapter's gradients must be BIT-identical to the full-tape step.  Only dA / dB may differ: the checkpointed
backward sums them over the token axis in p2t_lora_wgrad's order.  Both are fp32 sums of the same products over at most a few hundred
tokens here; the summation bound M 2^-24 sum |terms| puts their difference below 1e-5 of the gradient's norm.
Goldens: tests/golden/sft_lora_tiny.npz and sft_esm_lora_tiny.npz (dropout 0, so the golden comparisons run with dropout 0; the on / off
comparisons run with lora_dropout = 0.1 in train mode, the step counter reset before each run so that both draw the same masks)."""
import warnings

import numpy as np
import pytest
import torch

import esm_lora_reference as R
import test_gpu_instruct_trainer as TT
import test_gpu_sft_lora as SL
from gpu_util import build_model, dev, observe, rel, to_dev, to_np
from p2t_hip import specs

pytestmark = pytest.mark.gpu
ADAPTER = SL.ADAPTER


@pytest.fixture(scope="module")
def g():
    return _load_sft_lora()


def _load_sft_lora():
    import json
    import os
    z = np.load(os.path.join(SL.HERE, "golden", "sft_lora_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _set(model, on):
    model.gradient_checkpointing_enable() if on else model.gradient_checkpointing_disable()


def _decoder_step(model, lora, embeds, mask, labels, on, **kw):
    """One step of the decoder on its own -> (loss, d loss / d inputs_embeds, {pair parameter: gradient}, last_tape_bytes)."""
    _set(model, on)
    lora.step_count = 0
    for q in lora.parameters():
        q.grad = None
    e = embeds.clone().requires_grad_(True)
    loss = model.llama_decoder(inputs_embeds=e, attention_mask=mask, labels=labels, **kw).loss
    loss.backward()
    return loss.detach().clone(), e.grad.clone(), {n: q.grad.clone() for n, q in lora.named_parameters()}, model.llama_decoder.last_tape_bytes


def _assert_on_equals_off(off, off2, on, what):
    assert torch.equal(off[0], off2[0]) and torch.equal(off[1], off2[1]), f"{what}: two full-tape runs differ (loss / d inputs_embeds): a kernel of the step is not deterministic"
    for n in off[2]:
        assert torch.equal(off[2][n], off2[2][n]), f"{what}: two full-tape runs differ in {n}: p2t_gemm_nt's dA / dB products are not deterministic"
    assert torch.equal(off[0], on[0]), f"{what}: loss differs"
    assert torch.equal(off[1], on[1]), f"{what}: gradient at inputs_embeds differs"
    worst = 0.0
    for n in off[2]:
        e = rel(to_np(on[2][n]), to_np(off[2][n]))
        worst = max(worst, e)
        assert e <= 1e-5, f"{what}: {n} differs from the full-tape value by {e:.2e}"
    print(f"{what}: worst dA / dB difference on vs off {worst:.2e}; tape {off[3]} -> {on[3]} bytes")
    assert on[3] < off[3]


def _decoder_case(g, case, dtype, **kw):
    model, lora = SL._model(g, case, dtype, dropout=0.1)
    lora.train()
    B, T = g["input_ids"].shape
    H = model.llama_decoder.spec.hidden_size
    rs = np.random.RandomState(5)
    embeds = to_dev(rs.standard_normal((B, T, H)).astype(np.float32) * 0.5)
    return model, lora, embeds, to_dev(g["attention_mask"]), to_dev(g["labels"])


@pytest.mark.parametrize("case", ["d16", "d64", "qwen3_lora"])
def test_decoder_fp32_on_equals_off(g, case):
    model, lora, e, mask, labels = _decoder_case(g, case, torch.float32)
    off = _decoder_step(model, lora, e, mask, labels, False)
    off2 = _decoder_step(model, lora, e, mask, labels, False)
    on = _decoder_step(model, lora, e, mask, labels, True)
    _assert_on_equals_off(off, off2, on, case)


def test_decoder_packed_rows_with_loss_weights_on_equals_off(g):
    """Two documents per row through position_ids (document-confined attention, positional rotary) and per-target loss weights."""
    model, lora, e, _, _ = _decoder_case(g, "d16", torch.float32)
    B, T = e.shape[:2]
    cut = T // 3 + 1
    pos = to_dev(np.tile(np.concatenate([np.arange(cut), np.arange(T - cut)]), (B, 1)).astype(np.int64))
    mask = torch.ones((B, T), dtype=torch.int64, device=dev())
    rs = np.random.RandomState(2)
    labels = to_dev(rs.randint(0, model.llama_decoder.spec.vocab_size, (B, T)).astype(np.int64))
    w = to_dev((rs.rand(B, T) / (B * T)).astype(np.float32))
    kw = dict(position_ids=pos, loss_weights=w)
    off = _decoder_step(model, lora, e, mask, labels, False, **kw)
    off2 = _decoder_step(model, lora, e, mask, labels, False, **kw)
    on = _decoder_step(model, lora, e, mask, labels, True, **kw)
    _assert_on_equals_off(off, off2, on, "packed")


def _golden_decoder_step(g, case, dtype):
    model, lora = SL._model(g, case, dtype)
    model.gradient_checkpointing_enable()
    out = model(**SL._inputs(g), labels=to_dev(g["labels"]))
    out.loss.backward()
    return model, lora, out


@pytest.mark.parametrize("case", ["d16", "d64"])
def test_decoder_fp32_checkpointed_step_matches_the_golden(g, case):
    model, lora, out = _golden_decoder_step(g, case, torch.float32)
    assert abs(float(out.loss) - float(g[f"{case}.loss"])) < 2e-5 * max(1.0, float(g[f"{case}.loss"]))
    for n in ADAPTER:
        assert rel(to_np(dict(model.adapter.named_parameters())[n].grad), g[f"{case}.grad.{n}"]) < 5e-4, (case, n)
    for i in range(model.llama_decoder.spec.num_hidden_layers):
        for t in g["meta"]["targets"]:
            a, b = lora.get(i, t)
            ea, eb = rel(to_np(a.grad), g[f"{case}.lora.{i}.{t}.dA"]), rel(to_np(b.grad), g[f"{case}.lora.{i}.{t}.dB"])
            assert ea < 5e-4 and eb < 5e-4, (case, i, t, ea, eb)


def test_decoder_bf16_checkpointed_step_close_to_the_golden(g):
    case = "d128"
    model, lora, out = _golden_decoder_step(g, case, torch.bfloat16)
    observe(f"checkpointing.sft_lora[{case}].bf16.loss", abs(float(out.loss) - float(g[f"{case}.loss"])) / float(g[f"{case}.loss"]), 3e-2)
    for n in ADAPTER:
        observe(f"checkpointing.sft_lora[{case}].bf16.{n}", rel(to_np(dict(model.adapter.named_parameters())[n].grad), g[f"{case}.grad.{n}"]), 1.5e-1)
    ga, gb, ra, rb = [], [], [], []
    for i in range(model.llama_decoder.spec.num_hidden_layers):
        for t in g["meta"]["targets"]:
            a, b = lora.get(i, t)
            ga.append(to_np(a.grad).ravel()); ra.append(g[f"{case}.lora.{i}.{t}.dA"].ravel())
            gb.append(to_np(b.grad).ravel()); rb.append(g[f"{case}.lora.{i}.{t}.dB"].ravel())
    observe(f"checkpointing.sft_lora[{case}].bf16.dA", rel(np.concatenate(ga), np.concatenate(ra)), 1.5e-1)
    observe(f"checkpointing.sft_lora[{case}].bf16.dB", rel(np.concatenate(gb), np.concatenate(rb)), 1.5e-1)


# ------------------------------------------------------------------------------------------------------------------------------
# encoder (and both towers at once), through model(...)
def _encoder_model(golden, case, dtype, dropout):
    g, meta = golden, golden["meta"]
    m = meta["cases"][case]
    esm, llama = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**meta["llama"])
    model = build_model(esm, llama, specs.AdapterSpec(esm.hidden_size, meta["adapter_hidden"], llama.hidden_size, 0.3), dtype, 0)
    model.config.placeholder_id = meta["placeholder_id"]
    model.eval()
    model.requires_grad_(False)
    model.add_lora(meta["r"], meta["alpha"], dropout, m["enc_targets"] + m["dec_targets"])
    model.adapter.requires_grad_(True)
    enc, dec = R.golden_pairs(g, case)
    el, dl = model.esm_encoder.lora, getattr(model.llama_decoder, "lora", None)
    with torch.no_grad():
        for lo, pairs in ((el, enc), (dl, dec)):
            for (i, t), (a, b) in pairs.items():
                qa, qb = lo.get(i, t)
                qa.copy_(a), qb.copy_(b)
    T = lambda k: torch.from_numpy(g[k].copy()).to(dev())
    kw = dict(input_ids=T("input_ids"), attention_mask=T("attention_mask"), labels=T("labels"), protein_input_ids=T(f"{case}.protein_input_ids"),
              protein_attention_mask=T("protein_attention_mask"))
    return model, [lo for lo in (el, dl) if lo is not None], kw, (enc, dec)


def _model_step(model, loras, kw, on):
    _set(model, on)
    model.zero_grad(set_to_none=True)
    for lo in loras:
        lo.step_count = 0
    loss = model(**kw).loss
    loss.backward()
    pair_names = {id(q) for lo in loras for q in lo.parameters()}
    others = {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None and id(q) not in pair_names}
    pairs = {f"{k}.{n}": q.grad.clone() for k, lo in enumerate(loras) for n, q in lo.named_parameters()}
    return loss.detach().clone(), others, pairs, model.esm_encoder.last_tape_bytes


@pytest.mark.parametrize("case,dtype", [("enc_d16_td", torch.float32), ("mix_d64", torch.float32), ("mix_d64", torch.bfloat16)],
                         ids=["enc_d16_td-f32", "mix_d64-f32", "mix_d64-bf16"])
def test_encoder_on_equals_off(golden, case, dtype):
    model, loras, kw, _ = _encoder_model(golden, case, dtype, 0.1)
    for lo in loras:
        lo.train()
    off, off2, on = _model_step(model, loras, kw, False), _model_step(model, loras, kw, False), _model_step(model, loras, kw, True)
    assert torch.equal(off[0], off2[0]) and all(torch.equal(off[1][n], off2[1][n]) for n in off[1]) and all(torch.equal(off[2][n], off2[2][n]) for n in off[2]), \
        "two full-tape runs differ: a kernel of the step (p2t_gemm_nt's dA / dB products included) is not deterministic"
    assert torch.equal(off[0], on[0]), "loss differs"
    assert len(off[1]) == 4
    for n in off[1]:
        assert torch.equal(off[1][n], on[1][n]), f"adapter gradient {n} differs"
    for n in off[2]:
        e = rel(to_np(on[2][n]), to_np(off[2][n]))
        assert e <= 1e-5, f"{n} differs from the full-tape value by {e:.2e}"
    assert on[3] < off[3]


@pytest.mark.parametrize("case", ["enc_d16", "mix_d64"])
def test_encoder_fp32_checkpointed_step_matches_the_golden(golden, case):
    g = golden
    model, loras, kw, (enc, dec) = _encoder_model(golden, case, torch.float32, 0.0)
    loss, others, _, _ = _model_step(model, loras, kw, True)
    assert abs(float(loss) - float(g[f"{case}.loss"])) / float(g[f"{case}.loss"]) < 5e-4
    for tower, lo, pairs in (("enc", model.esm_encoder.lora, enc), ("dec", getattr(model.llama_decoder, "lora", None), dec)):
        for (i, t) in pairs:
            a, b = lo.get(i, t)
            assert rel(a.grad.cpu(), g[f"{case}.{tower}.{i}.{t}.dA"]) < 5e-4, (tower, i, t)
            assert rel(b.grad.cpu(), g[f"{case}.{tower}.{i}.{t}.dB"]) < 5e-4, (tower, i, t)
    P_ = dict(model.adapter.named_parameters())
    for n in ADAPTER:
        assert rel(P_[n].grad.cpu(), g[f"{case}.grad.{n}"]) < 5e-4, n


# ------------------------------------------------------------------------------------------------------------------------------
# tape accounting on synthetic 8-layer towers
L8, HID, FFN, B8, T8 = 8, 256, 1024, 2, 192


@pytest.fixture(scope="module")
def synthetic():
    esm = specs.EsmSpec(num_hidden_layers=L8, hidden_size=HID, intermediate_size=FFN, num_attention_heads=4)
    llama = specs.LlamaSpec(num_hidden_layers=L8, hidden_size=HID, intermediate_size=FFN, num_attention_heads=4, num_key_value_heads=2, vocab_size=512)
    model = build_model(esm, llama, specs.AdapterSpec(HID, 192, HID, 0.0), torch.bfloat16, 0)
    model.eval()
    model.requires_grad_(False)
    model.add_lora(8, 16.0, 0.1, ["q_proj", "down_proj", "gate_proj", "query", "dense"])
    return model


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def test_decoder_tape_accounting(synthetic):
    model, dec = synthetic, synthetic.llama_decoder
    M, es = B8 * T8, 2
    rs = np.random.RandomState(0)
    e = to_dev(rs.standard_normal((B8, T8, HID)).astype(np.float32) * 0.5).requires_grad_(True)
    mask = torch.ones((B8, T8), dtype=torch.int64, device=dev())
    labels = to_dev(rs.randint(0, 512, (B8, T8)).astype(np.int64))
    step = lambda: dec(inputs_embeds=e, attention_mask=mask, labels=labels).loss.backward()
    head = M * HID * 4 + M * 512 * es + M * 8 + 4 + M + 2 * B8 * 4      # x_last f32, logits [M, 512], labels i64, the target count, key mask, kv_info
    peak, tape = {}, {}
    for on in (False, True, False):                       # the last pass: disable() restores the full tape
        _set(model, on)
        peak[on] = _peak(step)
        tape[on] = dec.last_tape_bytes
        if on:
            assert tape[True] == L8 * M * HID * 4 + head
    assert tape[False] >= tape[True] + L8 * M * 2 * FFN * es            # the interleaved gate / up alone
    print(f"decoder tape {tape[False]} -> {tape[True]} bytes, peak {peak[False]} -> {peak[True]} bytes")
    assert peak[True] < peak[False]


def test_encoder_tape_accounting(synthetic):
    model, enc = synthetic, synthetic.esm_encoder
    M, es = B8 * T8, 2
    rs = np.random.RandomState(1)
    ids = to_dev(rs.randint(4, 24, (B8, T8)).astype(np.int64))
    mask = torch.ones((B8, T8), dtype=torch.int64, device=dev())
    from p2t_hip.encoder_train import encoder_lora_forward
    enc.lora.train()

    def step(on):
        out = encoder_lora_forward(enc, enc.lora, ids, mask, checkpoint=on)
        out.float().square().sum().backward()
    head = M * HID * 4 + M + 2 * B8 * 4                                  # x_last f32, key mask, kv_info
    peak, tape = {}, {}
    step(False)                                                          # builds the transposed frozen weights the dX GEMMs keep (`_lora_wT`)
    for on in (False, True):
        peak[on] = _peak(lambda: step(on))
        tape[on] = enc.last_tape_bytes
    assert tape[True] == L8 * M * HID * 4 + head
    assert tape[False] >= tape[True] + L8 * M * FFN * es                 # Z alone
    print(f"encoder tape {tape[False]} -> {tape[True]} bytes, peak {peak[False]} -> {peak[True]} bytes")
    assert peak[True] < peak[False]


def test_flag_reaches_both_towers_and_the_lora_step_no_longer_warns(g):
    model, lora = SL._model(g, "d16", torch.float32, dropout=0.1)
    assert not getattr(model.esm_encoder, "gradient_checkpointing", False) and not getattr(model.llama_decoder, "gradient_checkpointing", False)
    model.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": False})
    assert model.esm_encoder.gradient_checkpointing is True and model.llama_decoder.gradient_checkpointing is True and model.is_gradient_checkpointing
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model(**SL._inputs(g), labels=to_dev(g["labels"])).loss.backward()
    on = model.llama_decoder.last_tape_bytes
    model.gradient_checkpointing_disable()
    assert model.esm_encoder.gradient_checkpointing is False and model.llama_decoder.gradient_checkpointing is False
    model(**SL._inputs(g), labels=to_dev(g["labels"])).loss.backward()
    assert model.llama_decoder.last_tape_bytes > on


def test_trainer_two_steps_on_equals_off(g):
    """InstructTrainer, two steps, bf16 (the dtype stage 2 trains in), no clipping (the clip factor would carry dA / dB's summation order
    into every parameter).  The adapter's gradients are bit-identical in both modes, so its parameters must be; the LoRA masters take
    dA / dB from two differently ordered fp32 sums and are compared at 1e-5; the second step's loss sees them through bf16 operands."""
    import p2t_hip as P
    res = {}
    for on in (False, True):
        model, lora = TT._model(g, "d64", torch.bfloat16, dropout=0.1)
        lora.train()
        _set(model, on)
        tr = P.InstructTrainer(model, lr=1e-3)
        b = TT._batch(g)
        losses = [float(tr.step(b)) for _ in range(2)]
        torch.cuda.synchronize()
        res[on] = (losses, {n: q.detach().clone() for n, q in model.adapter.named_parameters()},
                   {n: q.detach().clone() for n, q in lora.named_parameters()})
    print(f"losses off {res[False][0]} on {res[True][0]}")
    assert res[False][0] == res[True][0], f"losses differ: off {res[False][0]}, on {res[True][0]}"
    for n, q in res[False][1].items():
        assert torch.equal(res[True][1][n], q), f"adapter parameter {n} differs"
    for n, q in res[False][2].items():
        e = rel(to_np(res[True][2][n]), to_np(q))
        assert e <= 1e-5, f"LoRA master {n} differs by {e:.2e}"
