"""The stage-2 step with `fused_lm_loss()` (p2t_hip/lm_head.py: the LM loss over the target rows only, no logits kept) against the
goldens of the unfused step -- tests/golden/sft_grad_tiny.npz through the frozen-decoder chain, tests/golden/sft_lora_tiny.npz through
the per-layer LoRA step with the full tape and checkpointed -- at the unfused step's own fp32 bounds; in bf16 against twice the
unfused step's own error on the same case; and, with the option off, bit for bit against the head spelled out with ops.* calls."""
import json
import os

import numpy as np
import pytest
import torch

import p2t_hip as P
from gpu_util import build_model, dev, rel, to_dev, to_np
from p2t_hip import _lib, lm_head, ops, specs, synth
from p2t_hip.ops import ptr, stream

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ADAPTER = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
KEYS = ("input_ids", "attention_mask", "labels", "protein_input_ids", "protein_attention_mask")
FP32_TOL, FP32_TOL_EMB = 5e-4, 3e-4                    # the unfused step's bounds (tests/test_gpu_sft_backward.py, test_gpu_sft_lora.py)


def _golden(name):
    z = np.load(os.path.join(HERE, "golden", f"{name}.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


@pytest.fixture(scope="module")
def gl():
    return _golden("sft_lora_tiny")


@pytest.fixture(scope="module")
def gg():
    return _golden("sft_grad_tiny")


def _model(g, case, dtype, fused=True, chunk_rows=1024):
    meta = g["meta"]
    m = meta["cases"][case]
    model = build_model(specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"]), dtype, 0)
    model.config.placeholder_id = meta["placeholder_id"]
    model.eval()
    model.requires_grad_(False)
    lora = None
    if m.get("lora"):
        lora = model.add_lora(meta["r"], meta["alpha"], 0.0, meta["targets"])
        Pm = dict(model.llama_decoder.model.named_parameters())
        with torch.no_grad():
            for i in range(model.llama_decoder.spec.num_hidden_layers):
                for t in meta["targets"]:
                    a, b = lora.get(i, t)
                    w = Pm[f"layers.{i}.{t}.weight"]
                    a.copy_(to_dev(synth.uniform_f32(meta["lora_seed"], f"lora.{i}.{t}.A", (meta["r"], w.shape[1]), 0.25)))
                    b.copy_(to_dev(synth.uniform_f32(meta["lora_seed"], f"lora.{i}.{t}.B", (w.shape[0], meta["r"]), 0.25)))
    model.adapter.requires_grad_(True)
    if fused:
        assert model.fused_lm_loss(True, chunk_rows=chunk_rows) is model
    return model, lora


def _host(g):
    return {k: torch.from_numpy(np.ascontiguousarray(g[k])) for k in KEYS}


def _dev(batch):
    return {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items() if k != "pack_layout"}


def _step(model, batch, expect_logits):
    for q in model.parameters():
        q.grad = None
    out = model(**_dev(batch))
    assert (out.logits is not None) == expect_logits
    out.loss.backward()
    return out.loss.detach().clone()


def _grads(model, lora):
    ad = dict(model.adapter.named_parameters())
    out = {n: ad[n].grad.detach().clone() for n in ADAPTER}
    if lora is not None:
        for name, q in lora.named_parameters():
            out[name] = q.grad.detach().clone()
    return out


def _errors(g, case, model, lora, loss):
    """Relative errors of one step against the golden: the loss, the adapter's four gradients, all dA, all dB."""
    e = {"loss": abs(float(loss) - float(g[f"{case}.loss"])) / abs(float(g[f"{case}.loss"]))}
    ad = dict(model.adapter.named_parameters())
    for n in ADAPTER:
        e[n] = rel(to_np(ad[n].grad), g[f"{case}.grad.{n}"])
    if lora is not None:
        for which, idx in (("dA", 0), ("dB", 1)):
            got, ref = [], []
            for i in range(model.llama_decoder.spec.num_hidden_layers):
                for t in g["meta"]["targets"]:
                    got.append(to_np(lora.get(i, t)[idx].grad).ravel())
                    ref.append(g[f"{case}.lora.{i}.{t}.{which}"].ravel())
            e[which] = rel(np.concatenate(got), np.concatenate(ref))
    return e


def _emb_grad(model, g, labels):
    """d loss / d inputs_embeds of the decoder on the model's own decoder inputs."""
    emb, mask = model(**{k: to_dev(g[k]) for k in KEYS if k != "labels"}, return_decoder_inputs=True)
    emb = emb.detach().requires_grad_(True)
    res = model.llama_decoder(inputs_embeds=emb, attention_mask=mask, labels=labels)
    res.loss.backward()
    return emb.grad


# ---------------------------------------------------------------------------------------------
# fp32 against the goldens, at the unfused step's bounds
CASES = [("grad", "d16", False), ("grad", "d64", False), ("grad", "d128", False),
         ("lora", "d16", False), ("lora", "d64", False), ("lora", "d128", False), ("lora", "qwen3_lora", False),
         ("lora", "d16", True), ("lora", "d64", True), ("lora", "d128", True), ("lora", "qwen3_lora", True)]
_case_id = lambda c: f"{c[0]}.{c[1]}{'.ckpt' if c[2] else ''}"


@pytest.mark.parametrize("golden,case,ckpt", CASES, ids=[_case_id(c) for c in CASES])
def test_fp32_fused_step_matches_golden(gl, gg, golden, case, ckpt):
    g = gl if golden == "lora" else gg
    model, lora = _model(g, case, torch.float32)
    assert (lora is not None) == (golden == "lora")
    if ckpt:
        model.gradient_checkpointing_enable()
    loss = _step(model, _host(g), expect_logits=False)
    e = _errors(g, case, model, lora, loss)
    print(f"{_case_id((golden, case, ckpt))}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < FP32_TOL, (k, v)
    assert model.llama_decoder.lm_head.weight.grad is None
    key = f"{case}.d_inputs_embeds"
    if key in g:
        valid = g["attention_mask"] != 0
        got = _emb_grad(model, g, to_dev(g["labels"]))
        assert rel(to_np(got)[valid], g[key][valid]) < FP32_TOL_EMB
    if lora is not None:
        assert model.llama_decoder.last_tape_bytes > 0


# ---------------------------------------------------------------------------------------------
# bf16: no further from the golden than twice the unfused step on the same case (floored at the fp32 bound)
BF16 = [("grad", "d64", False), ("grad", "d128", False), ("lora", "d64", False), ("lora", "d128", True), ("lora", "qwen3_lora", False)]


@pytest.mark.parametrize("golden,case,ckpt", BF16, ids=[_case_id(c) for c in BF16])
def test_bf16_fused_step_no_worse_than_twice_the_unfused(gl, gg, golden, case, ckpt):
    g = gl if golden == "lora" else gg
    errs = {}
    for fused in (False, True):
        model, lora = _model(g, case, torch.bfloat16, fused=fused)
        if ckpt:
            model.gradient_checkpointing_enable()
        loss = _step(model, _host(g), expect_logits=not fused)
        errs[fused] = _errors(g, case, model, lora, loss)
    for k in errs[True]:
        print(f"{_case_id((golden, case, ckpt))} bf16 {k}: unfused {errs[False][k]:.3e}, fused {errs[True][k]:.3e}")
    for k in errs[True]:
        assert errs[True][k] <= max(2.0 * errs[False][k], FP32_TOL), (k, errs[True][k], errs[False][k])


# ---------------------------------------------------------------------------------------------
# more target rows than one chunk: (B, T) = (2, 130), packed rows, chunk_rows = 128
def _packed_2x130(model, seed=3):
    s = model.llama_decoder.spec
    B, T, H, V = 2, 130, s.hidden_size, s.vocab_size
    rng = np.random.default_rng(seed)
    lens = ([40, 1, 60, 29], [100, 20])                 # row 1 ends in 10 padding positions
    pos, mask = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64)
    for b, ls in enumerate(lens):
        t = 0
        for n in ls:
            pos[b, t:t + n], mask[b, t:t + n] = np.arange(n), 1
            t += n
    labels = rng.integers(0, V, size=(B, T)).astype(np.int64)
    labels[mask == 0] = -100
    labels[0, 5:12] = -100
    w = (rng.uniform(0.5, 1.5, (B, T)) / 200.0).astype(np.float32)
    emb = (rng.standard_normal((B, T, H)) * 0.5).astype(np.float32)
    return emb, mask, pos, labels, w


@pytest.mark.parametrize("golden,case,weighted", [("lora", "d64", False), ("grad", "d64", True)], ids=["lora.d64.mean", "grad.d64.weighted"])
def test_fp32_more_target_rows_than_one_chunk(gl, gg, golden, case, weighted):
    g = gl if golden == "lora" else gg
    model, lora = _model(g, case, torch.float32, fused=False)
    dec = model.llama_decoder
    emb, mask, pos, labels, w = _packed_2x130(model)
    n_targets = int(((labels[:, 1:] != -100) & (pos[:, 1:] != 0)).sum())
    assert n_targets > 128 + 64                         # two chunks of 128, the second one partly pad rows
    res = {}
    for fused in (False, True):
        dec.fused_lm_loss(fused, chunk_rows=128)
        for q in model.parameters():
            q.grad = None
        e = to_dev(emb).requires_grad_(True)
        out = dec(inputs_embeds=e, attention_mask=to_dev(mask), position_ids=to_dev(pos), labels=to_dev(labels),
                  loss_weights=to_dev(w) if weighted else None)
        assert (out.logits is None) == fused
        out.loss.backward()
        lg = {n: q.grad.detach().clone() for n, q in lora.named_parameters()} if lora is not None else {}      # (the adapter is not in this graph)
        res[fused] = (float(out.loss), to_np(e.grad), lg)
    assert abs(res[True][0] - res[False][0]) < 1e-5 * abs(res[False][0])
    assert rel(res[True][1], res[False][1]) < FP32_TOL_EMB
    for k in res[True][2]:
        assert rel(to_np(res[True][2][k]), to_np(res[False][2][k])) < FP32_TOL, k


# ---------------------------------------------------------------------------------------------
# packed batch with per-sample weights; the host bound
@pytest.mark.parametrize("golden,case", [("lora", "d64"), ("grad", "d128")])
def test_fp32_sample_weighted_packed_batch_and_the_host_bound(gl, gg, golden, case):
    g = gl if golden == "lora" else gg
    packed = P.pack_instruct_batch(_host(g), 30, loss_weighting="sample")
    lab = packed["labels"]
    assert packed["num_targets"] == int((lab[:, 1:] != -100).sum()) > 0
    model, lora = _model(g, case, torch.float32, fused=False)
    l_ref = _step(model, packed, expect_logits=True)
    g_ref = _grads(model, lora)
    model.fused_lm_loss(True)
    l_bound = _step(model, packed, expect_logits=False)             # the batch carries num_targets: no count is read
    g_bound = _grads(model, lora)
    assert abs(float(l_bound) - float(l_ref)) < 1e-5 * abs(float(l_ref))
    for k in g_ref:
        assert rel(to_np(g_bound[k]), to_np(g_ref[k])) < FP32_TOL, k
    # the synced count gives the same bits as the bound
    synced = {k: v for k, v in packed.items() if k != "num_targets"}
    l_sync = _step(model, synced, expect_logits=False)
    g_sync = _grads(model, lora)
    assert torch.equal(l_sync, l_bound)
    for k in g_sync:
        assert torch.equal(g_sync[k], g_bound[k]), k
    # a bound one too small: NaN, not a loss over a subset
    with torch.no_grad():
        short = model(**_dev(dict(packed, num_targets=packed["num_targets"] - 1)))
    assert short.logits is None and torch.isnan(short.loss)


# ---------------------------------------------------------------------------------------------
# eval
def test_no_grad_loss_equals_the_training_loss_and_keeps_nothing(gl):
    """(The LoRA step: its training and no-grad forwards are the same per-layer kernels.  The frozen-decoder chain trains through
    p2t_llama_train_forward and evaluates per layer -- two drivers whose losses agree to rounding, with or without this head.)"""
    g, case = gl, "d64"
    model, lora = _model(g, case, torch.bfloat16)
    l_train = _step(model, _host(g), expect_logits=False)
    with torch.no_grad():
        out = model(**_dev(_host(g)))
    assert out.logits is None and not out.loss.requires_grad
    assert torch.equal(out.loss, l_train)
    # the head itself: nothing kept without gradients, no tensor of vocabulary width with them
    dec = model.llama_decoder
    s = dec.spec
    lab = to_dev(g["labels"])
    x = torch.randn((lab.numel(), s.hidden_size), device=dev())
    with torch.no_grad():
        l0, saved0 = lm_head.lm_head_loss(dec, x, lab)
    assert saved0 is None
    l1, saved1 = lm_head.lm_head_loss(dec, x, lab)
    assert torch.equal(l0, l1)
    kept = lm_head.head_saved_tensors(saved1)
    assert kept and all(t.dim() < 2 or t.shape[-1] <= s.hidden_size for t in kept)
    assert sum(t.numel() * t.element_size() for t in kept) < 3 * saved1["d_a"].numel() * 4
    d = lm_head.lm_head_backward(dec, saved1, torch.full((1,), 0.5, device=dev()))
    assert tuple(d.shape) == tuple(x.shape) and d.dtype == torch.float32
    rows, _, count = ops.lm_target_rows(lab, s.vocab_size, lab.numel())
    listed = set(to_np(rows)[:int(count[0])].tolist())
    others = [r for r in range(lab.numel()) if r not in listed]
    assert not d[others].any() and d[sorted(listed)].abs().sum() > 0


# ---------------------------------------------------------------------------------------------
# the trainer
def test_two_trainer_steps_fused_against_unfused(gl):
    params = {}
    for fused in (False, True):
        model, lora = _model(gl, "d64", torch.float32, fused=False)
        lora.train()
        tr = P.InstructTrainer(model, fused_lm_loss=fused)
        assert (getattr(model.llama_decoder, "_fused_lm_loss", None) is not None) == fused
        batch = _dev(_host(gl))
        losses = [float(tr.step(batch)) for _ in range(2)]
        ev = float(tr.evaluate(batch))
        params[fused] = (tr.flat_p.detach().clone(), losses, ev)
    assert float((params[True][0] - params[False][0]).abs().max()) <= 1e-5
    for a, b in zip(params[True][1] + [params[True][2]], params[False][1] + [params[False][2]]):
        assert abs(a - b) < 1e-5 * max(1.0, abs(b))
    assert params[True][1][1] != params[True][1][0]                   # the step moved the parameters


# ---------------------------------------------------------------------------------------------
# option off: the shared unfused head is the head both steps spelled out before, bit for bit
@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("norm", [True, False], ids=["prenorm", "postnorm"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_unfused_head_is_the_ops_sequence_bit_for_bit(gg, dtype, norm, weighted):
    model, _ = _model(gg, "d64", dtype, fused=False)
    dec = model.llama_decoder
    s = dec.spec
    H, V = s.hidden_size, s.vocab_size
    lab = to_dev(gg["labels"])
    B, T = lab.shape
    M = B * T
    g = torch.Generator().manual_seed(1)
    x = torch.randn((M, H), generator=g).to(dev())
    w = (torch.rand((B, T), generator=g) / 20).to(dev()).contiguous() if weighted else None
    loss, logits, saved = lm_head.head_loss(dec, x, lab, weights=w, norm=norm)
    d = lm_head.head_backward(dec, saved)
    # the sequence as p2t_hip/modeling.py (_DecoderLossFn) and p2t_hip/decoder_train.py (DecoderLoraLossFn) wrote it
    nw = dict(dec.model.named_parameters())["norm.weight"].detach().float().contiguous()
    if norm:
        a = ops.rmsnorm(x, nw, s.rms_norm_eps, out_dtype=dtype)
    else:
        a = x if dtype == torch.float32 else ops.cast(x, dtype)
    want_logits = ops.gemm_nt(a, dec._lm_head_padded(), None, n=V, k=H, out_dtype=dtype).view(B, T, -1)
    want_loss, count = ops.cross_entropy_shifted(want_logits, lab, V, weights=w)
    d_logits = ops.cross_entropy_shifted_backward(want_logits, lab, V, count, weights=w)
    d_h = ops.gemm_nt(d_logits.view(M, -1), dec._lm_head_transposed(), None, n=H, k=ops.round_up(V, 64), epilogue=_lib.EPI_STORE_F32)
    if norm:
        want_d = torch.empty((M, H), dtype=torch.float32, device=dev())
        _lib.call("p2t_rmsnorm_backward", ptr(x), x.stride(0), ptr(nw), float(s.rms_norm_eps), ptr(d_h), d_h.stride(0), 0, ptr(want_d), want_d.stride(0),
                  M, H, 0, stream())
    else:
        want_d = d_h
    assert torch.equal(loss, want_loss) and torch.equal(logits, want_logits) and torch.equal(d, want_d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_frozen_step_with_the_option_off_is_the_ops_sequence_bit_for_bit(gg, dtype):
    model, _ = _model(gg, "d64", dtype, fused=False)
    dec = model.llama_decoder
    s = dec.spec
    H, V = s.hidden_size, s.vocab_size
    labels = to_dev(gg["labels"])
    B, T = labels.shape
    emb, mask = model(**{k: to_dev(gg[k]) for k in KEYS if k != "labels"}, return_decoder_inputs=True)
    emb = emb.detach().requires_grad_(True)
    out = dec(inputs_embeds=emb, attention_mask=mask, labels=labels)
    (out.loss * 0.5).backward()
    h, handle = dec.model.train_forward(emb.detach(), mask)
    a = h.view(B * T, H) if dtype == torch.float32 else ops.cast(h.view(B * T, H), dtype)
    logits = ops.gemm_nt(a, dec._lm_head_padded(), None, n=V, k=H, out_dtype=dtype).view(B, T, -1)
    loss, count = ops.cross_entropy_shifted(logits, labels, V)
    d_logits = ops.cross_entropy_shifted_backward(logits, labels, V, count)
    d_h = ops.gemm_nt(d_logits.view(B * T, -1), dec._lm_head_transposed(), None, n=H, k=ops.round_up(V, 64), epilogue=_lib.EPI_STORE_F32)
    d_in = dec.model.train_backward(d_h.view(B, T, H), handle)
    half = torch.full((1,), 0.5, device=dev())
    _lib.call("p2t_scale_by_device_scalar", ptr(d_in), d_in.numel(), ptr(half), stream())
    assert torch.equal(out.loss, loss[0]) and torch.equal(out.logits, logits[..., :V]) and torch.equal(emb.grad, d_in)
