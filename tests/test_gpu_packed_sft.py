"""Stage 2 on packed, padding-free rows (include/p2t_hip.h "packed rows"; p2t_hip.data.pack_instruct_batch):

* kernel level: document-confined attention forward (out, lse) and backward (dq, dk, dv) equal per-document separate runs, in the
  exact fp32 kernels and the bf16 MFMA kernels, at head_dim 64 and 128 with GQA (32 / 8 heads of 128 included), T = 1024 with
  documents of length 1, documents across 64- and 128-row tile boundaries and one longer than 256; no leakage: changing one
  document's keys / values leaves every other document's outputs bit-identical;
* model level: the 3-sample batches of tests/golden/sft_lora_tiny.npz (LoRA / Qwen3 per-layer path) and sft_grad_tiny.npz (the
  fused frozen-decoder engine) packed into one and into two rows give the golden loss and gradients (fp32: the bounds of
  test_gpu_sft_lora.py); bf16 packed and padded runs of the same model agree;
* "sample" loss weights = the mean of the per-sample batch-1 losses and gradients; one InstructTrainer step on a packed batch = the
  step on the padded batch; position_ids = arange is the ordinary batch; generate / the stage-1 tower still refuse position_ids."""
import json
import os

import numpy as np
import pytest
import torch

from gpu_util import build_model, dev, observe, rel, to_dev, to_np
import p2t_hip as P
from p2t_hip import ops, specs, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ADAPTER = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
KEYS = ("input_ids", "attention_mask", "labels", "protein_input_ids", "protein_attention_mask")


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


# ---------------------------------------------------------------------------------------------
# kernel level
ROW_LENS = ([1, 63, 1, 130, 301, 1, 65, 200, 129], [512, 1, 511])        # row 0: 891 valid tokens of 1024, row 1: full


def _packed_layout(T=1024):
    B = len(ROW_LENS)
    pos = torch.zeros((B, T), dtype=torch.int64)
    mask = torch.zeros((B, T), dtype=torch.int64)
    docs = []
    for b, lens in enumerate(ROW_LENS):
        t = 0
        for n in lens:
            pos[b, t:t + n] = torch.arange(n)
            mask[b, t:t + n] = 1
            docs.append((b, t, n))
            t += n
    return pos.to(dev()), mask.to(dev()), docs


def _attn_case(nh, nkv, d, dtype, seed):
    B, T = len(ROW_LENS), 1024
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda h: (torch.randn((B, h, T, d), generator=g) * 0.5).to(device=dev(), dtype=dtype)
    q, k, v = mk(nh), mk(nkv), mk(nkv)
    d_o = (torch.randn((B * T, ops.round_up(nh * d, 64)), generator=g) * 0.5).to(device=dev(), dtype=dtype)
    return q, k, v, d_o


def _run(q, k, v, d_o, mask, d, exact, docs=None):
    B, nh, T, _ = q.shape
    key_mask, kv_info, _ = ops.mask_prepare(mask)
    l2s = not exact
    scale = 1.0 if l2s else d ** -0.5
    lse = torch.empty((B, nh, T), dtype=torch.float32, device=q.device)
    out = ops.attention(q, k, v, key_mask, kv_info, d, scale, True, use_mfma=0 if exact else 2, log2_scores=l2s, lse=lse, docs=docs)
    c_s = 0.6931471805599453 if l2s else scale
    dq, dk, dv = ops.attention_backward(q, k, v, out, d_o, lse, key_mask, kv_info, d, c_s, True, log2_scores=l2s, use_mfma=0 if exact else 1,
                                        docs=docs)
    return out, lse, dq, dk, dv


@pytest.mark.parametrize("nh,nkv,d,exact", [(4, 2, 64, True), (4, 2, 128, True), (8, 2, 64, False), (32, 8, 128, False), (4, 4, 128, False)])
def test_document_attention_equals_separate_documents(nh, nkv, d, exact):
    dtype = torch.float32 if exact else torch.bfloat16
    pos, mask, docs_list = _packed_layout()
    q, k, v, d_o = _attn_case(nh, nkv, d, dtype, seed=nh * 1000 + d)
    docs = ops.doc_prepare(pos, mask)
    assert docs is not None
    T = q.shape[2]
    out, lse, dq, dk, dv = _run(q, k, v, d_o, mask, d, exact, docs)
    worst = dict(out=0.0, lse=0.0, dq=0.0, dk=0.0, dv=0.0)
    for b, s, n in docs_list:
        sl = lambda x: x[b:b + 1, :, s:s + n].contiguous()
        o1, l1, q1, k1, v1 = _run(sl(q), sl(k), sl(v), d_o[b * T + s:b * T + s + n].contiguous(), torch.ones((1, n), dtype=torch.int64, device=dev()),
                                  d, exact)
        rows = slice(b * T + s, b * T + s + n)
        pairs = dict(out=(out[rows, :nh * d], o1[:, :nh * d]), lse=(lse[b, :, s:s + n], l1[0]), dq=(dq[b, :, s:s + n], q1[0]),
                     dk=(dk[b, :, s:s + n], k1[0]), dv=(dv[b, :, s:s + n], v1[0]))
        for key, (x, y) in pairs.items():
            x, y = to_np(x.float()), to_np(y.float())
            worst[key] = max(worst[key], float(np.max(np.abs(x - y))) / max(float(np.max(np.abs(y))), 1e-6))
    for key, e in worst.items():
        if exact:
            assert e < 1e-5, (key, e)
        else:
            observe(f"packed_attention[{nh}/{nkv}x{d}].bf16.{key}", e, 3e-2)


@pytest.mark.parametrize("nh,nkv,d,exact", [(4, 2, 64, True), (8, 2, 64, False), (32, 8, 128, False)])
def test_document_attention_has_no_leakage(nh, nkv, d, exact):
    dtype = torch.float32 if exact else torch.bfloat16
    pos, mask, docs_list = _packed_layout()
    q, k, v, d_o = _attn_case(nh, nkv, d, dtype, seed=7)
    docs = ops.doc_prepare(pos, mask)
    T = q.shape[2]
    base = _run(q, k, v, d_o, mask, d, exact, docs)
    b0, s0, n0 = docs_list[4]                       # the 301-token document of row 0
    k2, v2 = k.clone(), v.clone()
    k2[b0, :, s0:s0 + n0] = -k2[b0, :, s0:s0 + n0] * 3.0
    v2[b0, :, s0:s0 + n0] = v2[b0, :, s0:s0 + n0] + 1.0
    pert = _run(q, k2, v2, d_o, mask, d, exact, docs)
    changed = False
    for b, s, n in docs_list:
        rows = slice(b * T + s, b * T + s + n)
        same = (torch.equal(base[0][rows, :nh * d], pert[0][rows, :nh * d]) and torch.equal(base[1][b, :, s:s + n], pert[1][b, :, s:s + n])
                and all(torch.equal(x[b, :, s:s + n], y[b, :, s:s + n]) for x, y in zip(base[2:], pert[2:])))
        if (b, s, n) == (b0, s0, n0):
            changed = not same
        else:
            assert same, ("leak into document", b, s, n)
    assert changed


def test_doc_prepare_refuses_malformed_positions():
    mask = torch.ones((1, 8), dtype=torch.int64, device=dev())
    assert ops.doc_prepare(torch.arange(8, device=dev()).view(1, 8), mask) is None          # an arange: the ordinary batch
    with pytest.raises(ValueError):
        ops.doc_prepare(torch.tensor([[0, 1, 2, 4, 0, 1, 2, 3]], device=dev()), mask)       # not a run
    with pytest.raises(ValueError):
        ops.doc_prepare(torch.tensor([[1, 2, 3, 4, 0, 1, 2, 3]], device=dev()), mask)       # does not start at 0
    with pytest.raises(ValueError):
        ops.doc_prepare(torch.tensor([[0, 1, 2, 0, 1]], device=dev()), mask)                # shape mismatch
    left = torch.tensor([[0, 0, 1, 1, 1, 1, 1, 1]], device=dev())
    with pytest.raises(ValueError):
        ops.doc_prepare(torch.tensor([[0, 0, 0, 1, 2, 0, 1, 2]], device=dev()), left)       # not right-padded


# ---------------------------------------------------------------------------------------------
# model level against the reference goldens
def _lora_model(g, case, dtype):
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
    return model, lora


def _host_batch(g):
    return {k: torch.from_numpy(np.ascontiguousarray(g[k])) for k in KEYS}


def _dev(batch):
    return {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items() if k != "pack_layout"}


def _grads(model, lora):
    ad = dict(model.adapter.named_parameters())
    out = {n: to_np(ad[n].grad) for n in ADAPTER}
    if lora is not None:
        for name, q in lora.named_parameters():
            out[name] = to_np(q.grad)
    return out


def _step(model, batch):
    for q in model.parameters():
        q.grad = None
    out = model(**_dev(batch))
    out.loss.backward()
    return float(out.loss)


@pytest.mark.parametrize("max_tokens", [64, 30])                          # one row / two rows
@pytest.mark.parametrize("golden,case", [("lora", "d16"), ("lora", "d64"), ("lora", "d128"), ("lora", "qwen3"), ("lora", "qwen3_lora"),
                                         ("grad", "d16"), ("grad", "d64"), ("grad", "d128")])
def test_fp32_packed_step_matches_golden(gl, gg, golden, case, max_tokens):
    g = gl if golden == "lora" else gg
    model, lora = _lora_model(g, case, torch.float32)
    packed = P.pack_instruct_batch(_host_batch(g), max_tokens)
    assert packed["input_ids"].shape[0] == (1 if max_tokens == 64 else 2)
    loss = _step(model, packed)
    assert abs(loss - float(g[f"{case}.loss"])) < 2e-5 * max(1.0, float(g[f"{case}.loss"])), (loss, float(g[f"{case}.loss"]))
    for n in ADAPTER:
        got = dict(model.adapter.named_parameters())[n].grad
        assert rel(to_np(got), g[f"{case}.grad.{n}"]) < 5e-4, (case, n)
    if lora is not None:
        for i in range(model.llama_decoder.spec.num_hidden_layers):
            for t in g["meta"]["targets"]:
                a, b = lora.get(i, t)
                assert rel(to_np(a.grad), g[f"{case}.lora.{i}.{t}.dA"]) < 5e-4, (case, i, t, "dA")
                assert rel(to_np(b.grad), g[f"{case}.lora.{i}.{t}.dB"]) < 5e-4, (case, i, t, "dB")


@pytest.mark.parametrize("golden,case", [("lora", "d64"), ("lora", "d128"), ("lora", "qwen3_lora"), ("grad", "d64"), ("grad", "d128")])
def test_bf16_packed_step_matches_padded(gl, gg, golden, case):
    g = gl if golden == "lora" else gg
    model, lora = _lora_model(g, case, torch.bfloat16)
    l_pad = _step(model, _host_batch(g))
    g_pad = _grads(model, lora)
    l_pk = _step(model, P.pack_instruct_batch(_host_batch(g), 30))
    g_pk = _grads(model, lora)
    observe(f"packed_sft[{golden}.{case}].bf16.loss", abs(l_pk - l_pad) / abs(l_pad), 3e-2)
    for n in ADAPTER:
        observe(f"packed_sft[{golden}.{case}].bf16.{n}", rel(g_pk[n], g_pad[n]), 1.5e-1)
    if lora is not None:
        keys = [k for k in g_pad if k not in ADAPTER]
        observe(f"packed_sft[{golden}.{case}].bf16.lora", rel(np.concatenate([g_pk[k].ravel() for k in keys]),
                                                            np.concatenate([g_pad[k].ravel() for k in keys])), 1.5e-1)


@pytest.mark.parametrize("golden,case", [("lora", "d64"), ("grad", "d128")])
def test_sample_weights_equal_mean_of_batch1_steps(gl, gg, golden, case):
    g = gl if golden == "lora" else gg
    model, lora = _lora_model(g, case, torch.float32)
    host = _host_batch(g)
    losses, grads = [], []
    for i in range(3):
        one = {k: v[i:i + 1] for k, v in host.items()}
        losses.append(_step(model, one))
        grads.append(_grads(model, lora))
    loss = _step(model, P.pack_instruct_batch(host, 30, loss_weighting="sample"))
    got = _grads(model, lora)
    want = float(np.mean(losses))
    assert abs(loss - want) < 5e-4 * max(1.0, abs(want)), (loss, want)
    for key in got:
        assert rel(got[key], np.mean([gr[key] for gr in grads], 0)) < 5e-4, key


def test_position_ids_arange_is_the_ordinary_batch(gl):
    model, lora = _lora_model(gl, "d64", torch.float32)
    host = _host_batch(gl)
    l0 = _step(model, host)
    g0 = _grads(model, lora)
    T = host["input_ids"].shape[1]
    l1 = _step(model, dict(host, position_ids=torch.arange(T).expand(3, T).contiguous()))
    g1 = _grads(model, lora)
    assert abs(l1 - l0) <= 1e-6 * max(1.0, abs(l0))
    for key in g0:
        assert rel(g1[key], g0[key]) <= 1e-6, key
    with torch.no_grad():                                                      # no-grad loss path too (per-layer, no tape)
        model.adapter.requires_grad_(False)
        lora.requires_grad_(False)
        ev = float(model(**_dev(P.pack_instruct_batch(host, 30))).loss)
    assert abs(ev - float(gl["d64.loss"])) < 2e-5 * max(1.0, float(gl["d64.loss"]))


def test_position_ids_still_refused_outside_the_loss_path(gl):
    model, _ = _lora_model(gl, "d16", torch.float32)
    model.llama_decoder.lora = None
    host = _dev(_host_batch(gl))
    T = host["input_ids"].shape[1]
    pos = torch.arange(T, device=dev()).expand(3, T)
    with pytest.raises(NotImplementedError):
        model.llama_decoder.model(input_ids=host["input_ids"], attention_mask=host["attention_mask"], position_ids=pos)
    with pytest.raises(NotImplementedError):
        model.llama_decoder(input_ids=host["input_ids"], attention_mask=host["attention_mask"], position_ids=pos)
    with pytest.raises(Exception):
        model.generate(host["input_ids"], attention_mask=host["attention_mask"], protein_input_ids=host["protein_input_ids"],
                       protein_attention_mask=host["protein_attention_mask"], position_ids=pos, max_new_tokens=2)


def test_instruct_trainer_packed_step_matches_padded(gl):
    """One optimizer step (GA 1) of InstructTrainer on the packed batch = the step on the padded batch (fp32 parameters, 5e-4);
    train_epoch / eval_epoch run over a packed loader."""
    from p2t_hip import loop
    params = {}
    for name, make in (("padded", lambda h: h), ("packed", lambda h: P.pack_instruct_batch(h, 30))):
        model, lora = _lora_model(gl, "d64", torch.float32)
        tr = P.InstructTrainer(model, gradient_accumulation_steps=1)
        tr.step(_dev(make(_host_batch(gl))))
        params[name] = {n: to_np(q.detach()) for n, q in list(lora.named_parameters()) + list(model.adapter.named_parameters())}
    for n in params["padded"]:
        assert rel(params["packed"][n], params["padded"][n]) < 5e-4, n
    model, _ = _lora_model(gl, "d64", torch.float32)
    tr = P.InstructTrainer(model, gradient_accumulation_steps=1)
    batches = [_dev(P.pack_instruct_batch(_host_batch(gl), 30)) for _ in range(2)]
    tl = loop.train_epoch(tr, batches, log=lambda s: None)
    el = loop.eval_epoch(tr, batches, log=lambda s: None)
    assert tl and el and all(np.isfinite(float(x)) for x in list(tl.values()) + list(el.values())), (tl, el)
