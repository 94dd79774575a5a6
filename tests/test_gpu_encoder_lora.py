"""Stage 2 with LoRA on the ESM2 encoder (p2t_hip/encoder_train.py): the new entry points against fp64 torch, the whole step
(encoder LoRA -> adapter -> placeholder scatter -> decoder, with and without decoder LoRA) against the fp64 restatement of
tests/esm_lora_reference.py, the B = 0 start against the decoder-only step, the dropout mask's consistency, a 2-layer encoder at
ESM2-3B layer shapes, and the merge for inference."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import esm_lora_reference as R
from gpu_util import adapter_forward_case, build_model, dev, observe, rel, to_dev
from p2t_hip import _lib, ops, specs, synth
from p2t_hip._lib import call
from p2t_hip.encoder_train import TARGETS as ENC, encoder_lora_forward
from p2t_hip.ops import ptr, round_up, stream

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ADAPTER = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
LLAMA = specs.LlamaSpec(num_hidden_layers=2, hidden_size=64, intermediate_size=160, num_attention_heads=4, num_key_value_heads=2, vocab_size=512)
ESM = {"d16": specs.EsmSpec(num_hidden_layers=2, hidden_size=64, intermediate_size=128, num_attention_heads=4),
       "d64": specs.EsmSpec(num_hidden_layers=2, hidden_size=128, intermediate_size=256, num_attention_heads=2),
       "d16_td": specs.EsmSpec(num_hidden_layers=2, hidden_size=64, intermediate_size=128, num_attention_heads=4)}
PLACEHOLDER = 511                                       # tests/golden/sft_grad_tiny.npz meta["placeholder_id"]
MASKED = {"d16_td"}                                     # cases whose proteins carry <mask> tokens (token dropout's rescale)


@pytest.fixture(scope="module")
def batch():
    z = np.load(os.path.join(HERE, "golden", "sft_grad_tiny.npz"))          # sft_batch: unequal right-padded proteins, left-padded prompts
    meta = json.loads(bytes(z["meta_json"]).decode())
    d = {k: torch.from_numpy(z[k].copy()) for k in ("protein_input_ids", "protein_attention_mask", "input_ids", "attention_mask", "labels")}
    d["placeholder_id"] = meta["placeholder_id"]
    return d


def _model(esm, dtype, targets, p=0.0, r=4, seed=0):
    model = build_model(esm, LLAMA, specs.AdapterSpec(esm.hidden_size, 96, LLAMA.hidden_size, 0.3), dtype, seed)
    model.config.placeholder_id = PLACEHOLDER
    model.eval()
    model.requires_grad_(False)
    model.add_lora(r, 2.0 * r, p, targets)
    model.adapter.requires_grad_(True)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():                                # both factors non-zero (peft's B = 0 start would make every dA vanish)
        for lo in (getattr(model.esm_encoder, "lora", None), getattr(model.llama_decoder, "lora", None)):
            for q in (lo.parameters() if lo is not None else ()):
                q.copy_(torch.rand(tuple(q.shape), generator=g, dtype=torch.float32).sub_(0.5).mul_(0.5))
    return model


def _pairs(lo, n_layers):
    return {(i, t): lo.get(i, t) for i in range(n_layers) for t in lo.targets} if lo is not None else {}


def _inputs(b, pid=None):
    return dict(input_ids=b["input_ids"].to(dev()), attention_mask=b["attention_mask"].to(dev()), labels=b["labels"].to(dev()),
                protein_input_ids=(b["protein_input_ids"] if pid is None else pid).to(dev()), protein_attention_mask=b["protein_attention_mask"].to(dev()))


def _pid(b, esm, masked):
    pid = b["protein_input_ids"].clone()
    if masked:                                          # a few <mask> tokens under the mask: the token-dropout rescale is exercised
        pid[0, 3], pid[1, 2] = esm.mask_token_id, esm.mask_token_id
    return pid


# ---------------------------------------------------------------------------------------------------------------------------
def test_layernorm_backward_vs_fp64():
    rows, cols, eps = 37, 200, 1e-5
    g = torch.Generator().manual_seed(1)
    x = torch.randn((rows, cols), generator=g) * 2 + 0.5
    w, dy = torch.randn(cols, generator=g), torch.randn((rows, cols), generator=g)
    xd = x.double().requires_grad_(True)
    want = torch.autograd.grad(torch.nn.functional.layer_norm(xd, (cols,), w.double(), torch.zeros(cols, dtype=torch.float64), eps), xd, dy.double())[0]
    xg, wg = x.to(dev()), w.to(dev())
    for dyt, tol in ((torch.float32, 1e-5), (torch.bfloat16, 1e-5)):
        dyg = dy.to(dev()).to(dyt).contiguous()
        base = torch.randn((rows, cols), generator=g)
        out = base.to(dev()).clone()
        call("p2t_layernorm_backward", ptr(xg), cols, ptr(wg), eps, ptr(dyg), cols, ops.dt_of(dyg), ptr(out), cols, rows, cols, 1, stream())
        ref = want if dyt == torch.float32 else torch.autograd.grad(torch.nn.functional.layer_norm(xd, (cols,), w.double(), None, eps), xd,
                                                                     dyg.double().cpu())[0]
        assert rel(out.cpu() - base, ref) < tol


def test_gelu_rows_vs_fp64():
    M, N, ld = 19, 100, 128
    g = torch.Generator().manual_seed(2)
    z = (torch.randn((M, ld), generator=g) * 3).to(dev())
    dy = torch.randn((M, N), generator=g).to(dev())
    zd = z[:, :N].double().cpu().requires_grad_(True)
    y = torch.nn.functional.gelu(zd)
    dz = torch.autograd.grad(y, zd, dy.double().cpu())[0]
    out = torch.full((M, ld), 7.0, device=dev())
    call("p2t_gelu_rows", ptr(z), 0, ld, None, 0, 0, ptr(out), 0, ld, M, N, stream())
    assert rel(out[:, :N].cpu(), y.detach()) < 1e-6 and bool((out[:, N:] == 0).all())
    call("p2t_gelu_rows", ptr(z), 0, ld, ptr(dy), 0, N, ptr(out), 0, ld, M, N, stream())
    assert rel(out[:, :N].cpu(), dz) < 1e-6 and bool((out[:, N:] == 0).all())
    ob = torch.empty((M, ld), dtype=torch.bfloat16, device=dev())
    call("p2t_gelu_rows", ptr(z), 0, ld, None, 0, 0, ptr(ob), 1, ld, M, N, stream())
    assert rel(ob[:, :N].float().cpu(), y.detach()) < 4e-3


def test_adapter_backward_dx_vs_autograd_with_dropout():
    _adapter_dx_case(128, 96, 64, 45, "encoder_lora.adapter_dx.fp32")


def test_adapter_backward_dx_at_the_real_adapter_shape():
    """ESM2-3B hidden -> 2048 -> the decoder's 4096, one 611-residue protein: same reference, same bound."""
    _adapter_dx_case(2560, 2048, 4096, 611, "encoder_lora.adapter_dx.fp32.2560_2048_4096", 2560 ** -0.5, 2048 ** -0.5)


def _adapter_dx_case(X, I, O, M, name, s1=0.1, s2=0.1):
    """s1 / s2: the weights' scale (the real shape: fan_in^-1/2 as nn.Linear initialises, so that pre-activations stay O(1) and the
    keep-masks can be read back from the non-zero outputs)."""
    c = adapter_forward_case(X, I, O, M, s1, s2)
    p, cfg, wts, saved, dyg, y = c.p, c.cfg, c.wts, c.saved, c.dyg, c.y
    x, w1, b1, w2, b2, dy, m1, m2 = c.x, c.w1, c.b1, c.w2, c.b2, c.dy, c.m1, c.m2
    nb = call("p2t_adapter_backward_dx_workspace_bytes", C.byref(cfg), M)
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev())
    dx = torch.full((M, X), 3.0, device=dev())
    call("p2t_adapter_backward_dx", C.byref(cfg), C.byref(wts), M, C.byref(saved), ptr(dyg), ptr(dx), X, 0, ptr(ws), nb, stream())
    sc = 1.0 / (1.0 - p)
    xd = x.double().requires_grad_(True)
    gl = torch.nn.functional.gelu
    h = gl(xd @ w1.double().T + b1.double()) * m1 * sc
    yy = torch.nn.functional.normalize(gl(h @ w2.double().T + b2.double()) * m2 * sc, dim=-1)
    want = torch.autograd.grad(yy, xd, dy.double())[0]
    assert rel(y[:, :O].cpu(), yy.detach()) < 1e-5
    observe(name, rel(dx.cpu(), want), 1e-5)
    acc = dx.clone()
    call("p2t_adapter_backward_dx", C.byref(cfg), C.byref(wts), M, C.byref(saved), ptr(dyg), ptr(acc), X, 1, ptr(ws), nb, stream())
    assert rel(acc.cpu(), 2 * want) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------
def _check_step(model, b, esm, tag, tol, masked=False):
    pid = _pid(b, esm, masked)
    loss = model(**_inputs(b, pid)).loss
    loss.backward()
    el, dl = getattr(model.esm_encoder, "lora", None), getattr(model.llama_decoder, "lora", None)
    enc_pairs, dec_pairs = _pairs(el, esm.num_hidden_layers), _pairs(dl, LLAMA.num_hidden_layers)
    cpu = lambda d: {k: (a.detach().cpu(), bb.detach().cpu()) for k, (a, bb) in d.items()}
    lref, dA, dB, dAd, dBd, dAdp = R.full_step(model, pid, b["protein_attention_mask"], b["input_ids"], b["attention_mask"], b["labels"],
                                                b["placeholder_id"], cpu(enc_pairs), cpu(dec_pairs) or None, 2.0)
    observe(f"encoder_lora.{tag}.loss", abs(float(loss.detach()) - float(lref)) / abs(float(lref)), tol)
    for k, (a, bb) in enc_pairs.items():
        observe(f"encoder_lora.{tag}.enc.dA", rel(a.grad.float().cpu(), dA[k]), tol)
        observe(f"encoder_lora.{tag}.enc.dB", rel(bb.grad.float().cpu(), dB[k]), tol)
    for k, (a, bb) in dec_pairs.items():
        observe(f"encoder_lora.{tag}.dec.dA", rel(a.grad.float().cpu(), dAd[k]), tol)
        observe(f"encoder_lora.{tag}.dec.dB", rel(bb.grad.float().cpu(), dBd[k]), tol)
    P = dict(model.adapter.named_parameters())
    for n in ADAPTER:
        observe(f"encoder_lora.{tag}.adapter.{n}", rel(P[n].grad.float().cpu(), dAdp[n]), tol)
    assert all(float(a.grad.norm()) > 0 and float(bb.grad.norm()) > 0 for a, bb in enc_pairs.values())


@pytest.mark.parametrize("case,targets", [("d16", ["dense", "query", "key", "value"]),                           # encoder only, all six
                                          ("d16", ["query", "value", "output.dense", "self_attn.q_proj", "mlp.down_proj"]),
                                          ("d64", list(ENC) + ["self_attn.v_proj", "mlp.up_proj"]),
                                          ("d16_td", ["intermediate.dense", "attention.self.key"])])
def test_fp32_step_matches_fp64_restatement(batch, case, targets):
    model = _model(ESM[case], torch.float32, targets)
    _check_step(model, batch, ESM[case], f"{case}.{len(targets)}", 5e-4, case in MASKED)


def test_bf16_step_against_fp64(batch):
    # bf16 GEMM operands, MFMA attention and the bf16 adapter against the UNROUNDED fp64 step: observed 4.2e-2 at most (encoder
    # dA / dB; decoder and adapter groups <= 1.9e-2, loss 6e-5) -- the cap is twice that, under the 1.5e-1 the decoder's bf16 LoRA
    # step is held to against its unrounded reference (tests/test_gpu_sft_lora.py)
    model = _model(ESM["d64"], torch.bfloat16, list(ENC) + ["self_attn.q_proj"])
    _check_step(model, batch, ESM["d64"], "d64.bf16", 8e-2)


def test_zero_b_eval_equals_decoder_only_step(batch):
    tg = ["self_attn.q_proj", "mlp.gate_proj"]
    m1 = _model(ESM["d16"], torch.float32, tg + ["dense"], p=0.1)
    m0 = _model(ESM["d16"], torch.float32, tg, p=0.1)
    with torch.no_grad():
        for q in m1.esm_encoder.lora.parameters():
            if q.shape[1] == 4:                         # B [out, r]
                q.zero_()
        for (a, b_), (a0, b0) in zip(_pairs(m1.llama_decoder.lora, 2).values(), _pairs(m0.llama_decoder.lora, 2).values()):
            a0.copy_(a), b0.copy_(b_)
    m1.esm_encoder.lora.eval(), m1.llama_decoder.lora.eval(), m0.llama_decoder.lora.eval()
    out = []
    for m in (m1, m0):
        m.llama_decoder.lora.p = 0.0                    # the decoder branch's mask is not what is compared here
        loss = m(**_inputs(batch)).loss
        loss.backward()
        P = dict(m.adapter.named_parameters())
        out.append((float(loss.detach()), [q.grad.cpu() for q in m.llama_decoder.lora.parameters()], [P[n].grad.cpu() for n in ADAPTER]))
    assert abs(out[0][0] - out[1][0]) < 1e-5 * abs(out[1][0])
    for x, y in zip(out[0][1] + out[0][2], out[1][1] + out[1][2]):
        assert rel(x, y) < 1e-5
    assert all(float(a.grad.norm()) == 0 for (a, _) in _pairs(m1.esm_encoder.lora, 2).values())     # B = 0: dA = 0
    assert all(float(b_.grad.norm()) > 0 for (_, b_) in _pairs(m1.esm_encoder.lora, 2).values())


def test_dropout_directional_derivative_and_eval(batch):
    model = _model(ESM["d16"], torch.float32, ["dense", "query", "key", "value"], p=0.2)
    lo = model.esm_encoder.lora
    lo.train()
    B0 = lo.get(1, "intermediate.dense")[1]
    v = torch.randn(tuple(B0.shape), generator=torch.Generator().manual_seed(5)).to(dev()) * 0.2     # steps of 1e-2 on entries of ~0.1

    def loss_at(eps):
        lo.step_count = 6                               # the mask of step 7, every time
        with torch.no_grad():
            B0.add_(v, alpha=eps)
        try:
            return model(**_inputs(batch)).loss
        finally:
            with torch.no_grad():
                B0.sub_(v, alpha=eps)

    lo.zero_grad(set_to_none=True)
    loss_at(0.0).backward()
    gd = float((B0.grad * v).sum())
    h = 5e-2
    with torch.no_grad():
        fd = (float(loss_at(h)) - float(loss_at(-h))) / (2 * h)
    # central difference at steps of ~1e-2 on entries of ~0.1: observed 7e-3 (3.7e-2 at five times the step); a mask that differed
    # between the forward and the backward would be off by the dropped fraction, O(1e-1) and more
    observe("encoder_lora.dropout.directional", abs(fd - gd) / abs(gd), 2e-2)
    lo.eval()
    with torch.no_grad():
        e1 = float(model(**_inputs(batch)).loss)
        lo.p = 0.0
        e0 = float(model(**_inputs(batch)).loss)
    assert e1 == e0 and lo.step_count == 7


def test_esm2_3b_layer_shapes_directional_derivative():
    esm = specs.EsmSpec(num_hidden_layers=2, hidden_size=2560, intermediate_size=10240, num_attention_heads=40)
    llama = specs.LlamaSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=1, vocab_size=128)
    from p2t_hip import Esm2LlamaInstructForCausalLM
    model = Esm2LlamaInstructForCausalLM.from_specs(esm, llama, specs.AdapterSpec(2560, 128, 64, 0.0), dtype=torch.float32, device=dev(), seed=1)
    model.requires_grad_(False)
    lo = model.add_lora(16, 32.0, 0.0, ["dense", "query", "key", "value"])
    with torch.no_grad():
        for q in lo.parameters():
            if q.shape[1] == 16:
                q.normal_(0.0, 0.01)
    T, lens = 1024, [1024, 611]
    pid, pmask = synth.protein_batch(4, 2, T, lens)
    pid, pmask = to_dev(pid), to_dev(pmask)
    R_ = torch.randn((2, T, round_up(2560, 64)), generator=torch.Generator().manual_seed(9)).to(dev()) * pmask[..., None]
    Bq = lo.get(0, "attention.self.query")[1]         # layer 0's query: the whole chain (both layers, dq / rope backward) is on the path
    v = torch.randn(tuple(Bq.shape), generator=torch.Generator().manual_seed(8)).to(dev()) * 0.01

    def f(eps):
        with torch.no_grad():
            Bq.add_(v, alpha=eps)
        try:
            return (encoder_lora_forward(model.esm_encoder, lo, pid, pmask).float() * R_).sum()
        finally:
            with torch.no_grad():
                Bq.sub_(v, alpha=eps)

    f(0.0).backward()
    gd = float((Bq.grad * v).sum())
    with torch.no_grad():
        fd = (float(f(1.0)) - float(f(-1.0))) / 2.0
    observe("encoder_lora.esm3b_shapes.directional", abs(fd - gd) / abs(gd), 5e-3)


ESM3B_2L = specs.EsmSpec(num_hidden_layers=2, hidden_size=2560, intermediate_size=10240, num_attention_heads=40)


def _esm3b_step_errors(dtype, targets):
    """One encoder LoRA step of a 2-layer encoder at ESM2-3B layer shapes (H = 2560, F = 10240, 40 heads of 64) on proteins of 384, 211 and 1
    residues, r = 16 at peft's scale (kaiming A, B ~ N(0, 0.02), alpha / r = 2), p = 0, loss = sum(last_hidden_state * R) over valid
    residues -- against tests/esm_lora_reference.encoder in fp64 with autograd on the CPU, on the weights as the model stores them.
    -> ({"output" | "dA.<target>" | "dB.<target>": relative error, dA / dB concatenated over the layers}, last_hidden_state, seconds of the reference)."""
    import time
    from p2t_hip import Esm2LlamaInstructForCausalLM
    llama = specs.LlamaSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=1, vocab_size=128)
    model = Esm2LlamaInstructForCausalLM.from_specs(ESM3B_2L, llama, specs.AdapterSpec(2560, 128, 64, 0.0), dtype=dtype, device=dev(), seed=1)
    model.requires_grad_(False)
    model.add_lora(16, 32.0, 0.0, targets)
    lo = model.esm_encoder.lora
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for q in lo.parameters():
            if q.shape[1] == 16:                         # B [out, r]: trained-looking, as tests/test_gpu_stage2_matched.py
                q.copy_((torch.randn(tuple(q.shape), generator=g) * 0.02).to(q.device))
    H, L = 2560, 2
    T, lens = 384, [384, 211, 1]
    pid, pmask = synth.protein_batch(4, len(lens), T, lens)
    pid_c, pmask_c = torch.from_numpy(pid), torch.from_numpy(pmask)
    Rw = torch.randn((len(lens), T, H), generator=torch.Generator().manual_seed(9), dtype=torch.float64) * pmask_c[..., None]
    out = encoder_lora_forward(model.esm_encoder, lo, to_dev(pid), to_dev(pmask))
    Rd = torch.zeros(tuple(out.shape), dtype=torch.float32, device=dev())
    Rd[..., :H] = Rw.float().to(dev())
    (out.float() * Rd).sum().backward()
    pairs = _pairs(lo, L)
    t0 = time.time()
    We, _, _, ecfg, _ = R.model_weights(model)
    leaves = {k: (a.detach().cpu().double().requires_grad_(True), b.detach().cpu().double().requires_grad_(True)) for k, (a, b) in pairs.items()}
    h = R.encoder(We, ecfg, pid_c, pmask_c, leaves, 2.0)
    keys = list(leaves)
    gr = torch.autograd.grad((h * Rw).sum(), [leaves[k][0] for k in keys] + [leaves[k][1] for k in keys])
    secs = time.time() - t0
    dA, dB = dict(zip(keys, gr[:len(keys)])), dict(zip(keys, gr[len(keys):]))
    valid = pmask_c.bool()
    err = {"output": rel(out.detach().float().cpu()[..., :H][valid], h.detach()[valid])}
    for t in lo.targets:
        cat = lambda f: np.concatenate([np.asarray(f(i), dtype=np.float64).ravel() for i in range(L)])
        err["dA." + t] = rel(cat(lambda i: pairs[(i, t)][0].grad.float().cpu().numpy()), cat(lambda i: dA[(i, t)].numpy()))
        err["dB." + t] = rel(cat(lambda i: pairs[(i, t)][1].grad.float().cpu().numpy()), cat(lambda i: dB[(i, t)].numpy()))
    grads = [q.grad for ab in pairs.values() for q in ab]
    assert all(gq is not None and bool(torch.isfinite(gq).all()) and float(gq.norm()) > 0 for gq in grads), "a gradient is missing, NaN / Inf or zero"
    print(f"esm3b step {dtype} {len(lo.targets)} targets: fp64 reference {secs:.1f} s; " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    return err, out.detach(), secs


def test_esm2_3b_layer_shapes_fp32_step_vs_fp64():
    """The fp32 step (FMA GEMMs, exact attention) at ESM2-3B layer shapes: the output and every dA / dB group within 1e-4 of fp64, the fp32
    caps of tests/test_gpu_stage2_matched.py.  The fp64 reference (forward + autograd backward, ~1 TFLOP) measured at about 1 s on 16 threads."""
    err, _, secs = _esm3b_step_errors(torch.float32, list(ENC))
    assert secs < 120
    for k, e in err.items():
        observe(f"encoder_lora.esm3b_step.fp32.{k}", e, 1e-4)


@pytest.mark.parametrize("targets", [list(ENC), ["query", "value"]], ids=["all6", "query_value"])
def test_esm2_3b_layer_shapes_bf16_step_vs_fp64(targets):
    """The bf16 step (MFMA GEMMs and attention) against the UNROUNDED fp64 reference on the stored weights, held to the bf16 group cap of
    tests/test_gpu_stage2_matched.py (3e-2).  query_value: no branch on the FFN, so fc1 runs the fused P2T_EPI_GELU and fc2's dX GEMM the
    fused P2T_EPI_GELU_BWD at F = 10240; all6: Z assembled in fp32, p2t_gelu_rows forward, backward and the gelu(bf16(Z)) recompute."""
    err, out, secs = _esm3b_step_errors(torch.bfloat16, targets)
    assert secs < 120
    Hp = round_up(2560, 64)
    assert out.shape[-1] == Hp and not bool(out[..., 2560:].any()), "the padding columns [H, Hp) of last_hidden_state are exact zeros"
    assert bool(torch.isfinite(out.float()).all())
    for k, e in err.items():
        observe(f"encoder_lora.esm3b_step.bf16.{len(targets)}.{k}", e, 3e-2)


def test_merge_matches_unmerged_forward_and_generate_runs(batch, tmp_path):
    from p2t_hip.lora import load_and_merge_adapter
    esm = ESM["d16"]
    model = _model(esm, torch.float32, ["dense", "query", "self_attn.o_proj"])
    el = model.esm_encoder.lora
    el.eval()
    pid, pmask = batch["protein_input_ids"].to(dev()), batch["protein_attention_mask"].to(dev())
    with torch.no_grad():
        want = encoder_lora_forward(model.esm_encoder, el, pid, pmask)
    tensors = {**el.peft_state_dict(), **model.llama_decoder.lora.peft_state_dict()}
    assert "base_model.model.esm_encoder.encoder.layer.1.attention.self.query.lora_A.weight" in tensors
    from safetensors.torch import save_file
    save_file({k: v.cpu().contiguous() for k, v in tensors.items()}, str(tmp_path / "adapter_model.safetensors"))
    (tmp_path / "adapter_config.json").write_text(json.dumps({"peft_type": "LORA", "r": el.r, "lora_alpha": el.alpha, "target_modules": ["dense", "query", "self_attn.o_proj"]}))
    fresh = build_model(esm, LLAMA, specs.AdapterSpec(esm.hidden_size, 96, LLAMA.hidden_size, 0.3), torch.float32, 0)
    fresh.config.placeholder_id = PLACEHOLDER
    fresh.eval()
    fresh.esm_encoder.encode(pid, pmask)                # an engine built before the merge must be rebuilt by it
    res = load_and_merge_adapter(fresh, str(tmp_path))
    assert res["merged"] == len(tensors) // 2
    with torch.no_grad():
        got = fresh.esm_encoder.encode(pid, pmask)
    assert rel(got.cpu(), want.cpu()) < 1e-5
    with pytest.raises(NotImplementedError, match="merge them for inference"):
        model.esm_encoder.encode(pid, pmask)
    with pytest.raises(NotImplementedError, match="merge them for inference"):
        model.generate(inputs=batch["input_ids"][:, :18].to(dev()), attention_mask=batch["attention_mask"][:, :18].to(dev()), protein_input_ids=pid,
                       protein_attention_mask=pmask, max_new_tokens=2)
    out = fresh.generate(inputs=batch["input_ids"][:, :18].to(dev()), attention_mask=batch["attention_mask"][:, :18].to(dev()), protein_input_ids=pid,
                         protein_attention_mask=pmask, max_new_tokens=3)
    assert out.shape[0] == 3


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.mark.parametrize("case", ["enc_d16", "enc_d16_td", "mix_d16", "mix_d64"])
def test_fp32_step_matches_reference_class_golden(golden, case):
    """tests/golden/sft_esm_lora_tiny.npz: torch autograd through the reference class with LoRA-wrapped ESM2 (and decoder) linears."""
    g, meta = golden, golden["meta"]
    m = meta["cases"][case]
    esm, llama = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**meta["llama"])
    model = build_model(esm, llama, specs.AdapterSpec(esm.hidden_size, meta["adapter_hidden"], llama.hidden_size, 0.3), torch.float32, 0)
    model.config.placeholder_id = meta["placeholder_id"]
    model.eval()
    model.requires_grad_(False)
    model.add_lora(meta["r"], meta["alpha"], 0.0, m["enc_targets"] + m["dec_targets"])
    model.adapter.requires_grad_(True)
    enc, dec = R.golden_pairs(g, case)
    el, dl = model.esm_encoder.lora, getattr(model.llama_decoder, "lora", None)
    with torch.no_grad():
        for lo, pairs in ((el, enc), (dl, dec)):
            for (i, t), (a, b) in pairs.items():
                qa, qb = lo.get(i, t)
                qa.copy_(a), qb.copy_(b)
    T = lambda k: torch.from_numpy(g[k].copy()).to(dev())
    loss = model(input_ids=T("input_ids"), attention_mask=T("attention_mask"), labels=T("labels"), protein_input_ids=T(f"{case}.protein_input_ids"),
                 protein_attention_mask=T("protein_attention_mask")).loss
    loss.backward()
    observe(f"encoder_lora.golden.{case}.loss", abs(float(loss.detach()) - float(g[f"{case}.loss"])) / float(g[f"{case}.loss"]), 5e-4)
    for tower, lo, pairs in (("enc", el, enc), ("dec", dl, dec)):
        for (i, t) in pairs:
            a, b = lo.get(i, t)
            observe(f"encoder_lora.golden.{case}.{tower}.dA", rel(a.grad.cpu(), g[f"{case}.{tower}.{i}.{t}.dA"]), 5e-4)
            observe(f"encoder_lora.golden.{case}.{tower}.dB", rel(b.grad.cpu(), g[f"{case}.{tower}.{i}.{t}.dB"]), 5e-4)
    P_ = dict(model.adapter.named_parameters())
    for n in ADAPTER:
        observe(f"encoder_lora.golden.{case}.adapter", rel(P_[n].grad.cpu(), g[f"{case}.grad.{n}"]), 5e-4)


# ---------------------------------------------------------------------------------------------------------------------------
TRAIN_TARGETS = ["self_attn.q_proj", "mlp.down_proj", "dense", "query", "key"]


def _trained(model):
    """The tensors InstructTrainer optimises, in its order: decoder LoRA, encoder LoRA, adapter."""
    return list(model.llama_decoder.lora.parameters()) + list(model.esm_encoder.lora.parameters()) + \
        [dict(model.adapter.named_parameters())[n] for n in ADAPTER]


def test_trainer_matches_torch_adamw_on_a_twin(batch):
    import p2t_hip as P
    model, twin = (_model(ESM["d16"], torch.float32, TRAIN_TARGETS, p=0.1) for _ in range(2))
    tr = P.InstructTrainer(model, lr=2e-3, max_norm=1.0)
    assert tr.n_lora == len(list(model.llama_decoder.lora.parameters())) + len(list(model.esm_encoder.lora.parameters()))
    params = _trained(twin)
    topt = torch.optim.AdamW(params, lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
    b = _inputs(batch)
    for step in range(3):
        l_tr = float(tr.step(b))
        out = twin(**b)
        out.loss.backward()
        assert abs(l_tr - float(out.loss.detach())) <= 1e-5 * abs(float(out.loss.detach())), step
        torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
        topt.step()
        topt.zero_grad(set_to_none=True)
    assert model.esm_encoder.lora.step_count == twin.esm_encoder.lora.step_count == 3
    for q_tr, q_tw in zip(_trained(model), params):
        assert rel(q_tr.detach().cpu(), q_tw.detach().cpu()) <= 1e-5
    sc = model.esm_encoder.lora.step_count
    e = float(tr.evaluate(b))                            # eval: no encoder dropout, the mask counter stays
    assert model.esm_encoder.lora.step_count == sc and np.isfinite(e)


def test_checkpoint_resume_is_bit_identical(batch, tmp_path):
    import p2t_hip as P
    from p2t_hip import instruct
    from p2t_hip.training_state import CosineWarmupSchedule
    b = _inputs(batch)

    def trainer():
        model = _model(ESM["d16"], torch.float32, TRAIN_TARGETS, p=0.1)
        return P.InstructTrainer(model, lr=1e-3, max_norm=1.0, schedule=CosineWarmupSchedule(1e-3, 1, 4))

    t1 = trainer()
    for _ in range(2):
        t1.step(b)
    adir, opath = instruct.save_instruct_checkpoint(t1, str(tmp_path), 1)
    cfg = json.load(open(os.path.join(adir, "adapter_config.json")))
    assert "attention.self.query" in cfg["target_modules"] and "self_attn.q_proj" in cfg["target_modules"]
    t1.step(b)
    t2 = trainer()
    instruct.load_instruct_checkpoint(t2, adir, opath)
    assert t2.enc_lora.step_count == 2 and t2.step_count == 2
    t2.step(b)
    for q1, q2 in zip(_trained(t1.model), _trained(t2.model)):
        assert torch.equal(q1.detach().view(torch.int32), q2.detach().view(torch.int32))
