"""MXFP4 decoder weights on the decode step's weight stream (include/p2t_hip.h "MXFP4 decoder weights"; csrc/quant.hip,
csrc/gemm_skinny.hip gemm_skinny_mxfp4_kernel, p2t_llama_decode_step_mxfp4; `set_gemm_dtype("mxfp4")`).

* the quantiser and de-quantiser against the fp64 restatement (tests/mxfp4_reference.py): scale bytes and values equal, nothing written
  behind the outputs, and the fp8 row quantiser loses nothing on the de-quantised matrix;
* the lane map of the 4-bit MFMA with exact integer data: any error in nibble order, K permutation, scale byte selection or tile tails
  changes an integer;
* random operands against numpy and against the fp8 form on quant_rows_fp8(W~);
* the model: graph + stream copy == eager + row-major bit for bit; a twin whose decoder MASTERS are W~ in "fp8" mode holds the same e4m3
  bytes and returns the same first logits; later steps differ by the MFMA's inner sum and bf16 rounding flips (measured, see
  test_model_mxfp4); the fp8 oracle fed W~ and the model's own cache-less forward hold their fp8 bounds."""
import json
import os

import numpy as np
import pytest
import torch

import mxfp4_reference as R
from oracle import p2t_oracle as O
from gpu_util import bf16r, build_model, dev, observe, rel, rnd, to_dev, to_np
from helpers import model_weights
from p2t_hip import specs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENT = 0xA5


def _quant_raw(x, cols, ld_codes_extra=16):
    """p2t_quant_rows_mxfp4 into buffers larger than the contract writes, filled with a sentinel -> (codes buffer, scales buffer, Kq)."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    rows, Kq = x.shape[0], ops.round_up(cols, 128)
    codes = torch.full((rows + 1, Kq // 2 + ld_codes_extra), SENT, dtype=torch.uint8, device=dev())
    sc = torch.full((rows * (Kq // 32) + 64,), SENT, dtype=torch.uint8, device=dev())
    _lib.call("p2t_quant_rows_mxfp4", ptr(x), ops.dt_of(x), x.stride(0), rows, cols, ptr(codes), codes.stride(0), ptr(sc), stream())
    return codes, sc, Kq


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", [(3, 32), (5, 100), (17, 384), (16, 4096)])
def test_quantiser_and_dequantiser_vs_restatement(shape, dt):
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    rows, K = shape
    w = R.adversarial_rows(rows * 10000 + K, rows, K, bf16=dt == torch.bfloat16)
    ld_x = ops.round_up(K, 8) + 8
    x = np.full((rows, ld_x), np.nan, np.float32)                   # NaN behind the row: columns at or beyond K are not read
    x[:, :K] = w
    codes, sc, Kq = _quant_raw(to_dev(x, dt), K)
    ref_codes, ref_sc, ref_val = R.quantise(w)
    cb, sb = to_np(codes), to_np(sc)
    assert (cb[:rows, Kq // 2:] == SENT).all() and (cb[rows] == SENT).all() and (sb[rows * (Kq // 32):] == SENT).all()
    got_sc = sb[: rows * (Kq // 32)].reshape(rows, Kq // 32)
    assert np.array_equal(got_sc, ref_sc)
    assert np.array_equal(R.dequantise(cb[:rows], got_sc, K), ref_val + 0.0)            # values, not signs of zero
    assert np.array_equal(R.unpack(cb[:rows, : Kq // 2]) & 7, ref_codes & 7)
    # the de-quantiser: exact, and nothing behind column K
    out = torch.full((rows + 1, K + 8), 7.0, dtype=torch.bfloat16, device=dev())
    _lib.call("p2t_dequant_rows_mxfp4", ptr(codes), codes.stride(0), ptr(sc), rows, K, ptr(out), out.stride(0), stream())
    o = to_np(out)
    assert np.array_equal(o[:rows, :K].astype(np.float64), ref_val + 0.0) and (o[:rows, K:] == 7.0).all() and (o[rows] == 7.0).all()
    # the wrappers agree, and the fp8 row quantiser loses nothing on W~ (this is what lets the prefill run the e4m3 kernels on it)
    c2, s2 = ops.quant_rows_mxfp4(to_dev(x, dt), K)
    assert torch.equal(c2, codes[:rows, : Kq // 2]) and torch.equal(s2.reshape(-1), sc[: rows * (Kq // 32)])
    wt = ops.dequant_rows_mxfp4(c2, s2, K, ops.round_up(K, 64))
    q8, s8 = ops.quant_rows_fp8(wt, cols=K)
    deq, E, _ = O.quant_rows_e4m3(ref_val.astype(np.float32))
    assert np.array_equal(deq, ref_val.astype(np.float32)) and np.array_equal(to_np(s8), E)
    back = q8.cpu().view(torch.float8_e4m3fn).float().numpy().astype(np.float64)[:, :K] * np.ldexp(1.0, E.astype(np.int64) - 127)[:, None]
    assert np.array_equal(back, ref_val + 0.0)


def _gemm(a8, sa, w, ldw, bs, pre, out, M, N, Kq, odt, epi):
    from p2t_hip import _lib
    from p2t_hip.ops import ptr, stream
    _lib.call("p2t_gemm_nt_skinny_mxfp4", ptr(a8), a8.stride(0), ptr(sa), ptr(w), ldw, ptr(bs) if bs is not None else None, pre, ptr(out), out.stride(0),
              M, N, Kq, odt, epi, stream())
    return out


@pytest.mark.parametrize("shape", [(1, 16, 128), (5, 96, 256), (19, 1000, 512), (33, 48, 1792), (64, 640, 384), (16, 6144, 4096), (8, 4096, 14336)])
def test_lane_map_witness_is_exact(shape):
    """Activations: integers in [-8, 8]; weights: grid values times block scales 2^0 .. 2^3 that differ per block and per row.  Every sum
    of absolute products is below 2^20 (asserted), so every f32 partial sum is exact in any order: the result must EQUAL the integer
    product.  Row-major and stream forms bit-equal; f32 store, bf16 store, residual +=, SwiGLU (N % 64 == 0); sentinel columns survive."""
    from p2t_hip import _lib, ops
    from p2t_hip.generation import preshuffle_mxfp4
    M, N, K = shape
    rs = np.random.RandomState(M * 1000003 + N * 101 + K)
    a = rs.randint(-8, 9, size=(M, K)).astype(np.float32)
    idx = rs.randint(0, 8, size=(N, K)).astype(np.uint8)
    sign = rs.randint(0, 2, size=(N, K)).astype(np.uint8)
    e = rs.randint(0, 4, size=(N, K // 32))
    e[:, 0] = np.arange(N) % 4                                      # per row as well as per block
    w = R.GRID.astype(np.float32)[idx] * np.repeat(np.ldexp(np.float32(1.0), e).astype(np.float32), 32, axis=1)
    assert (np.abs(a) @ w.T).max() < 2 ** 20                        # multiples of 0.5 below 2^20: the f32 products below are exact as well
    w *= np.where(sign, np.float32(-1.0), np.float32(1.0))
    ref = a @ w.T
    codes, bs = to_dev(R.pack(idx | (sign << 3))), to_dev((e + 127).astype(np.uint8))
    a8, sa = ops.quant_rows_fp8(to_dev(a))                          # integers up to 8 are e4m3-exact under any row scale
    assert np.array_equal(a8.cpu().view(torch.float8_e4m3fn).float().numpy()[:, :K] * np.ldexp(1.0, to_np(sa).astype(np.int64) - 127)[:, None], a)
    stream_w = preshuffle_mxfp4(codes, bs, N)
    ldc = ops.round_up(N, 4) + 4
    forms = ((0, codes, K // 2, bs), (1, stream_w, 0, None))
    outs = [_gemm(a8, sa, w_, ldw, s_, pre, torch.full((M, ldc), 7.0, dtype=torch.float32, device=dev()), M, N, K, _lib.F32, _lib.EPI_STORE)
            for pre, w_, ldw, s_ in forms]
    for o in outs:
        assert np.array_equal(to_np(o)[:, :N], ref) and (to_np(o)[:, N:] == 7.0).all()
    assert torch.equal(outs[0], outs[1])
    ref_bf = torch.from_numpy(ref).to(torch.bfloat16)
    base = rs.randint(-50, 51, size=(M, ldc)).astype(np.float32)
    for pre, w_, ldw, s_ in forms:
        ob = _gemm(a8, sa, w_, ldw, s_, pre, torch.full((M, ldc), 7.0, dtype=torch.bfloat16, device=dev()), M, N, K, _lib.BF16, _lib.EPI_STORE)
        assert torch.equal(ob[:, :N].cpu(), ref_bf) and (to_np(ob)[:, N:] == 7.0).all()
        acc = _gemm(a8, sa, w_, ldw, s_, pre, to_dev(base.copy()), M, N, K, _lib.F32, _lib.EPI_RESID)
        assert np.array_equal(to_np(acc)[:, :N], base[:, :N] + ref) and np.array_equal(to_np(acc)[:, N:], base[:, N:])
    if N % 64 == 0:
        F = N // 2
        blocks = ref.reshape(M, N // 64, 2, 32)
        gate, up = blocks[:, :, 0].reshape(M, F), blocks[:, :, 1].reshape(M, F)
        acts = [_gemm(a8, sa, w_, ldw, s_, pre, torch.full((M, F + 4), 7.0, dtype=torch.bfloat16, device=dev()), M, N, K, _lib.BF16, _lib.EPI_SWIGLU)
                for pre, w_, ldw, s_ in forms]
        assert torch.equal(acts[0], acts[1]) and (to_np(acts[0])[:, F:] == 7.0).all()
        with np.errstate(over="ignore"):
            want = gate / (1.0 + np.exp(-gate)) * up
        assert rel(to_np(acts[0])[:, :F], want) < 4e-3


@pytest.mark.parametrize("shape", [(5, 96, 256), (19, 1000, 512), (64, 640, 384), (8, 4096, 4096)])
def test_random_operands_vs_numpy_and_the_fp8_form(shape):
    """Products of e2m1 x e4m3 values are exact and only the f32 sum differs: the fp8 form's bound, 3e-5, against numpy on the de-quantised
    operands and against p2t_gemm_nt_skinny_fp8 on quant_rows_fp8(W~)."""
    from p2t_hip import _lib, ops
    from p2t_hip.generation import preshuffle_mxfp4
    from p2t_hip.ops import ptr, stream
    M, N, K = shape
    a = rnd(61, "mx.a", (M, K), 1.0) * np.exp(rnd(61, "mx.as", (M, 1), 2.0)).astype(np.float32)
    w = rnd(61, "mx.w", (N, K), 0.5) * np.exp(rnd(61, "mx.ws", (N, 1), 2.0)).astype(np.float32) / np.float32(np.sqrt(K))
    a8, sa = ops.quant_rows_fp8(to_dev(a))
    codes, bs = ops.quant_rows_mxfp4(to_dev(w))
    wt = R.dequantise(to_np(codes), to_np(bs), K)
    assert np.array_equal(wt, R.quantise(w)[2] + 0.0)
    ref = O.quant_rows_e4m3(a)[0].astype(np.float64) @ wt.T
    ldc = ops.round_up(N, 4)
    out = _gemm(a8, sa, codes, K // 2, bs, 0, torch.zeros((M, ldc), dtype=torch.float32, device=dev()), M, N, K, _lib.F32, _lib.EPI_STORE)
    out_s = _gemm(a8, sa, preshuffle_mxfp4(codes, bs, N), 0, None, 1, torch.zeros((M, ldc), dtype=torch.float32, device=dev()), M, N, K, _lib.F32, _lib.EPI_STORE)
    assert torch.equal(out, out_s)
    observe(f"skinny_mxfp4[{M}x{N}x{K}].f32", rel(to_np(out)[:, :N], ref), 3e-5)
    w8, sw = ops.quant_rows_fp8(ops.dequant_rows_mxfp4(codes, bs, K))
    o8 = torch.zeros((M, ldc), dtype=torch.float32, device=dev())
    _lib.call("p2t_gemm_nt_skinny_fp8", ptr(a8), K, ptr(sa), ptr(w8), K, ptr(sw), 0, ptr(o8), ldc, M, N, K, _lib.F32, _lib.EPI_STORE, stream())
    observe(f"skinny_mxfp4[{M}x{N}x{K}].vs_fp8_form", rel(to_np(out)[:, :N], to_np(o8)[:, :N]), 3e-5)


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(HERE, "golden", "generate_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


def _model(g, case):
    m = g["meta"]["cases"][case]
    model = build_model(specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"]), torch.bfloat16, m["weight_seed"])
    model.config.placeholder_id = g["meta"]["placeholder_id"]
    return model.eval()


def _inputs(g):
    return dict(inputs=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                protein_attention_mask=to_dev(g["protein_attention_mask"]))


_PROJ = tuple(f"self_attn.{n}_proj.weight" for n in "qkvo") + tuple(f"mlp.{n}_proj.weight" for n in ("gate", "up", "down"))


class _Patched:
    """The oracle's weights with the decoder projections replaced by their MXFP4 values."""

    def __init__(self, base, spec):
        self.base, self.over = base, {}
        for i in range(spec.num_hidden_layers):
            for n in _PROJ:
                k = f"llama_decoder.model.layers.{i}.{n}"
                self.over[k] = R.quantise(bf16r(base[k]))[2].astype(np.float32)

    def __contains__(self, k):
        return k in self.base

    def __getitem__(self, k):
        return self.over[k] if k in self.over else self.base[k]


@pytest.mark.parametrize("case", ["d64", "d128", "d16", "qwen3"])
def test_model_mxfp4(g, case):
    """6 greedy tokens with per-step logits.  Against the fp8 twin on W~ the first step is bit-equal (same prefill kernels, same bytes);
    later steps differ by the 4-bit MFMA's inner summation order and the bf16 rounding flips that follow.  Measured relative
    differences of the later steps, the largest of a case's three rows (MI355X): d64 2.2e-4, d128 9.0e-3, d16 3.5e-4, qwen3 2.5e-4
    (MEASURED_TWIN; eight of the twelve rows are bit-equal: the flips are few and discrete in six tokens); the inline bound is 4 x the
    largest of the four."""
    from p2t_hip import ops
    meta = g["meta"]
    m = meta["cases"][case]
    n, pad = 6, meta["pad_id"]
    model = _model(g, case)
    model.set_gemm_dtype("mxfp4")
    kw = dict(max_new_tokens=n, eos_token_id=None, pad_token_id=pad, do_sample=False, return_dict_in_generate=True, output_logits=True)
    out = model.generate(**_inputs(g), **kw)
    out_n = model.generate(**_inputs(g), **kw, stream_copy=False, use_graph=False)
    assert torch.equal(out.sequences, out_n.sequences) and torch.equal(torch.stack(out.logits, 0), torch.stack(out_n.logits, 0))
    toks, lg = to_np(out.sequences), to_np(torch.stack(out.logits, 0))
    assert toks.shape == (3, n) and np.isfinite(lg).all()
    # the twin: decoder masters = W~, mode "fp8"
    twin = _model(g, case)
    for name, p in twin.llama_decoder.model.named_parameters():
        if name.startswith("layers.") and name.endswith(_PROJ):
            codes, bs = ops.quant_rows_mxfp4(p.data.contiguous())
            p.data.copy_(ops.dequant_rows_mxfp4(codes, bs, p.shape[1]))
    twin.llama_decoder.model.invalidate_engine()
    twin.set_gemm_dtype("fp8")
    L = m["llama"]["num_hidden_layers"]
    e1, e2 = model.llama_decoder.model.ensure_engine(L), twin.llama_decoder.model.ensure_engine(L)
    for t1, t2 in zip(e1["keep"][:L], e2["keep"][:L]):
        for name in ("qkv", "o", "gu", "down"):
            assert torch.equal(t1[name + "_w"], t2[name + "_w"]) and torch.equal(t1[name + "_ws"], t2[name + "_ws"]), name
    out_t = twin.generate(**_inputs(g), **kw)
    assert torch.equal(out.logits[0], out_t.logits[0])
    tt, lt = to_np(out_t.sequences), to_np(torch.stack(out_t.logits, 0))
    for b in range(toks.shape[0]):                                   # compare while both engines were fed the same tokens
        same = 1 + int(np.cumprod(toks[b, : n - 1] == tt[b, : n - 1]).sum())
        assert same >= 2
        observe(f"generate[{case}].mxfp4_vs_fp8_twin.row{b}", rel(lg[1:same, b], lt[1:same, b]), TWIN_BOUND)
    # the model's own cache-less forward over prompt + generated ids, and the fp8 oracle fed W~ and the same tokens: the fp8 bounds
    emb, mask = model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                      protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)
    dec = model.llama_decoder
    for b in range(toks.shape[0]):
        valid = to_np(mask)[b] != 0
        row = torch.cat([emb[b][torch.from_numpy(valid).to(emb.device)], dec.model.embed(to_dev(toks[b:b + 1, :-1]))[0]], 0)[None]
        full = to_np(dec(inputs_embeds=row).logits.float())[0]
        n0 = int(valid.sum())
        observe(f"generate[{case}].mxfp4_cache_vs_full_forward.row{b}", rel(lg[:, b], full[n0 - 1:n0 - 1 + n]), 8e-2)
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    W = _Patched(model_weights(esm, llama, ad, m["weight_seed"], lm_head=True), llama)
    _, ref = O.generate_greedy(llama, W, to_np(emb), to_np(mask), n, (), pad, prec=O.FP8, forced=toks)
    observe(f"generate[{case}].mxfp4_vs_fp8oracle_on_wtilde.logits", rel(lg, ref), 1e-1)


# largest relative difference of steps 2..6 against the fp8 twin, per case (see test_model_mxfp4), and the bound that follows from it
MEASURED_TWIN = dict(d64=2.24e-4, d128=8.98e-3, d16=3.50e-4, qwen3=2.55e-4)
TWIN_BOUND = 4 * max(MEASURED_TWIN.values())


def test_beam_search_and_seeded_sampling_run_on_top(g):
    """The selection paths see only logits: one beam search (3 beams, on the device) and one seeded sampling call, graph == eager."""
    meta = g["meta"]
    model = _model(g, "d64")
    model.set_gemm_dtype("mxfp4")
    kw = dict(max_new_tokens=6, eos_token_id=meta["cases"]["d64"]["eos"], pad_token_id=meta["pad_id"])
    a = model.generate(**_inputs(g), **kw, num_beams=3, beam_select="device")
    b = model.generate(**_inputs(g), **kw, num_beams=3, beam_select="device", use_graph=False)
    assert torch.equal(a, b) and a.shape[0] == 3
    c = model.generate(**_inputs(g), **kw, do_sample=True, top_k=20, seed=5)
    d = model.generate(**_inputs(g), **kw, do_sample=True, top_k=20, seed=5, use_graph=False)
    assert torch.equal(c, d) and c.shape[0] == 3
