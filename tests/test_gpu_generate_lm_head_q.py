"""generate(lm_head_dtype=None | "fp8" | "mxfp4"): the quantised LM head of the prefill's first token and of every decode step
(p2t_hip/generation.py lm_head_q / DecodeEngine; include/p2t_hip.h p2t_lm_head_q, p2t_llama_decode_step_q, p2t_lm_head_logits_q), on
the tiny decoders of tests/golden/generate_tiny.npz.

The twin: the same model with the bf16 head master replaced by the de-quantised head W~ (every W~ value is a bf16 value; with tied
embeddings the twin's head is untied so that its embedding table stays the model's).  Under lm_head_dtype=None the twin's logits differ
from the quantised-head call's only by the e4m3 rounding of the normalised row (the bf16 path rounds it to bf16 instead) and the order
of the f32 sum.  Measured relative differences against the twin, the largest of a case's rows over the first token and the steps that
were fed the same tokens (MI355X): 2.6e-2 .. 2.9e-2 on the first token, 2.7e-2 .. 2.9e-2 on the steps, both formats (MEASURED_TWIN below,
case by case); the bound is 4 x the largest over the tiny decoders (4 x 2.944e-2 = 1.18e-1), the margin
tests/test_gpu_mxfp4.py takes for its twin and for the same reason (random tiny models, three rows)."""
import numpy as np
import pytest
import torch

import lm_head_q_reference as Q
from gpu_util import observe, rel, to_dev, to_np
from test_gpu_generate import _inputs, _model, g  # noqa: F401  (g: the module-scoped golden fixture)
from test_gpu_generate_sampling import _rederive

pytestmark = pytest.mark.gpu
CASES = ["d64", "d128", "d16", "qwen3"]
FMTS = ["fp8", "mxfp4"]
# largest relative difference to the twin per (case, head format): first token | later steps (see the module docstring)
MEASURED_TWIN = {
    ("d64", "fp8"): (2.731e-2, 2.740e-2), ("d64", "mxfp4"): (2.717e-2, 2.728e-2), ("d128", "fp8"): (2.616e-2, 2.655e-2),
    ("d128", "mxfp4"): (2.586e-2, 2.718e-2), ("d16", "fp8"): (2.923e-2, 2.734e-2), ("d16", "mxfp4"): (2.944e-2, 2.889e-2),
    ("qwen3", "fp8"): (2.639e-2, 2.700e-2), ("qwen3", "mxfp4"): (2.665e-2, 2.816e-2),
}                                                                    # an e4m3 rounding is up to 2^-4 relative, ~2.7e-2 r.m.s. over a row
TWIN_BOUND = 4 * max(max(v) for v in MEASURED_TWIN.values())


def _kw(g, n=6, **more):
    return dict(max_new_tokens=n, eos_token_id=None, pad_token_id=g["meta"]["pad_id"], do_sample=False, return_dict_in_generate=True, output_logits=True,
                **more)


def _stack(out):
    return torch.stack(out.logits, 0)


def _twin(g, case, fmt):
    """The model of `case` with its bf16 head master <- W~ (untied from the embedding table where the two are one tensor)."""
    from p2t_hip import ops
    twin = _model(g, case, torch.bfloat16)
    dec = twin.llama_decoder
    w = dec.lm_head.weight.detach()
    H = w.shape[1]
    if fmt == "fp8":
        c, s = ops.quant_rows_fp8(w.contiguous(), H)
        wt = torch.from_numpy(Q.e4m3_values(to_np(c), to_np(s), H)).to(torch.bfloat16).to(w.device)
    else:
        c, s = ops.quant_rows_mxfp4(w.contiguous(), H)
        wt = ops.dequant_rows_mxfp4(c, s, H)
    assert np.array_equal(to_np(wt).astype(np.float64), Q.head_values(fmt, to_np(c), to_np(s), H))          # W~ is bf16-exact
    dec.lm_head.weight = torch.nn.Parameter(wt.clone(), requires_grad=False)
    assert dec.lm_head.weight is not dec.model.embed_tokens.weight
    dec.model.invalidate_engine()
    return twin


@pytest.mark.parametrize("case", CASES)
def test_default_is_the_parent_path(g, case):
    model = _model(g, case, torch.bfloat16)
    a = model.generate(**_inputs(g), **_kw(g))
    b = model.generate(**_inputs(g), **_kw(g), lm_head_dtype=None)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(_stack(a), _stack(b))
    assert getattr(model.llama_decoder.model, "_lm_head_q", None) is None                                 # nothing built


@pytest.mark.parametrize("gemm", ["model", "fp8", "mxfp4"])
@pytest.mark.parametrize("fmt", FMTS)
def test_graph_and_stream_copy_equal_eager_row_major(g, fmt, gemm):
    """All six combinations of tower GEMM dtype and head dtype run; graph + stream copy == eager + row-major, tokens and logits."""
    model = _model(g, "d64", torch.bfloat16)
    model.set_gemm_dtype(gemm)
    a = model.generate(**_inputs(g), **_kw(g), lm_head_dtype=fmt)
    b = model.generate(**_inputs(g), **_kw(g), lm_head_dtype=fmt, stream_copy=False, use_graph=False)
    assert a.sequences.shape == (3, 6) and np.isfinite(to_np(_stack(a))).all()
    assert torch.equal(a.sequences, b.sequences) and torch.equal(_stack(a), _stack(b))
    base = model.generate(**_inputs(g), **_kw(g))
    assert not torch.equal(_stack(a), _stack(base))                                                       # another matrix scores the tokens


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", CASES)
def test_twin_first_token_and_steps(g, case, fmt):
    """Also the tied-embedding check (qwen3): the twin's embedding table is the model's bf16 table, so the first STEP's logits agree
    with the twin's only if the token fed after the first one was looked up in the bf16 table, not in the quantised head."""
    from p2t_hip import generation, ops
    model, twin = _model(g, case, torch.bfloat16), _twin(g, case, fmt)
    n = 6
    out = model.generate(**_inputs(g), **_kw(g, n), lm_head_dtype=fmt)
    ref = twin.generate(**_inputs(g), **_kw(g, n))
    toks, tt, lg, lt = to_np(out.sequences), to_np(ref.sequences), to_np(_stack(out)), to_np(_stack(ref))
    first = max(rel(lg[0, b], lt[0, b]) for b in range(toks.shape[0]))
    later = 0.0
    for b in range(toks.shape[0]):                                   # compare while both engines were fed the same tokens
        same = 1 + int(np.cumprod(toks[b, : n - 1] == tt[b, : n - 1]).sum())
        if same >= 2:
            later = max(later, rel(lg[1:same, b], lt[1:same, b]))
    print(f"MEASURED twin {case} {fmt}: first {first:.3e} later {later:.3e}")
    observe(f"generate[{case}].lm_head_{fmt}_vs_twin.first", first, TWIN_BOUND)
    observe(f"generate[{case}].lm_head_{fmt}_vs_twin.steps", later, TWIN_BOUND)
    assert (toks[:, 0] == tt[:, 0]).any()                            # at least one row's first step was compared
    # the cached head is the quantisers' output on the padded bf16 head, and the restatements' (values and scale bytes)
    dec = model.llama_decoder
    st = generation.lm_head_q(dec, fmt)
    H = dec.spec.hidden_size
    c, s = (ops.quant_rows_fp8 if fmt == "fp8" else ops.quant_rows_mxfp4)(dec._lm_head_padded(), H)
    assert torch.equal(st["codes"], c) and torch.equal(st["scales"], s)
    vals, sc = Q.quantise_head(fmt, to_np(dec.lm_head.weight.detach()))
    assert np.array_equal(Q.head_values(fmt, to_np(c), to_np(s), H), vals) and np.array_equal(to_np(s).reshape(sc.shape), sc)
    # built once per model; an in-place update of the head rebuilds it
    assert generation.lm_head_q(dec, fmt) is st
    with torch.no_grad():
        dec.lm_head.weight.mul_(2.0)                                 # bumps _version: every scale byte of a non-zero row moves up by one
    st2 = generation.lm_head_q(dec, fmt)
    assert st2 is not st and not torch.equal(st2["scales"], st["scales"])


@pytest.mark.parametrize("fmt", FMTS)
def test_prefill_scores_token_0_with_the_same_head(g, fmt):
    from p2t_hip import generation
    model = _model(g, "d128", torch.bfloat16)
    dec = model.llama_decoder
    emb, mask = model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                      protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)
    V = dec.spec.vocab_size
    for stream_copy in (True, False):
        eng = generation.DecodeEngine(dec, emb.shape[0], 1, emb.shape[1], 4, stream_copy, lm_head_dtype=fmt)
        e2, m2 = eng.compact(emb, mask)
        first = eng.prefill(e2, m2)
        # the prefill's last hidden rows again, through the standalone entry point on the row-major head
        import ctypes as C
        from p2t_hip._lib import call
        from p2t_hip.ops import ptr, stream
        ws = torch.empty((call("p2t_llama_prefill_workspace_bytes", C.byref(eng.e["cfg"]), e2.shape[0], e2.shape[1]),), dtype=torch.uint8, device=emb.device)
        last = torch.empty((e2.shape[0], e2.shape[2]), dtype=torch.float32, device=emb.device)
        call("p2t_llama_prefill", C.byref(eng.e["cfg"]), C.byref(eng.e["w"]), ptr(e2), ptr(m2), e2.shape[0], e2.shape[1], C.byref(eng.cache), ptr(last), ptr(ws),
             ws.numel(), stream())
        head, _ = generation.head_q_struct(dec, generation.lm_head_q(dec, fmt), False, e2.shape[0])
        again = generation.lm_head_logits_q(last, None, 0.0, head, V, eng.ld_logits)
        assert torch.equal(first[:, :V], again[:, :V])
    out = model.generate(**_inputs(g), **_kw(g, 2), lm_head_dtype=fmt)
    assert torch.equal(out.logits[0], first[:, :V].float())


@pytest.mark.parametrize("fmt", FMTS)
def test_sampling_beams_processors_and_kv8_run_around_it(g, fmt):
    meta = g["meta"]
    model = _model(g, "d64", torch.bfloat16)
    kw = dict(max_new_tokens=6, pad_token_id=meta["pad_id"], lm_head_dtype=fmt)
    eos = meta["cases"]["d64"]["eos"]
    # seeded sampling: every token re-derivable from the returned logits; graph == eager; num_return_sequences
    a = model.generate(**_inputs(g), **kw, eos_token_id=None, do_sample=True, temperature=0.7, top_k=5, top_p=0.9, seed=3, return_dict_in_generate=True,
                       output_logits=True)
    _rederive(a, 3, 0.7, 5, 0.9)
    b = model.generate(**_inputs(g), **kw, eos_token_id=None, do_sample=True, temperature=0.7, top_k=5, top_p=0.9, seed=3, use_graph=False)
    assert torch.equal(a.sequences, b)
    r2 = model.generate(**_inputs(g), **kw, eos_token_id=None, do_sample=True, top_k=5, seed=3, num_return_sequences=2)
    assert r2.shape == (6, 6)
    gen = torch.Generator(device=r2.device).manual_seed(1)
    assert model.generate(**_inputs(g), **kw, eos_token_id=eos, do_sample=True, top_k=5, generator=gen).shape[0] == 3
    # greedy with processors
    p = model.generate(**_inputs(g), **kw, eos_token_id=eos, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3)
    p2 = model.generate(**_inputs(g), **kw, eos_token_id=eos, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3, use_graph=False)
    assert torch.equal(p, p2)
    # device beam search, with and without processors, and beam sampling; the first step's logits are the greedy call's rows
    greedy = model.generate(**_inputs(g), **kw, eos_token_id=eos, return_dict_in_generate=True, output_logits=True)
    for more in (dict(), dict(repetition_penalty=1.3, no_repeat_ngram_size=2), dict(do_sample=True, top_k=12, seed=7)):
        s = model.generate(**_inputs(g), **kw, eos_token_id=eos, num_beams=3, beam_select="device", return_dict_in_generate=True, output_logits=True, **more)
        s2 = model.generate(**_inputs(g), **kw, eos_token_id=eos, num_beams=3, beam_select="device", use_graph=False, **more)
        assert torch.equal(s.sequences, s2) and s.sequences.shape[0] == 3
        assert torch.equal(s.logits[0], greedy.logits[0].repeat_interleave(3, dim=0))
    t = model.generate(**_inputs(g), **kw, eos_token_id=eos, num_beams=3, beam_select="torch")
    assert t.shape[0] == 3
    # with the fp8 prompt segment of the KV cache
    k = model.generate(**_inputs(g), **_kw(g), lm_head_dtype=fmt, prompt_kv_dtype="fp8")
    k2 = model.generate(**_inputs(g), **_kw(g), lm_head_dtype=fmt, prompt_kv_dtype="fp8", stream_copy=False, use_graph=False)
    assert torch.equal(k.sequences, k2.sequences) and torch.equal(_stack(k), _stack(k2))
    assert torch.equal(k.logits[0], greedy.logits[0])                # the prefill attends before the store


@pytest.mark.parametrize("gemm", ["model", "mxfp4"])
@pytest.mark.parametrize("fmt", FMTS)
def test_more_than_64_rows(g, fmt, gemm):
    """80 greedy rows and 16 prompts x 5 beams run the general fp8 GEMM on row-major e4m3 codes (a requested stream copy falls back);
    their logits agree with the same prompts' rows of a <= 64-row call within the twin bound."""
    model = _model(g, "d64", torch.bfloat16)
    model.set_gemm_dtype(gemm)
    inp = _inputs(g)
    rep = lambda t, n: t.repeat((n + t.shape[0] - 1) // t.shape[0], *([1] * (t.dim() - 1)))[:n]
    few = model.generate(**inp, **_kw(g, 3), lm_head_dtype=fmt)
    many = model.generate(**{k: rep(v, 80) for k, v in inp.items()}, **_kw(g, 3), lm_head_dtype=fmt, stream_copy=True)
    assert many.sequences.shape == (80, 3)
    lf, lm = to_np(_stack(few)), to_np(_stack(many))
    for b in range(80):
        src = b % 3
        same = 1 + int(np.cumprod(to_np(few.sequences)[src, :2] == to_np(many.sequences)[b, :2]).sum())
        observe(f"generate[d64].lm_head_{fmt}_{gemm}.80rows_vs_3rows", rel(lm[:same, b], lf[:same, src]), TWIN_BOUND)
    beams = model.generate(**{k: rep(v, 16) for k, v in inp.items()}, max_new_tokens=4, eos_token_id=g["meta"]["cases"]["d64"]["eos"],
                           pad_token_id=g["meta"]["pad_id"], num_beams=5, beam_select="device", lm_head_dtype=fmt, return_dict_in_generate=True,
                           output_logits=True)
    assert beams.sequences.shape[0] == 16
    first = to_np(beams.logits[0])
    for b in range(16):
        observe(f"generate[d64].lm_head_{fmt}_{gemm}.80beams_first_vs_3rows", rel(first[5 * b], lf[0, b % 3]), TWIN_BOUND)


def test_refusals(g):
    model = _model(g, "d64", torch.bfloat16)
    with pytest.raises(ValueError, match="lm_head_dtype must be None, 'fp8' or 'mxfp4'"):
        model.generate(**_inputs(g), max_new_tokens=2, lm_head_dtype="int8")
    with pytest.raises(ValueError, match="lm_head_dtype must be"):
        model.generate(**_inputs(g), max_new_tokens=2, num_beams=2, lm_head_dtype="bf16")
    f32 = _model(g, "d64", torch.float32)
    for fmt in FMTS:
        with pytest.raises(ValueError, match="serves bf16 models only"):
            f32.generate(**_inputs(g), max_new_tokens=2, lm_head_dtype=fmt)


def test_vocabulary_not_a_multiple_of_16_is_refused_beyond_64_rows():
    """Up to 64 rows the skinny kernels cut the last tile; beyond that the general GEMM would refuse at the prefill: the engine says so first."""
    import p2t_hip as P
    from p2t_hip import generation, specs
    esm = specs.EsmSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2)
    llama = specs.LlamaSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=1, vocab_size=500)
    model = P.Esm2LlamaInstructForCausalLM.from_specs(esm, llama, specs.AdapterSpec(64, 64, 64, 0.0), dtype=torch.bfloat16, device=torch.device("cuda:0"), seed=0)
    for fmt in FMTS:
        with pytest.raises(ValueError, match="multiple of 16"):
            generation.DecodeEngine(model.llama_decoder, 80, 1, 8, 4, lm_head_dtype=fmt)
        with pytest.raises(ValueError, match="multiple of 16"):
            generation.DecodeEngine(model.llama_decoder, 16, 5, 8, 4, lm_head_dtype=fmt)
        assert generation.DecodeEngine(model.llama_decoder, 64, 1, 8, 4, lm_head_dtype=fmt).head_q is not None


def test_the_bf16_head_has_no_stream_copy_while_the_quantised_head_serves(g):
    """stream_weights builds the bf16 head's stream-order copy (1.05 GB at Llama-8B sizes) only for a call that reads it."""
    model = _model(g, "d64", torch.bfloat16)
    a = model.generate(**_inputs(g), **_kw(g, 3), lm_head_dtype="fp8")
    st = model.llama_decoder.model._stream_engine
    assert st["lm_head"] is None and st["layers"] is not None
    b = model.generate(**_inputs(g), **_kw(g, 3))
    assert model.llama_decoder.model._stream_engine is st and st["lm_head"] is not None
    c = model.generate(**_inputs(g), **_kw(g, 3), stream_copy=False, use_graph=False)
    assert torch.equal(_stack(b), _stack(c)) and not torch.equal(_stack(a), _stack(b))
