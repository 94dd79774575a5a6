"""`generate(prefill="packed")`: the padding-free prefill of ragged prompts (p2t_llama_prefill_packed; p2t_hip/generation.py) behind
every door of generate.  Only the writer of the cache's prompt segment changes, so the references and bounds are the padded path's:
the reference class's goldens in fp32 (tests/golden/generate_tiny.npz), the bf16-rounding oracle and the model's own cache-less forward
in bf16, the patched oracle of tests/kv8_reference.py under the fp8 prompt segment."""
import json
import os

import numpy as np
import pytest
import torch

import kv8_reference as K
from oracle import p2t_oracle as O
from gpu_util import build_model, dev, observe, rel, rnd, to_dev, to_np
from helpers import model_weights
from p2t_hip import specs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["d16", "d64", "d128", "qwen3"]
TWO_ROWS = 20                # the golden prompts hold 15 / 11 / 8 tokens: rows of at most 20 are [15] and [11, 8]


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(HERE, "golden", "generate_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


def _model(g, case, dtype):
    m = g["meta"]["cases"][case]
    model = build_model(specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"]), dtype, m["weight_seed"])
    model.config.placeholder_id = g["meta"]["placeholder_id"]
    model.eval()
    return model


def _weights(g, case):
    m = g["meta"]["cases"][case]
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    return llama, model_weights(esm, llama, ad, m["weight_seed"], lm_head=True)


def _inputs(g):
    return dict(inputs=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                protein_attention_mask=to_dev(g["protein_attention_mask"]))


def _decoder_inputs(model, g):
    return model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                 protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)


def _greedy(model, g, n, **kw):
    return model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=g["meta"]["pad_id"], do_sample=False, return_dict_in_generate=True,
                          output_logits=True, **kw)


def _lg(out):
    return to_np(torch.stack(out.logits, 0))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack_tokens", [None, TWO_ROWS], ids=["one_row", "two_rows"])
@pytest.mark.parametrize("case", CASES)
def test_fp32_greedy_and_beams_vs_reference_generate(g, case, pack_tokens):
    """test_fp32_greedy_vs_reference_generate's assertions and the `lp` loop of test_fp32_beam_search_vs_reference_generate, with their
    bounds, on the packed prefill: greedy ids equal, logits within 2e-4, the early-stopping rows equal, 3 beams at both length penalties
    with equal sequences and scores within 1e-4 -- as one packed row and as two."""
    model = _model(g, case, torch.float32)
    meta = g["meta"]
    n, pad, eos = meta["max_new_tokens"], meta["pad_id"], meta["cases"][case]["eos"]
    pk = dict(prefill="packed", pack_tokens=pack_tokens)
    out = _greedy(model, g, n, num_beams=1, **pk)
    assert np.array_equal(to_np(out.sequences), g[f"{case}.greedy"])
    err = np.abs(_lg(out) - g[f"{case}.greedy_logits"]).max()
    print(f"prefill_packed[{case},{pack_tokens}]: fp32 greedy logits vs the reference class, max abs {err:.3e}")
    assert err < 2e-4
    seq = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=eos, pad_token_id=pad, return_dict_in_generate=False, num_beams=1, length_penalty=1.0,
                         temperature=1.0, do_sample=False, top_p=1.0, top_k=50, sync_every=4, **pk)
    assert np.array_equal(to_np(seq), g[f"{case}.greedy_eos"])
    for lp in ("1.0", "0.5"):
        out = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=eos, pad_token_id=pad, do_sample=False, num_beams=3, length_penalty=float(lp),
                             return_dict_in_generate=True, output_scores=True, **pk)
        assert np.array_equal(to_np(out.sequences), g[f"{case}.beam3_lp{lp}"]), lp
        assert np.abs(to_np(out.sequences_scores) - g[f"{case}.beam3_lp{lp}_scores"]).max() < 1e-4, lp


@pytest.mark.parametrize("case", CASES)
def test_bf16_steps_vs_bf16_oracle_and_own_forward(g, case):
    """8 greedy steps in bf16 from the packed prefill, teacher-forced: the bf16 oracle fed the same tokens (4e-2) and the model's own
    cache-less forward per row (3e-2) -- the padded path's bounds against the same references; the packed path is the same arithmetic up
    to summation order (and the rotation's place) and must meet them.  The packed-vs-padded difference of the first token's logits is
    printed and recorded under the oracle's bound, no tighter one."""
    model = _model(g, case, torch.bfloat16)
    n = 8
    out = _greedy(model, g, n, prefill="packed")
    toks, lg = to_np(out.sequences), _lg(out)
    llama, W = _weights(g, case)
    emb, mask = _decoder_inputs(model, g)
    _, ref = O.generate_greedy(llama, W, to_np(emb), to_np(mask), n, (), g["meta"]["pad_id"], prec=O.BF16, forced=toks)
    observe(f"prefill_packed[{case}].bf16_vs_bf16oracle.logits", rel(lg, ref), 4e-2)
    dec = model.llama_decoder
    for b in range(toks.shape[0]):
        valid = to_np(mask)[b] != 0
        row = torch.cat([emb[b][torch.from_numpy(valid).to(emb.device)], dec.model.embed(to_dev(toks[b:b + 1, :-1]))[0]], 0)[None]
        full = to_np(dec(inputs_embeds=row).logits.float())[0]
        n0 = int(valid.sum())
        observe(f"prefill_packed[{case}].bf16_cache_vs_full_forward.row{b}", rel(lg[:, b], full[n0 - 1:n0 - 1 + n]), 3e-2)
    padded = _greedy(model, g, 1)
    diff = rel(lg[0], _lg(padded)[0])
    print(f"prefill_packed[{case}]: bf16 first-token logits, packed vs padded, relative {diff:.3e}")
    observe(f"prefill_packed[{case}].bf16_first_logits_vs_padded", diff, 4e-2)


# ---------------------------------------------------------------------------------------------
EDGE_LENS = [100, 7, 64, 129, 1]             # prompts that end on, before and behind the 64-key tile edges; one crosses two


def _edge_inputs(hidden, seed=41, replace=None):
    """Synthetic decoder inputs: EDGE_LENS tokens per prompt, left-padded to 129.  `replace`: that prompt's embeddings drawn afresh."""
    T = max(EDGE_LENS)
    emb = rnd(seed, "edge.emb", (len(EDGE_LENS), T, hidden), 1.0)
    if replace is not None:
        emb[replace] = rnd(seed + 1, "edge.other", (T, hidden), 1.0)
    mask = np.zeros((len(EDGE_LENS), T), dtype=np.int64)
    for b, n in enumerate(EDGE_LENS):
        mask[b, T - n:] = 1
    return emb, mask


def _edge_run(model, emb, mask, n, pad, **kw):
    out = model.llama_decoder.generate(inputs_embeds=to_dev(emb), attention_mask=to_dev(mask), max_new_tokens=n, eos_token_id=None, pad_token_id=pad,
                                       do_sample=False, return_dict_in_generate=True, output_logits=True, **kw)
    return to_np(out.sequences), _lg(out), out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", ["d64", "d128"])
def test_tile_edges_through_the_model(g, case, dtype):
    """Prompt lengths 100 / 7 / 64 / 129 / 1, 6 greedy steps, as one packed row (320 tokens) and with pack_tokens=192 (two rows), per-step
    logits against the cache-less oracle fed each run's own tokens: 2e-4 absolute in fp32, 4e-2 relative against the bf16 oracle in bf16
    -- the golden tests' bounds.  The padded path runs on the same inputs in the same test and is recorded beside them."""
    model = _model(g, case, dtype)
    llama, W = _weights(g, case)
    pad, n = g["meta"]["pad_id"], 6
    emb, mask = _edge_inputs(llama.hidden_size)
    f32 = dtype == torch.float32
    refs = {}

    def err(toks, lg):
        key = toks.tobytes()
        if key not in refs:
            refs[key] = O.generate_greedy(llama, W, emb, mask, n, (), pad, forced=toks, **({} if f32 else dict(prec=O.BF16)))[1]
        return float(np.abs(lg - refs[key]).max()) if f32 else rel(lg, refs[key])

    tol, what, tag = (2e-4, "abs", "f32") if f32 else (4e-2, "rel", "bf16")
    toks, lg, _ = _edge_run(model, emb, mask, n, pad)
    e_pad = err(toks, lg)
    print(f"prefill_packed.edges[{case},{tag}]: padded {what} {e_pad:.3e}")
    observe(f"prefill_packed.edges[{case},{tag}].padded", e_pad, tol, what=what)
    for name, pk in (("one_row", None), ("two_rows", 192)):
        toks, lg, _ = _edge_run(model, emb, mask, n, pad, prefill="packed", pack_tokens=pk)
        e = err(toks, lg)
        print(f"prefill_packed.edges[{case},{tag}]: packed {name} {what} {e:.3e}")
        observe(f"prefill_packed.edges[{case},{tag}].{name}", e, tol, what=what)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_prompt_does_not_see_its_neighbours(g, dtype):
    """The same lengths with prompt 1's embeddings replaced: every step's logits and tokens of prompts 0 and 2 -- its neighbours in the
    packed row -- are bit-identical to the first run (rows of a GEMM are independent at equal M; attention and rotation are confined to
    the document), while prompt 1's change."""
    model = _model(g, "d64", dtype)
    pad, n = g["meta"]["pad_id"], 6
    H = model.llama_decoder.spec.hidden_size
    runs = []
    for replace in (None, 1):
        emb, mask = _edge_inputs(H, replace=replace)
        _, _, out = _edge_run(model, emb, mask, n, pad, prefill="packed")
        runs.append((out.sequences, torch.stack(out.logits, 0)))
    for b in (0, 2, 3, 4):
        assert torch.equal(runs[0][0][b], runs[1][0][b]) and torch.equal(runs[0][1][:, b], runs[1][1][:, b]), b
    assert not torch.equal(runs[0][1][:, 1], runs[1][1][:, 1])


@pytest.mark.parametrize("dtype,tail", [(torch.float32, "nan"), (torch.float32, "junk"), (torch.bfloat16, "junk")], ids=["f32-nan", "f32-junk", "bf16-junk"])
def test_a_poisoned_padded_tail_and_a_nan_cache_change_nothing(g, dtype, tail):
    """The padded tail of the packed rows is poisoned and the whole cache (both segments) holds NaN before the prefill: the first token's
    logits and two steps give the bits of the clean run.  Nothing behind a prompt's length is written or read, and no prompt's result
    depends on the tail.  fp32: NaN in the tail, as in the cache.  bf16: large, distinct, FINITE junk in the tail (up to 3e3, both signs;
    the RMSNorm brings every row back to O(1), so nothing overflows through the layers) -- the finite-padding contract of
    p2t_llama_prefill_packed (include/p2t_hip.h): the bf16 prefill attention multiplies the exact zeros of masked probabilities with the V
    rows of its whole 64-key tile, 0 x finite = 0 but 0 x NaN = NaN.  Measured with NaN in the tail in bf16: every first-token logit is
    NaN; that is the documented limit, and p2t_pack_rows' zeros are what keeps it away."""
    from p2t_hip.generation import DecodeEngine
    model = _model(g, "d64", dtype)
    emb, mask = _decoder_inputs(model, g)
    eos, pad, V = torch.zeros((0,), dtype=torch.int64, device=dev()), g["meta"]["pad_id"], model.llama_decoder.spec.vocab_size
    outs = []
    for poison in (False, True):
        eng = DecodeEngine(model.llama_decoder, emb.shape[0], 1, emb.shape[1], 8)
        packed = eng.pack(emb, mask)
        used = int(sum(n for _, _, n in packed.place))
        assert packed.embeds.shape[0] == 1 and 0 < used < packed.embeds.shape[1]
        if poison:
            n_tail = packed.embeds.shape[1] - used
            junk = torch.linspace(-3e3, 3e3, n_tail * packed.embeds.shape[2], device=dev()).reshape(n_tail, -1)
            packed.embeds[0, used:] = float("nan") if tail == "nan" else junk
            for t in (eng.k_prompt, eng.vt_prompt, eng.k_gen, eng.vt_gen):
                t.fill_(float("nan"))
        first = eng.prefill_packed(packed)
        eng.greedy_select(first, eos, pad)
        for _ in range(2):
            eng.feed(eng.next_tokens)
            eng.decode_step()
            eng.greedy_select(eng.logits, eos, pad)
        outs.append((first[:, :V].clone(), eng.logits[:, :V].clone(), eng.out_tokens[:, :3].clone()))
    assert torch.isfinite(outs[1][0].float()).all() and torch.isfinite(outs[1][1].float()).all()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d16", "d128"])
def test_fp8_prompt_segment_behind_the_packed_prefill(g, case):
    """prompt_kv_dtype="fp8" with prefill="packed": 6 steps against the patched bf16 oracle under tests/test_gpu_generate_kv8.py's 4e-2,
    and the replayed graph equals the eager steps bit for bit."""
    model = _model(g, case, torch.bfloat16)
    n = 6
    out = _greedy(model, g, n, prompt_kv_dtype="fp8", prefill="packed")
    eager = _greedy(model, g, n, prompt_kv_dtype="fp8", prefill="packed", use_graph=False)
    assert torch.equal(out.sequences, eager.sequences) and torch.equal(torch.stack(out.logits, 0), torch.stack(eager.logits, 0))
    toks, lg = to_np(out.sequences), _lg(out)
    llama, W = _weights(g, case)
    emb, mask = _decoder_inputs(model, g)
    mask = to_np(mask)
    with K.patched_oracle((mask != 0).sum(1), llama.num_hidden_layers):
        _, ref = O.generate_greedy(llama, W, to_np(emb), mask, n, (), g["meta"]["pad_id"], prec=O.BF16, forced=toks)
    observe(f"prefill_packed[{case}].kv8_bf16_vs_patched_bf16oracle.logits", rel(lg, ref), 4e-2)


@pytest.mark.parametrize("door", ["sampling", "ancestry", "lm_head_fp8", "processors"])
def test_the_other_doors_run_behind_the_packed_prefill(g, door):
    """bf16, d64: seeded sampling with two sequences per prompt, beam search on the ancestry table, the fp8 LM head and a logits-processor
    run, each from the packed prefill: it runs, returns the padded call's shape and repeats its bits on a second call."""
    model = _model(g, "d64", torch.bfloat16)
    meta = g["meta"]
    base = dict(max_new_tokens=6, eos_token_id=meta["cases"]["d64"]["eos"], pad_token_id=meta["pad_id"])
    kw = dict(sampling=dict(do_sample=True, seed=7, temperature=0.8, top_k=8, top_p=0.9, num_return_sequences=2),
              ancestry=dict(num_beams=3, beam_cache="ancestry", return_dict_in_generate=True, output_scores=True),
              lm_head_fp8=dict(lm_head_dtype="fp8", return_dict_in_generate=True, output_logits=True),
              processors=dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3, return_dict_in_generate=True, output_scores=True))[door]
    a = model.generate(**_inputs(g), **base, **kw, prefill="packed")
    b = model.generate(**_inputs(g), **base, **kw, prefill="packed")
    p = model.generate(**_inputs(g), **base, **kw)
    seqs = lambda o: o if isinstance(o, torch.Tensor) else o.sequences
    assert torch.equal(seqs(a), seqs(b)) and seqs(a).shape[0] == seqs(p).shape[0] == (6 if door == "sampling" else 3)
    assert seqs(a).dtype == seqs(p).dtype and seqs(a).shape[1] <= 6
    if door == "ancestry":
        assert torch.equal(a.sequences_scores, b.sequences_scores) and a.sequences_scores.shape == p.sequences_scores.shape
    if door == "lm_head_fp8":
        assert torch.equal(torch.stack(a.logits, 0), torch.stack(b.logits, 0)) and a.logits[0].shape == p.logits[0].shape
        assert torch.isfinite(torch.stack(a.logits, 0)).all()
    if door == "processors":
        assert torch.equal(torch.stack(a.scores, 0), torch.stack(b.scores, 0)) and a.scores[0].shape == p.scores[0].shape


def test_refusals(g):
    model = _model(g, "d64", torch.bfloat16)
    kw = dict(max_new_tokens=2, pad_token_id=g["meta"]["pad_id"])
    with pytest.raises(ValueError, match="prefill = 'ragged'"):
        model.generate(**_inputs(g), **kw, prefill="ragged")
    with pytest.raises(ValueError, match="pack_tokens is the row capacity of prefill='packed'"):
        model.generate(**_inputs(g), **kw, pack_tokens=64)
    with pytest.raises(ValueError, match="pack_tokens"):
        model.generate(**_inputs(g), **kw, prefill="padded", pack_tokens=64)
    with pytest.raises(ValueError, match="more than pack_tokens = 10"):
        model.generate(**_inputs(g), **kw, prefill="packed", pack_tokens=10)
    with pytest.raises(NotImplementedError, match="prefill='packed'"):
        model.continuous_generator(2, 64, 8, prefill="packed")
    for mode in ("fp8", "mxfp4"):
        model.set_gemm_dtype(mode)
        with pytest.raises(ValueError, match="packed.*model-dtype GEMMs"):
            model.generate(**_inputs(g), **kw, prefill="packed")
        assert model.generate(**_inputs(g), **kw).shape == (3, 2)                      # the padded path serves them as before
    model.set_gemm_dtype("model")
    assert model.generate(**_inputs(g), **kw, prefill="packed").shape == (3, 2)
    assert torch.equal(model.generate(**_inputs(g), **kw, prefill="padded"), model.generate(**_inputs(g), **kw))


def test_inference_epoch_writes_the_same_json(g, tmp_path):
    """inference_epoch in fp32 with args["prefill"] = "packed" (and with args["pack_tokens"]) writes the JSON it writes without it, on the
    golden prompts (their top-2 gaps are wide: tests/test_gpu_generate_continuous.py, _gaps_hold)."""
    import p2t_hip as P
    model = _model(g, "d64", torch.float32)
    meta = g["meta"]
    n, pad, eos = meta["max_new_tokens"], meta["pad_id"], meta["cases"]["d64"]["eos"]

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=False):
            return [" ".join(str(int(t)) for t in row if not (skip_special_tokens and int(t) in (pad, eos))) for row in ids]

    batch = dict(name=["P1", "P2", "P3"], input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.from_numpy(g["attention_mask"]),
                 protein_input_ids=torch.from_numpy(g["protein_input_ids"]), protein_attention_mask=torch.from_numpy(g["protein_attention_mask"]),
                 description_input_ids=torch.tensor([[7, 8, pad], [9, eos, pad], [1, 2, 3]]))
    recs = []
    for i, extra in enumerate((dict(), dict(prefill="packed"), dict(prefill="packed", pack_tokens=TWO_ROWS))):
        d = tmp_path / str(i)
        d.mkdir()
        args = dict(max_generation_length=n, num_beams=1, length_penalty=1.0, temperature=1.0, do_sample=False, top_p=1.0, top_k=50,
                    save_generation_dir=str(d), save_generation_postfix_identifier="test", **extra)
        recs.append(open(P.inference_epoch(0, model, [batch], Tok(), args)).read())
    assert recs[0] == recs[1] == recs[2] and list(json.loads(recs[0])) == ["P1", "P2", "P3"]
    out = P.iterative_generation_loop(0, model, batch, n, eos_token_id=eos, pad_token_id=pad, prefill="packed")
    assert np.array_equal(to_np(out), g["d64.greedy_eos"])
