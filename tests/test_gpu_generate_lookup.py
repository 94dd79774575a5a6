"""`generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n)` (p2t_hip/lookup.py over p2t_lookup_draft_rows,
p2t_llama_decode_step_multi, p2t_lookup_verify_rows): greedy decoding's tokens in fewer steps.

* fp32, the four golden decoder shapes (tests/golden/generate_tiny.npz, the REFERENCE class's generate): ids exact, the logits that chose
  every token to 2e-4, lookup_stats equal to the numpy simulator's run on the golden tokens (tests/lookup_reference.py) -- every case
  accepts, rejects and leaves its rows out of step; the eos rule with rows that stop early;
* 70 new tokens (rows cross the 64-key tile of the generated segment at different steps), k = 3 / n = 2 and k = 7 / n = 3, against the
  cache-less oracle teacher-forced with the tokens returned;
* bf16 (and with the fp8 prompt segment, the fp8 LM head and the packed prefill around it): the logged logits against the bf16 oracle fed
  the same tokens, and every returned token the argmax of the logged row before it."""
import json
import os

import numpy as np
import pytest
import torch

import lookup_reference as R
from oracle import p2t_oracle as O
from gpu_util import build_model, observe, rel, to_dev, to_np
from helpers import model_weights
from p2t_hip import specs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["d16", "d64", "d128", "qwen3"]
# (verify steps, accepted tokens) per row at k = 3, n = 2 on the golden greedy tokens (test_lookup_host.py checks the simulator on them)
TABLE = {"d16": [(11, 2), (9, 4), (13, 0)], "d64": [(9, 5), (13, 0), (11, 2)], "d128": [(12, 2), (12, 1), (13, 0)],
         "qwen3": [(12, 2), (13, 0), (12, 1)]}


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


def _inputs(g):
    return dict(inputs=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                protein_attention_mask=to_dev(g["protein_attention_mask"]))


def _oracle_inputs(g, model, case):
    m = g["meta"]["cases"][case]
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    W = model_weights(esm, llama, ad, m["weight_seed"], lm_head=True)
    emb, mask = model(**{("input_ids" if k == "inputs" else k): v for k, v in _inputs(g).items()}, return_decoder_inputs=True)
    return llama, W, to_np(emb), to_np(mask)


def _stats(tokens, k, n, eos=()):
    return [list(R.simulate(row, k, n, eos)) for row in tokens]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_fp32_lookup_is_the_reference_greedy_generate(g, case, use_graph):
    model = _model(g, case, torch.float32)
    meta = g["meta"]
    n, pad = meta["max_new_tokens"], meta["pad_id"]
    out = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=pad, do_sample=False, num_beams=1,
                         return_dict_in_generate=True, output_logits=True, use_graph=use_graph, prompt_lookup_num_tokens=3, max_matching_ngram_size=2,
                         sync_every=4)
    gold = g[f"{case}.greedy"]
    assert np.array_equal(to_np(out.sequences), gold)
    err = np.abs(to_np(torch.stack(out.logits, 0)) - g[f"{case}.greedy_logits"]).max()
    print(f"lookup[{case}] fp32 logits vs golden: {err:.3e}")
    assert err < 2e-4
    stats = to_np(out.lookup_stats).tolist()
    assert stats == _stats(gold, 3, 2)
    assert [(s, a) for s, _, a in stats] == TABLE[case]
    # n defaults to HF's 2
    again = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=pad, return_dict_in_generate=True, use_graph=use_graph,
                           prompt_lookup_num_tokens=3)
    assert torch.equal(again.sequences, out.sequences) and torch.equal(again.lookup_stats, out.lookup_stats) and again.logits is None
    # rows that stop early (the second row's 5th token is the eos): pad behind the eos, the other rows go on
    eos = meta["cases"][case]["eos"]
    res = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=eos, pad_token_id=pad, return_dict_in_generate=True, use_graph=use_graph,
                         sync_every=3, prompt_lookup_num_tokens=3, max_matching_ngram_size=2)
    assert np.array_equal(to_np(res.sequences), g[f"{case}.greedy_eos"])
    assert to_np(res.lookup_stats).tolist() == _stats(gold, 3, 2, (eos,))
    seq = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=eos, pad_token_id=pad, prompt_lookup_num_tokens=7, max_matching_ngram_size=4)
    assert np.array_equal(to_np(seq), g[f"{case}.greedy_eos"])


@pytest.mark.parametrize("case", ["d64", "qwen3"])
@pytest.mark.parametrize("k,ngram", [(3, 2), (7, 3)])
def test_long_lookup_crosses_the_tile_boundary_row_by_row(g, case, k, ngram):
    """70 new tokens: the rows reach key 64 of the generated segment at different steps, inside a step's tokens.  The logits of every
    position against the cache-less oracle fed the returned tokens (2e-4); ids = the oracle's argmax wherever its top-2 gap is no
    near-tie; the simulator on the returned tokens must tell the counters; every row accepts and rejects."""
    model = _model(g, case, torch.float32)
    n, pad = 70, g["meta"]["pad_id"]
    out = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=pad, return_dict_in_generate=True, output_logits=True,
                         sync_every=32, prompt_lookup_num_tokens=k, max_matching_ngram_size=ngram)
    toks, lg = to_np(out.sequences), to_np(torch.stack(out.logits, 0))
    assert toks.shape == (3, n)
    llama, W, emb, mask = _oracle_inputs(g, model, case)
    _, ref = O.generate_greedy(llama, W, emb, mask, n, (), pad, forced=toks)
    err = np.abs(lg - ref).max()
    print(f"lookup[{case},k{k},n{ngram}] fp32 logits vs forced oracle: {err:.3e}")
    assert err < 2e-4
    top2 = np.sort(ref, axis=-1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 1e-3                       # [n, B]
    assert np.array_equal(toks.T[clear], ref.argmax(-1)[clear]) and clear.mean() > 0.95
    stats = to_np(out.lookup_stats).tolist()
    print(f"lookup[{case},k{k},n{ngram}] (steps, drafted, accepted) per row: {stats}")
    assert stats == _stats(toks, k, ngram)
    for row, (steps, drafted, accepted) in zip(toks, stats):
        assert accepted >= 5 and R.simulate(row, k, ngram, detail=True)[3] >= 5 and steps < n - 1      # [3]: the drafts that were rejected
    # the eager loop replays nothing and must return the same
    eager = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=pad, use_graph=False, prompt_lookup_num_tokens=k,
                           max_matching_ngram_size=ngram)
    assert np.array_equal(to_np(eager), toks)


def _consistent(out, V):
    """every returned token is the argmax of the logged row that chose it"""
    toks, lg = out.sequences, torch.stack(out.logits, 0)               # [B, n], [n, B, V]
    assert torch.equal(lg.argmax(-1).T, toks)
    return to_np(toks), to_np(lg)


@pytest.mark.parametrize("case", CASES)
def test_bf16_lookup_vs_bf16_oracle_on_the_same_tokens(g, case):
    model = _model(g, case, torch.bfloat16)
    n, pad = 24, g["meta"]["pad_id"]
    kw = dict(max_new_tokens=n, eos_token_id=None, pad_token_id=pad, return_dict_in_generate=True, output_logits=True, prompt_lookup_num_tokens=3,
              max_matching_ngram_size=2)
    out = model.generate(**_inputs(g), **kw)
    toks, lg = _consistent(out, model.llama_decoder.spec.vocab_size)
    assert toks.shape == (3, n)
    llama, W, emb, mask = _oracle_inputs(g, model, case)
    _, ref = O.generate_greedy(llama, W, emb, mask, n, (), pad, prec=O.BF16, forced=toks)
    observe(f"generate_lookup[{case}].bf16_vs_bf16oracle.logits", rel(lg, ref), 4e-2)
    assert to_np(out.lookup_stats).tolist() == _stats(toks, 3, 2)
    # the unfused rotation (its own launch) and the row-major weights: the same step
    for other in (dict(fuse_rope=False), dict(stream_copy=False, use_graph=False)):
        o2 = model.generate(**_inputs(g), **kw, **other)
        t2, l2 = _consistent(o2, model.llama_decoder.spec.vocab_size)
        observe(f"generate_lookup[{case}].bf16_vs_bf16oracle.logits", rel(l2, O.generate_greedy(llama, W, emb, mask, n, (), pad, prec=O.BF16, forced=t2)[1]),
                4e-2)


@pytest.mark.parametrize("case", ["d64", "d128"])
def test_bf16_lookup_with_fp8_prompt_segment_fp8_head_and_packed_prefill(g, case):
    model = _model(g, case, torch.bfloat16)
    n, pad = 24, g["meta"]["pad_id"]
    kw = dict(max_new_tokens=n, eos_token_id=None, pad_token_id=pad, return_dict_in_generate=True, output_logits=True, prompt_kv_dtype="fp8",
              lm_head_dtype="fp8", prefill="packed")
    out = model.generate(**_inputs(g), **kw, prompt_lookup_num_tokens=3, max_matching_ngram_size=2)
    toks, _ = _consistent(out, model.llama_decoder.spec.vocab_size)
    assert toks.shape == (3, n) and to_np(out.lookup_stats).tolist() == _stats(toks, 3, 2)
    plain = model.generate(**_inputs(g), **kw)
    assert torch.equal(plain.sequences[:, 0], out.sequences[:, 0]) and torch.equal(plain.logits[0], out.logits[0])


@pytest.mark.parametrize("mode", ["fp8", "mxfp4"])
def test_lookup_on_quantised_decoder_weights(g, mode):
    """set_gemm_dtype("fp8") / ("mxfp4") decoders: the multi-token step streams the same e4m3 / MXFP4 weights; internal consistency and the
    existing fp8 bound against the fp8 oracle fed the same tokens (the MXFP4 codes are not the oracle's: consistency only)."""
    case = "d64"
    model = _model(g, case, torch.bfloat16)
    model.set_gemm_dtype(mode)
    n, pad = 12, g["meta"]["pad_id"]
    out = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=pad, return_dict_in_generate=True, output_logits=True,
                         prompt_lookup_num_tokens=3)
    toks, lg = _consistent(out, model.llama_decoder.spec.vocab_size)
    assert toks.shape == (3, n) and to_np(out.lookup_stats).tolist() == _stats(toks, 3, 2)
    if mode == "fp8":
        model.set_gemm_dtype("model")
        llama, W, emb, mask = _oracle_inputs(g, model, case)
        _, ref = O.generate_greedy(llama, W, emb, mask, n, (), pad, prec=O.FP8, forced=toks)
        observe(f"generate_lookup[{case}].fp8_vs_fp8oracle.logits", rel(lg, ref), 1e-1)


def test_eos_and_limit_inside_an_accepted_run(g):
    """An accepted draft token was generated before, so an eos can only end a run as the model's own token behind accepted ones: d64's
    third row starts 42 291 42 291 407 -- at 42 291 42 the draft is (291, 42), 291 is accepted and 407 follows it in the same step.  With
    407 as the eos that step ends the row.  d64's first row ends in 103 230 103 230 ...: limits of 9 and 10 fall inside an accepted run."""
    case = "d64"
    model = _model(g, case, torch.float32)
    pad, gold = g["meta"]["pad_id"], g["d64.greedy"]
    assert gold[2, :5].tolist() == [42, 291, 42, 291, 407] and gold[0, 5:10].tolist() == [103, 230, 103, 230, 103]
    res = model.generate(**_inputs(g), max_new_tokens=14, eos_token_id=407, pad_token_id=pad, return_dict_in_generate=True, prompt_lookup_num_tokens=3)
    want = model.generate(**_inputs(g), max_new_tokens=14, eos_token_id=407, pad_token_id=pad)
    assert torch.equal(res.sequences, want) and to_np(res.sequences)[2, 3:].tolist() == [291, 407] + [pad] * 9
    stats = to_np(res.lookup_stats).tolist()
    assert stats == _stats(gold, 3, 2, (407,)) and stats[2] == [3, 2, 1]
    for limit in (9, 10, 2):
        res = model.generate(**_inputs(g), max_new_tokens=limit, eos_token_id=None, pad_token_id=pad, return_dict_in_generate=True, prompt_lookup_num_tokens=3)
        assert np.array_equal(to_np(res.sequences), gold[:, :limit])
        assert to_np(res.lookup_stats).tolist() == _stats(gold[:, :limit], 3, 2)
    one = model.generate(**_inputs(g), max_new_tokens=1, eos_token_id=None, pad_token_id=pad, return_dict_in_generate=True, output_logits=True,
                         prompt_lookup_num_tokens=3)
    assert np.array_equal(to_np(one.sequences), gold[:, :1]) and len(one.logits) == 1 and not to_np(one.lookup_stats).any()
