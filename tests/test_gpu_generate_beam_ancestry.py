"""`generate(..., num_beams > 1, beam_cache="ancestry")`: beam search without the per-step copy of the generated keys and values
(p2t_kv_ancestry_update + p2t_llama_decode_step_beams in p2t_kv_reorder + the step's place), on the tiny golden models of
tests/test_gpu_generate.py (fixtures imported from there, helpers from tests/test_gpu_generate_beam.py): the goldens of the reference's
own beam search, graph against eager, the copy path, a stop between two host reads, 70 tokens against the oracle, 16 beams, bf16 with
the bf16 and the fp8 prompt segment and MXFP4 weights, the logits processors and seeded sampling under beams, the refusals, and
`inference_epoch`."""
import json
import os

import numpy as np
import pytest
import torch

import beam_sample_reference as SR
from gpu_util import to_dev, to_np
from helpers import model_weights
from oracle import p2t_oracle as O
from p2t_hip import specs
from test_gpu_generate import CASES, _inputs, _model, g  # noqa: F401  (g: the module-scoped golden fixture)
from test_gpu_generate_beam import _gen, _rederive, _same
from test_gpu_generate_beam_sample import WARP, _gen as _gen_sample

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ANC = dict(beam_select="device", beam_cache="ancestry")


@pytest.fixture(autouse=True)
def _no_copy(monkeypatch):
    """Every test of this file runs with DecodeEngine.reorder raising on an engine that carries a table: the ancestry runs never call it
    (the copy path's engines, which the comparisons build, still re-order)."""
    from p2t_hip.generation import DecodeEngine
    real = DecodeEngine.reorder

    def refuse(self, src_rows):
        if self.ancestry is not None:
            raise AssertionError("DecodeEngine.reorder was called under beam_cache='ancestry'")
        return real(self, src_rows)

    monkeypatch.setattr(DecodeEngine, "reorder", refuse)


def _both(model, g, n, what, **kw):
    """-> the replayed ancestry run, after comparing it with its eager run (bit for bit) and with the copy path (ids and beam indices
    equal, scores under `_same`'s bound for two log-softmax evaluations)."""
    a = _gen(model, g, n, **ANC, **kw)
    _same(a, _gen(model, g, n, use_graph=False, **ANC, **kw), (what, "graph vs eager"))
    _same(a, _gen(model, g, n, beam_select="device", **kw), (what, "ancestry vs copy"), scores_exact=False)
    return a


@pytest.mark.parametrize("case", CASES)
def test_fp32_reproduces_the_reference_beam_search(g, case):
    model = _model(g, case, torch.float32)
    meta = g["meta"]
    n = meta["max_new_tokens"]
    for lp in ("1.0", "0.5"):
        out = _both(model, g, n, (case, lp), eos_token_id=meta["cases"][case]["eos"], num_beams=3, length_penalty=float(lp))
        assert np.array_equal(to_np(out.sequences), g[f"{case}.beam3_lp{lp}"]), lp
        assert np.abs(to_np(out.sequences_scores) - g[f"{case}.beam3_lp{lp}_scores"]).max() < 1e-4, lp
    for es in (True, "never"):                              # two eos ids, two hypotheses per prompt
        out = _both(model, g, n, (case, es), eos_token_id=meta["cases"][case]["eos2"], num_beams=3, length_penalty=0.8, early_stopping=es,
                    num_return_sequences=2)
        assert np.array_equal(to_np(out.sequences), g[f"{case}.beam3_es{es}"]), es
        assert np.abs(to_np(out.sequences_scores) - g[f"{case}.beam3_es{es}_scores"]).max() < 1e-4, es
    plain = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=meta["cases"][case]["eos"], pad_token_id=meta["pad_id"], num_beams=3,
                           beam_cache="ancestry")
    assert np.array_equal(to_np(plain), g[f"{case}.beam3_lp1.0"])          # beam_select=None resolves to the device path


def test_the_engine_never_copies_and_never_allocates_the_second_segment(g, monkeypatch):
    from p2t_hip import generation
    engines = []
    real = generation.DecodeEngine.__init__

    def spy(self, *a, **kw):
        real(self, *a, **kw)
        engines.append(self)

    monkeypatch.setattr(generation.DecodeEngine, "__init__", spy)
    model = _model(g, "d64", torch.float32)
    _gen(model, g, 9, num_beams=3, **ANC)
    _gen(model, g, 9, num_beams=3, beam_select="device")
    anc, copy = engines
    assert anc.ancestry is not None and anc.ancestry.dtype == torch.uint8 and tuple(anc.ancestry.shape) == (9, 64)
    assert anc.k_alt is None and anc.vt_alt is None
    assert copy.ancestry is None and copy.k_alt is not None
    tab = to_np(anc.ancestry)
    assert (tab < 3).all() and np.array_equal(tab[:, 7], np.arange(9) % 3) and not tab[:, 8:].any()      # 8 steps: the last one's own keys


def test_long_search_vs_the_oracle(g):
    """3 beams x 70 new tokens: the table grows past one 64-key tile while the graph replays pairs of steps."""
    case = "d64"
    model = _model(g, case, torch.float32)
    meta = g["meta"]
    m = meta["cases"][case]
    n, pad = 70, meta["pad_id"]
    out = _gen(model, g, n, eos_token_id=m["eos"], num_beams=3, length_penalty=1.0, **ANC)
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    W = model_weights(esm, llama, ad, m["weight_seed"], lm_head=True)
    emb, mask = model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                      protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)
    seq, sc = O.generate_beam(llama, W, to_np(emb), to_np(mask), n, 3, (m["eos"],), pad, 1.0)
    assert np.array_equal(to_np(out.sequences), seq) and seq.shape[1] > 64
    assert np.abs(to_np(out.sequences_scores) - sc).max() < 1e-4


def test_a_stop_between_two_host_reads_and_odd_and_even_lengths(g):
    model = _model(g, "d64", torch.float32)
    free = _gen(model, g, 6, num_beams=3, output_logits=True, **ANC)
    eos = [int(t) for t in torch.topk(torch.log_softmax(free.logits[2], -1).mean(0), 20)[1]]
    kw = dict(num_beams=3, eos_token_id=eos, early_stopping=True, length_penalty=1.0)
    n = 14
    one = _gen(model, g, n, sync_every=1, **ANC, **kw)
    steps = len(one.scores)
    assert 2 <= steps < n - 1                               # it stops before the end: the replayed steps after it must change nothing
    for use_graph in (True, False):
        for sync_every in (4, 5, 16):
            _same(one, _gen(model, g, n, sync_every=sync_every, use_graph=use_graph, **ANC, **kw), (use_graph, sync_every))
    _same(one, _gen(model, g, n, beam_select="device", **kw), "copy", scores_exact=False)
    for n in (7, 8, 2, 1):                                  # the two-step graph's remainder; 1 and 2 never reach the graph
        out = _both(model, g, n, n, num_beams=3, length_penalty=1.0)
        assert out.sequences.shape == (3, n) and len(out.scores) == n


def test_sixteen_beams(g):
    model = _model(g, "d16", torch.float32)
    out = _both(model, g, 4, 16, num_beams=16, num_return_sequences=16)      # the widest group: one chunk of 16 slots per kv head and more
    assert out.sequences.shape == (48, 4)


def test_bf16_scores_like_the_copy_path(g):
    model = _model(g, "d64", torch.bfloat16)
    meta = g["meta"]
    eos, pad, n = meta["cases"]["d64"]["eos"], meta["pad_id"], 12
    kw = dict(num_beams=3, eos_token_id=eos, length_penalty=1.0, output_logits=True)
    anc = _gen(model, g, n, **ANC, **kw)
    _same(anc, _gen(model, g, n, use_graph=False, **ANC, **kw), "bf16 graph vs eager")
    copy = _gen(model, g, n, beam_select="device", **kw)
    diff = np.abs(to_np(anc.sequences_scores) - to_np(copy.sequences_scores))
    print("bf16 ancestry vs copy score differences", diff)
    assert np.isfinite(diff).all() and np.median(diff) < 5e-2 and diff.max() < 0.3, diff     # bf16 logits: near-tied beams may swap
    ok, st = _rederive(anc, 3, [eos], 1.0, False, n, pad)
    print("bf16: prompts decidable at every step:", ok)
    for b in np.nonzero(ok)[0]:                             # ids only where the returned logits decide every step
        assert np.array_equal(to_np(anc.sequences)[b], st["sequences"][b, 0, : anc.sequences.shape[1]]), b


@pytest.mark.parametrize("mode", ["kv8", "mxfp4"])
def test_bf16_with_the_fp8_prompt_segment_and_with_mxfp4_weights(g, mode):
    """The F8 prompt tiles under the 16 (beam, head) slots, and the MXFP4 step door: graph == eager bit for bit, scores like the copy
    path's under test_bf16_scores_like_the_copy_path's rule, the ids re-derived from the run's own logits where they decide."""
    model = _model(g, "d64", torch.bfloat16)
    extra = dict(prompt_kv_dtype="fp8")
    if mode == "mxfp4":
        model.set_gemm_dtype("mxfp4")
        extra = {}
    meta = g["meta"]
    eos, pad, n = meta["cases"]["d64"]["eos"], meta["pad_id"], 10
    kw = dict(num_beams=3, eos_token_id=eos, length_penalty=1.0, output_logits=True, **extra)
    anc = _gen(model, g, n, **ANC, **kw)
    _same(anc, _gen(model, g, n, use_graph=False, **ANC, **kw), (mode, "graph vs eager"))
    copy = _gen(model, g, n, beam_select="device", **kw)
    diff = np.abs(to_np(anc.sequences_scores) - to_np(copy.sequences_scores))
    print(mode, "ancestry vs copy score differences", diff)
    assert np.isfinite(diff).all() and np.median(diff) < 5e-2 and diff.max() < 0.3, diff
    ok, st = _rederive(anc, 3, [eos], 1.0, False, n, pad)
    for b in np.nonzero(ok)[0]:
        assert np.array_equal(to_np(anc.sequences)[b], st["sequences"][b, 0, : anc.sequences.shape[1]]), b


@pytest.mark.parametrize("case", CASES)
def test_processors_under_beams_reproduce_the_reference(g, case):
    z = np.load(os.path.join(HERE, "golden", "generate_beam_processors_tiny.npz"))
    sets = json.loads(bytes(z["meta_json"]).decode())["sets"][case]
    assert sets
    model = _model(g, case, torch.float32)
    for name, args in sets.items():
        for kw in ({}, dict(use_graph=False)):
            out = _gen(model, g, g["meta"]["max_new_tokens"], num_beams=3, num_return_sequences=3, **ANC, **args, **kw)
            assert np.array_equal(to_np(out.sequences), z[f"{case}.{name}"]), (case, name, kw)
            assert np.abs(to_np(out.sequences_scores) - z[f"{case}.{name}_scores"]).max() < 1e-4, (case, name, kw)


def test_beam_sampling_follows_from_the_returned_logits(g):
    """Seeded beam sampling with the switch on: every step re-derived from the run's own logits by tests/beam_sample_reference.py, as
    tests/test_gpu_generate_beam_sample.py does for the copy path; first, at least one step of every prompt is decidable."""
    model = _model(g, "d64", torch.float32)
    meta = g["meta"]
    eos, pad, n, nb = meta["cases"]["d64"]["eos2"], meta["pad_id"], 9, 3
    warp = WARP
    kw = dict(eos_token_id=eos, length_penalty=0.8, output_logits=True)          # _gen_sample: 3 beams, seed 3, the device selection, WARP
    a = _gen_sample(model, g, n, beam_cache="ancestry", **kw)
    b = _gen_sample(model, g, n, beam_cache="ancestry", use_graph=False, **kw)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores, b.sequences_scores)
    B = a.logits[0].shape[0] // nb
    st = SR.fresh_state(B, nb, n, pad)
    refs = []
    for cur, lg in enumerate(a.logits):
        refs.append(SR.step(to_np(lg), st, cur, nb, eos, 0.8, False, n, pad, warp["temperature"], warp["top_k"], warp["top_p"], 3, 0))
        st = refs[-1]["state"]
    ok = np.all([r["decidable"] & (r["running_decidable"] | bool(r["state"]["done"])) for r in refs], axis=0)
    assert ok.any(), "no prompt is decidable at every step"
    L = a.sequences.shape[1]
    for p in np.nonzero(ok)[0]:
        assert np.array_equal(to_np(a.sequences)[p], st["sequences"][p, 0, :L]) and np.array_equal(to_np(a.beam_indices)[p], st["beam_idx"][p, 0, :L]), p


def test_refusals(g):
    model = _model(g, "d16", torch.float32)
    with pytest.raises(ValueError, match="num_beams > 1"):
        model.generate(**_inputs(g), max_new_tokens=3, beam_cache="ancestry")
    with pytest.raises(ValueError, match="not 'torch'"):
        _gen(model, g, 3, num_beams=3, beam_select="torch", beam_cache="ancestry")
    with pytest.raises(ValueError, match="beam_cache='ancestry'"):                          # outside p2t_beam_select's range
        _gen(model, g, 3, num_beams=17, beam_cache="ancestry")
    with pytest.raises(ValueError, match="beam_cache='ancestry'"):
        _gen(model, g, 3, num_beams=17, **ANC)
    with pytest.raises(ValueError, match="beam_cache = 'table'"):
        _gen(model, g, 3, num_beams=3, beam_cache="table")
    from p2t_hip.generation import DecodeEngine
    with pytest.raises(ValueError, match="beam_cache must be"):
        DecodeEngine(model.llama_decoder, 3, 3, 40, 8, beam_cache="table")
    with pytest.raises(ValueError, match="rows per prompt"):
        DecodeEngine(model.llama_decoder, 3, 1, 40, 8, beam_cache="ancestry")
    wide = specs.LlamaSpec(num_hidden_layers=1, hidden_size=34 * 16, intermediate_size=64, num_attention_heads=34, num_key_value_heads=2, vocab_size=64)
    assert wide.num_attention_heads // wide.num_key_value_heads == 17

    class Wide:                                             # more than 16 query heads per kv head: refused before anything is built
        spec = wide

    from p2t_hip import generation
    with pytest.raises(ValueError, match="16 query heads per kv head"):
        generation.generate(Wide(), inputs_embeds=torch.zeros((1, 4, wide.hidden_size)), max_new_tokens=2, num_beams=2, beam_cache="ancestry")


def test_inference_epoch_writes_the_same_json_with_and_without_the_switch(g, tmp_path):
    import p2t_hip as P
    model = _model(g, "d64", torch.float32)

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=False):
            return [" ".join(str(int(t)) for t in row) for row in ids]

    batch = dict(name=["P1", "P2", "P3"], input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.from_numpy(g["attention_mask"]),
                 protein_input_ids=torch.from_numpy(g["protein_input_ids"]), protein_attention_mask=torch.from_numpy(g["protein_attention_mask"]),
                 description_input_ids=torch.tensor([[7], [9], [1]]))
    recs = []
    for cache in (None, "ancestry"):
        args = dict(max_generation_length=7, num_beams=3, length_penalty=0.8, do_sample=False, save_generation_dir=str(tmp_path),
                    save_generation_postfix_identifier=str(cache), beam_select="device", beam_cache=cache)
        recs.append(json.load(open(P.inference_epoch(0, model, [batch], Tok(), args))))
    assert recs[0] == recs[1] and len(recs[0]) == 3 and all(len(r["pred"].split()) == 7 for r in recs[0].values())
