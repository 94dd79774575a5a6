"""`generate(..., num_beams > 1, beam_select=)`: p2t_beam_select in the torch bookkeeping's place, eagerly and under replay of the
two-step graph, on the tiny golden models of tests/test_gpu_generate.py (fixtures imported from there): the goldens of the reference's
own beam search, graph against eager against the torch path, a stop between two host reads, odd and even lengths, a 70-token run
against the oracle, the per-step outputs against the fp64 restatement (tests/beam_reference.py), the range limits, bf16, and
`inference_epoch`."""
import json

import numpy as np
import pytest
import torch

import beam_reference as BR
from gpu_util import to_dev, to_np
from helpers import model_weights
from oracle import p2t_oracle as O
from p2t_hip import specs
from test_gpu_generate import CASES, _inputs, _model, g  # noqa: F401  (g: the module-scoped golden fixture)

pytestmark = pytest.mark.gpu


def _gen(model, g, n, **kw):
    return model.generate(**_inputs(g), max_new_tokens=n, pad_token_id=g["meta"]["pad_id"], do_sample=False,
                          **{"eos_token_id": None, "return_dict_in_generate": True, "output_scores": True, **kw})


def _same(a, b, what, scores_exact=True):
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.beam_indices, b.beam_indices), what
    if scores_exact:
        assert torch.equal(a.sequences_scores, b.sequences_scores), what
    else:                                                   # another log-softmax: inside the bound of the formula's f32 error over the run
        sa, sb = to_np(a.sequences_scores).astype(np.float64), to_np(b.sequences_scores).astype(np.float64)
        V, steps = a.scores[0].shape[1], len(a.scores)
        tol = np.array([min(2 * BR.score_delta(V, s, steps), 1e-4) for s in sa])           # and never above the goldens' own bound
        print(f"{what}: largest score difference {np.abs(sa - sb).max():.3g} (bound {tol.min():.3g})")
        assert (np.abs(sa - sb) <= tol).all(), (what, sa, sb)


def _three_ways(model, g, n, what, **kw):
    """-> the replayed run, after comparing it with the eager device run (bit for bit) and with the torch path."""
    a = _gen(model, g, n, beam_select="device", **kw)
    _same(a, _gen(model, g, n, beam_select="device", use_graph=False, **kw), (what, "graph vs eager"))
    t = _gen(model, g, n, beam_select="torch", **kw)
    _same(a, t, (what, "device vs torch"), scores_exact=False)
    assert len(a.scores) == len(t.scores)
    return a


@pytest.mark.parametrize("case", CASES)
def test_fp32_device_beam_search_vs_reference_generate(g, case):
    model = _model(g, case, torch.float32)
    meta = g["meta"]
    n = meta["max_new_tokens"]
    for lp in ("1.0", "0.5"):
        out = _three_ways(model, g, n, (case, lp), eos_token_id=meta["cases"][case]["eos"], num_beams=3, length_penalty=float(lp))
        assert np.array_equal(to_np(out.sequences), g[f"{case}.beam3_lp{lp}"]), lp
        assert np.abs(to_np(out.sequences_scores) - g[f"{case}.beam3_lp{lp}_scores"]).max() < 1e-4, lp
    for es in (True, "never"):                              # two eos ids, two hypotheses per prompt
        out = _three_ways(model, g, n, (case, es), eos_token_id=meta["cases"][case]["eos2"], num_beams=3, length_penalty=0.8, early_stopping=es,
                          num_return_sequences=2)
        assert out.sequences.shape[0] == 6
        assert np.array_equal(to_np(out.sequences), g[f"{case}.beam3_es{es}"]), es
        assert np.abs(to_np(out.sequences_scores) - g[f"{case}.beam3_es{es}_scores"]).max() < 1e-4, es
    plain = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=meta["cases"][case]["eos"], pad_token_id=meta["pad_id"], num_beams=3)
    assert np.array_equal(to_np(plain), g[f"{case}.beam3_lp1.0"])          # the default takes the device path and returns the ids alone


def test_a_stop_between_two_host_reads_and_odd_and_even_lengths(g):
    model = _model(g, "d64", torch.float32)
    free = _gen(model, g, 6, beam_select="device", num_beams=3, output_logits=True)
    # the 20 likeliest tokens of step 2 as eos ids (keep = 21 * 3 = 63): hypotheses finish at once and early_stopping=True ends the search
    eos = [int(t) for t in torch.topk(torch.log_softmax(free.logits[2], -1).mean(0), 20)[1]]
    kw = dict(num_beams=3, eos_token_id=eos, early_stopping=True, length_penalty=1.0)
    n = 14
    one = _gen(model, g, n, beam_select="device", sync_every=1, **kw)
    steps = len(one.scores)
    print("the search stopped after", steps, "of", n, "steps")
    assert 2 <= steps < n - 1                               # it stops before the end: the replayed steps after it must change nothing
    for use_graph in (True, False):
        for sync_every in (4, 5, 16):                       # reads at other steps than the stop: the steps in between change nothing
            _same(one, _gen(model, g, n, beam_select="device", sync_every=sync_every, use_graph=use_graph, **kw), (use_graph, sync_every))
    _same(one, _gen(model, g, n, beam_select="torch", **kw), "torch", scores_exact=False)
    for n in (7, 8, 2, 1):                                  # the two-step graph's remainder; 1 and 2 never reach the graph
        out = _three_ways(model, g, n, n, num_beams=3, length_penalty=1.0)
        assert out.sequences.shape == (3, n) and len(out.scores) == n


def test_long_device_beam_search_vs_the_oracle(g):
    """3 beams x 70 new tokens: the re-ordered cache segment grows past one 64-key tile while the graph replays pairs of steps."""
    case = "d64"
    model = _model(g, case, torch.float32)
    meta = g["meta"]
    m = meta["cases"][case]
    n, pad = 70, meta["pad_id"]
    out = _gen(model, g, n, beam_select="device", eos_token_id=m["eos"], num_beams=3, length_penalty=1.0)
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    W = model_weights(esm, llama, ad, m["weight_seed"], lm_head=True)
    emb, mask = model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                      protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)
    seq, sc = O.generate_beam(llama, W, to_np(emb), to_np(mask), n, 3, (m["eos"],), pad, 1.0)
    assert np.array_equal(to_np(out.sequences), seq) and seq.shape[1] > 64
    assert np.abs(to_np(out.sequences_scores) - sc).max() < 1e-4


def _rederive(out, nb, eos_ids, lp, es, L, pad, R=1):
    """The restatement chained over the run's own logits.  -> (prompts whose every step was decidable, the restatement's final state)."""
    B = out.logits[0].shape[0] // nb
    st, ok = BR.fresh_state(B, nb, L, pad), np.ones(B, dtype=bool)
    for cur, lg in enumerate(out.logits):
        ref = BR.step(to_np(lg), st, cur, nb, eos_ids, lp, es, L, pad)
        lp_gpu = to_np(out.scores[cur]).astype(np.float64)
        assert (np.abs(lp_gpu - ref["log_probs"]) <= ref["lp_err"][:, None]).all(), cur          # HF's per-step scores: the log-probabilities
        ok &= ref["decidable"] & (ref["running_decidable"] | ref["state"]["done"])
        st = ref["state"]
    return ok, st


def test_per_step_outputs_are_the_log_probabilities_of_the_returned_logits(g):
    model = _model(g, "d64", torch.float32)
    meta = g["meta"]
    eos, pad, n = meta["cases"]["d64"]["eos2"], meta["pad_id"], 9
    kw = dict(num_beams=3, eos_token_id=eos, length_penalty=0.8, output_logits=True, beam_select="device")
    a, b = _gen(model, g, n, **kw), _gen(model, g, n, use_graph=False, **kw)
    assert 1 <= len(a.scores) == len(a.logits) == len(b.scores) <= n and a.scores[0].shape == (9, 512) and a.scores[0].dtype == torch.float32
    for x, y in zip(a.scores + a.logits, b.scores + b.logits):
        assert torch.equal(x, y)
    for lg, sc in zip(a.logits, a.scores):
        assert (sc - torch.log_softmax(lg, -1)).abs().max() < 1e-5
    ok, st = _rederive(a, 3, eos, 0.8, False, n, pad)
    assert ok.all()                                         # fp32, no ties: the ids follow from the returned logits alone
    assert np.array_equal(to_np(a.sequences), st["sequences"][:, 0, : a.sequences.shape[1]])
    assert np.array_equal(to_np(a.beam_indices), st["beam_idx"][:, 0, : a.sequences.shape[1]])
    only = _gen(model, g, n, **{**kw, "output_logits": False})
    assert only.logits is None and all(torch.equal(x, y) for x, y in zip(only.scores, a.scores))


def test_range_limits(g):
    model = _model(g, "d16", torch.float32)
    with pytest.raises(ValueError, match="beam_select='device'"):
        _gen(model, g, 3, num_beams=17, beam_select="device")
    with pytest.raises(ValueError, match="beam_select"):
        _gen(model, g, 3, num_beams=3, beam_select="gpu")
    wide = _gen(model, g, 3, num_beams=17)                  # the default falls back to the torch bookkeeping
    assert wide.sequences.shape == (3, 3)
    assert torch.equal(wide.sequences, _gen(model, g, 3, num_beams=17, beam_select="torch").sequences)
    with pytest.raises(NotImplementedError):
        model.generate(**_inputs(g), max_new_tokens=2, num_beams=2, do_sample=True, beam_select="device")
    sixteen = _three_ways(model, g, 4, 16, num_beams=16, num_return_sequences=16)              # the widest supported search
    assert sixteen.sequences.shape == (48, 4)


def test_bf16_device_path_scores_like_the_torch_path(g):
    model = _model(g, "d64", torch.bfloat16)
    meta = g["meta"]
    eos, pad, n = meta["cases"]["d64"]["eos"], meta["pad_id"], 12
    kw = dict(num_beams=3, eos_token_id=eos, length_penalty=1.0, output_logits=True)
    dev_out = _gen(model, g, n, beam_select="device", **kw)
    _same(dev_out, _gen(model, g, n, beam_select="device", use_graph=False, **kw), "bf16 graph vs eager")
    tor = _gen(model, g, n, beam_select="torch", **kw)
    diff = np.abs(to_np(dev_out.sequences_scores) - to_np(tor.sequences_scores))
    print("bf16 device vs torch score differences", diff)
    assert np.isfinite(diff).all() and np.median(diff) < 5e-2 and diff.max() < 0.3, diff     # bf16 logits: near-tied beams may swap
    ok, st = _rederive(dev_out, 3, [eos], 1.0, False, n, pad)
    print("bf16: prompts decidable at every step:", ok)
    for b in np.nonzero(ok)[0]:                             # ids only where the returned logits decide every step
        assert np.array_equal(to_np(dev_out.sequences)[b], st["sequences"][b, 0, : dev_out.sequences.shape[1]]), b


def test_inference_epoch_with_beams_writes_the_same_json_on_both_paths(g, tmp_path):
    import p2t_hip as P
    model = _model(g, "d64", torch.float32)

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=False):
            return [" ".join(str(int(t)) for t in row) for row in ids]

    batch = dict(name=["P1", "P2", "P3"], input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.from_numpy(g["attention_mask"]),
                 protein_input_ids=torch.from_numpy(g["protein_input_ids"]), protein_attention_mask=torch.from_numpy(g["protein_attention_mask"]),
                 description_input_ids=torch.tensor([[7], [9], [1]]))
    recs = []
    for sel in (None, "device", "torch"):
        args = dict(max_generation_length=7, num_beams=3, length_penalty=0.8, do_sample=False, save_generation_dir=str(tmp_path),
                    save_generation_postfix_identifier=str(sel), beam_select=sel)
        recs.append(json.load(open(P.inference_epoch(0, model, [batch], Tok(), args))))
    assert recs[0] == recs[1] == recs[2] and len(recs[0]) == 3 and all(len(r["pred"].split()) == 7 for r in recs[0].values())
