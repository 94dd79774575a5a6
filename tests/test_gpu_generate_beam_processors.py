"""`generate(..., num_beams > 1, beam_select="device" | "torch", repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, bad_words_ids=,
suppress_tokens=)`: the logits processors under beam search, on the tiny golden models of tests/test_gpu_generate.py (fixtures imported
from there).  The device path (p2t_beam_logprobs_process + p2t_beam_select_logprobs inside the two-step graph) against the torch path
(p2t_logits_process on torch's log-softmax), graph replay against the eager loop bit for bit, the returned scores against the numpy
restatement bit for bit, the properties on the returned hypotheses, the off values, bf16, the refusals, and the fp32 models against the
REFERENCE model's own `generate` with HF's processors on under beam search (tests/golden/generate_beam_processors_tiny.npz,
make_golden_generate_beam_processors.py)."""
import json
import os

import numpy as np
import pytest
import torch

import logits_process_reference as LR
from gpu_util import to_np
from p2t_hip import generation as G
from test_gpu_beam_process import _lp0
from test_gpu_generate import CASES, HERE, _inputs, _model, g  # noqa: F401  (g: the module-scoped golden fixture)

pytestmark = pytest.mark.gpu
RP = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
FULL = dict(RP, min_new_tokens=5, suppress_tokens=[3], bad_words_ids=[[7, 9], [11]])
NEW = ("p2t_beam_logprobs_process", "p2t_beam_select_logprobs")


def _gen(model, g, n, **kw):
    return model.generate(**_inputs(g), max_new_tokens=n, pad_token_id=g["meta"]["pad_id"], do_sample=False,
                          **{"eos_token_id": None, "return_dict_in_generate": True, "output_scores": True, "num_beams": 3, **kw})


@pytest.fixture(scope="module")
def gb():
    z = np.load(os.path.join(HERE, "golden", "generate_beam_processors_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


def _lengths(o):
    return (to_np(o.beam_indices) >= 0).sum(axis=1)


@pytest.mark.parametrize("which", ["rp", "all"])
def test_device_equals_torch_and_graph_equals_eager(g, which):
    model = _model(g, "d64", torch.float32)
    args = RP if which == "rp" else dict(FULL, eos_token_id=g["meta"]["cases"]["d64"]["eos"])
    plain = _gen(model, g, 10, beam_select="device", eos_token_id=args.get("eos_token_id"))
    for n in (9, 10):                                         # the two-step graph with and without an eager remainder
        for sync_every in (1, 16):
            a = _gen(model, g, n, beam_select="device", sync_every=sync_every, num_return_sequences=3, **args)
            b = _gen(model, g, n, beam_select="device", sync_every=sync_every, num_return_sequences=3, use_graph=False, **args)
            assert torch.equal(a.sequences, b.sequences) and torch.equal(a.beam_indices, b.beam_indices), (which, n, sync_every)
            assert torch.equal(a.sequences_scores, b.sequences_scores), (which, n, sync_every)
            assert len(a.scores) == len(b.scores) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
        t = _gen(model, g, n, beam_select="torch", num_return_sequences=3, **args)
        assert torch.equal(a.sequences, t.sequences) and torch.equal(a.beam_indices, t.beam_indices), (which, n)
        d = (a.sequences_scores - t.sequences_scores).abs().max().item()
        print(f"{which} n = {n}: device vs torch, largest sequences_scores difference {d:.3g}")
        assert d < 1e-4
        assert len(a.scores) == len(t.scores)
    one = _gen(model, g, 10, beam_select="device", **args)
    assert not torch.equal(one.sequences, plain.sequences)    # the processors changed the search


def test_returned_scores_are_the_processed_rows_and_the_hypotheses_obey_the_processors(g):
    model = _model(g, "d64", torch.float32)
    eos, n, nb, V = g["meta"]["cases"]["d64"]["eos"], 10, 3, 512
    args = dict(FULL, eos_token_id=eos)
    o = _gen(model, g, n, beam_select="device", num_return_sequences=3, output_logits=True, **args)
    seq, idx, lens = to_np(o.sequences), to_np(o.beam_indices), _lengths(o)
    assert len(o.scores) == len(o.logits) >= lens.max() and o.scores[0].shape == (9, V) and o.scores[0].dtype == torch.float32
    words = LR.words_of(FULL["bad_words_ids"], FULL["suppress_tokens"], [eos])
    kw = dict(penalty=1.3, ngram=2, min_new=5, eos_ids=[eos], words=words)
    checked = changed = 0
    for s in range(int(lens.max())):
        lg = o.logits[s].contiguous()
        lp0 = _lp0(lg, V, 3, nb)                              # the log-softmax of the returned raw rows, in p2t_beam_select's summation order
        assert (torch.from_numpy(lp0).to(lg.device) - torch.log_softmax(lg, -1)).abs().max() < 1e-5
        sc = to_np(o.scores[s])
        for h in range(seq.shape[0]):
            if s >= lens[h]:
                continue
            row = int(idx[h, s])                              # the row this hypothesis' token s was continued from; its history: the tokens before
            assert h // nb * nb <= row < (h // nb + 1) * nb
            want = LR.process_row(lp0[row], seq[h, :s], **kw)
            assert np.array_equal(sc[row].view(np.uint32), want.view(np.uint32)), (s, h)
            assert np.isfinite(want[seq[h, s]])               # the token that was chosen is not a banned one
            checked += 1
            changed += int((want.view(np.uint32) != lp0[row].view(np.uint32)).sum())
    assert checked >= 30 and changed > 0
    for h in range(seq.shape[0]):                             # the properties, on every returned hypothesis
        t = seq[h, : lens[h]].tolist()
        pairs = list(zip(t[:-1], t[1:]))
        assert len(set(pairs)) == len(pairs), h               # no repeated 2-gram
        assert (7, 9) not in pairs and 11 not in t and 3 not in t, h
        assert eos not in t[:5], h
    only = _gen(model, g, n, beam_select="device", num_return_sequences=3, **args)
    assert only.logits is None and all(torch.equal(x, y) for x, y in zip(only.scores, o.scores))
    hidden = _gen(model, g, n, beam_select="device", num_return_sequences=3, output_scores=False, **args)      # one buffer for both steps
    assert hidden.scores is None and torch.equal(hidden.sequences, o.sequences) and torch.equal(hidden.beam_indices, o.beam_indices)


def test_off_values_are_the_plain_beam_search_and_launch_nothing_new(g, monkeypatch):
    model = _model(g, "d64", torch.float32)
    calls = []
    real = G.call
    monkeypatch.setattr(G, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    eos = g["meta"]["cases"]["d64"]["eos"]
    plain = _gen(model, g, 9, beam_select="device", eos_token_id=eos)
    off = _gen(model, g, 9, beam_select="device", eos_token_id=eos, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0,
               bad_words_ids=None, suppress_tokens=None)
    assert torch.equal(off.sequences, plain.sequences) and torch.equal(off.sequences_scores, plain.sequences_scores)
    assert "p2t_beam_select" in calls and not any(c in calls for c in NEW)
    none = _gen(model, g, 9, eos_token_id=None, min_new_tokens=3)                      # min_new_tokens without an eos id: not installed
    assert torch.equal(none.sequences, _gen(model, g, 9).sequences) and not any(c in calls for c in NEW)
    _gen(model, g, 9, beam_select="device", eos_token_id=eos, **RP)
    assert all(c in calls for c in NEW)


def test_bf16_device_path_scores_like_the_torch_path(g):
    model = _model(g, "d64", torch.bfloat16)
    eos, n = g["meta"]["cases"]["d64"]["eos"], 12
    kw = dict(FULL, eos_token_id=eos, length_penalty=1.0)
    a = _gen(model, g, n, beam_select="device", **kw)
    b = _gen(model, g, n, beam_select="device", use_graph=False, **kw)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores, b.sequences_scores)
    t = _gen(model, g, n, beam_select="torch", **kw)
    diff = np.abs(to_np(a.sequences_scores) - to_np(t.sequences_scores))
    print("bf16 device vs torch score differences", diff)
    assert np.isfinite(diff).all() and np.median(diff) < 5e-2 and diff.max() < 0.3, diff     # bf16 logits: near-tied beams may swap


def test_refusals(g):
    model = _model(g, "d16", torch.float32)
    with pytest.raises(NotImplementedError, match="num_beams.*beam_select='device'"):
        _gen(model, g, 3, **RP)
    with pytest.raises(NotImplementedError, match="beam sampling"):
        model.generate(**_inputs(g), max_new_tokens=3, num_beams=3, do_sample=True, seed=1, beam_select="device", **RP)
    with pytest.raises(ValueError, match="beam_select='device'"):
        _gen(model, g, 3, num_beams=17, beam_select="device", **RP)
    with pytest.raises(ValueError, match="penalty"):                                    # the argument checks still run first
        _gen(model, g, 3, beam_select="device", repetition_penalty=-1.0)
    wide = _gen(model, g, 3, num_beams=17, beam_select="torch", **RP)                    # the torch path serves what the kernels do not
    assert wide.sequences.shape == (3, 3)


@pytest.mark.parametrize("case", CASES)
def test_fp32_reproduces_the_reference_beam_search_with_hf_processors(g, gb, case):
    model = _model(g, case, torch.float32)
    sets = gb["meta"]["sets"][case]
    assert sets
    for name, args in sets.items():
        want, want_sc = gb[f"{case}.{name}"], gb[f"{case}.{name}_scores"]
        for kw in (dict(beam_select="device"), dict(beam_select="device", use_graph=False), dict(beam_select="torch")):
            out = _gen(model, g, g["meta"]["max_new_tokens"], num_return_sequences=3, **args, **kw)
            assert np.array_equal(to_np(out.sequences), want), (case, name, kw)
            d = np.abs(to_np(out.sequences_scores) - want_sc).max()
            print(f"{case}.{name} {kw}: largest sequences_scores difference to the reference {d:.3g}")
            assert d < 1e-4, (case, name, kw)
