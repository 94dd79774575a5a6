"""`generate(..., repetition_penalty=, no_repeat_ngram_size=, min_new_tokens=, bad_words_ids=, suppress_tokens=)`: p2t_logits_process in
front of the greedy / sampled choice, inside the replayed step graph, on the tiny golden models of tests/test_gpu_generate.py (fixtures
imported from there).  Every greedy token is re-derived on the host from the returned raw logits and the tokens emitted so far with the
numpy restatement (tests/logits_process_reference.py), the returned scores are the restatement's bit for bit, and the fp32 models
reproduce the sequences of the REFERENCE model's `generate` with HF's processors on (tests/golden/generate_processors_tiny.npz,
make_golden_generate_processors.py)."""
import json
import os

import numpy as np
import pytest
import torch

import logits_process_reference as LR
from gpu_util import dev, to_np
from test_gpu_generate import HERE, _inputs, _model, g  # noqa: F401  (g: the module-scoped golden fixture)

pytestmark = pytest.mark.gpu
RP = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)


def _gen(model, g, n, inputs=None, **kw):
    return model.generate(**(inputs or _inputs(g)), max_new_tokens=n, pad_token_id=g["meta"]["pad_id"], **{"eos_token_id": None, **kw})


@pytest.fixture(scope="module")
def gp():
    z = np.load(os.path.join(HERE, "golden", "generate_processors_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_greedy_tokens_and_scores_equal_the_restatement(g, dt):
    """(a)"""
    model = _model(g, "d64", dt)
    n = 14
    o = _gen(model, g, n, **RP, return_dict_in_generate=True, output_logits=True, output_scores=True)
    ids = to_np(o.sequences)
    assert ids.shape == (3, n) and len(o.logits) == len(o.scores) == n
    for s, (lg, sc) in enumerate(zip(o.logits, o.scores)):
        lg, sc = to_np(lg), to_np(sc)
        assert sc.dtype == np.float32 and sc.shape == lg.shape == (3, 512)
        want = LR.process(lg, [ids[r, :s] for r in range(3)], penalty=1.3, ngram=2)
        assert np.array_equal(sc.view(np.uint32), want.view(np.uint32)), s
        assert [LR.argmax_first(want[r]) for r in range(3)] == ids[:, s].tolist(), s
    assert not np.array_equal(ids, to_np(_gen(model, g, n)))                     # the processors changed the decode
    only = _gen(model, g, n, **RP, return_dict_in_generate=True, output_scores=True)
    assert only.logits is None and all(torch.equal(a, b) for a, b in zip(only.scores, o.scores))


def test_properties(g):
    """(b)"""
    model = _model(g, "d64", torch.float32)
    n, pad = 14, g["meta"]["pad_id"]
    plain = to_np(_gen(model, g, n))
    ids = to_np(_gen(model, g, n, no_repeat_ngram_size=2))
    for r in range(3):
        pairs = list(zip(ids[r, :-1].tolist(), ids[r, 1:].tolist()))
        assert len(set(pairs)) == len(pairs), r
    eos = int(plain[0, 1])
    short = to_np(_gen(model, g, n, eos_token_id=eos))
    assert short[0, 1] == eos and (short[0, 2:] == pad).all()                    # without min_new_tokens row 0 stops after two tokens
    ids = to_np(_gen(model, g, n, eos_token_id=eos, min_new_tokens=4))
    assert ids.shape[1] >= 4 and not (ids[:, :4] == eos).any()
    sup = [int(plain[0, 0]), int(plain[2, 3])]
    ids = to_np(_gen(model, g, n, suppress_tokens=sup))
    assert not np.isin(ids, sup).any() and np.isin(plain, sup).any()
    a, b = int(plain[0, 2]), int(plain[0, 3])
    ids = to_np(_gen(model, g, n, bad_words_ids=[[a, b]]))
    assert np.array_equal(ids[0, :3], plain[0, :3]) and ids[0, 3] != b
    assert not ((ids[:, :-1] == a) & (ids[:, 1:] == b)).any()


def test_graph_replay_equals_the_eager_loop(g):
    """(c)"""
    model = _model(g, "d64", torch.float32)
    full = dict(RP, min_new_tokens=5, suppress_tokens=[3], bad_words_ids=[[7, 9], [11]])
    eos = int(to_np(_gen(model, g, 3))[1, 2])
    for kw in (dict(), dict(do_sample=True, temperature=0.8, top_k=5, top_p=0.9, seed=3)):
        for args in (RP, dict(full, eos_token_id=eos)):
            a = _gen(model, g, 14, **args, **kw, use_graph=True, sync_every=4)
            b = _gen(model, g, 14, **args, **kw, use_graph=False, sync_every=4)
            assert torch.equal(a, b) and a.shape[1] >= 5, (kw, args)


def test_seeded_sampling_and_the_torch_path(g):
    """(d), (e)"""
    model = _model(g, "d64", torch.float32)
    n = 10
    greedy = _gen(model, g, n, **RP)
    seeded = _gen(model, g, n, **RP, do_sample=True, top_k=1, seed=5)
    assert torch.equal(seeded, greedy)
    o = _gen(model, g, n, **RP, do_sample=True, top_k=1, seed=5, return_dict_in_generate=True, output_scores=True, output_logits=True)
    ids = to_np(o.sequences)
    for s, (lg, sc) in enumerate(zip(o.logits, o.scores)):                        # the processed AND warped scores: one finite column
        want = LR.process(to_np(lg), [ids[r, :s] for r in range(3)], penalty=1.3, ngram=2)
        sc = to_np(sc)
        for r in range(3):
            assert np.isfinite(sc[r]).sum() == 1 and sc[r, ids[r, s]] == want[r, ids[r, s]], (s, r)
    full = _inputs(g)
    for r in range(3):                                                            # a prompt alone draws and decodes as it does in the batch
        one = {k: v[r:r + 1] for k, v in full.items()}
        alone = _gen(model, g, n, inputs=one, **RP, do_sample=True, top_k=1, seed=5)
        assert torch.equal(alone[0], seeded[r]), r
    gen = torch.Generator(device=dev())
    assert torch.equal(_gen(model, g, n, **RP, do_sample=True, top_k=1, generator=gen.manual_seed(1)), seeded)


def test_off_values_are_plain_greedy(g):
    """(f)"""
    model = _model(g, "d64", torch.float32)
    ids = _gen(model, g, 14, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
    assert np.array_equal(to_np(ids), g["d64.greedy"])
    ids = _gen(model, g, 14, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=3, bad_words_ids=None, suppress_tokens=None)
    assert np.array_equal(to_np(ids), g["d64.greedy"])                            # min_new_tokens without an eos id: not installed


def test_refusals(g):
    """(g)"""
    model = _model(g, "d16", torch.float32)
    with pytest.raises(NotImplementedError, match="num_beams"):
        _gen(model, g, 2, num_beams=2, repetition_penalty=1.2)
    with pytest.raises(ValueError, match="penalty"):
        _gen(model, g, 2, repetition_penalty=0)
    with pytest.raises(ValueError, match="ngram_size"):
        _gen(model, g, 2, no_repeat_ngram_size=-1)
    with pytest.raises(ValueError, match="min_new_tokens"):
        _gen(model, g, 2, min_new_tokens=-1)
    for bad in ([], [[]], [3], [[-1]], [[512]]):
        with pytest.raises(ValueError):
            _gen(model, g, 2, bad_words_ids=bad)
    with pytest.raises(ValueError, match="penalty"):                              # checked before the beam refusal
        _gen(model, g, 2, num_beams=2, repetition_penalty=-1.0)
    with pytest.raises(NotImplementedError, match="min_length"):
        _gen(model, g, 2, min_length=3)
    assert to_np(_gen(model, g, 2, num_beams=2, repetition_penalty=1.0, eos_token_id=g["meta"]["cases"]["d16"]["eos"])).shape[0] == 3


@pytest.mark.parametrize("case", ["d16", "d64", "d128", "qwen3"])
def test_fp32_reproduces_the_reference_generate_with_hf_processors(g, gp, case):
    """(h)"""
    model = _model(g, case, torch.float32)
    sets = gp["meta"]["sets"][case]
    assert sets
    for name, args in sets.items():
        want = gp[f"{case}.{name}"]
        for use_graph in (True, False):
            got = to_np(_gen(model, g, g["meta"]["max_new_tokens"], **args, use_graph=use_graph))
            assert np.array_equal(got, want), (case, name, use_graph)
