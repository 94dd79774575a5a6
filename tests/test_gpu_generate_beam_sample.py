"""`generate(num_beams > 1, do_sample=True, seed=, beam_select="device")`: p2t_beam_sample_select in the beam search's loop, eagerly and
under replay of the two-step graph, on the tiny golden models of tests/test_gpu_generate.py (fixtures imported from there): graph
against eager bit for bit, another seed, odd and even lengths, a stop between two host reads, every step re-derived on the host from the
returned logits with the fp64 restatement (tests/beam_sample_reference.py), two hypotheses per prompt, the up-front errors, the
refusals that stay, the torch path with a generator, and `inference_epoch`."""
import json
import warnings

import numpy as np
import pytest
import torch

import beam_sample_reference as R
from gpu_util import to_np
from test_gpu_generate import CASES, _inputs, _model, g  # noqa: F401  (g: the module-scoped golden fixture)

pytestmark = pytest.mark.gpu
WARP = dict(temperature=0.8, top_k=20, top_p=0.95)


def _gen(model, g, n, **kw):
    return model.generate(**_inputs(g), max_new_tokens=n, pad_token_id=g["meta"]["pad_id"], do_sample=True,
                          **{"eos_token_id": None, "return_dict_in_generate": True, "output_scores": True, "num_beams": 3, "seed": 3,
                             "beam_select": "device", **WARP, **kw})


def _same(a, b, what):
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.beam_indices, b.beam_indices), what
    assert torch.equal(a.sequences_scores, b.sequences_scores), what
    assert len(a.scores) == len(b.scores) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores)), what


@pytest.mark.parametrize("case,dtype", [("d16", torch.float32), ("d64", torch.float32), ("d64", torch.bfloat16)])
def test_graph_replay_equals_eager_and_another_seed_differs(g, case, dtype):
    model = _model(g, case, dtype)
    n, V = 12, 512
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # neither flag bit on these rows
        a = _gen(model, g, n)
        _same(a, _gen(model, g, n, use_graph=False), (case, dtype, "graph vs eager"))
        other = _gen(model, g, n, seed=4)
    assert a.sequences.shape == (3, n) and len(a.scores) == n and a.scores[0].shape == (9, V)
    assert ((a.sequences >= 0) & (a.sequences < V)).all() and torch.isfinite(a.sequences_scores).all()
    assert not torch.equal(a.sequences, other.sequences)
    for sc in a.scores:                                       # the processed scores: at least one kept per row, at most top_k (bf16: plus the ties at the k-th logit)
        kept = torch.isfinite(sc).sum(1)
        assert (kept >= 1).all() and (dtype == torch.bfloat16 or (kept <= WARP["top_k"]).all()) and not torch.isnan(sc).any()


def test_odd_and_even_lengths_and_a_stop_between_two_host_reads(g):
    model = _model(g, "d64", torch.float32)
    for n in (7, 8, 2, 1):                                    # the two-step graph's remainder; 1 and 2 never reach the graph
        out = _gen(model, g, n)
        _same(out, _gen(model, g, n, use_graph=False), n)
        assert out.sequences.shape == (3, n) and len(out.scores) == n
    free = _gen(model, g, 6, output_logits=True)
    # the 20 likeliest tokens of step 2 as eos ids (keep = 21 * 3 = 63): hypotheses finish at once and early_stopping=True ends the search
    eos = [int(t) for t in torch.topk(torch.log_softmax(free.logits[2], -1).mean(0), 20)[1]]
    kw = dict(eos_token_id=eos, early_stopping=True, length_penalty=1.0, temperature=1.0, top_k=100, top_p=1.0)
    n = 14
    one = _gen(model, g, n, sync_every=1, **kw)
    steps = len(one.scores)
    print("the search stopped after", steps, "of", n, "steps")
    assert 1 <= steps < n - 1                                 # it stops before the end: the replayed steps after it must change nothing
    for use_graph in (True, False):
        for sync_every in (4, 16):
            _same(one, _gen(model, g, n, sync_every=sync_every, use_graph=use_graph, **kw), (use_graph, sync_every))


def test_every_step_follows_from_the_returned_logits(g):
    model = _model(g, "d64", torch.float32)
    meta = g["meta"]
    eos, pad, n, nb = meta["cases"]["d64"]["eos2"], meta["pad_id"], 9, 3
    kw = dict(eos_token_id=eos, length_penalty=0.8, output_logits=True)
    a = _gen(model, g, n, **kw)
    assert 1 <= len(a.scores) == len(a.logits) <= n and a.scores[0].shape == (9, 512) and a.scores[0].dtype == torch.float32
    B = a.logits[0].shape[0] // nb
    st = R.fresh_state(B, nb, n, pad)
    drift, fin_err = 0.0, 0.0                                               # a running score's f32 error passes through every later addition one to one
    for cur, lg in enumerate(a.logits):
        ref = R.step(to_np(lg), st, cur, nb, eos, 0.8, False, n, pad, WARP["temperature"], WARP["top_k"], WARP["top_p"], 3, 0)
        print(f"step {cur}: margins {ref['margin']}")
        assert ref["decidable"].all() and not ref["flagged"].any(), (cur, ref["margin"])
        assert (ref["running_decidable"] | bool(ref["state"]["done"])).all(), cur
        sc = to_np(a.scores[cur]).astype(np.float64)
        cut = np.isinf(ref["scores"])
        assert np.array_equal(np.isneginf(sc), cut), cur
        assert (np.abs(sc[~cut] - ref["scores"][~cut]) <= ref["e_scores"][~cut]).all(), cur
        drift += float(ref["running_err"].max())
        fin_err = max(fin_err, float(ref["beam_err"].max()))
        st = ref["state"]
    assert st["done"] and st["steps"] == len(a.logits)
    L = a.sequences.shape[1]
    assert np.array_equal(to_np(a.sequences), st["sequences"][:, 0, :L]) and np.array_equal(to_np(a.beam_indices), st["beam_idx"][:, 0, :L])
    err = np.abs(to_np(a.sequences_scores).astype(np.float64) - st["beam_scores"][:, 0])
    bound = 2 * (drift + fin_err) + 2.0 ** -23 * np.abs(st["beam_scores"][:, 0])      # both chains keep their scores as f32 between steps
    print("final score errors", err, "bounds", bound)
    assert (err <= bound).all()
    only = _gen(model, g, n, **{**kw, "output_logits": False})
    assert only.logits is None and all(torch.equal(x, y) for x, y in zip(only.scores, a.scores))
    two = _gen(model, g, n, num_return_sequences=2, **kw)
    assert two.sequences.shape[0] == 6 and torch.equal(two.sequences[0::2], a.sequences) and torch.equal(two.sequences_scores[0::2], a.sequences_scores)
    assert (two.sequences_scores[0::2] >= two.sequences_scores[1::2]).all()
    ids = model.generate(**_inputs(g), max_new_tokens=n, pad_token_id=pad, do_sample=True, num_beams=3, seed=3, beam_select="device", **WARP, **kw)
    assert torch.equal(ids, a.sequences)                      # without return_dict_in_generate: the ids alone


def test_errors_up_front_and_the_refusals_that_stay(g):
    model = _model(g, "d16", torch.float32)
    for kw, msg in ((dict(top_k=1025), "1 .. 1024"), (dict(top_k=0, top_p=0.9), "1 .. 1024"), (dict(temperature=0.0), "temperature"),
                    (dict(top_k=5), "cannot supply"), (dict(generator=torch.Generator()), "not both"), (dict(num_beams=17, top_k=0, top_p=1.0), "beam_select='device'")):
        with pytest.raises(ValueError, match=msg):
            _gen(model, g, 3, **kw)
    plain = dict(**_inputs(g), max_new_tokens=2, num_beams=2, do_sample=True)
    for kw in (dict(), dict(beam_select="device"), dict(seed=1), dict(seed=1, beam_select="torch"), dict(generator=torch.Generator(), beam_select="device")):
        with pytest.raises(NotImplementedError, match="seed=.*beam_select='device'"):
            model.generate(**plain, **kw)


def test_the_torch_path_with_a_generator_runs(g):
    model = _model(g, "d16", torch.float32)
    gen = torch.Generator(device="cuda").manual_seed(1)
    out = _gen(model, g, 5, seed=None, generator=gen, beam_select="torch")
    assert out.sequences.shape == (3, 5) and ((out.sequences >= 0) & (out.sequences < 512)).all()
    assert len(out.scores) == 5 and out.scores[0].shape == (9, 512) and torch.isfinite(out.sequences_scores).all()


def test_inference_epoch_with_beam_sampling_writes_its_json(g, tmp_path):
    import p2t_hip as P
    model = _model(g, "d64", torch.float32)

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=False):
            return [" ".join(str(int(t)) for t in row) for row in ids]

    batch = dict(name=["P1", "P2", "P3"], input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.from_numpy(g["attention_mask"]),
                 protein_input_ids=torch.from_numpy(g["protein_input_ids"]), protein_attention_mask=torch.from_numpy(g["protein_attention_mask"]),
                 description_input_ids=torch.tensor([[7], [9], [1]]))
    recs = []
    for _ in range(2):
        args = dict(max_generation_length=7, num_beams=2, length_penalty=0.8, do_sample=True, seed=42, beam_select="device", top_k=50,
                    save_generation_dir=str(tmp_path), save_generation_postfix_identifier="bs")
        recs.append(json.load(open(P.inference_epoch(0, model, [batch], Tok(), args))))
    assert recs[0] == recs[1] and len(recs[0]) == 3 and all(len(r["pred"].split()) == 7 for r in recs[0].values())
