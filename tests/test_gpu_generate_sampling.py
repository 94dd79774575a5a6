"""`generate(..., do_sample=True, seed=)`: the device sampler (p2t_sample_select) in the greedy choice's place, inside the replayed step
graph, on the tiny golden models of tests/test_gpu_generate.py (fixtures imported from there).  Row b * R + r at step n draws
synth.sample_uniform(seed, row, n): every sampled id is re-derived on the host from the returned logits with the fp64 restatement
(tests/sampling_reference.py), the processed scores are HF's own warpers applied to those logits, and the torch path (`generator=`)
stays what it was."""
import numpy as np
import pytest
import torch

import sampling_reference as SR
from gpu_util import dev, to_np
from p2t_hip import synth
from test_gpu_generate import _inputs, _model, g  # noqa: F401  (g: the module-scoped golden fixture)

pytestmark = pytest.mark.gpu
KW = dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9)


def _gen(model, g, n, **kw):
    return model.generate(**_inputs(g), max_new_tokens=n, pad_token_id=g["meta"]["pad_id"], **{"eos_token_id": None, **kw})


def _rederive(out, seed, temperature, top_k, top_p):
    """Every (step, row) of a run with output_logits: asserted decidable, then the restatement's token for the host's own u."""
    ids = to_np(out.sequences)
    for n, lg in enumerate(out.logits):
        lg = to_np(lg)
        for r in range(ids.shape[0]):
            ref = SR.sample_row(lg[r], temperature, top_k, top_p, synth.sample_uniform(seed, r, n))
            assert ref["decidable"], (n, r, ref["m_p"], ref["m_u"])
            assert ids[r, n] == ref["token"], (n, r)


@pytest.mark.parametrize("case,dt", [("d64", torch.float32), ("d16", torch.float32), ("d64", torch.bfloat16)])
def test_seeded_ids_replay_the_graph_and_match_the_restatement(g, case, dt):
    model = _model(g, case, dt)
    n = 12
    a = _gen(model, g, n, **KW, seed=3, return_dict_in_generate=True, output_logits=True)
    b = _gen(model, g, n, **KW, seed=3)
    c = _gen(model, g, n, **KW, seed=4)
    assert a.sequences.shape == (3, n) and torch.equal(a.sequences, b) and not torch.equal(b, c)
    # steps 2 .. 11 of `b` were replays of one captured graph: the device step counter is the draw's counter, so they are fresh draws
    # and the same ones the eager loop makes
    eager = _gen(model, g, n, **KW, seed=3, use_graph=False)
    assert torch.equal(b, eager)
    assert len({tuple(r) for r in to_np(b).T.tolist()}) > 2                  # not one draw repeated along the sequence
    _rederive(a, 3, 0.7, 5, 0.9)
    # a large seed, top_k alone, and no filter at all
    big = 2 ** 63 + 12345
    o = _gen(model, g, 6, do_sample=True, temperature=1.5, top_k=50, top_p=1.0, seed=big, return_dict_in_generate=True, output_logits=True)
    _rederive(o, big, 1.5, 50, 1.0)
    o = _gen(model, g, 6, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, seed=5, return_dict_in_generate=True, output_logits=True)
    ids = to_np(o.sequences)
    V = model.llama_decoder.spec.vocab_size
    assert ids.shape == (3, 6) and ((ids >= 0) & (ids < V)).all()
    for n_, lg in enumerate(o.logits):
        for r in range(3):
            ref = SR.sample_row(to_np(lg)[r], 1.0, 0, 1.0, synth.sample_uniform(5, r, n_))
            assert not ref["decidable"] or ids[r, n_] == ref["token"], (n_, r)


def test_top_k_1_is_greedy_and_rows_of_a_prompt_draw_on_their_own(g):
    model = _model(g, "d64", torch.float32)
    for seed in (0, 9):
        d = _gen(model, g, 6, do_sample=True, top_k=1, seed=seed)
        assert np.array_equal(to_np(d), g["d64.greedy"][:, :6])
    r3 = _gen(model, g, 6, do_sample=True, top_k=1, num_return_sequences=3, seed=1)
    assert np.array_equal(to_np(r3), np.repeat(g["d64.greedy"][:, :6], 3, axis=0))
    s3 = _gen(model, g, 8, **KW, num_return_sequences=3, seed=5, return_dict_in_generate=True, output_logits=True)
    ids = to_np(s3.sequences)
    assert ids.shape == (9, 8)
    for b in range(3):                                                       # the three samples of a prompt: rows 3 b .. 3 b + 2, each its own draw
        assert len({tuple(ids[3 * b + r]) for r in range(3)}) > 1
    assert torch.equal(s3.sequences, _gen(model, g, 8, **KW, num_return_sequences=3, seed=5))
    _rederive(s3, 5, 0.7, 5, 0.9)                                            # row index b * 3 + r


def test_eos_rows_pad_and_the_others_go_on(g):
    model = _model(g, "d64", torch.float32)
    pad, n = g["meta"]["pad_id"], 10
    base = to_np(_gen(model, g, n, **KW, seed=7))
    eos = int(base[0, 1])
    assert eos != pad
    want = base.copy()
    ends = []
    for r in range(3):
        hit = np.nonzero(base[r] == eos)[0]
        ends.append(int(hit[0]) + 1 if hit.size else n)
        want[r, ends[-1]:] = pad
    assert ends[0] == 2 or base[0, 0] == eos
    for use_graph in (True, False):
        got = to_np(_gen(model, g, n, **KW, seed=7, eos_token_id=eos, use_graph=use_graph, sync_every=4))
        assert np.array_equal(got, want[:, : max(ends)]), use_graph


def test_processed_scores_equal_hf_warpers_on_the_returned_logits(g):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    model = _model(g, "d64", torch.float32)
    out = _gen(model, g, 8, **KW, seed=11, return_dict_in_generate=True, output_scores=True, output_logits=True)
    assert len(out.scores) == len(out.logits) == 8
    for n, (sc, lg) in enumerate(zip(out.scores, out.logits)):
        lg = lg.cpu()
        assert sc.shape == lg.shape and sc.dtype == torch.float32
        for r in range(lg.shape[0]):                                         # HF's result is defined where no survivors tie and the cut is clear
            ref = SR.sample_row(lg[r].numpy(), 0.7, 5, 0.9, 0.5)
            assert ref["ties_at_kth"] == 1 and ref["m_p"] > SR.delta(ref["n_survivors"]), (n, r)
        hf = TopPLogitsWarper(0.9)(None, TopKLogitsWarper(5)(None, TemperatureLogitsWarper(0.7)(None, lg)))
        assert torch.equal(sc.cpu(), hf), n                                  # kept values bit for bit, -inf elsewhere
    only = _gen(model, g, 8, **KW, seed=11, return_dict_in_generate=True, output_scores=True)
    assert only.logits is None and all(torch.equal(a, b) for a, b in zip(only.scores, out.scores))


def test_refusals_and_the_torch_path(g):
    model = _model(g, "d16", torch.float32)
    gen = torch.Generator(device=dev())
    with pytest.raises(ValueError, match="generator"):
        _gen(model, g, 2, **KW, seed=1, generator=gen)
    with pytest.raises(ValueError, match="top_k 1 .. 1024"):
        _gen(model, g, 2, do_sample=True, top_k=1025, seed=1)
    with pytest.raises(ValueError, match="top_k 1 .. 1024"):
        _gen(model, g, 2, do_sample=True, top_k=0, top_p=0.9, seed=1)
    with pytest.raises(ValueError, match="top_k 1 .. 1024"):
        _gen(model, g, 2, do_sample=True, top_k=None, top_p=0.5, seed=1)
    with pytest.raises(ValueError, match="temperature"):
        _gen(model, g, 2, do_sample=True, temperature=0.0, seed=1)
    with pytest.raises(NotImplementedError):
        _gen(model, g, 2, do_sample=True, num_beams=2, seed=1)
    with pytest.raises(NotImplementedError):                                 # without `seed` nothing pins the processed scores: still refused
        _gen(model, g, 2, **KW, return_dict_in_generate=True, output_scores=True)
    # seed under greedy decoding is ignored, as HF ignores sampling arguments there
    assert np.array_equal(to_np(_gen(model, g, 6, do_sample=False, seed=5, top_k=0, top_p=0.5)), g["d16.greedy"][:, :6])
    # seed=None: torch's generator stream, reproducible as before, never a graph, and not the device stream
    a = _gen(model, g, 6, **KW, generator=gen.manual_seed(3))
    b = _gen(model, g, 6, **KW, generator=gen.manual_seed(3))
    c = _gen(model, g, 6, **KW, generator=gen.manual_seed(4))
    assert torch.equal(a, b) and a.shape == (3, 6) and not torch.equal(a, c)
    o = _gen(model, g, 4, **KW, generator=gen.manual_seed(3), return_dict_in_generate=True, output_logits=True)
    for n, lg in enumerate(o.logits):                                        # the torch path's ids stay inside HF's filter of its own logits
        kept = torch.isfinite(__import__("p2t_hip").generation.filter_logits(lg, 0.7, 5, 0.9))
        assert kept[torch.arange(3), o.sequences[:, n]].all()


def test_inference_epoch_passes_a_seed_per_rank_and_batch(g, tmp_path):
    import p2t_hip as P
    from p2t_hip.loop import generation_seed
    model = _model(g, "d64", torch.float32)
    meta = g["meta"]
    pad = meta["pad_id"]

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=False):
            return [" ".join(str(int(t)) for t in row) for row in ids]

    batch = dict(name=["P1", "P2", "P3"], input_ids=torch.from_numpy(g["input_ids"]), attention_mask=torch.from_numpy(g["attention_mask"]),
                 protein_input_ids=torch.from_numpy(g["protein_input_ids"]), protein_attention_mask=torch.from_numpy(g["protein_attention_mask"]),
                 description_input_ids=torch.tensor([[7], [9], [1]]))
    batch2 = dict(batch, name=["Q1", "Q2", "Q3"])
    args = dict(max_generation_length=6, num_beams=1, temperature=0.7, do_sample=True, top_p=0.9, top_k=5, seed=42, save_generation_dir=str(tmp_path),
                save_generation_postfix_identifier="s")
    import json
    rec = json.load(open(P.inference_epoch(0, model, [batch, batch2], Tok(), args)))
    # upstream's loop hard-codes the Llama-3 eos / pad ids, which this 512-token fixture never emits: all 6 tokens are kept
    for names, i in ((("P1", "P2", "P3"), 0), (("Q1", "Q2", "Q3"), 1)):
        want = to_np(_gen(model, g, 6, **KW, seed=generation_seed(42, 0, i)))
        assert [rec[n]["pred"] for n in names] == [" ".join(str(int(t)) for t in row) for row in want]
    assert [rec[n]["pred"] for n in ("P1", "P2", "P3")] != [rec[n]["pred"] for n in ("Q1", "Q2", "Q3")]    # the same prompts, another stream
