"""Continuous batching with `choice="device"` end to end (p2t_hip/continuous.py: seeded sampling, the logits processors and output_scores
per row) on the tiny golden models (fixtures imported from tests/test_gpu_generate.py / test_gpu_generate_continuous.py): against the
REFERENCE model's own `generate` with HF's processors (fp32, tests/golden/generate_processors_tiny.npz), against the numpy restatement
request by request (tests/continuous_choice_reference.py: every token re-derived from the request's returned logits, its own earlier
tokens, its key and its step), against `model.generate(seed=)` bit for bit where nothing is refilled (bf16), and against itself under
another order, another number of slots and through `inference_epoch`.

Decidability (tests/sampling_reference.py): a draw is compared with the restatement where both of its thresholds are further than the
f32 summation error from the fp64 value.  Where two RUNS are compared with each other -- their prefills are composed differently, so
their logits differ by up to the 2e-4 the fp32 tests allow -- every draw of the first run must keep a margin above 10 x 2e-4 of the
row's mass (MARGIN); the seed is the first of a short fixed list for which that holds, and the test says which comparison it made."""
import json

import numpy as np
import pytest
import torch

import continuous_choice_reference as ccr
import logits_process_reference as LR
from gpu_util import to_np
from test_gpu_generate import _model, g  # noqa: F401  (g: the module-scoped golden fixture)
from test_gpu_generate_continuous import LOGIT_TOL, _cut, _generator, _inputs
from test_gpu_generate_processors import gp  # noqa: F401

pytestmark = pytest.mark.gpu
RP = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
PROC = dict(penalty=1.3, ngram=2, min_new=0, words=[])
SAMPLE = dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.8)
MARGIN = 10 * LOGIT_TOL


def _run(gen, ids):
    """-> {request id: (tokens list, *the arrays that came with them)}; every id exactly once."""
    out = {}
    for item in gen.run():
        assert item[0] not in out
        out[item[0]] = (to_np(item[1]).tolist(),) + tuple(to_np(a) for a in item[2:])
    assert sorted(out) == sorted(ids)
    return out


def _rederive(lg, toks, key, seed, proc=PROC):
    return ccr.rederive(lg, toks, key, seed, SAMPLE["temperature"], SAMPLE["top_k"], SAMPLE["top_p"], proc=proc)


@pytest.mark.parametrize("sync_every", [1, 4])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", ["d16", "d64", "d128", "qwen3"])
def test_fp32_greedy_with_hf_processors_vs_the_reference_golden(g, gp, case, use_graph, sync_every):
    """The golden's 3 prompts through 2 slots with each argument set of generate_processors_tiny.npz (the reference model's own
    `generate` with HF's processors): its sequences, each cut after its eos.  Exact ids are a fair demand: the fixture kept only sets
    whose smallest top-2 gap of the PROCESSED scores is 5e-3, 25 x the logit tolerance."""
    assert gp["meta"]["min_top2_gap"] >= 10 * LOGIT_TOL
    model = _model(g, case, torch.float32)
    sets = gp["meta"]["sets"][case]
    assert sets
    for name, args in sets.items():
        gen = _generator(model, g, 2, choice="device", use_graph=use_graph, sync_every=sync_every, **args)
        ids = gen.submit(**_inputs(g))
        got = _run(gen, ids)
        eos = args.get("eos_token_id")
        for b, rid in enumerate(ids):
            want = gp[f"{case}.{name}"][b].tolist()
            assert got[rid][0] == (_cut(want, eos) if eos is not None else want), (case, name, b)
        assert (gen.decoder.engine().graph is not None) == use_graph


def test_seven_requests_with_refills_are_rederived_by_the_restatement(g):
    """d64, fp32, 2 slots, limits [3, 14, 1, 9, 14, 2, 5] (every slot is refilled), repetition penalty + bi-gram ban + seeded top-k /
    top-p sampling, logits and scores returned.  Request i's token t is the restatement's draw from ITS logits row t, processed with ITS
    tokens [: t], under key i and step t; its score row is the restatement's bit for bit.  The seed is fixed: at most 2 of the 48 draws
    may be undecidable (delta ~ 13 * 2^-23 around <= 5 thresholds: the expectation is << 1); those are only held to the kept set."""
    model = _model(g, "d64", torch.float32)
    seed, limits = 20240607, [3, 14, 1, 9, 14, 2, 5]
    rows = [i % 3 for i in range(7)]
    gen = _generator(model, g, 2, choice="device", sync_every=4, output_logits=True, output_scores=True, seed=seed, **RP, **SAMPLE)
    ids = gen.submit(**_inputs(g, rows), max_new_tokens=limits)
    got = _run(gen, ids)
    undecidable, draws = 0, 0
    for i, rid in enumerate(ids):
        toks, lg, sc = got[rid]
        assert len(toks) == limits[i] and lg.shape == sc.shape == (limits[i], 512) and sc.dtype == np.float32
        for t, ref in enumerate(_rederive(lg, toks, rid, seed)):
            draws += 1
            if ref["decidable"]:
                assert toks[t] == ref["token"], (i, t)
                assert np.array_equal(sc[t].view(np.uint32), ref["scores"].view(np.uint32)), (i, t)
            else:
                undecidable += 1
                assert toks[t] in ref["kept"] or np.isfinite(sc[t, toks[t]]), (i, t)
    print(f"seven requests: {undecidable} of {draws} draws undecidable")
    assert draws == sum(limits) and undecidable <= 2
    plain = _generator(model, g, 2, sync_every=4)                       # the choice rule changed the decode
    pids = plain.submit(**_inputs(g, rows), max_new_tokens=limits)
    greedy = _run(plain, pids)
    assert any(greedy[p][0] != got[r][0] for p, r in zip(pids, ids))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_bf16_without_refills_equals_generate_bit_for_bit(g, use_graph):
    """slots = number of prompts, one submission, default keys (request id = row index): tokens, logits and scores of
    `model.generate(seed=, the same processors)`, whose row r draws sample_uniform(seed, r, step) -- with and without an eos id."""
    model = _model(g, "d64", torch.bfloat16)
    n, pad, seed = g["meta"]["max_new_tokens"], g["meta"]["pad_id"], 77
    kw = dict(RP, **SAMPLE, seed=seed)
    ref = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=pad, return_dict_in_generate=True, output_logits=True,
                         output_scores=True, use_graph=use_graph, **kw)
    ref_lg, ref_sc = torch.stack(ref.logits, 0), torch.stack(ref.scores, 0)       # [n, 3, V] f32
    gen = _generator(model, g, 3, choice="device", output_logits=True, output_scores=True, use_graph=use_graph, **kw)
    ids = gen.submit(**_inputs(g))
    done = {item[0]: item for item in gen.run()}
    for b, rid in enumerate(ids):
        assert torch.equal(done[rid][1], ref.sequences[b]), b
        assert torch.equal(done[rid][2], ref_lg[:, b]) and torch.equal(done[rid][3].view(torch.int32), ref_sc[:, b].view(torch.int32)), b
    eos = int(ref.sequences[1, 4])                                                # row 1 ends at its fifth token at the latest
    ref_eos = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=eos, pad_token_id=pad, use_graph=use_graph, **kw)
    gen = _generator(model, g, 3, choice="device", eos_token_id=eos, sync_every=3, use_graph=use_graph, **kw)
    ids = gen.submit(**_inputs(g))
    got = _run(gen, ids)
    for b, rid in enumerate(ids):
        assert got[rid][0] == _cut(to_np(ref_eos[b]).tolist(), eos), b
    assert len(got[ids[1]][0]) <= 5


def test_top_k_1_sampling_is_greedy(g):
    """One survivor: the draw cannot matter -- seeded sampling with top_k = 1 returns the greedy decode under the same processors."""
    model = _model(g, "d64", torch.float32)
    limits, rows = [5, 14, 2, 9], [0, 1, 2, 1]
    runs = []
    for kw in (dict(), dict(do_sample=True, top_k=1, seed=9, temperature=0.7)):
        gen = _generator(model, g, 2, choice="device", sync_every=3, **RP, **kw)
        ids = gen.submit(**_inputs(g, rows), max_new_tokens=limits)
        got = _run(gen, ids)
        runs.append([got[r][0] for r in ids])
    assert runs[0] == runs[1] and [len(t) for t in runs[0]] == limits


KEYED = dict(do_sample=True, top_k=3, top_p=0.9, temperature=0.8)     # three survivors: fewer thresholds for a draw to fall close to


def _keyed_run(model, g, slots, order, rows, limits, keys, seed):
    gen = _generator(model, g, slots, choice="device", sync_every=2, output_logits=True, seed=seed, **RP, **KEYED)
    ids = gen.submit(**_inputs(g, [rows[j] for j in order]), max_new_tokens=[limits[j] for j in order], sample_keys=[keys[j] for j in order])
    got = _run(gen, ids)
    return {keys[j]: got[rid] for j, rid in zip(order, ids)}


def _margin(refs):
    return min(min(r["m_p"], r["m_u"]) for r in refs)


def test_tokens_depend_on_the_key_not_on_order_or_slots(g):
    """Five requests with explicit keys (beyond 2^40, one negative), forward through 2 slots and reversed through 2 and through 3: per
    key the same tokens.  fp32: the runs' logits differ by the tolerance of differently composed prefills, so the seed is the first of
    1 .. 12 whose forward run keeps every draw's margins above MARGIN; if none does, each run is held to its own re-derivation instead
    (the printed line says which comparison was made)."""
    model = _model(g, "d64", torch.float32)
    rows, limits = [0, 1, 2, 0, 1], [4, 6, 3, 5, 2]
    keys = [2 ** 41 + 3, -9, 7, 2 ** 62 + 1, 123456789012]
    fwd, rev = list(range(5)), list(range(4, -1, -1))
    mode = "own"
    derive = lambda run, k, seed: ccr.rederive(run[k][1], run[k][0], k, seed, KEYED["temperature"], KEYED["top_k"], KEYED["top_p"], proc=PROC)
    for seed in range(1, 13):
        a = _keyed_run(model, g, 2, fwd, rows, limits, keys, seed)
        refs = {k: derive(a, k, seed) for k in keys}
        if min(_margin(r) for r in refs.values()) > MARGIN:
            mode = "cross"
            break
    print(f"key invariance: seed {seed}, comparison '{mode}'")
    runs = [a, _keyed_run(model, g, 2, rev, rows, limits, keys, seed), _keyed_run(model, g, 3, rev, rows, limits, keys, seed)]
    for j, k in enumerate(keys):
        assert all(len(run[k][0]) == limits[j] for run in runs)
        if mode == "cross":
            assert runs[0][k][0] == runs[1][k][0] == runs[2][k][0] == [r["token"] for r in refs[k]], k
            assert all(np.abs(run[k][1] - a[k][1]).max() < 2 * LOGIT_TOL for run in runs[1:]), k      # each within LOGIT_TOL of the reference model
        else:
            for run in runs:
                assert all(r["token"] == t for r, t in zip(derive(run, k, seed), run[k][0]) if r["decidable"]), k
    # the key IS the draw: the same requests under other keys decode differently
    other = _keyed_run(model, g, 2, fwd, rows, limits, [k + 1 for k in keys], seed)
    assert any(other[k + 1][0] != a[k][0] for k in keys)


def test_70_tokens_cross_the_tile_edge_with_a_history_of_their_own(g):
    """d64, fp32, 2 slots, no_repeat_ngram_size = 3: request 0 generates 70 tokens -- past the first 64-key tile and past 64 history
    entries -- while the other slot serves four short requests (three refills, each resetting that slot's counter).  Its history stays its
    own: no tri-gram repeats in it, and every token of every request is the argmax of ITS logits row processed with ITS earlier tokens."""
    model = _model(g, "d64", torch.float32)
    rows, limits = [0, 1, 2, 1, 2], [70, 6, 10, 8, 5]
    gen = _generator(model, g, 2, new=70, choice="device", sync_every=4, output_logits=True, no_repeat_ngram_size=3)
    ids = gen.submit(**_inputs(g, rows), max_new_tokens=limits)
    got = _run(gen, ids)
    banned = 0
    for i, rid in enumerate(ids):
        toks, lg = got[rid]
        assert len(toks) == limits[i]
        tri = list(zip(toks, toks[1:], toks[2:]))
        assert len(set(tri)) == len(tri), i
        for t in range(len(toks)):
            y = LR.process_row(lg[t], toks[:t], ngram=3)
            banned += int(np.isinf(y).sum())
            assert toks[t] == LR.argmax_first(y), (i, t)
    assert banned > 0                                                     # the ban did fire (greedy decoding of these models loops)
    eng = gen.decoder.engine()
    assert eng.G == 128 and eng.steps_run >= 69


def test_inference_epoch_with_choice_device_does_not_depend_on_the_slots(g, tmp_path):
    """`inference_epoch` with continuous_slots, choice="device", do_sample and a seed over two batches (3 + 2 prompts): the same JSON for
    2 and for 3 slots (seed = generation_seed(args seed, rank, 0), keys = request ids).  The args seed is the first of a short list for
    which every draw of a 2-slot run of the same requests keeps its margins above MARGIN; num_beams = 3 still raises."""
    import p2t_hip as P
    from p2t_hip.loop import generation_seed
    model = _model(g, "d64", torch.float32)
    pad, eos = g["meta"]["pad_id"], g["meta"]["cases"]["d64"]["eos"]
    n, order = 6, [0, 1, 2, 2, 0]
    choice = dict(choice="device", do_sample=True, top_k=3, top_p=0.9, temperature=0.8, repetition_penalty=1.3, no_repeat_ngram_size=2)

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=False):
            return [" ".join(str(int(t)) for t in row if not (skip_special_tokens and int(t) in (pad, eos, 128002))) for row in ids]

    def batch(rows, names, desc):
        t = lambda k: torch.from_numpy(g[k][rows])
        return dict(name=names, input_ids=t("input_ids"), attention_mask=t("attention_mask"), protein_input_ids=t("protein_input_ids"),
                    protein_attention_mask=t("protein_attention_mask"), description_input_ids=torch.tensor(desc))

    batches = [batch([0, 1, 2], ["P1", "P2", "P3"], [[7, 8, pad], [9, eos, pad], [1, 2, 3]]), batch([2, 0], ["P4", "P5"], [[4, 5], [6, pad]])]
    found = None
    for arg_seed in range(8):
        seed = generation_seed(arg_seed, 0, 0)
        gen = _generator(model, g, 2, new=n, eos_token_id=128009, output_logits=True, seed=seed, **choice)
        ids = gen.submit(**_inputs(g, order[:3])) + gen.submit(**_inputs(g, order[3:]))          # batch by batch, as inference_epoch submits
        got = _run(gen, ids)
        refs = [ccr.rederive(got[r][1], got[r][0], r, seed, 0.8, 3, 0.9, proc=PROC) for r in ids]
        if min(_margin(r) for r in refs) > MARGIN and all([x["token"] for x in r] == got[i][0] for r, i in zip(refs, ids)):
            found = arg_seed
            break
    assert found is not None, "no args seed below 8 keeps every draw's margin above 10 x the logit tolerance"
    args = dict(max_generation_length=n, num_beams=1, length_penalty=1.0, seed=found, save_generation_dir=str(tmp_path), **choice)
    two = json.load(open(P.inference_epoch(0, model, batches, Tok(), dict(args, continuous_slots=2, save_generation_postfix_identifier="two"))))
    three = json.load(open(P.inference_epoch(0, model, batches, Tok(), dict(args, continuous_slots=3, save_generation_postfix_identifier="three"))))
    assert list(two) == ["P1", "P2", "P3", "P4", "P5"] and two == three
    for name, rid in zip(two, ids):                                       # ... and it is the run whose draws were re-derived above
        assert two[name]["pred"].split() == [str(t) for t in got[rid][0] if t not in (pad, eos, 128002)], name
    assert two["P3"]["pred"] != two["P4"]["pred"] or two["P1"]["pred"] != two["P5"]["pred"]      # the same prompt under another key
    with pytest.raises(NotImplementedError, match="num_beams"):
        P.inference_epoch(0, model, batches, Tok(), dict(args, continuous_slots=2, num_beams=3))
