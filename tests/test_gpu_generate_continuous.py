"""Continuous batching end to end (p2t_hip/continuous.py: ContinuousDecoder / Esm2LlamaInstructForCausalLM.continuous_generator) on the
generate_tiny.npz models: requests through fewer slots than requests, each against the REFERENCE class's own `generate` (fp32: exact
ids, logits to 2e-4), against `model.generate` bit for bit where nothing is refilled (bf16, every quantised variant), against the
model's own cache-less forward where slots are refilled (bf16), across the 64-key tile edge of the generated segment, and through
`inference_epoch`."""
import json
import os

import numpy as np
import pytest
import torch

from gpu_util import build_model, dev, observe, rel, to_dev, to_np
from p2t_hip import specs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["d16", "d64", "d128", "qwen3"]
LOGIT_TOL = 2e-4                         # test_fp32_greedy_vs_reference_generate's


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


def _inputs(g, rows=None):
    pick = (lambda a: a) if rows is None else (lambda a: a[list(rows)])
    return dict(inputs=to_dev(pick(g["input_ids"])), attention_mask=to_dev(pick(g["attention_mask"])), protein_input_ids=to_dev(pick(g["protein_input_ids"])),
                protein_attention_mask=to_dev(pick(g["protein_attention_mask"])))


def _generator(model, g, slots, new=None, **kw):
    T = int(g["input_ids"].shape[1])
    return model.continuous_generator(slots=slots, max_prompt_tokens=T, max_new_tokens=new or g["meta"]["max_new_tokens"], pad_token_id=g["meta"]["pad_id"], **kw)


def _run(gen, ids):
    """-> {request id: (tokens list, logits [n, V] or None)}; every id exactly once."""
    out = {}
    for item in gen.run():
        assert item[0] not in out
        out[item[0]] = (to_np(item[1]).tolist(), to_np(item[2]) if len(item) > 2 else None)
    assert sorted(out) == sorted(ids)
    return out


def _gaps_hold(g, case):
    """Exact ids are a fair demand where the reference's own top-2 gap is far above what the logits may differ by: the golden records
    the smallest gap over all rows and steps; re-derived here from its logits and held to >= 10 x the logit tolerance."""
    lg = np.sort(g[f"{case}.greedy_logits"].astype(np.float64), axis=-1)
    gap = float((lg[..., -1] - lg[..., -2]).min())
    assert abs(gap - g["meta"]["cases"][case]["min_top2_gap"]) < 1e-6 and gap >= 10 * LOGIT_TOL, (case, gap)


def _cut(row, eos):
    row = list(row)
    return row[: row.index(eos) + 1] if eos in row else row


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", CASES)
def test_fp32_three_prompts_through_two_slots_vs_reference_generate(g, case, use_graph):
    """The golden's 3 prompts with the case's eos: row 1 stops at its eos (token 5), and the third prompt waits for that slot.  Each
    request is its `greedy_eos` row cut after its eos -- ids exact, per-step logits within 2e-4 of the reference's."""
    _gaps_hold(g, case)
    model = _model(g, case, torch.float32)
    eos = g["meta"]["cases"][case]["eos"]
    gen = _generator(model, g, 2, eos_token_id=eos, use_graph=use_graph, sync_every=4, output_logits=True)
    ids = gen.submit(**_inputs(g))
    got = _run(gen, ids)
    want = g[f"{case}.greedy_eos"]
    assert _cut(want[1], eos)[-1] == eos and len(_cut(want[1], eos)) == 5
    for b, rid in enumerate(ids):
        toks, lg = got[rid]
        assert toks == _cut(want[b], eos), (b, toks)
        assert np.abs(lg - g[f"{case}.greedy_logits"][: len(toks), b]).max() < LOGIT_TOL, b
    eng = gen.decoder.engine()
    assert (eng.graph is not None) == use_graph and eng.B0 == 2


@pytest.mark.parametrize("sync_every", [1, 4])
@pytest.mark.parametrize("case", CASES)
def test_fp32_seven_requests_through_two_slots_with_their_own_limits(g, case, sync_every):
    """The golden prompts cycled, per-request limits [3, 14, 1, 9, 14, 2, 5], no eos: request i is the first limit[i] tokens of its
    `greedy` row, ids exact and logits within 2e-4, whatever it shared the engine with."""
    _gaps_hold(g, case)
    model = _model(g, case, torch.float32)
    limits = [3, 14, 1, 9, 14, 2, 5]
    rows = [i % 3 for i in range(7)]
    gen = _generator(model, g, 2, sync_every=sync_every, output_logits=True)
    ids = gen.submit(**_inputs(g, rows), max_new_tokens=limits)
    got = _run(gen, ids)
    for i, rid in enumerate(ids):
        toks, lg = got[rid]
        assert toks == g[f"{case}.greedy"][rows[i], : limits[i]].tolist(), i
        assert lg.shape[0] == limits[i] and np.abs(lg - g[f"{case}.greedy_logits"][: limits[i], rows[i]]).max() < LOGIT_TOL, i


VARIANTS = {"plain": ("model", {}), "kv8": ("model", dict(prompt_kv_dtype="fp8")), "head_fp8": ("model", dict(lm_head_dtype="fp8")),
            "head_mxfp4": ("model", dict(lm_head_dtype="mxfp4")), "mxfp4_model": ("mxfp4", {}), "row_major": ("model", dict(stream_copy=False))}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_bf16_without_refills_equals_generate_bit_for_bit(g, variant):
    """slots = number of prompts, one submission: the same compaction, the same prefill (into the staging cache), the same steps with
    equal counters -- tokens and every step's logits equal `model.generate`'s bit for bit, plain and with the fp8 prompt segment, both
    quantised heads, an MXFP4 model and row-major weights; with the case's eos, each request is generate's row cut after its eos."""
    case = "d64"
    gemm, kw = VARIANTS[variant]
    model = _model(g, case, torch.bfloat16)
    if gemm != "model":
        model.set_gemm_dtype(gemm)
    n, pad, eos = g["meta"]["max_new_tokens"], g["meta"]["pad_id"], g["meta"]["cases"][case]["eos"]
    ref = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=pad, do_sample=False, return_dict_in_generate=True,
                         output_logits=True, **kw)
    ref_lg = torch.stack(ref.logits, 0)                          # [n, 3, V] f32
    gen = _generator(model, g, 3, output_logits=True, **kw)
    ids = gen.submit(**_inputs(g))
    done = {item[0]: item for item in gen.run()}
    for b, rid in enumerate(ids):
        assert torch.equal(done[rid][1], ref.sequences[b]) and torch.equal(done[rid][2], ref_lg[:, b]), b
    ref_eos = model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=eos, pad_token_id=pad, do_sample=False, **kw)
    gen = _generator(model, g, 3, eos_token_id=eos, sync_every=3, **kw)
    ids = gen.submit(**_inputs(g))
    got = _run(gen, ids)
    for b, rid in enumerate(ids):
        assert got[rid][0] == _cut(to_np(ref_eos[b]).tolist(), eos), b


@pytest.mark.parametrize("case", ["d64", "d128", "d16"])
def test_bf16_with_refills_vs_the_models_own_cacheless_forward(g, case):
    """6 requests through 2 slots (limits [6, 3, 8, 2, 5, 7]: every slot is refilled): each request's per-step logits against the
    model's own cache-less forward over its compacted prompt + the ids it chose -- the bound the project observes for
    generate[case].bf16_cache_vs_full_forward (3e-2 relative)."""
    model = _model(g, case, torch.bfloat16)
    limits = [6, 3, 8, 2, 5, 7]
    rows = [i % 3 for i in range(6)]
    gen = _generator(model, g, 2, sync_every=2, output_logits=True)
    ids = gen.submit(**_inputs(g, rows), max_new_tokens=limits)
    got = _run(gen, ids)
    with torch.no_grad():
        emb, mask = model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                          protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)
    dec = model.llama_decoder
    for i, rid in enumerate(ids):
        toks, lg = got[rid]
        b, n = rows[i], limits[i]
        assert len(toks) == n
        valid = to_np(mask)[b] != 0
        prompt = emb[b][torch.from_numpy(valid).to(emb.device)]
        tail = dec.model.embed(to_dev(np.array([toks[:-1]], dtype=np.int64)))[0] if n > 1 else prompt[:0]
        with torch.no_grad():
            full = to_np(dec(inputs_embeds=torch.cat([prompt, tail.to(prompt.dtype)], 0)[None]).logits.float())[0]
        n0 = int(valid.sum())
        observe(f"generate_continuous[{case}].bf16_cache_vs_full_forward.req{i}", rel(lg, full[n0 - 1:n0 - 1 + n]), 3e-2)


def test_70_tokens_cross_the_tile_edge_while_the_neighbour_slot_is_refilled(g):
    """d64, fp32, 2 slots: request 0 generates 70 tokens -- its generated segment grows past the first 64-key tile -- while the other slot
    serves four short requests one after another (three refills, each resetting that slot's counter to 0).  Request 0's ids equal the
    plain `generate` of its prompt; the short ones equal the first tokens of their `greedy` rows."""
    case = "d64"
    model = _model(g, case, torch.float32)
    pad = g["meta"]["pad_id"]
    want = to_np(model.generate(**_inputs(g, [0]), max_new_tokens=70, eos_token_id=None, pad_token_id=pad, do_sample=False))[0].tolist()
    assert want[:14] == g[f"{case}.greedy"][0].tolist()
    rows, limits = [0, 1, 2, 1, 2], [70, 6, 10, 8, 5]
    gen = _generator(model, g, 2, new=70, sync_every=4)
    ids = gen.submit(**_inputs(g, rows), max_new_tokens=limits)
    got = _run(gen, ids)
    assert got[ids[0]][0] == want
    for i in range(1, 5):
        assert got[ids[i]][0] == g[f"{case}.greedy"][rows[i], : limits[i]].tolist(), i
    eng = gen.decoder.engine()
    assert eng.G == 128 and eng.steps_run >= 69


def test_inference_epoch_with_continuous_slots_writes_the_same_json(g, tmp_path):
    """`inference_epoch` with args["continuous_slots"] = 2 over two batches (3 + 2 prompts): the JSON of the lock-step path, names in
    dataset order (fp32; the stub tokenizer of test_inference_epoch_writes_the_reference_json)."""
    import p2t_hip as P
    model = _model(g, "d64", torch.float32)
    meta = g["meta"]
    n, pad, eos = meta["max_new_tokens"], meta["pad_id"], meta["cases"]["d64"]["eos"]

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=False):
            return [" ".join(str(int(t)) for t in row if not (skip_special_tokens and int(t) in (pad, eos, 128002))) for row in ids]

    def batch(rows, names, desc):
        t = lambda k: torch.from_numpy(g[k][rows])
        return dict(name=names, input_ids=t("input_ids"), attention_mask=t("attention_mask"), protein_input_ids=t("protein_input_ids"),
                    protein_attention_mask=t("protein_attention_mask"), description_input_ids=torch.tensor(desc))

    batches = [batch([0, 1, 2], ["P1", "P2", "P3"], [[7, 8, pad], [9, eos, pad], [1, 2, 3]]), batch([2, 0], ["P4", "P5"], [[4, 5], [6, pad]])]
    args = dict(max_generation_length=n, num_beams=1, length_penalty=1.0, temperature=1.0, do_sample=False, top_p=1.0, top_k=50,
                save_generation_dir=str(tmp_path), save_generation_postfix_identifier="lock")
    lock = json.load(open(P.inference_epoch(0, model, batches, Tok(), args)))
    cont = json.load(open(P.inference_epoch(0, model, batches, Tok(), dict(args, continuous_slots=2, save_generation_postfix_identifier="cont"))))
    assert list(cont) == ["P1", "P2", "P3", "P4", "P5"] and cont == lock
    assert cont["P2"]["pred"].split() == [str(t) for t in g["d64.greedy"][1] if t not in (pad, eos)] and cont["P4"]["pred"] == cont["P3"]["pred"]
    with pytest.raises(NotImplementedError, match="num_beams"):
        P.inference_epoch(0, model, batches, Tok(), dict(args, continuous_slots=2, num_beams=3))
