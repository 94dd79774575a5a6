"""CPU: the fp64 restatement of a beam-search step (tests/beam_reference.py) against the factored torch step of the torch path
(p2t_hip.generation.beam_step_torch) on tie-free cases, chained over whole runs against oracle.generate_beam on the tiny golden
models, and the share of undecidable (prompt, step) cases among the synthetic cases of tests/test_gpu_beam_select.py -- bounded here,
by the restatement alone, so that the GPU test cannot hide a failure behind undecidable cases."""
import numpy as np
import pytest
import torch

import beam_reference as BR


def _np_state(st, done=False):
    return dict(running=st["running"].numpy().copy(), running_idx=st["running_idx"].numpy().copy(), running_scores=st["running_scores"].numpy().copy(),
                sequences=st["sequences"].numpy().copy(), beam_idx=st["beam_idx_tab"].numpy().copy(), beam_scores=st["beam_scores"].numpy().copy(),
                is_finished=st["is_finished"].numpy().copy(), heuristic_open=st["heuristic_open"].numpy()[:, 0].copy(), done=done, steps=0)


@pytest.mark.parametrize("early_stopping", [False, True, "never"])
@pytest.mark.parametrize("n_eos", [0, 1, 2])
@pytest.mark.parametrize("length_penalty", [0.0, 0.8, 2.0])
def test_restatement_equals_the_torch_step(early_stopping, n_eos, length_penalty):
    from p2t_hip import generation as G
    B, nb, V, L, pad = 2, 3, 61, 7, 0
    eos_ids = BR.case_eos(V, n_eos)
    eos = torch.tensor(eos_ids, dtype=torch.int64)
    st = G.beam_state_init(B, nb, L, pad, "cpu")
    went_on = True
    for cur in range(L):
        logits = BR.case_logits(11 + n_eos, cur, B * nb, V, "f32", eos_ids)
        ref = BR.step(logits, _np_state(st), cur, nb, eos_ids, length_penalty, early_stopping, L, pad)
        assert ref["decidable"].all(), (cur, ref["margin"])               # the cases are free of ties: nothing is skipped
        new, log_probs, src_rows, hits, go_on = G.beam_step_torch(st, torch.from_numpy(logits), cur, nb, eos, length_penalty, early_stopping, L)
        r = ref["state"]
        assert np.abs(log_probs.numpy() - ref["log_probs"]).max() < 1e-5
        # an unfinished slot and a masked candidate both score exactly -1e9 in f32: which of them torch.topk keeps there is unspecified
        # (the restatement keeps the slot, by position), so the slots are compared where they hold a hypothesis
        fin = r["is_finished"]
        assert np.array_equal(new["is_finished"].numpy(), fin)
        assert np.array_equal(new["sequences"].numpy()[fin], r["sequences"][fin]) and np.array_equal(new["beam_idx_tab"].numpy()[fin], r["beam_idx"][fin])
        assert np.allclose(new["beam_scores"].numpy()[fin], r["beam_scores"][fin], rtol=1e-6, atol=1e-5)
        assert (new["beam_scores"].numpy()[~fin] <= -1e9).all() and (r["beam_scores"][~fin] == -1e9).all()
        if ref["running_decidable"].all():
            assert np.array_equal(new["running"].numpy(), r["running"]) and np.array_equal(new["running_idx"].numpy(), r["running_idx"])
            assert np.array_equal(src_rows.numpy(), ref["src_rows"])
            assert np.array_equal(new["running"].numpy()[:, :, cur].reshape(-1), ref["next_tokens"])
            assert np.array_equal(new["heuristic_open"].numpy()[:, 0], r["heuristic_open"])
        else:
            assert cur + 1 == L                                           # only the step in which everything finishes
        went_on = bool(go_on) and cur + 1 < L
        assert r["done"] == (not went_on), cur
        st = new
        for k, v in (("sequences", r["sequences"]), ("beam_idx_tab", r["beam_idx"]), ("beam_scores", r["beam_scores"])):      # see above
            st[k] = torch.where(torch.from_numpy(fin).reshape(fin.shape + (1,) * (st[k].dim() - 2)), st[k], torch.from_numpy(v))
        if not went_on:
            break
    assert not went_on
    again = BR.step(logits, r, cur + 1, nb, eos_ids, length_penalty, early_stopping, L, pad)      # a stopped search stays as it is
    assert again["state"] is r and (again["next_tokens"] == pad).all() and np.array_equal(again["src_rows"], np.arange(B * nb))


@pytest.mark.parametrize("case", ["d16", "d64"])
def test_chained_restatement_reproduces_the_oracle_beam_search(case):
    from conftest import load_golden
    from helpers import model_weights
    from oracle import p2t_oracle as O
    from p2t_hip import specs
    g = load_golden("generate_tiny")
    meta = g["meta"]
    m = meta["cases"][case]
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    W = model_weights(esm, llama, ad, m["weight_seed"], lm_head=True)
    enc = O.esm2_forward(esm, W, g["protein_input_ids"], g["protein_attention_mask"], O.FP32, prefix="esm_encoder.")
    emb = O.sft_decoder_inputs(llama, W, g["input_ids"], O.adapter_forward(W, enc, O.FP32, prefix="adapter."), g["protein_attention_mask"],
                               meta["placeholder_id"])
    rows0 = O._prompt_rows(emb, g["attention_mask"])
    E = W["llama_decoder.model.embed_tokens.weight"]
    L, pad, nb, B = meta["max_new_tokens"], meta["pad_id"], 3, len(rows0)
    for eos_ids, lp, es, R, key in (((m["eos"],), 1.0, False, 1, "beam3_lp1.0"), (tuple(m["eos2"]), 0.8, True, 2, "beam3_esTrue")):
        st = BR.fresh_state(B, nb, L, pad)
        for cur in range(L):
            rows = [np.concatenate([rows0[b], E[st["running"][b, j, :cur]].astype(np.float32)], 0) for b in range(B) for j in range(nb)]
            logits = O.llama_next_token_logits(llama, W, rows, O.FP32, "llama_decoder.")
            out = BR.step(logits, st, cur, nb, list(eos_ids), lp, es, L, pad)
            assert out["decidable"].all(), (key, cur)
            st = out["state"]
            if st["done"]:
                break
        assert st["done"]
        want = g[f"{case}.{key}"]
        got = st["sequences"][:, :R].reshape(B * R, L)[:, : want.shape[1]]
        assert np.array_equal(got, want), key
        assert np.abs(st["beam_scores"][:, :R].reshape(-1) - g[f"{case}.{key}_scores"]).max() < 1e-4


def run_case(case, on_step):
    """The chain of one synthetic case: on_step(cur, logits f32, state before, reference result) -> the state to go on from (None: the
    reference's)."""
    name, V, ld, B0, nb, n_eos, dtype, steps, L, lp, es = case
    eos_ids = BR.case_eos(V, n_eos)
    st = BR.fresh_state(B0, nb, L, 0)
    for cur in range(steps):
        logits = BR.case_logits(sum(map(ord, name)), cur, B0 * nb, V, dtype, eos_ids)
        ref = BR.step(logits, st, cur, nb, eos_ids, lp, es, L, 0)
        nxt = on_step(cur, logits, st, ref)
        st = ref["state"] if nxt is None else nxt


def test_undecidable_share_of_the_gpu_cases():
    count = {"f32": [0, 0], "bf16": [0, 0]}
    for case in BR.CASES:
        def on_step(cur, logits, st, ref, dtype=case[6]):
            if not st["done"]:
                count[dtype][0] += int((~ref["decidable"]).sum())
                count[dtype][1] += len(ref["decidable"])
        run_case(case, on_step)
    assert count["f32"][1] > 20 and count["bf16"][1] > 20
    assert count["f32"][0] <= 0.02 * count["f32"][1], count
    assert count["bf16"][0] <= 0.05 * count["bf16"][1], count
