"""p2t_beam_sample_select (csrc/beam_sample_select.hip) alone, on synthetic logits and states, against the fp64 restatement
(tests/beam_sample_reference.py): every prompt of every step the restatement calls decidable must equal it exactly in tokens, src_rows,
tables and flags, with the scores inside the restatement's error bounds; a flagged prompt (bit 1: its results are unspecified) and an
undecidable one must keep every index in range and the tables free of NaN.  The chains of beam_sample_reference.CASES feed each step the
state the kernel itself left; tests/test_beam_sample_reference_host.py bounds the share of undecidable cases on the CPU.  Padding
columns hold NaN and +inf; the specific cases follow the chains."""
import numpy as np
import pytest
import torch

import beam_sample_reference as R
from gpu_util import dev
from p2t_hip import generation as G
from test_gpu_beam_select import GCAP, PAD, TABLES, _load, _read, _snapshot, _tensor

pytestmark = pytest.mark.gpu


def _state(B0, nb):
    return G.BeamState(B0, nb, GCAP, PAD, dev(), sample=True)


def _call(st, logits, V, cur, eos_ids, lp, es, L, T, k, p, seed, prompt0=0, scores=None):
    """-> (next_tokens, src_rows, the flag bits this call raised)."""
    BB = st.B * st.nb
    step = torch.tensor([cur], dtype=torch.int32, device=dev())
    nxt = torch.full((BB,), -7, dtype=torch.int64, device=dev())
    src = torch.full((BB,), -7, dtype=torch.int64, device=dev())
    eos = torch.tensor(eos_ids, dtype=torch.int64, device=dev())
    st.flags.zero_()
    G.beam_sample_select(logits, V, st, eos, PAD, lp, es, L, step, nxt, src, T, k, p, seed, scores, prompt0)
    torch.cuda.synchronize()
    return nxt.cpu().numpy(), src.cpu().numpy(), int(st.flags.item())


def _in_range(got, nxt, src, b, nb, V, cur, ctx):
    rows = slice(b * nb, (b + 1) * nb)
    assert ((nxt[rows] >= 0) & (nxt[rows] < V)).all() and ((src[rows] >= b * nb) & (src[rows] < (b + 1) * nb)).all(), (ctx, cur, b, nxt[rows], src[rows])
    for k in ("running", "sequences"):
        assert ((got[k][b, :, : cur + 1] >= 0) & (got[k][b, :, : cur + 1] < V)).all(), (ctx, cur, b, k)
    for k in ("running_idx", "beam_idx"):
        t = got[k][b, :, : cur + 1]
        assert ((t >= -1) & (t < (b + 1) * nb)).all(), (ctx, cur, b, k)
    assert not np.isnan(got["running_scores"][b]).any() and not np.isnan(got["beam_scores"][b]).any(), (ctx, cur, b)


def _compare(ref, got, nxt, src, flags, cur, nb, V, ctx):
    """Every decidable prompt: tables, flags and outputs exactly, scores within their bounds; every other one: in range.  -> the number
    of prompts compared exactly."""
    r, n = ref["state"], 0
    for b in range(len(ref["decidable"])):
        _in_range(got, nxt, src, b, nb, V, cur, ctx)
        if not ref["decidable"][b] or ref["flagged"][b]:
            continue
        n += 1
        rows = slice(b * nb, (b + 1) * nb)
        assert np.array_equal(got["sequences"][b], r["sequences"][b]) and np.array_equal(got["beam_idx"][b], r["beam_idx"][b]), (ctx, cur, b)
        assert np.array_equal(got["is_finished"][b], r["is_finished"][b]), (ctx, cur, b)
        err = np.abs(got["beam_scores"][b].astype(np.float64) - r["beam_scores"][b])
        print(f"{ctx} cur {cur} prompt {b}: margin {ref['margin'][b]:.3g}  finished-score error {err.max():.3g} (bound {ref['beam_err'][b].max():.3g})")
        assert (err <= ref["beam_err"][b] + 2.0 ** -24 * np.abs(r["beam_scores"][b])).all(), (ctx, cur, b, err, ref["beam_err"][b])
        carried = ref["beam_err"][b] == 0
        assert np.array_equal(got["beam_scores"][b][carried], r["beam_scores"][b][carried])          # a carried slot keeps its bits
        if ref["running_decidable"][b]:
            assert np.array_equal(got["running"][b], r["running"][b]) and np.array_equal(got["running_idx"][b], r["running_idx"][b]), (ctx, cur, b)
            assert np.array_equal(nxt[rows], ref["next_tokens"][rows]) and np.array_equal(src[rows], ref["src_rows"][rows]), (ctx, cur, b)
            err = np.abs(got["running_scores"][b].astype(np.float64) - r["running_scores"][b])
            assert (err <= ref["running_err"][b] + 2.0 ** -24 * np.abs(r["running_scores"][b])).all(), (ctx, cur, b, err, ref["running_err"][b])
            assert got["heuristic_open"][b] == r["heuristic_open"][b], (ctx, cur, b)
    if ref["decidable"].all():                                # every flag decision of the step is decidable
        assert flags == ref["flags"], (ctx, cur, flags, ref["flags"])
        if not ref["flagged"].any() and (ref["running_decidable"].all() or (r["done"] and cur + 1 >= r["running"].shape[2])):
            assert got["done"] == r["done"] and (not r["done"] or got["steps"] == r["steps"]), (ctx, cur)
    return n


def _compare_scores(ref, sc, V, nb, ctx, cur):
    """The processed scores of the decidable prompts' rows: the same kept set, y within its bound."""
    assert (sc[:, V:] == -5.0).all()
    for b in np.nonzero(ref["decidable"])[0]:
        rows = slice(b * nb, (b + 1) * nb)
        want, got = ref["scores"][rows], sc[rows, :V]
        cut = np.isinf(want)
        assert np.array_equal(np.isneginf(got), cut), (ctx, cur, b)
        assert (np.abs(got[~cut] - want[~cut]) <= ref["e_scores"][rows][~cut]).all(), (ctx, cur, b)


def _stopped_call_changes_nothing(st, logits, V, cur, eos_ids, lp, es, L, T, k, p):
    snap = _snapshot(st)
    nxt, src, flags = _call(st, logits, V, cur, eos_ids, lp, es, L, T, k, p, R.SEED)
    assert (nxt == PAD).all() and np.array_equal(src, np.arange(len(src))) and flags == 0
    for key, v in snap.items():
        assert torch.equal(getattr(st, key), v), key


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_chain_against_the_restatement(case):
    name, V, ld, B0, nb, n_eos, dtype, steps, L, lp, es, T, k, p = case
    eos_ids = R.case_eos(V, n_eos)
    st = _state(B0, nb)
    scores = torch.full((B0 * nb, V + 3), -5.0, dtype=torch.float32, device=dev())
    compared = 0
    for cur in range(steps):
        vals = R.case_logits(R.case_seed(name), cur, B0 * nb, V, dtype, eos_ids)
        logits = _tensor(vals, ld, dtype)
        before = _read(st, cur & 1, L)
        if before["done"]:
            _stopped_call_changes_nothing(st, logits, V, cur, eos_ids, lp, es, L, T, k, p)
            continue
        ref = R.step(vals, before, cur, nb, eos_ids, lp, es, L, PAD, T, k, p, R.SEED, 0)
        nxt, src, flags = _call(st, logits, V, cur, eos_ids, lp, es, L, T, k, p, R.SEED, 0, scores)
        got = _read(st, (cur + 1) & 1, L)
        compared += _compare(ref, got, nxt, src, flags, cur, nb, V, name)
        _compare_scores(ref, scores.cpu().numpy().astype(np.float64), V, nb, name, cur)
        assert (st.run_seq[:, :, :, L:] == PAD).all() and (st.fin_idx[:, :, :, L:] == -1).all()      # nothing beyond the search's columns
        assert (got["running"][:, :, cur + 1:] == PAD).all() and (got["running_idx"][:, :, cur + 1:] == -1).all()
    assert compared > 0, name
    if not bool(st.done[0].item()):
        st.done.copy_(torch.tensor([1, steps], dtype=torch.int32))
    for cur in (steps, steps + 1):                            # a stopped search: whatever cur is, nothing moves
        _stopped_call_changes_nothing(st, logits, V, min(cur, L - 1), eos_ids, lp, es, L, T, k, p)


def test_one_beam_and_top_k_one_is_the_greedy_continuation():
    """nb = 1, top_k = 1: one kept candidate per row, so the first draw is forced.  keep = 2 asks for a second one that does not exist:
    bit 1 is raised (header, item 6) -- and the forced token still goes on."""
    V, B0, L = 257, 2, 5
    st = _state(B0, 1)
    want = np.zeros((B0, L), dtype=np.int64)
    for cur in range(L):
        vals = R.case_logits(77, cur, B0, V, "f32", [])
        nxt, src, flags = _call(st, _tensor(vals, V, "f32"), V, cur, [], 0.0, False, L, 0.7, 1, 1.0, R.SEED)
        want[:, cur] = vals.argmax(1)
        assert np.array_equal(nxt, want[:, cur]) and np.array_equal(src, np.arange(B0)) and flags == 2, (cur, nxt, flags)
    got = _read(st, L & 1, L)
    assert got["done"] and got["steps"] == L
    assert np.array_equal(got["running"][:, 0], want) and np.array_equal(got["sequences"][:, 0], want) and got["is_finished"].all()


def test_a_row_of_one_repeated_value_fills_the_table_and_raises_bit_0():
    V, nb, L = 4096, 2, 4
    vals = np.full((nb, V), R.to_dtype(np.float32(1.37), "bf16"), dtype=np.float32)
    st = _state(1, nb)
    ref = R.step(vals, R.fresh_state(1, nb, L, PAD), 0, nb, [], 1.0, False, L, PAD, 1.0, 1024, 1.0, R.SEED, 0)
    assert ref["flags"] == 1 and ref["decidable"].all() and ref["running_decidable"].all()
    scores = torch.full((nb, V + 3), -5.0, dtype=torch.float32, device=dev())
    nxt, src, flags = _call(st, _tensor(vals, V, "bf16"), V, 0, [], 1.0, False, L, 1.0, 1024, 1.0, R.SEED, 0, scores)
    assert flags == 1
    assert _compare(ref, _read(st, 1, L), nxt, src, flags, 0, nb, V, "ties") == 1
    assert (nxt < R.CAP).all()                                # the table took the first 2048 columns
    sc = scores.cpu().numpy()
    assert np.isfinite(sc[:, :R.CAP]).all() and np.isneginf(sc[:, R.CAP:V]).all()


def test_one_survivor_per_row_raises_bit_1_and_stays_in_range():
    V, B0, nb, L = 257, 2, 3, 6
    st = _state(B0, nb)
    for cur in range(3):
        vals = R.case_logits(78, cur, B0 * nb, V, "f32", [])
        before = _read(st, cur & 1, L)
        if before["done"]:
            break
        nxt, src, flags = _call(st, _tensor(vals, 320, "f32"), V, cur, [], 1.0, False, L, 1.0, 2, 0.01, R.SEED)
        assert flags & 2, (cur, flags)
        got = _read(st, (cur + 1) & 1, L)
        for b in range(B0):
            _in_range(got, nxt, src, b, nb, V, cur, "dry")


def test_same_inputs_same_bits_and_the_seed_and_prompt0_change_the_draw():
    V, B0, nb, L, cur = 1000, 3, 3, 8, 2
    s = R.fresh_state(B0, nb, L, PAD)
    rng = np.random.default_rng(3)
    s["running"][:, :, :cur] = rng.integers(1, V - 1, (B0, nb, cur))
    s["running_idx"][:, :, :cur] = rng.integers(0, nb, (B0, nb, cur)) + (np.arange(B0) * nb)[:, None, None]
    s["running_scores"][:] = -1.0 - 0.3 * np.arange(nb)
    vals = R.case_logits(79, cur, B0 * nb, V, "bf16", [])
    outs = {}
    for key, (seed, prompt0) in dict(a=(11, 0), b=(11, 0), seed=(12, 0), prompt0=(11, 5)).items():
        st = _state(B0, nb)
        _load(st, cur & 1, s)
        nxt, src, flags = _call(st, _tensor(vals, 1024, "bf16"), V, cur, [], 1.0, False, L, 2.0, 50, 0.95, seed, prompt0)
        assert flags == 0
        outs[key] = (_snapshot(st), nxt, src, st.workspace.clone())
    for k in TABLES:
        assert torch.equal(outs["a"][0][k], outs["b"][0][k]), k
    assert np.array_equal(outs["a"][1], outs["b"][1]) and np.array_equal(outs["a"][2], outs["b"][2]) and torch.equal(outs["a"][3], outs["b"][3])
    for other in ("seed", "prompt0"):
        assert not np.array_equal(outs["a"][1], outs[other][1]), other
    # prompt0 = 5 draws for prompt b what prompt0 = 0 draws for prompt b + 5: the restatement says which
    ref = R.step(vals, s, cur, nb, [], 1.0, False, L, PAD, 2.0, 50, 0.95, 11, 5)
    for b in np.nonzero(ref["decidable"] & ref["running_decidable"])[0]:
        assert np.array_equal(outs["prompt0"][1][b * nb:(b + 1) * nb], ref["next_tokens"][b * nb:(b + 1) * nb]), b
