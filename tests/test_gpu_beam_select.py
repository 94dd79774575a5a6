"""p2t_beam_select (csrc/beam_select.hip) alone, on synthetic logits and states, against the fp64 restatement (tests/beam_reference.py):
every prompt of every step the restatement calls decidable must equal it exactly in tokens, src_rows, tables and flags, with scores
inside the restatement's error bounds.  The chains of beam_reference.CASES feed each step the state the kernel itself left (so cur is
odd and even in turn, and an undecidable prompt cannot make later steps drift); tests/test_beam_reference_host.py bounds the share
of undecidable cases on the CPU.  Padding columns hold NaN and +inf; the specific cases follow the chains."""
import numpy as np
import pytest
import torch

import beam_reference as BR
from gpu_util import dev
from p2t_hip import generation as G

pytestmark = pytest.mark.gpu
GCAP, PAD = 64, 0
TABLES = ("run_seq", "run_idx", "run_scores", "fin_seq", "fin_idx", "fin_scores", "is_finished", "heuristic_open", "done", "sync")


def _tensor(vals, ld, dtype):
    """f32 values [BB, V] -> a [BB, ld] tensor of `dtype` whose padding columns hold NaN and +inf."""
    BB, V = vals.shape
    t = torch.full((BB, ld), float("nan"), dtype=torch.float32)
    t[:, V::2] = float("inf")
    t[:, :V] = torch.from_numpy(vals)
    return t.to(dev()).to(torch.bfloat16 if dtype == "bf16" else torch.float32)


def _read(st, half, L):
    g = lambda t: t[half].cpu().numpy()
    done = st.done.cpu().numpy()
    return dict(running=g(st.run_seq)[:, :, :L].copy(), running_idx=g(st.run_idx)[:, :, :L].copy(), running_scores=g(st.run_scores).copy(),
                sequences=g(st.fin_seq)[:, :, :L].copy(), beam_idx=g(st.fin_idx)[:, :, :L].copy(), beam_scores=g(st.fin_scores).copy(),
                is_finished=g(st.is_finished).astype(bool), heuristic_open=st.heuristic_open.cpu().numpy().astype(bool), done=bool(done[0]),
                steps=int(done[1]))


def _load(st, half, s):
    L = s["running"].shape[2]
    put = lambda t, a: t[half].copy_(torch.from_numpy(np.ascontiguousarray(a)).to(t.dtype))
    for t, k in ((st.run_seq, "running"), (st.run_idx, "running_idx"), (st.fin_seq, "sequences"), (st.fin_idx, "beam_idx")):
        t[half, :, :, :L].copy_(torch.from_numpy(s[k]))
    put(st.run_scores, s["running_scores"]); put(st.fin_scores, s["beam_scores"]); put(st.is_finished, s["is_finished"].astype(np.int32))
    st.heuristic_open.copy_(torch.from_numpy(s["heuristic_open"].astype(np.int32)))
    st.done.copy_(torch.tensor([int(s["done"]), int(s["steps"])], dtype=torch.int32))


def _snapshot(st):
    return {k: getattr(st, k).clone() for k in TABLES}


def _call(st, logits, V, cur, eos_ids, lp, es, L, scores=None):
    BB = st.B * st.nb
    step = torch.tensor([cur], dtype=torch.int32, device=dev())
    nxt = torch.full((BB,), -7, dtype=torch.int64, device=dev())
    src = torch.full((BB,), -7, dtype=torch.int64, device=dev())
    eos = torch.tensor(eos_ids, dtype=torch.int64, device=dev())
    G.beam_select(logits, V, st, eos, PAD, lp, es, L, step, nxt, src, scores)
    torch.cuda.synchronize()
    return nxt.cpu().numpy(), src.cpu().numpy()


def _compare(ref, got, nxt, src, before, cur, nb, ctx):
    """Every decidable prompt: tables, flags and outputs exactly, scores within their bounds.  -> number of prompts compared."""
    r, n = ref["state"], 0
    for b in np.nonzero(ref["decidable"])[0]:
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
    if ref["decidable"].all() and ref["running_decidable"].all() or (ref["decidable"].all() and r["done"] and cur + 1 >= r["running"].shape[2]):
        assert got["done"] == r["done"] and (not r["done"] or got["steps"] == r["steps"]), (ctx, cur)
    return n


def _stopped_call_changes_nothing(st, logits, V, cur, eos_ids, lp, es, L):
    snap = _snapshot(st)
    nxt, src = _call(st, logits, V, cur, eos_ids, lp, es, L)
    assert (nxt == PAD).all() and np.array_equal(src, np.arange(len(src)))
    for k, v in snap.items():
        assert torch.equal(getattr(st, k), v), k


@pytest.mark.parametrize("case", BR.CASES, ids=[c[0] for c in BR.CASES])
def test_chain_against_the_restatement(case):
    name, V, ld, B0, nb, n_eos, dtype, steps, L, lp, es = case
    eos_ids = BR.case_eos(V, n_eos)
    st = G.BeamState(B0, nb, GCAP, PAD, dev())
    scores = torch.full((B0 * nb, V + 3), -5.0, dtype=torch.float32, device=dev())
    compared = total = 0
    for cur in range(steps):
        vals = BR.case_logits(sum(map(ord, name)), cur, B0 * nb, V, dtype, eos_ids)
        logits = _tensor(vals, ld, dtype)
        before = _read(st, cur & 1, L)
        if before["done"]:
            _stopped_call_changes_nothing(st, logits, V, cur, eos_ids, lp, es, L)
            continue
        ref = BR.step(vals, before, cur, nb, eos_ids, lp, es, L, PAD)
        nxt, src = _call(st, logits, V, cur, eos_ids, lp, es, L, scores)
        got = _read(st, (cur + 1) & 1, L)
        compared += _compare(ref, got, nxt, src, before, cur, nb, name)
        total += B0
        sc = scores.cpu().numpy().astype(np.float64)
        assert (sc[:, V:] == -5.0).all()
        assert (np.abs(sc[:, :V] - ref["log_probs"]) <= ref["lp_err"][:, None]).all(), (name, cur)
        assert (st.run_seq[:, :, :, L:] == PAD).all() and (st.fin_idx[:, :, :, L:] == -1).all()      # nothing beyond the search's columns
        # columns the search has not reached keep the fill in the half just written
        assert (got["running"][:, :, cur + 1:] == PAD).all() and (got["running_idx"][:, :, cur + 1:] == -1).all()
    assert compared >= 0.9 * total > 0, (compared, total)
    # a stopped search: whatever cur is, nothing moves
    if not bool(st.done[0].item()):
        st.done.copy_(torch.tensor([1, steps], dtype=torch.int32))
    for cur in (steps, steps + 1):
        _stopped_call_changes_nothing(st, logits, V, min(cur, L - 1), eos_ids, lp, es, L)


def test_exact_bf16_ties_across_the_keep_cut_follow_the_column_rule():
    V, nb, L = 1000, 2, 8
    vals = BR.case_logits(5, 0, nb, V, "bf16", [])
    top = float(np.sort(vals[0])[-1]) + 1.0
    tied = [911, 17, 500, 3, 640, 88, 250]                   # seven equal maxima, keep = 4: columns 3, 17, 88, 250 in this order
    vals[0, tied] = BR.to_dtype(np.float32(top), "bf16")
    st = G.BeamState(1, nb, GCAP, PAD, dev())
    ref = BR.step(vals, BR.fresh_state(1, nb, L, PAD), 0, nb, [], 1.0, False, L, PAD)
    assert ref["decidable"].all() and ref["running_decidable"].all()
    assert list(ref["next_tokens"]) == [3, 17]
    nxt, src = _call(st, _tensor(vals, 1024, "bf16"), V, 0, [], 1.0, False, L)
    assert list(nxt) == [3, 17] and list(src) == [0, 0]
    assert _compare(ref, _read(st, 1, L), nxt, src, None, 0, nb, "ties") == 1


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_plateau_wider_than_the_table_keeps_its_first_columns(dtype):
    """3000 columns at or above the keep-th value, kCap = 2048 slots: the ordered collection takes the one value above the plateau,
    then the plateau in ascending column order."""
    V, ld, nb, L = 3000, 3008, 2, 8
    vals = np.full((nb, V), 1.25, dtype=np.float32)
    vals[0, 2999] = vals[1, 5] = 2.5
    st = G.BeamState(1, nb, GCAP, PAD, dev())
    ref = BR.step(vals, BR.fresh_state(1, nb, L, PAD), 0, nb, [], 1.0, False, L, PAD)
    assert ref["decidable"].all() and ref["running_decidable"].all()
    assert list(ref["next_tokens"]) == [2999, 0] and list(ref["src_rows"]) == [0, 0]
    nxt, src = _call(st, _tensor(vals, ld, dtype), V, 0, [], 1.0, False, L)
    assert list(nxt) == [2999, 0] and list(src) == [0, 0]
    assert _compare(ref, _read(st, 1, L), nxt, src, None, 0, nb, "plateau " + dtype) == 1


def test_eos_enters_the_finished_slots_only_from_a_rank_below_nb():
    V, nb, L, eos = 257, 2, 8, 256
    vals = BR.case_logits(6, 0, 2 * nb, V, "f32", [])
    for row, rank in ((0, 0), (nb, 2)):                      # prompt 0: eos is the best candidate; prompt 1: the third (rank 2 >= nb)
        order = np.argsort(-vals[row])
        order = order[order != eos]
        vals[row, eos] = (vals[row, order[rank - 1]] + vals[row, order[rank]]) / np.float32(2) if rank else vals[row, order[0]] + np.float32(0.25)
        assert list(np.argsort(-vals[row])).index(eos) == rank
    st = G.BeamState(2, nb, GCAP, PAD, dev())
    ref = BR.step(vals, BR.fresh_state(2, nb, L, PAD), 0, nb, [eos], 1.0, False, L, PAD)
    assert ref["decidable"].all() and ref["running_decidable"].all()
    assert list(ref["state"]["is_finished"].reshape(-1)) == [True, False, False, False] and ref["state"]["sequences"][0, 0, 0] == eos
    nxt, src = _call(st, _tensor(vals, 320, "f32"), V, 0, [eos], 1.0, False, L)
    got = _read(st, 1, L)
    assert _compare(ref, got, nxt, src, None, 0, nb, "eos") == 2
    assert eos not in nxt and list(got["is_finished"].reshape(-1)) == [True, False, False, False]


@pytest.mark.parametrize("nb", [2, 5])
def test_rows_swap_between_beams_on_both_parities_and_repeat_bit_for_bit(nb):
    """Beam 0 continues from beam nb - 1 and beam nb - 1's old rank goes to beam 0's row: an in-place gather would read a row it has
    already overwritten.  The same state in half 0 at cur = 2 and in half 1 at cur = 3."""
    V, L, B0 = 257, 8, 3
    base = BR.fresh_state(B0, nb, L, PAD)
    rng = np.random.default_rng(8)
    for cur in (2, 3):
        s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        s["running"][:, :, :cur] = rng.integers(1, V - 1, (B0, nb, cur))
        s["running_idx"][:, :, :cur] = rng.integers(0, nb, (B0, nb, cur)) + (np.arange(B0) * nb)[:, None, None]
        s["running_scores"][:] = -1.0 - 3.0 * np.arange(nb)[::-1]               # the LAST beam scores best
        vals = BR.case_logits(9, cur, B0 * nb, V, "f32", [])
        for r in range(B0 * nb):
            vals[r, 10 + r] = vals[r].max() + np.float32(40.0)                   # one dominant column per row: a beam's second candidate is far below
        ref = BR.step(vals, s, cur, nb, [], 1.0, False, L, PAD)
        assert ref["decidable"].all() and ref["running_decidable"].all()
        assert list(ref["src_rows"][:nb]) == list(range(nb))[::-1]              # the rows reverse
        outs = []
        for _ in range(2):
            st = G.BeamState(B0, nb, GCAP, PAD, dev())
            _load(st, cur & 1, s)
            nxt, src = _call(st, _tensor(vals, 320, "f32"), V, cur, [], 1.0, False, L)
            assert _compare(ref, _read(st, (cur + 1) & 1, L), nxt, src, s, cur, nb, "swap") == B0
            outs.append((_snapshot(st), nxt, src))
        for k in TABLES:
            assert torch.equal(outs[0][0][k], outs[1][0][k]), k
        assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
