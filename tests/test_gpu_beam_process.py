"""The logits processors under beam search at kernel level: p2t_beam_logprobs_process (csrc/beam_process.hip) and
p2t_beam_select_logprobs (csrc/beam_select.hip), bit for bit.
Entry 1 is held to tests/logits_process_reference.py applied to lp0, the `scores` rows the EXISTING p2t_beam_select writes for the same
logits on a scratch state (step 1 of its contract, which the new kernel must reproduce bit for bit), with the histories the loaded
state holds in half cur & 1.  Entry 2 and the chain are held to tests/beam_logprobs_reference.py (numpy f32) on the rows entry 1
left: tokens, src_rows, every table of the written half, flags and done, no margins, nothing skipped.
Shapes: V = 67 (scalar path, unaligned ld and ld_lp), V = 4099 with ld = 4104 (16-byte path + scalar tail), V = 128256 with six rows (a
second round of the unrolled pass); f32 and bf16; nb 2, 3 and 5; 0, 1 and 2 eos ids; G = 64 and one case with G = 1152, cur = 1100
(a history longer than the block)."""
import numpy as np
import pytest
import torch

import beam_logprobs_reference as BL
import beam_reference as BR
import logits_process_reference as LR
from gpu_util import SENT, dev, to_dev, to_np
from p2t_hip import generation as G
from test_gpu_beam_select import TABLES, _load, _read, _snapshot, _tensor

pytestmark = pytest.mark.gpu
PAD = 0


def _alphabet(V):
    return [1, 4, 9, V // 2, V - 2, V - 1]


def _setting(V, which):
    a = _alphabet(V)
    words = [[a[1], a[2], a[3]], [21], [a[0], V + 1], [a[4], a[4]]]          # a 3-token word, a suppressed id, a last token that names no column
    full = dict(penalty=1.3, ngram=2, min_new=7, eos_ids=[V - 1, 7], words=words)
    return {"penalty": dict(penalty=1.3), "ngram1": dict(ngram=1), "ngram2": dict(ngram=2), "ngram3": dict(ngram=3), "words": dict(words=words),
            "min_new": dict(min_new=7, eos_ids=[V - 1, 7]), "all": full, "all-n3": dict(full, ngram=3, penalty=0.8)}[which]


def _state(B0, nb, L, cur, V, seed, finished=True):
    """A search in mid-flight at `cur` (tests/beam_reference.py's layout) and the tokens the OTHER half of run_seq is filled with."""
    rng = np.random.default_rng([seed, B0, nb, cur, V])
    a = np.array(_alphabet(V), dtype=np.int64)
    s = BR.fresh_state(B0, nb, L, PAD)
    other = a[rng.integers(0, len(a), (B0, nb, L))]
    if cur > 0:
        s["running"][:, :, :cur] = a[rng.integers(0, len(a), (B0, nb, cur))]
        s["running_idx"][:, :, :cur] = rng.integers(0, nb, (B0, nb, cur)) + (np.arange(B0) * nb)[:, None, None]
        s["running_scores"][:] = (-1.0 - 0.37 * np.arange(nb)[None, :] - rng.random((B0, nb))).astype(np.float32)
        if cur >= 2:
            s["running"][0, 0, 1] = V                                       # an id equal to V: compared like any other, never written to
            s["running"][0, nb - 1, 1:min(3, cur)] = a[1:min(3, cur)]       # the 3-token word's first two tokens: applies from cur = 3 on
            s["running"][-1, 0, :cur] = np.resize(a[[1, 2]], cur)           # a repeated 2- and 3-gram, and a token many times over
            if finished:
                s["is_finished"][0, 0], s["beam_scores"][0, 0] = True, np.float32(-2.5)
                s["sequences"][0, 0, :2], s["beam_idx"][0, 0, :2] = [5, V - 1], [0, 1]
    return s, other


def _put(B0, nb, Gcap, L, cur, s, other):
    st = G.BeamState(B0, nb, Gcap, PAD, dev())
    _load(st, cur & 1, s)
    st.run_seq[(cur + 1) & 1, :, :, :L].copy_(torch.from_numpy(other))
    return st


def _lp0(logits, V, B0, nb):
    """The rows p2t_beam_select writes as `scores` for these logits (a fresh scratch state, step 0)."""
    st = G.BeamState(B0, nb, 64, PAD, dev())
    sc = torch.zeros((B0 * nb, V), dtype=torch.float32, device=dev())
    z = lambda: torch.zeros((B0 * nb,), dtype=torch.int64, device=dev())
    G.beam_select(logits, V, st, torch.zeros((0,), dtype=torch.int64, device=dev()), PAD, 1.0, False, 64, torch.zeros((1,), dtype=torch.int32,
                  device=dev()), z(), z(), sc)
    return to_np(sc)


def _lp_buffer(BB, V, ld_lp):
    flat = torch.full((BB * ld_lp + 8,), SENT, dtype=torch.float32, device=dev())
    return flat, flat[: BB * ld_lp].view(BB, ld_lp)


def _process(logits, V, st, cur, L, s, lp):
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    import ctypes as C
    ids, offs = LR.pack_words(s.get("words", []))
    eos = np.array(s.get("eos_ids", []), dtype=np.int64)
    ids_d, offs_d, eos_d = to_dev(ids), to_dev(offs), to_dev(eos)
    step = torch.tensor([cur], dtype=torch.int32, device=dev())
    opt = lambda t: ptr(t) if t.numel() else None
    _lib.call("p2t_beam_logprobs_process", ptr(logits), ops.dt_of(logits), logits.stride(0), st.B, st.nb, V, ptr(step), st.G, L, C.byref(st.c),
              float(s.get("penalty", 1.0)), int(s.get("ngram", 0)), int(s.get("min_new", 0)), opt(eos_d), eos.size, opt(ids_d),
              ptr(offs_d) if len(ids) else None, len(offs) - 1 if len(ids) else 0, len(ids), ptr(lp), lp.stride(0), stream())
    torch.cuda.synchronize()


def _select(lp, V, st, cur, eos_ids, lp_pen, es, L):
    BB = st.B * st.nb
    step = torch.tensor([cur], dtype=torch.int32, device=dev())
    nxt = torch.full((BB,), -7, dtype=torch.int64, device=dev())
    src = torch.full((BB,), -7, dtype=torch.int64, device=dev())
    G.beam_select_logprobs(lp, V, st, torch.tensor(eos_ids, dtype=torch.int64, device=dev()), PAD, lp_pen, es, L, step, nxt, src)
    torch.cuda.synchronize()
    return to_np(nxt), to_np(src)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else np.ascontiguousarray(a)


def _assert_state(got, want, cur, ctx):
    """Every table of the written half, bit for bit (columns 0 .. cur: a step writes no further)."""
    for k in ("running", "running_idx", "sequences", "beam_idx"):
        assert np.array_equal(got[k][:, :, :cur + 1], want[k][:, :, :cur + 1]), (ctx, k)
    for k in ("running_scores", "beam_scores"):
        assert np.array_equal(_bits(got[k]), _bits(want[k].astype(np.float32))), (ctx, k, got[k], want[k])
    for k in ("is_finished", "heuristic_open"):
        assert np.array_equal(got[k], want[k]), (ctx, k)
    assert got["done"] == want["done"] and (not want["done"] or got["steps"] == want["steps"]), ctx


def _histories(s, cur):
    B0, nb, L = s["running"].shape
    return [s["running"].reshape(B0 * nb, L)[r, :cur] for r in range(B0 * nb)]


# (V, ld, ld_lp, B0, nb, n_eos, the step counters, the settings)
SMALL = ("penalty", "ngram1", "ngram2", "ngram3", "words", "min_new", "all", "all-n3")
SHAPES = {
    "v67-scalar": (67, 67, 71, 2, 2, 0, (0, 1, 2, 3, 6, 7), SMALL),
    "v4099-vec+tail": (4099, 4104, 4104, 2, 5, 2, (0, 1, 2, 3, 6, 7), SMALL),
    "v4099-out-unaligned": (4099, 4104, 4101, 1, 2, 1, (3, 6), ("all",)),
    "v128256-two-rounds": (128256, 128256, 128260, 2, 3, 1, (0, 7), ("all",)),
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_both_entry_points_bit_for_bit(shape, dtype):
    V, ld, ld_lp, B0, nb, n_eos, curs, settings = SHAPES[shape]
    BB, L, Gcap = B0 * nb, 40, 64
    eos_ids = BR.case_eos(V, n_eos)
    vals = BR.case_logits(41, 0, BB, V, dtype, eos_ids)
    logits = _tensor(vals, ld, dtype)
    before_logits = logits.clone()
    lp0 = _lp0(logits, V, B0, nb)
    changed = halves_differ = 0
    for which in settings:
        s = _setting(V, which)
        for cur in curs:
            state, other = _state(B0, nb, L, cur, V, 3)
            st = _put(B0, nb, Gcap, L, cur, state, other)
            flat, lp = _lp_buffer(BB, V, ld_lp)
            _process(logits, V, st, cur, L, s, lp)
            got = to_np(lp)
            want = LR.process(lp0, _histories(state, cur), **s)
            assert np.array_equal(got[:, :V].view(np.uint32), want.view(np.uint32)), (shape, which, cur)
            assert (got[:, V:] == SENT).all() and (to_np(flat)[BB * ld_lp:] == SENT).all(), (shape, which, cur)      # column V keeps its sentinel
            wrong_half = LR.process(lp0, [other.reshape(BB, L)[r, :cur] for r in range(BB)], **s)
            halves_differ += int(not np.array_equal(wrong_half.view(np.uint32), want.view(np.uint32)))
            changed += int((want.view(np.uint32) != lp0.view(np.uint32)).sum())
            flat2, lp2 = _lp_buffer(BB, V, ld_lp)
            _process(logits, V, st, cur, L, s, lp2)
            assert torch.equal(flat.view(torch.int32), flat2.view(torch.int32)), (shape, which, cur)
            # entry 2 on the rows entry 1 left
            ref = BL.step(np.ascontiguousarray(got[:, :V]), state, cur, nb, eos_ids, 0.8, False, L, PAD)
            untouched = st.run_seq[(cur + 1) & 1, :, :, cur + 1:].clone()
            nxt, src = _select(lp, V, st, cur, eos_ids, 0.8, False, L)
            assert np.array_equal(nxt, ref["next_tokens"]) and np.array_equal(src, ref["src_rows"]), (shape, which, cur)
            _assert_state(_read(st, (cur + 1) & 1, L), ref["state"], cur, (shape, which, cur))
            assert torch.equal(st.run_seq[(cur + 1) & 1, :, :, cur + 1:], untouched)                  # no step writes past its own column
            assert torch.equal(lp, lp2)                                                               # the rows are never written by entry 2
    assert changed > 0 and halves_differ > 0                       # the settings bit, and the wrong half of run_seq would have shown
    assert torch.equal(logits.view(torch.int16 if dtype == "bf16" else torch.int32), before_logits.view(torch.int16 if dtype == "bf16" else torch.int32))


def test_the_two_halves_give_different_rows_and_min_new_ends_at_its_step():
    """The witnesses of the histories on the CPU side of the case above: what the planted tokens do to the expected rows."""
    V, B0, nb, L = 67, 2, 2, 40
    lp0 = BL.log_softmax_f32(BR.case_logits(41, 0, B0 * nb, V, "f32", []))
    a = _alphabet(V)
    for cur in (1, 6, 7):
        state, other = _state(B0, nb, L, cur, V, 3)
        s = _setting(V, "all")
        here = LR.process(lp0, _histories(state, cur), **s)
        there = LR.process(lp0, [other.reshape(B0 * nb, L)[r, :cur] for r in range(B0 * nb)], **s)
        assert not np.array_equal(here.view(np.uint32), there.view(np.uint32)), cur
        assert np.isneginf(here[:, [V - 1, 7]]).all() == (cur < 7)                      # both eos ids banned below min_new_tokens = 7 only
        assert np.isneginf(here[:, 21]).all()                                          # the suppressed id
    s2, _ = _state(B0, nb, L, 2, V, 3)
    s3, _ = _state(B0, nb, L, 3, V, 3)
    w = dict(words=_setting(V, "words")["words"])
    row = nb - 1                                                                       # prompt 0, last beam: history [.., a1, a2]
    assert not np.isneginf(LR.process(lp0, _histories(s2, 2), **w)[row, a[3]])         # cur = 2: the 3-token word is longer than the context
    assert np.isneginf(LR.process(lp0, _histories(s3, 3), **w)[row, a[3]])             # cur = 3: it applies
    s6, _ = _state(B0, nb, L, 6, V, 3)
    rep = LR.process(lp0, _histories(s6, 6), penalty=1.3)[B0 * nb - nb]                # the row whose history repeats a1, a2 three times each
    assert rep[a[1]] == lp0[B0 * nb - nb, a[1]] * np.float32(1.3)                      # penalised once, however often it occurs


def test_history_longer_than_the_block():
    V, ld, B0, nb, Gcap, L, cur = 4099, 4104, 1, 2, 1152, 1152, 1100
    vals = BR.case_logits(43, 0, nb, V, "bf16", [])
    logits = _tensor(vals, ld, "bf16")
    lp0 = _lp0(logits, V, B0, nb)
    rng = np.random.default_rng(5)
    state, other = _state(B0, nb, L, cur, V, 4, finished=False)
    state["running"][:, :, :cur] = rng.integers(0, V, (B0, nb, cur))
    state["running"][0, 0, 1050] = state["running"][0, 0, cur - 1]                     # the last token occurred before, beyond index 1024
    s = dict(penalty=1.3, ngram=2)
    st = _put(B0, nb, Gcap, L, cur, state, other)
    flat, lp = _lp_buffer(nb, V, ld)
    _process(logits, V, st, cur, L, s, lp)
    want = LR.process(lp0, _histories(state, cur), **s)
    assert np.isneginf(want[0, state["running"][0, 0, 1051]])
    assert np.array_equal(to_np(lp)[:, :V].view(np.uint32), want.view(np.uint32))
    ref = BL.step(want, state, cur, nb, [], 1.0, False, L, PAD)
    nxt, src = _select(lp, V, st, cur, [], 1.0, False, L)
    assert np.array_equal(nxt, ref["next_tokens"]) and np.array_equal(src, ref["src_rows"])
    _assert_state(_read(st, (cur + 1) & 1, L), ref["state"], cur, "long")


def test_a_penalised_top_token_leaves_the_candidates():
    """The raw top-1 of beam 0 is in its history; with penalty 3 it ends below rank keep = 4, so the `keep` best STORED logits are the
    wrong candidate set: the selection has to rank the processed row."""
    V, ld, B0, nb, L, cur = 257, 320, 1, 2, 8, 2
    vals = BR.case_logits(44, 0, nb, V, "f32", [])
    order = np.argsort(-vals[0])
    vals[0, order[:6]] = np.float32(9.0) - np.float32(0.1) * np.arange(6, dtype=np.float32)          # 9.0, 8.9, ..: the top six close together
    top = int(order[0])
    logits = _tensor(vals, ld, "f32")
    state, other = _state(B0, nb, L, cur, V, 6, finished=False)
    state["running"][0, 0, :cur] = [top, 3]
    st = _put(B0, nb, 64, L, cur, state, other)
    flat, lp = _lp_buffer(nb, V, ld)
    _process(logits, V, st, cur, L, dict(penalty=3.0), lp)
    got = np.ascontiguousarray(to_np(lp)[:, :V])
    lp0 = _lp0(logits, V, B0, nb)
    assert np.array_equal(got.view(np.uint32), LR.process(lp0, _histories(state, cur), penalty=3.0).view(np.uint32))
    ref, raw = (BL.step(x, state, cur, nb, [], 1.0, False, L, PAD) for x in (got, lp0))
    assert np.argmax(lp0[0]) == top and top in raw["cand_tokens"][0] and top not in ref["cand_tokens"][0]
    assert (np.argsort(-got[0], kind="stable")[:4] != top).all()                       # below rank keep inside its own beam
    assert not np.array_equal(ref["cand_tokens"], raw["cand_tokens"])
    nxt, src = _select(lp, V, st, cur, [], 1.0, False, L)
    assert np.array_equal(nxt, ref["next_tokens"]) and np.array_equal(src, ref["src_rows"]) and top not in nxt
    _assert_state(_read(st, (cur + 1) & 1, L), ref["state"], cur, "penalised top")


@pytest.mark.parametrize("nb,n_eos,n_suppressed", [(1, 3, 64), (2, 0, 66)])
def test_fewer_finite_values_than_keep(nb, n_eos, n_suppressed):
    """V = 67 with all but a few ids suppressed and keep = 4: the -inf columns rank by column, no NaN arises, every index stays in range."""
    V, ld, B0, L, cur = 67, 67, 2, 8, 0
    eos_ids = [2, 3, 5][:n_eos]
    vals = BR.case_logits(45, 0, B0 * nb, V, "f32", [])
    finite = [30, 11, 50][: V - n_suppressed]
    s = dict(words=[[t] for t in range(V) if t not in finite])
    logits = _tensor(vals, ld, "f32")
    state, other = _state(B0, nb, L, cur, V, 7)
    st = _put(B0, nb, 64, L, cur, state, other)
    flat, lp = _lp_buffer(B0 * nb, V, 71)
    _process(logits, V, st, cur, L, s, lp)
    got = np.ascontiguousarray(to_np(lp)[:, :V])
    assert np.array_equal(got.view(np.uint32), LR.process(_lp0(logits, V, B0, nb), _histories(state, cur), **s).view(np.uint32))
    assert (np.isfinite(got).sum(axis=1) == len(finite)).all()
    ref = BL.step(got, state, cur, nb, eos_ids, 1.0, False, L, PAD)
    keep = max(2, 1 + n_eos) * nb
    assert np.isfinite(ref["cand_acc"]).sum(axis=1).max() < keep
    banned = [t for t in range(V) if t not in finite]
    for b in range(B0):                                                                # the -inf candidates of beam 0 come in column order
        inf_tok = ref["cand_tokens"][b][np.isneginf(ref["cand_acc"][b]) & (ref["cand_beams"][b] == 0)]
        assert list(inf_tok) == banned[: len(inf_tok)] and len(inf_tok) > 0
    nxt, src = _select(lp, V, st, cur, eos_ids, 1.0, False, L)
    assert np.array_equal(nxt, ref["next_tokens"]) and np.array_equal(src, ref["src_rows"])
    g = _read(st, 1, L)
    _assert_state(g, ref["state"], cur, "few finite")
    assert not np.isnan(g["running_scores"]).any() and not np.isnan(g["beam_scores"]).any()
    assert ((nxt >= 0) & (nxt < V)).all() and ((src >= 0) & (src < B0 * nb)).all()
    assert ((g["running"][:, :, 0] >= 0) & (g["running"][:, :, 0] < V)).all()


def test_done_leaves_the_rows_and_the_state_alone():
    V, ld, B0, nb, L, cur = 67, 67, 2, 2, 8, 3
    logits = _tensor(BR.case_logits(46, 0, B0 * nb, V, "f32", []), ld, "f32")
    state, other = _state(B0, nb, L, cur, V, 8)
    for stopped, step in ((True, cur), (False, L), (False, -1)):                       # done set; cur outside [0, max_length)
        st = _put(B0, nb, 64, L, cur, state, other)
        if stopped:
            st.done.copy_(torch.tensor([1, cur], dtype=torch.int32))
        snap = _snapshot(st)
        flat, lp = _lp_buffer(B0 * nb, V, 71)
        _process(logits, V, st, step, L, _setting(V, "all"), lp)
        assert (to_np(flat) == SENT).all()
        nxt, src = _select(lp, V, st, step, [7], 1.0, False, L)
        assert (nxt == PAD).all() and np.array_equal(src, np.arange(B0 * nb))
        for k, v in snap.items():
            assert torch.equal(getattr(st, k), v), k


def _chain(seed, steps=6, device=True):
    """A 6-step chain, nb = 3: every step is fed the state the kernels left (on the CPU: the restatement's, on numpy log-softmax rows)."""
    V, ld, B0, nb, L = 257, 320, 2, 3, 8
    eos_ids, s = [V - 1], dict(penalty=1.3, ngram=2, min_new=2, eos_ids=[V - 1], words=[[21], [4, 9]])
    st = G.BeamState(B0, nb, 64, PAD, dev()) if device else None
    state, swaps, trace = BR.fresh_state(B0, nb, L, PAD), set(), []
    for cur in range(steps):
        vals = BR.case_logits(seed, cur, B0 * nb, V, "f32", eos_ids)
        vals[:, 1:9] += np.float32(5.0)                                                # a narrow alphabet: the histories repeat
        if device:
            before = _read(st, cur & 1, L)
            assert not before["done"]
            flat, lp = _lp_buffer(B0 * nb, V, ld)
            logits = _tensor(vals, ld, "f32")
            _process(logits, V, st, cur, L, s, lp)
            rows = np.ascontiguousarray(to_np(lp)[:, :V])
            assert np.array_equal(rows.view(np.uint32), LR.process(_lp0(logits, V, B0, nb), _histories(before, cur), **s).view(np.uint32)), cur
            ref = BL.step(rows, before, cur, nb, eos_ids, 1.0, False, L, PAD)
            nxt, src = _select(lp, V, st, cur, eos_ids, 1.0, False, L)
            assert np.array_equal(nxt, ref["next_tokens"]) and np.array_equal(src, ref["src_rows"]), cur
            _assert_state(_read(st, (cur + 1) & 1, L), ref["state"], cur, ("chain", cur))
            trace.append((rows.copy(), nxt, src, _snapshot(st)))
        else:
            rows = LR.process(BL.log_softmax_f32(vals), _histories(state, cur), **s)
            ref = BL.step(rows, state, cur, nb, eos_ids, 1.0, False, L, PAD)
            state = ref["state"]
        if not np.array_equal(ref["src_rows"], np.arange(B0 * nb)):
            swaps.add(cur & 1)
        if ref["state"]["done"]:
            break
    return swaps, trace, cur


def test_chain_of_six_steps_repeats_bit_for_bit():
    swaps, first, last = _chain(47)
    assert swaps == {0, 1} and last == 5                          # rows moved between beams on both parities, over all six steps
    _, second, _ = _chain(47)
    for (r1, n1, s1, t1), (r2, n2, s2, t2) in zip(first, second):
        assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32)) and np.array_equal(n1, n2) and np.array_equal(s1, s2)
        for k in TABLES:
            assert torch.equal(t1[k], t2[k]), k
