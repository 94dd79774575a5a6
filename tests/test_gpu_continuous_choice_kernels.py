"""p2t_sample_select_rows / p2t_logits_process_rows (csrc/sample_select.hip, csrc/logits_process.hip over csrc/row_model.h) through the C
ABI: with equal counters they are their lock-step twins bit for bit; with counters, limits, keys and a row map of their own they are
the numpy restatement (tests/continuous_choice_reference.py) -- tokens where the row is DECIDABLE (sampling_reference; the seed of each
case is the first of 0, 1, 2, ... for which every live row is, asserted, so nothing is skipped), processed rows bit for bit; and a
row's token and scores depend on its logits, key and counter alone.  f32 and bf16."""
import numpy as np
import pytest
import torch

import continuous_choice_reference as ccr
import logits_process_reference as lpr
import sampling_reference as SR
from gpu_util import dev, to_dev, to_np
from p2t_hip import synth

pytestmark = pytest.mark.gpu
G, LDT, SENT = 64, 72, -12352.0
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])


def make_logits(seed, rows, V, ld, dtype):
    """randn * 3 as stored in `dtype` (f32 values), NaN in columns V .. ld."""
    lg = (np.random.RandomState(seed).randn(rows, V) * 3).astype(np.float32)
    if dtype == BF16:
        lg = synth.bf16_round(lg)
    full = np.full((rows, ld), np.nan, dtype=np.float32)
    full[:, :V] = lg
    return full


def _i32(a):
    return to_dev(np.asarray(a, np.int32))


class State:
    """The engine's per-row arrays on the device, with sentinels around them: BB rows (+ 1 guard row) of out_tokens at pitch LDT > G."""

    def __init__(self, BB, row_step, row_limit=None, row_key=None, finished=None, out_tokens=None):
        self.BB = BB
        self.fin = _i32(np.zeros(BB) if finished is None else finished)
        self.nxt = torch.full((BB + 2,), -7, dtype=torch.int64, device=dev())
        tab = np.full((BB + 1, LDT), -1, np.int64)
        if out_tokens is not None:
            tab[:BB, :G] = out_tokens
        self.tab0 = tab
        self.out = to_dev(tab)
        self.row_step = _i32(row_step)
        self.row_limit = _i32(np.full(BB, G) if row_limit is None else row_limit)
        self.row_key = to_dev(np.asarray(np.arange(BB) if row_key is None else row_key, np.int64))

    def read(self):
        nx = to_np(self.nxt)
        assert nx[0] == -7 and nx[-1] == -7
        return dict(next=nx[1:-1], fin=to_np(self.fin), out=to_np(self.out))


def sample_rows(st, full, dtype, V, temperature, top_k, top_p, seed, row_map=None, eos=(), pad=0, scores=True, flags0=0):
    """One p2t_sample_select_rows call on `full` ([n, ld] f32 values stored as `dtype`) -> st.read() + scores [n, V] + flags; the guard
    regions of the scores are checked."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    n, ld = full.shape
    lgd = to_dev(full, dtype)
    eos_d = torch.tensor(list(eos), dtype=torch.int64, device=dev())
    lds = V + 5
    sc = torch.full((n + 1, lds), SENT, dtype=torch.float32, device=dev()) if scores else None
    flags = torch.tensor([flags0, 77], dtype=torch.int32, device=dev())
    rm = _i32(row_map) if row_map is not None else None
    _lib.call("p2t_sample_select_rows", ptr(lgd), ops.dt_of(dtype), ld, V, n, ptr(eos_d) if len(eos) else None, len(eos), pad, ptr(st.fin), ptr(st.nxt[1:]),
              ptr(st.out), LDT, ptr(st.row_step), ptr(st.row_limit), ptr(rm) if rm is not None else None, ptr(st.row_key), st.BB, G, float(temperature), top_k,
              float(top_p), seed, ptr(sc) if scores else None, lds, ptr(flags), stream())
    res = st.read()
    fl = to_np(flags)
    assert fl[1] == 77
    res["flags"] = int(fl[0])
    if scores:
        s = to_np(sc)
        assert (s[:n, V:] == SENT).all() and (s[n] == SENT).all()
        res["scores"] = s[:n, :V]
    return res


def sample_lock_step(full, dtype, V, temperature, top_k, top_p, seed, step, row0, eos=(), pad=0):
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    BB, ld = full.shape
    lgd = to_dev(full, dtype)
    eos_d = torch.tensor(list(eos), dtype=torch.int64, device=dev())
    fin, nxt = _i32(np.zeros(BB)), torch.zeros((BB,), dtype=torch.int64, device=dev())
    out = torch.full((BB, LDT), -1, dtype=torch.int64, device=dev())
    sc = torch.full((BB, V + 5), SENT, dtype=torch.float32, device=dev())
    flags, step_d = torch.zeros((1,), dtype=torch.int32, device=dev()), _i32([step])
    _lib.call("p2t_sample_select", ptr(lgd), ops.dt_of(dtype), ld, V, BB, ptr(eos_d) if len(eos) else None, len(eos), pad, ptr(fin), ptr(nxt), ptr(out), LDT,
              ptr(step_d), G, float(temperature), top_k, float(top_p), seed, row0, ptr(sc), V + 5, ptr(flags), stream())
    return dict(next=to_np(nxt), fin=to_np(fin), out=to_np(out), scores=to_np(sc)[:, :V], flags=int(flags.item()))


def _proc_args(proc):
    from p2t_hip.ops import ptr
    ids, off = lpr.pack_words(proc["words"])
    eos_d, ids_d, off_d = to_dev(np.asarray(proc["eos_ids"], np.int64)), to_dev(ids), to_dev(off)
    opt = lambda t: ptr(t) if t.numel() else None
    return (proc["penalty"], proc["ngram"], proc["min_new"], opt(eos_d), eos_d.numel(), opt(ids_d), opt(off_d), len(proc["words"]), ids_d.numel()), (eos_d, ids_d, off_d)


def process_rows(st, full, dtype, V, proc, row_map=None, finished=True, ld_out=None):
    """One p2t_logits_process_rows call -> the f32 output [n + 1, ld_out] as uint32, pre-filled with SENT."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    n, ld = full.shape
    ld_out = ld if ld_out is None else ld_out
    lgd = to_dev(full, dtype)
    out = torch.full((n + 1, ld_out), SENT, dtype=torch.float32, device=dev())
    rm = _i32(row_map) if row_map is not None else None
    args, keep = _proc_args(proc)
    _lib.call("p2t_logits_process_rows", ptr(lgd), ops.dt_of(dtype), ld, V, n, ptr(st.out), LDT, ptr(st.row_step), ptr(rm) if rm is not None else None,
              ptr(st.fin) if finished else None, st.BB, G, ptr(out), ld_out, *args, stream())
    assert np.array_equal(to_np(st.out), st.tab0)                    # the history is read, never written
    return to_np(out)


def process_lock_step(tab, full, dtype, V, proc, step, ld_out):
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    BB, ld = full.shape
    lgd, tab_d = to_dev(full, dtype), to_dev(tab)
    out = torch.full((BB + 1, ld_out), SENT, dtype=torch.float32, device=dev())
    args, keep = _proc_args(proc)
    _lib.call("p2t_logits_process", ptr(lgd), ops.dt_of(dtype), ld, V, BB, ptr(tab_d), LDT, ptr(_i32([step])), G, ptr(out), ld_out, *args, stream())
    return to_np(out)


# (V, ld, rows, top_k, top_p): the vector path, the scalar path, a table of 1024 ranks, both filters off, the real vocabulary
EQUAL = [(500, 512, 4, 50, 0.9), (1003, 1003, 4, 5, 0.5), (2051, 2051, 3, 1024, 1.0), (1003, 1003, 4, 0, 1.0), (128256, 128320, 2, 50, 0.9)]


@DTYPES
@pytest.mark.parametrize("case", EQUAL, ids=lambda c: f"V{c[0]}-ld{c[1]}-k{c[3]}-p{c[4]}")
def test_equal_counters_are_the_lock_step_sampler_bit_for_bit(case, dtype):
    """row_map NULL, no finished row, row_key[r] = row0 + r, every row_step = s: tokens, the eos bit, the written column and the scores of
    p2t_sample_select at step[0] = s.  Row 0's token is an eos id, so bit 0 is set somewhere; no limit is reached."""
    V, ld, BB, top_k, top_p = case
    s, row0, seed, temperature = 3, 5, 11, 0.7
    full = make_logits(V + BB, BB, V, ld, dtype)
    first = sample_lock_step(full, dtype, V, temperature, top_k, top_p, seed, s, row0)
    eos = (int(first["next"][0]), V + 9)
    lock = sample_lock_step(full, dtype, V, temperature, top_k, top_p, seed, s, row0, eos=eos, pad=4242)
    assert lock["fin"][0] == 1 and np.array_equal(lock["next"], first["next"])
    st = State(BB, np.full(BB, s), row_key=row0 + np.arange(BB))
    got = sample_rows(st, full, dtype, V, temperature, top_k, top_p, seed, eos=eos, pad=4242)
    assert np.array_equal(got["next"], lock["next"]) and np.array_equal(got["fin"] & 1, lock["fin"]) and not (got["fin"] & 2).any()
    assert np.array_equal(got["out"][:BB], lock["out"]) and (got["out"][BB] == -1).all()
    assert np.array_equal(got["scores"].view(np.uint32), lock["scores"].view(np.uint32)) and got["flags"] == lock["flags"] == 0
    # the counter is the draw's: another s draws another number (the tokens of 2 .. 4 rows all staying equal over 3 more steps is ~ impossible)
    other = [sample_rows(State(BB, np.full(BB, t), row_key=row0 + np.arange(BB)), full, dtype, V, temperature, top_k, top_p, seed)["next"] for t in (4, 5, 6)]
    assert any(not np.array_equal(o, got["next"]) for o in other)


@DTYPES
@pytest.mark.parametrize("case", [c[:3] for c in EQUAL if c[3] > 0], ids=lambda c: f"V{c[0]}-ld{c[1]}")
def test_equal_counters_are_the_lock_step_processors_bit_for_bit(case, dtype):
    """row_map NULL, finished all zero or NULL, every row_step = s: p2t_logits_process's rows at step[0] = s as uint32, guard columns and
    guard row included, and both equal the numpy restatement."""
    V, ld, BB = case
    s = 9
    rs = np.random.RandomState(V)
    full = make_logits(V, BB, V, ld, dtype)
    tab = np.full((BB + 1, LDT), -1, np.int64)
    tab[:BB, :G] = rs.randint(0, min(V, 12), (BB, G))             # few distinct tokens: repeats, bi-grams that recur
    last = int(tab[0, s - 1])
    proc = dict(penalty=1.3, ngram=2, min_new=12, eos_ids=[7, V - 1], words=[[3], [last, 4], [V + 3]])
    ld_out = ld + (4 if ld % 4 == 0 else 1)
    lock = process_lock_step(tab, full, dtype, V, proc, s, ld_out)
    st = State(BB, np.full(BB, s), out_tokens=tab[:BB, :G])
    for fin in (True, False):                                        # finished all zero, and NULL
        got = process_rows(st, full, dtype, V, proc, finished=fin, ld_out=ld_out)
        assert np.array_equal(got.view(np.uint32), lock.view(np.uint32))
    ref = lpr.process(full[:, :V], [tab[r, :s] for r in range(BB)], **proc)
    assert np.array_equal(lock[:BB, :V].view(np.uint32), ref.view(np.uint32)) and (lock[:BB, V:] == SENT).all() and (lock[BB] == SENT).all()
    assert np.isinf(ref[0, 4]) and np.isinf(ref[:, [7, V - 1, 3]]).all()


# ---- rows of their own ---------------------------------------------------------------------------------------------------------------
BB6, ROW_MAP = 6, [4, 0, 9, 2, 5]                                    # logits row 2 names a row the engine does not have; row 3 -> the finished row 2
STEPS = np.array([3, 11, 7, 20, 0, G - 1], np.int32)                 # engine rows 0 .. 5: the live ones are 4 (step 0), 0 (3), 5 (G - 1)
LIMITS = np.array([4, 30, 30, 30, 10, G], np.int32)                  # row 0 reaches its limit at step 3, row 5 at G - 1
KEYS = np.array([-17, 1, 2, 3, 2 ** 40 + 123, 2 ** 62 + 5], np.int64)
LIVE = {0: 4, 1: 0, 4: 5}                                            # logits row -> engine row
SAMPLER = dict(temperature=0.8, top_k=8, top_p=0.9)


def _own_rows_case(seed, V, ld, dtype):
    full = make_logits(1000 + seed, 5, V, ld, dtype)
    full[3, :V] = np.nan                                             # the finished row's logits are never read
    us = {i: synth.sample_uniform(seed, int(KEYS[r]), int(STEPS[r])) for i, r in LIVE.items()}
    return full, {i: SR.sample_row(full[i, :V], u=us[i], **SAMPLER) for i in LIVE}


def _first_decidable_seed(V, ld, dtype):
    for seed in range(64):
        full, refs = _own_rows_case(seed, V, ld, dtype)
        if all(r["decidable"] for r in refs.values()):
            return seed, full, refs
    raise AssertionError("no seed below 64 makes every live row decidable")


@DTYPES
@pytest.mark.parametrize("V,ld", [(1003, 1003), (500, 512)], ids=["scalar", "vector"])
def test_own_rows_sampler_vs_the_restatement(V, ld, dtype):
    """BB = 6, n = 5 through a row map with one entry out of range; engine row 2 is finished (its logits row is NaN, its scores row must
    keep the sentinel, its out_tokens and flag stay), rows 1 and 3 are not named at all.  Counters 0, 3 and G - 1, limits reached on two
    rows, an eos drawn on the third, keys beyond 2^40 and a negative one: a key or counter cut to 32 bits, or the launch index in the
    key's place, draws another number."""
    seed, full, refs = _first_decidable_seed(V, ld, dtype)
    assert all(r["decidable"] for r in refs.values())
    fin0 = np.array([0, 0, 1, 0, 0, 0], np.int32)
    eos, pad = (refs[0]["token"], V + 3), 4242                       # logits row 0 (engine row 4) draws an eos id
    tab = np.random.RandomState(3).randint(0, V, (BB6, G)).astype(np.int64)
    st = State(BB6, STEPS, LIMITS, KEYS, fin0, tab)
    got = sample_rows(st, full, dtype, V, seed=seed, row_map=ROW_MAP, eos=eos, pad=pad, **SAMPLER)
    want = dict(fin=fin0.copy(), next=np.full(BB6, -7, np.int64), out=tab.copy(), scores=np.full((5, V), SENT, np.float32))
    res = ccr.sample_select_rows(full, V, want["fin"], want["next"], want["out"], STEPS, LIMITS, KEYS, eos, pad, SAMPLER["temperature"], SAMPLER["top_k"],
                                 SAMPLER["top_p"], seed, row_map=ROW_MAP, scores=want["scores"])
    assert sorted(res) == sorted(LIVE) and all(res[i]["token"] == refs[i]["token"] for i in LIVE)
    assert want["fin"][4] & 1 and want["fin"][0] & 2 and want["fin"][5] & 2 and want["fin"][[1, 2, 3]].tolist() == [0, 1, 0] and want["next"][2] == pad
    assert np.array_equal(got["next"], want["next"]) and np.array_equal(got["fin"], want["fin"])
    assert np.array_equal(got["out"][:BB6, :G], want["out"]) and (got["out"][:, G:] == -1).all() and (got["out"][BB6] == -1).all()
    for i in range(5):
        if i not in LIVE:
            assert (got["scores"][i] == SENT).all(), i               # the row out of range and the finished row: not a byte
            continue
        kept = np.nonzero(got["scores"][i] != -np.inf)[0]
        assert np.array_equal(kept, refs[i]["kept"]), i
        assert np.array_equal(got["scores"][i].view(np.uint32), want["scores"][i].view(np.uint32)), i      # x = logit / temperature: one f32 division
    assert got["flags"] == 0
    # what a 32-bit key, the slot or the launch index would have drawn differs from the 64-bit draw, so the equality above tells them apart
    for i, r in LIVE.items():
        u = synth.sample_uniform(seed, int(KEYS[r]), int(STEPS[r]))
        assert all(u != synth.sample_uniform(seed, k, int(STEPS[r])) for k in (int(KEYS[r]) & 0xFFFFFFFF, r, i) if k != int(KEYS[r]))


@DTYPES
@pytest.mark.parametrize("V,ld", [(1003, 1003), (500, 512)], ids=["scalar", "vector"])
def test_own_rows_processors_vs_the_restatement(V, ld, dtype):
    """The same rows: histories of 0, 3 and G - 1 tokens read from each row's OWN table row, a bi-gram and a two-token bad word that fire
    on the row at step 3 only, min_new_tokens = 2 active at step 0 and not at 3; processed rows equal the numpy restatement bit for bit,
    the finished row's and the out-of-range row's output rows keep their bytes."""
    full = make_logits(77, 5, V, ld, dtype)
    full[3, :V] = np.nan
    tab = np.zeros((BB6, G), np.int64)
    for r in range(BB6):
        tab[r] = 100 + r + 6 * np.arange(G)                          # all different, row by row: no bi-gram recurs, no word matches
    tab[0, :3] = [21, 33, 21]                                        # engine row 0 (logits row 1) at step 3: (21, 33) bans 33, the word [21, 40] bans 40
    tab[2, :7] = [21, 33, 21, 33, 21, 33, 21]                        # the finished row's history would fire too: it must not be processed
    proc = dict(penalty=1.25, ngram=2, min_new=2, eos_ids=[5, 6], words=[[21, 40], [V + 1]])
    fin0 = np.array([0, 0, 1, 0, 0, 0], np.int32)
    st = State(BB6, STEPS, LIMITS, KEYS, fin0, tab)
    got = process_rows(st, full, dtype, V, proc, row_map=ROW_MAP)
    want = np.full((6, ld), SENT, np.float32)
    ccr.logits_process_rows(full, V, tab, STEPS, want, row_map=ROW_MAP, finished=fin0, **proc)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (want[[2, 3, 5]] == SENT).all() and not (want[[0, 1, 4], :V] == SENT).any()
    ninf = {i: np.nonzero(np.isinf(want[i, :V]) & ~np.isinf(full[i, :V]))[0].tolist() for i in LIVE}
    assert ninf == {0: [5, 6], 1: [33, 40], 4: []}                   # min_new at step 0; the bi-gram and the word at step 3; nothing at G - 1
    moved = {i: int((want[i, :V] != full[i, :V]).sum()) for i in LIVE}
    assert moved[0] == 2 and moved[1] == 3 and moved[4] == G - 1         # + the penalty on each row's own distinct tokens (21 and 33 at step 3)
    # finished = NULL: the finished row is processed like any other (its NaN logits go through), nothing else changes
    got2 = process_rows(st, full, dtype, V, proc, row_map=ROW_MAP, finished=False)
    assert np.array_equal(np.delete(got2, 3, 0).view(np.uint32), np.delete(want, 3, 0).view(np.uint32)) and np.isnan(got2[3, :V]).sum() >= V - 8


@DTYPES
@pytest.mark.parametrize("top_k,top_p", [(8, 0.9), (0, 1.0)], ids=["filtered", "unfiltered"])
def test_a_rows_choice_depends_on_its_logits_key_and_counter_alone(top_k, top_p, dtype):
    """The same logits row under the same key and counter as row 1 of 3 (no map) and as logits row 0 of 2 mapped to engine row 6 of 7,
    beside other rows and other keys: the same token, the same score row bit for bit, written at the same column of ITS row."""
    V, ld, key, step, seed = 1003, 1003, 2 ** 45 + 9, 5, 31
    row = make_logits(8, 1, V, ld, dtype)[0]
    a_full = make_logits(9, 3, V, ld, dtype)
    a_full[1] = row
    a = sample_rows(State(3, [2, step, 9], row_key=[4, key, -3]), a_full, dtype, V, 0.8, top_k, top_p, seed)
    b_full = make_logits(10, 2, V, ld, dtype)
    b_full[0] = row
    b_st = State(7, [0, 1, 2, 3, 4, 6, step], row_key=[0, 1, 2, 3, 4, 5, key])
    b = sample_rows(b_st, b_full, dtype, V, 0.8, top_k, top_p, seed, row_map=[6, 2])
    assert a["next"][1] == b["next"][6] == a["out"][1, step] == b["out"][6, step] and 0 <= a["next"][1] < V
    assert np.array_equal(a["scores"][1].view(np.uint32), b["scores"][0].view(np.uint32))
    assert (np.delete(b["out"][6], step) == -1).all() and (b["out"][[0, 1, 3, 4, 5]] == -1).all() and b["next"][[0, 1, 3, 4, 5]].tolist() == [-7] * 5
