"""p2t_sample_select (csrc/sample_select.hip) through the C ABI against its fp64 restatement (tests/sampling_reference.py): the kept set
and the processed scores, the token for the draw the host restates (p2t_hip.synth.sample_uniform), the finished / pad / eos
bookkeeping of the greedy kernel, the table's capacity rule, the unfiltered form, the draw's statistics and bit-for-bit repeats.

Where a comparison of tokens or kept sets is made, the rows are first asserted DECIDABLE (sampling_reference: both of the row's
thresholds further than the f32 summation error from the fp64 value); no row of a sweep is skipped -- the seeds below were chosen so
that every row is.  bf16 rows carry ties at the k-th value and across the top-p cut: there the kernel's own order (value descending,
column ascending) is what is checked."""
import numpy as np
import pytest
import torch

import sampling_reference as SR
from gpu_util import dev, to_dev, to_np
from p2t_hip import synth

pytestmark = pytest.mark.gpu
G, SENT = 64, -12352.0
F32, BF16 = torch.float32, torch.bfloat16


def make_logits(seed, BB, V, ld, dtype):
    """randn * 3 as stored in `dtype` (f32 values), NaN in columns V .. ld."""
    lg = (np.random.RandomState(seed).randn(BB, V) * 3).astype(np.float32)
    if dtype == BF16:
        lg = synth.bf16_round(lg)
    full = np.full((BB, ld), np.nan, dtype=np.float32)
    full[:, :V] = lg
    return full


def run(full, dtype, V, top_k, top_p, temperature, seed, step=0, row0=0, eos=(), pad=0, finished=None, flags0=0, want_scores=True):
    """One call -> dict(next, fin, scores, flags); the sentinels around every output and the one written column of out_tokens are checked."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    BB, ld = full.shape
    lgd = to_dev(full, dtype)
    eos_d = torch.tensor(list(eos), dtype=torch.int64, device=dev())
    fin = to_dev(np.zeros(BB, np.int32) if finished is None else np.asarray(finished, np.int32))
    nxt = torch.full((BB + 2,), -7, dtype=torch.int64, device=dev())
    out = torch.full((BB + 1, G + 8), -1, dtype=torch.int64, device=dev())
    lds = V + 5
    sc = torch.full((BB + 1, lds), SENT, dtype=torch.float32, device=dev()) if want_scores else None
    flags = torch.tensor([flags0, 77], dtype=torch.int32, device=dev())
    step_d = torch.tensor([step], dtype=torch.int32, device=dev())
    _lib.call("p2t_sample_select", ptr(lgd), ops.dt_of(dtype), ld, V, BB, ptr(eos_d) if len(eos) else None, len(eos), pad, ptr(fin), ptr(nxt[1:]),
              ptr(out), G + 8, ptr(step_d), G, float(temperature), top_k, float(top_p), seed, row0, ptr(sc) if want_scores else None, lds,
              ptr(flags), stream())
    nx, o, fl = to_np(nxt), to_np(out), to_np(flags)
    col = min(max(step, 0), G - 1)
    assert nx[0] == -7 and nx[-1] == -7 and fl[1] == 77
    assert (np.delete(o[:BB], col, axis=1) == -1).all() and (o[BB] == -1).all() and np.array_equal(o[:BB, col], nx[1:-1])
    res = dict(next=nx[1:-1], fin=to_np(fin), flags=int(fl[0]), scores=None)
    if want_scores:
        s = to_np(sc)
        assert (s[:BB, V:] == SENT).all() and (s[BB] == SENT).all()
        res["scores"] = s[:BB, :V]
    return res


def reference(full, V, top_k, top_p, temperature, seed, step=0, row0=0):
    us = [synth.sample_uniform(seed, row0 + r, step) for r in range(full.shape[0])]
    return SR.sample_rows(full[:, :V], temperature, top_k, top_p, us)


def check_scores(got, refs, full, V, temperature):
    for r, ref in enumerate(refs):
        kept = np.nonzero(got[r] != -np.inf)[0]
        assert np.array_equal(kept, ref["kept"]), (r, np.setxor1d(kept, ref["kept"])[:8])
        x = SR.scaled(full[r, :V], temperature)[kept]
        assert (np.abs(got[r][kept] - x) <= np.spacing(np.abs(x))).all(), r


# (V, ld, dtype, BB, top_k, top_p, temperature, seed): a subset of {300, 1000, 128256} x {f32, bf16} x {1, 3, 64} x {1, 5, 50, 1024} x
# {1.0, 0.9, 0.5} x {1.0, 0.7, 1.5}; 1024 survivors leave margins of the size of delta, so those cases have 1 or 3 rows.  `seed` seeds
# both the logits and the draw: the first of 0, 1, 2, ... for which every row of the case is decidable.  ld = 1003 puts the rows off the
# 16-byte grid (the kernel then reads them one column at a time); 320, 1008 and 128320 keep them on it, with a tail at V = 300.
SWEEP = [
    (300, 320, F32, 3, 5, 0.9, 0.7, 0), (300, 320, BF16, 64, 50, 0.5, 1.5, 0), (300, 320, F32, 1, 1024, 1.0, 1.0, 0), (300, 320, BF16, 3, 1, 0.9, 1.0, 0),
    (300, 320, F32, 64, 50, 0.9, 1.5, 0),
    (1000, 1008, F32, 64, 50, 0.9, 0.7, 0), (1000, 1003, BF16, 64, 5, 0.5, 1.0, 0), (1000, 1008, BF16, 3, 1024, 1.0, 1.5, 0), (1000, 1008, F32, 1, 1, 1.0, 0.7, 0),
    (1000, 1008, BF16, 64, 50, 0.9, 0.7, 0), (1000, 1003, F32, 3, 1024, 0.9, 1.0, 0),
    (128256, 128320, BF16, 64, 50, 0.9, 0.7, 0), (128256, 128320, F32, 64, 5, 0.5, 1.0, 0), (128256, 128320, F32, 3, 50, 0.9, 1.5, 0),
    (128256, 128320, BF16, 3, 1024, 1.0, 1.0, 0), (128256, 128320, F32, 1, 1024, 0.9, 0.7, 3), (128256, 128320, BF16, 1, 1, 0.5, 1.5, 0),
    (128256, 128320, BF16, 64, 50, 1.0, 1.5, 0),
]
_id = lambda c: f"V{c[0]}-{'bf16' if c[2] == BF16 else 'f32'}-BB{c[3]}-k{c[4]}-p{c[5]}-t{c[6]}"
STEP = 3


def sweep_inputs(case):
    """-> (logits as stored, with their NaN tail; the restatement's rows): numpy only."""
    V, ld, dtype, BB, top_k, top_p, temperature, seed = case
    full = make_logits(seed, BB, V, ld, dtype)
    return full, reference(full, V, top_k, top_p, temperature, seed, STEP)


@pytest.mark.parametrize("case", SWEEP, ids=_id)
def test_sweep_vs_restatement(case):
    V, ld, dtype, BB, top_k, top_p, temperature, seed = case
    full, refs = sweep_inputs(case)
    assert all(r["decidable"] for r in refs), [(i, r["m_p"], r["m_u"]) for i, r in enumerate(refs) if not r["decidable"]]
    if dtype == BF16 and V >= 1000 and BB == 64 and top_k == 50:
        assert sum(r["ties_at_kth"] > 1 for r in refs) >= 4                  # more survivors than k: HF's rule, ties at the k-th value stay
        assert any(r["n_survivors"] > top_k for r in refs)
        if top_p < 1:
            assert any(r["ties_at_cut"] for r in refs)                        # equal values on both sides of the top-p cut: column order decides
    toks = np.array([r["token"] for r in refs])
    # bookkeeping: row 1 was finished before (emits pad); row 0's token and one nobody draws are eos ids
    finished = np.zeros(BB, np.int32)
    if BB > 1:
        finished[1] = 1
    eos, pad = (int(toks[0]), V + 5), 4242
    got = run(full, dtype, V, top_k, top_p, temperature, seed, STEP, eos=eos, pad=pad, finished=finished)
    check_scores(got["scores"], refs, full, V, temperature)                  # finished rows are written like live ones
    want_next, want_fin = SR.bookkeeping(toks, finished, eos, pad)
    assert np.array_equal(got["next"], want_next), np.nonzero(got["next"] != want_next)[0]
    assert np.array_equal(got["fin"], want_fin) and got["flags"] == 0
    assert ((got["next"] >= 0) & (got["next"] < V) | (got["next"] == pad)).all()
    again = run(full, dtype, V, top_k, top_p, temperature, seed, STEP, eos=eos, pad=pad, finished=finished)
    assert np.array_equal(got["next"], again["next"]) and np.array_equal(got["scores"].view(np.int32), again["scores"].view(np.int32))
    none = run(full, dtype, V, top_k, top_p, temperature, seed, STEP, eos=eos, pad=pad, finished=finished, want_scores=False)      # scores = NULL
    assert np.array_equal(got["next"], none["next"]) and np.array_equal(got["fin"], none["fin"])


def test_step_is_clamped_into_the_token_table():
    full = make_logits(5, 2, 300, 320, F32)
    for step, col in ((-4, 0), (G + 100, G - 1)):
        got = run(full, F32, 300, 5, 1.0, 1.0, 9, step)                      # run() asserts only column `col` of out_tokens was written
        refs = reference(full, 300, 5, 1.0, 1.0, 9, step)                    # the draw's counter is step[0] itself, not the clamped column
        assert [r["token"] for r in refs if r["decidable"]] == [int(t) for t, r in zip(got["next"], refs) if r["decidable"]]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_capacity(dtype):
    """More than 2048 survivors: everything above the k-th value, then its ties in ascending column order until the table is full, and
    bit 0 of the flags word (OR-ed: other bits stay).  Row 0: constant (all masses are exactly 1, every partial sum is an integer and
    u * 2048 is exact: the token is the restatement's whatever the margin); row 1: 40 values above a 3000-wide plateau; row 2: an
    ordinary row in the same call."""
    V, ld, k, seed = 3000, 3008, 50, 4
    full = make_logits(seed, 3, V, ld, dtype)
    full[0, :V] = 0.5
    full[1, :V] = -1.0
    above = np.random.RandomState(1).permutation(V)[:40]
    full[1, above] = 2.0 + 0.125 * np.arange(40)
    refs = reference(full, V, k, 1.0, 1.0, seed)
    assert refs[0]["full"] and refs[1]["full"] and not refs[2]["full"] and refs[2]["decidable"]
    assert np.array_equal(refs[0]["kept"], np.arange(2048)) and np.isin(above, refs[1]["kept"]).all() and refs[1]["kept"].size == 2048
    got = run(full, dtype, V, k, 1.0, 1.0, seed, flags0=4)
    assert got["flags"] == 5
    check_scores(got["scores"], refs, full, V, 1.0)
    assert got["next"][0] == refs[0]["token"] and got["next"][2] == refs[2]["token"]
    assert got["next"][1] in refs[1]["kept"] and (not refs[1]["decidable"] or got["next"][1] == refs[1]["token"])
    alone = run(full[2:], dtype, V, k, 1.0, 1.0, seed, row0=2)              # the ordinary row alone: no flag, the same draw
    assert alone["flags"] == 0 and alone["next"][0] == refs[2]["token"]
    # top-p on a full table: the cut falls inside the plateau's ties, ascending column order again
    refs = reference(full, V, k, 0.5, 1.0, seed)
    got = run(full, dtype, V, k, 0.5, 1.0, seed)
    assert got["flags"] == 1 and np.array_equal(refs[0]["kept"], np.arange(1024))
    check_scores(got["scores"][:1], refs[:1], full, V, 1.0)                 # exact masses again: tail_j = (2048 - j) / 2048 against 0.5
    assert got["next"][0] == refs[0]["token"]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_extremes_top_k_1_is_greedy(dtype):
    """A spread of +-60 (exp underflows to 0 for most survivors) and -inf entries, down to a row with two finite values: top_k = 1 is
    p2t_greedy_select's token for any seed (no maximum is tied: HF's top-k keeps ties, which then share the draw); with 5 survivors the
    kept set and scores are the restatement's."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    V, ld, BB = 1000, 1008, 4
    rs = np.random.RandomState(2)
    full = np.full((BB, ld), np.nan, dtype=np.float32)
    full[:, :V] = rs.uniform(-60, 60, (BB, V)).astype(np.float32)
    if dtype == BF16:
        full = synth.bf16_round(full)
    full[:, rs.permutation(V)[:300]] = -np.inf
    for r, c in ((0, 777), (1, 20), (3, 409)):                               # one maximum per row, also after the rounding to bf16
        full[r, c] = 61.0 + r
    full[2, :V] = -np.inf
    full[2, [5, 900]] = [-59.0, -58.5]                                       # two finite entries in a row of -inf
    full[:, V:] = np.nan
    lgd = to_dev(full, dtype)
    nxt, out = torch.zeros((BB,), dtype=torch.int64, device=dev()), torch.zeros((BB, G), dtype=torch.int64, device=dev())
    fin, step = torch.zeros((BB,), dtype=torch.int32, device=dev()), torch.zeros((1,), dtype=torch.int32, device=dev())
    _lib.call("p2t_greedy_select", ptr(lgd), ops.dt_of(dtype), ld, V, BB, None, 0, 0, ptr(fin), ptr(nxt), ptr(out), G, ptr(step), G, stream())
    greedy = to_np(nxt)
    assert greedy.tolist() == [777, 20, 900, 409]
    for seed in (0, 1, 2, 12345678901234567):
        for top_p in (1.0, 0.5):
            got = run(full, dtype, V, 1, top_p, 0.7, seed)
            assert np.array_equal(got["next"], greedy), (seed, top_p)
    refs = reference(full, V, 5, 0.9, 1.5, 3)
    got = run(full, dtype, V, 5, 0.9, 1.5, 3)
    ok = [r for r in range(BB) if refs[r]["m_p"] > SR.delta(refs[r]["n_survivors"])]
    assert len(ok) >= 3
    check_scores(got["scores"][ok], [refs[r] for r in ok], full[ok], V, 1.5)
    assert all(got["next"][r] in refs[r]["kept"] for r in range(BB))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,ld", [(300, 320), (1000, 1008), (128256, 128320)])
def test_no_filters_inverse_cdf_in_column_order(V, ld, dtype):
    """top_k = 0, top_p = 1: the draw over all V columns in ascending column order.  delta grows with the number of terms (0.015 at
    V = 128256), so a row is decidable only where the drawn column carries a few per cent of the mass: every row gets 6 columns raised by
    14 .. 17, which then hold nearly all of it.  Rows that are decidable must give the restatement's column, and most rows are; every
    row's scores are logit / temperature on all V columns, and the token is a column of the row whatever the margin."""
    BB, seed, temperature = 16, 21, 0.7
    full = make_logits(seed, BB, V, ld, dtype)
    rs = np.random.RandomState(V)
    for r in range(BB):
        cols = rs.permutation(V)[:6]
        full[r, cols] = full[r, cols] + np.float32(14.0) + rs.randint(0, 4, 6).astype(np.float32)
    if dtype == BF16:
        full[:, :V] = synth.bf16_round(full[:, :V])
    refs = reference(full, V, 0, 1.0, temperature, seed, STEP)
    ok = np.array([r["decidable"] for r in refs])
    assert ok.sum() >= BB // 2, ok.sum()
    got = run(full, dtype, V, 0, 1.0, temperature, seed, STEP)
    toks = np.array([r["token"] for r in refs])
    assert np.array_equal(got["next"][ok], toks[ok])
    assert ((got["next"] >= 0) & (got["next"] < V)).all() and got["flags"] == 0
    x = SR.scaled(full[:, :V], temperature)
    assert (np.abs(got["scores"] - x) <= np.spacing(np.abs(x))).all()
    again = run(full, dtype, V, 0, 1.0, temperature, seed, STEP)
    assert np.array_equal(got["next"], again["next"]) and np.array_equal(got["scores"].view(np.int32), again["scores"].view(np.int32))


def test_draw_quality_and_row0():
    """64 identical rows x steps 0 .. 63 on a 5-survivor distribution, one call per step: every draw is the restatement's for
    sample_uniform(seed, row, step) (where decidable: all but a handful), each token's count over the 4096 draws is within 5 sigma of
    n p (binomial; deterministic for the fixed seed), and rows 7 .. 9 of the 64-row call are what a 3-row call with row0 = 7 draws."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    V, ld, BB, seed = 300, 320, 64, 2024
    p = np.array([0.35, 0.25, 0.2, 0.15, 0.05])
    cols = np.array([11, 250, 3, 299, 128])
    row = np.full(ld, -30.0, dtype=np.float32)
    row[cols] = np.log(p).astype(np.float32)
    row[V:] = np.nan
    full = np.tile(row, (BB, 1))
    lgd = to_dev(full)
    fin, nxt = torch.zeros((BB,), dtype=torch.int32, device=dev()), torch.zeros((BB,), dtype=torch.int64, device=dev())
    out, flags = torch.full((BB, G), -1, dtype=torch.int64, device=dev()), torch.zeros((1,), dtype=torch.int32, device=dev())
    out3 = torch.full((3, G), -1, dtype=torch.int64, device=dev())
    step = torch.zeros((1,), dtype=torch.int32, device=dev())
    for s in range(G):
        step.fill_(s)
        _lib.call("p2t_sample_select", ptr(lgd), _lib.F32, ld, V, BB, None, 0, 0, ptr(fin), ptr(nxt), ptr(out), G, ptr(step), G, 1.0, 5, 1.0, seed, 0,
                  None, 0, ptr(flags), stream())
        _lib.call("p2t_sample_select", ptr(lgd), _lib.F32, ld, V, 3, None, 0, 0, ptr(fin), ptr(nxt), ptr(out3), G, ptr(step), G, 1.0, 5, 1.0, seed, 7,
                  None, 0, ptr(flags), stream())
    draws = to_np(out)
    assert np.array_equal(to_np(out3), draws[7:10]) and int(flags.item()) == 0
    n = BB * G
    for c, pc in zip(cols, p):
        assert abs((draws == c).sum() - n * pc) <= 5 * np.sqrt(n * pc * (1 - pc)), (c, (draws == c).sum(), n * pc)
    assert np.isin(draws, cols).all()
    undecided = 0
    for r in range(BB):
        for s in range(G):
            ref = SR.sample_row(row[:V], 1.0, 5, 1.0, synth.sample_uniform(seed, r, s))
            if ref["decidable"]:
                assert draws[r, s] == ref["token"], (r, s)
            else:
                undecided += 1
    assert undecided <= 4                                                    # delta = 13 * 2^-23 around 5 thresholds: 4096 * 1.5e-5 expected
