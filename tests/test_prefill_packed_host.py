"""CPU: the host planner of the padding-free prefill (p2t_hip/generation.py, plan_prompt_rows) against the contract restated in
tests/prefill_packed_reference.py, and packing + unpacking a prompt batch on the numpy reference against p2t_compact_rows' result."""
import numpy as np
import pytest

import prefill_packed_reference as PR
from p2t_hip import generation as G


def _ragged(n, seed):
    rs = np.random.RandomState(seed)                      # bench.py's model of protein lengths + 64 chat tokens
    return (np.clip(rs.lognormal(5.75, 0.6, n), 16, 1024).astype(int) + 64).tolist()


@pytest.mark.parametrize("lens,pack_tokens", [
    ([15, 11, 8], None), ([15, 11, 8], 20), ([15, 11, 8], 15), ([100, 7, 64, 129, 1], None), ([100, 7, 64, 129, 1], 192), ([1], None), ([64, 64], 64),
    ([5, 9, 5, 9, 5], 14), (_ragged(8, 0), None), (_ragged(32, 1), 2048), (_ragged(256, 2), 4096), ([7] * 40, 64)],
    ids=lambda v: None if v is None else (str(v) if isinstance(v, int) else f"n{len(v)}"))
def test_plan_contract(lens, pack_tokens):
    """Every prompt placed once, no overlap, rows within pack_tokens, first-fit decreasing with ties in batch order, Tpk the fullest row
    rounded up to the documented multiple."""
    R, Tpk, place = G.plan_prompt_rows(lens, pack_tokens)
    PR.check_plan(lens, pack_tokens, R, Tpk, place)
    assert Tpk % G.PACK_ROW_MULTIPLE == 0 and G.PACK_ROW_MULTIPLE == PR.ROW_MULTIPLE == 64


def test_ties_keep_the_batch_order_and_the_longest_goes_first():
    R, Tpk, place = G.plan_prompt_rows([5, 9, 5, 9, 5], 14)
    # 9 (b1) opens row 0, 9 (b3) opens row 1, then the 5s in batch order: b0 -> row 0, b2 -> row 1, b4 -> row 2
    assert (R, Tpk) == (3, 64) and place == [(0, 9, 5), (0, 0, 9), (1, 9, 5), (1, 0, 9), (2, 0, 5)]


def test_one_row_by_default_and_the_split_beyond_the_cap():
    lens = _ragged(32, 3)
    R, Tpk, place = G.plan_prompt_rows(lens)
    assert R == 1 and Tpk == -(-sum(lens) // 64) * 64 and sum(lens) <= G.PACK_TOKENS_MAX == PR.TOKENS_MAX == 32768
    assert sorted(s for _, s, _ in place) == np.cumsum([0] + sorted(lens, reverse=True)[:-1]).tolist()
    lens = [1088] * 31                                    # 33 728 tokens: more than one row of 32 768
    R, Tpk, place = G.plan_prompt_rows(lens)
    PR.check_plan(lens, None, R, Tpk, place)
    assert R == 2 and Tpk == 30 * 1088 == 510 * 64 and [p[0] for p in place] == [0] * 30 + [1]
    assert G.plan_prompt_rows([32768])[:2] == (1, 32768)


def test_refusals():
    with pytest.raises(ValueError, match="prompt 1 has 21 tokens, more than pack_tokens = 20"):
        G.plan_prompt_rows([3, 21, 4], 20)
    with pytest.raises(ValueError, match="more than pack_tokens = 32768"):
        G.plan_prompt_rows([32769])
    with pytest.raises(ValueError, match="at least one token"):
        G.plan_prompt_rows([3, 0])
    with pytest.raises(ValueError):
        G.plan_prompt_rows([])
    with pytest.raises(ValueError):
        G.plan_prompt_rows([3], 0)


@pytest.mark.parametrize("pack_tokens", [None, 40, 320])
def test_unpacking_a_packed_batch_gives_the_compacted_rows(pack_tokens):
    """Left padding, right padding, holes, a full row, a single token: pack (numpy reference) -> unpack == p2t_compact_rows' result, and
    the packed mask / position_ids are what p2t_doc_prepare wants (a prefix; runs from 0)."""
    rs = np.random.RandomState(5)
    B, T, H = 6, 37, 8
    x = rs.randn(B, T, H).astype(np.float32)
    mask = np.zeros((B, T), dtype=np.int64)
    mask[0, 20:] = 1; mask[1, :9] = 1; mask[2] = rs.rand(T) < 0.5; mask[2, 3] = 1; mask[3] = 1; mask[4, 30] = 1; mask[5, 5:33] = 1
    idx, lens = PR.prompt_index(mask)
    assert lens.tolist() == mask.sum(1).tolist() and all((np.sort(idx[b][idx[b] >= 0]) == np.arange(lens[b])).all() for b in range(B))
    R, Tpk, place = G.plan_prompt_rows(lens, pack_tokens)
    PR.check_plan(lens, pack_tokens, R, Tpk, place)
    packed, pm, pos = PR.pack_rows(x, mask, R, Tpk, place)
    assert np.array_equal(PR.unpack_rows(packed, place, T), PR.compact_rows(x, mask))
    for r in range(R):
        n = int(pm[r].sum())
        assert pm[r, :n].all() and not pm[r, n:].any() and not pos[r, n:].any() and not packed[r, n:].any()
        starts = np.flatnonzero(pos[r, :n] == 0)
        assert sorted(starts.tolist()) == sorted(s for row, s, _ in place if row == r)
        assert all(pos[r, t] == pos[r, t - 1] + 1 for t in range(1, n) if pos[r, t] != 0)
