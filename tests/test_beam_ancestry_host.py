"""CPU: the ancestry table of beam search without the cache copy (tests/beam_ancestry_reference.py restates include/p2t_hip.h): reading
the generated segment through the table gives, index for index, the segment that p2t_kv_reorder's copy rule materialises step by step;
the update is the same in place as out of place; columns behind the counter keep their bytes."""
import numpy as np
import pytest

import beam_ancestry_reference as A

STEPS = 70


def _chain(B0, group, seed):
    """STEPS random beam selections with repeated sources (a beam that is nobody's source dies): yields (step, src_rows)."""
    rs = np.random.RandomState(seed)
    for s in range(STEPS):
        src = np.concatenate([b * group + rs.randint(0, group, size=group) for b in range(B0)])
        if s % 7 == 3:                                   # now and then every beam of a prompt continues ONE source
            src = np.concatenate([np.full(group, b * group + rs.randint(0, group)) for b in range(B0)])
        yield s, src.astype(np.int64)


@pytest.mark.parametrize("B0,group", [(2, 3), (1, 16)])
def test_gather_through_the_table_equals_the_copied_segment(B0, group):
    BB, G = B0 * group, 128
    written = lambda s: (np.arange(BB) * 1000 + s + 1).astype(np.float64)[:, None]      # what row r appends at index s: unique
    phys, mat = np.zeros((BB, G, 1)), np.zeros((BB, G, 1))
    anc = np.zeros((BB, G), dtype=np.uint8)
    dups = 0
    for s, src in _chain(B0, group, 5 + group):
        dups += len(set(src.tolist())) < BB
        mat = A.reorder(mat, src, s)                     # the copy path: reorder, then the step appends at index s
        mat[:, s] = written(s)
        anc = A.ancestry_update(anc, src, s, group)      # the table path: update, then the same append into the physical row
        phys[:, s] = written(s)
        assert (anc[:, : s + 1] < group).all()
        assert np.array_equal(A.gather(phys, anc, s + 1, group)[:, : s + 1], mat[:, : s + 1]), f"step {s}"
    assert dups > STEPS // 2                             # the chain did kill beams
    # the histories are not the physical rows: the identity reading of the same buffers differs
    ident = np.tile(np.arange(group, dtype=np.uint8), B0)[:, None].repeat(G, 1)
    assert not np.array_equal(A.gather(phys, ident, STEPS, group), mat)


def _update_in_place(anc, src, step, group):
    """The kernel's order: per (prompt, column <= s) read the prompt's `group` bytes, then write them."""
    BB, G = anc.shape
    s = min(max(step, 0), G - 1)
    for b0 in range(BB // group):
        for i in range(s + 1):
            col = anc[b0 * group:(b0 + 1) * group, i]
            v = [g if i == s else col[min(max(int(src[b0 * group + g]) - b0 * group, 0), group - 1)] for g in range(group)]
            col[:] = v
    return anc


@pytest.mark.parametrize("B0,group", [(2, 3), (1, 16)])
def test_in_place_update_equals_out_of_place_and_leaves_later_columns(B0, group):
    BB, G = B0 * group, 128
    a = np.full((BB, G), 0xFF, dtype=np.uint8)
    b = a.copy()
    for s, src in _chain(B0, group, 11):
        a = A.ancestry_update(a, src, s, group)
        b = _update_in_place(b, src, s, group)
        assert np.array_equal(a, b), f"step {s}"
        assert (a[:, s + 1:] == 0xFF).all() and (a[:, : s + 1] < group).all()


def test_sources_outside_the_prompt_are_clamped_and_the_counter_too():
    group, G = 3, 64
    anc = np.arange(6 * G, dtype=np.uint8).reshape(6, G) % group
    src = np.array([5, -1, 1, 0, 4, 99], dtype=np.int64)            # rows 0, 1 (prompt 0) and 3, 5 (prompt 1) name rows outside their prompt
    new = A.ancestry_update(anc, src, 10, group)
    for r, want in enumerate([2, 0, 1, 3, 4, 5]):
        assert np.array_equal(new[r, :10], anc[want, :10]) and new[r, 10] == r % group
    assert np.array_equal(new[:, 11:], anc[:, 11:])
    far = A.ancestry_update(anc, np.arange(6), 1000, group)         # the counter past the capacity: the last column
    assert np.array_equal(far[:, : G - 1], anc[:, : G - 1]) and np.array_equal(far[:, G - 1], np.arange(6) % group)
