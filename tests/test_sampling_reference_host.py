"""CPU: the fp64 restatement of p2t_sample_select (tests/sampling_reference.py) against the installed transformers' own warpers and
generation.filter_logits on tie-free f32 rows (where HF's result does not depend on its sort's tie order), the host restatement of the
draw (p2t_hip.synth.sample_uniform), and the inverse CDF on a hand-made distribution."""
import numpy as np
import pytest
import torch

import sampling_reference as SR
from p2t_hip import synth


def _rows(seed, rows, V):
    """randn * 3, f32, without a repeated value in a row."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < rows:
        v = np.unique((rs.randn(2 * V) * 3).astype(np.float32))
        out.append(rs.permutation(v)[:V])
    return np.stack(out)


@pytest.mark.parametrize("V,top_k,top_p,temperature", [(300, 5, 0.9, 0.7), (300, 50, 1.0, 1.0), (1000, 50, 0.9, 0.7), (1000, 1024, 0.5, 1.5),
                                                      (1000, 1, 0.9, 1.0), (5000, 1024, 0.9, 1.5), (5000, 50, 0.5, 0.7)])
def test_kept_set_and_scores_equal_hf_warpers_and_filter_logits(V, top_k, top_p, temperature):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    from p2t_hip.generation import filter_logits
    # rows whose top-p cut is clear of its threshold by the f32 summation error (SR.delta): elsewhere HF's own f32 softmax + cumsum may
    # fall on either side, and there is nothing to compare
    cand = _rows(V + top_k, 40, V)
    lg = np.stack([row for row in cand if np.unique(SR.scaled(row, temperature)).size == V
                   and SR.sample_row(row, temperature, top_k, top_p, 0.5)["m_p"] > SR.delta(min(top_k, V))][:6])
    assert lg.shape[0] == 6
    t = torch.from_numpy(lg)
    hf = t
    if temperature != 1.0:
        hf = TemperatureLogitsWarper(temperature)(None, hf)
    hf = TopKLogitsWarper(top_k)(None, hf)
    if top_p < 1.0:
        hf = TopPLogitsWarper(top_p)(None, hf)
    ours = filter_logits(t, temperature, top_k, top_p)
    for r in range(lg.shape[0]):
        ref = SR.sample_row(lg[r], temperature, top_k, top_p, 0.5)
        assert np.unique(SR.scaled(lg[r], temperature)).size == V          # still tie-free after the division
        assert ref["m_p"] > SR.delta(ref["n_survivors"])                    # HF's f32 softmax + cumsum decide the cut like fp64
        assert np.array_equal(ref["scores"], hf[r].numpy())                 # -inf == -inf, kept values bit for bit
        assert np.array_equal(ref["scores"], ours[r].numpy())
        assert np.array_equal(ref["kept"], np.nonzero(np.isfinite(hf[r].numpy()))[0])
        assert not ref["full"] and ref["n_survivors"] == min(top_k, V)


def test_ties_capacity_and_order():
    x = np.zeros(3000, dtype=np.float32)
    r = SR.sample_row(x, 1.0, 50, 1.0, 0.3)
    assert r["full"] and np.array_equal(r["kept"], np.arange(2048)) and r["token"] == int(0.3 * 2048)
    x[[2990, 17, 1500]] = 1.0                        # three above the plateau: all kept, ranks by ascending column
    r = SR.sample_row(x, 1.0, 2, 1.0, 0.0)
    assert not r["full"] and r["kept"].tolist() == [17, 1500, 2990] and r["token"] == 17 and r["ties_at_kth"] == 3
    r = SR.sample_row(x, 1.0, 50, 1.0, 0.0)
    assert r["full"] and r["kept"].tolist() == [*range(2047), 2990]           # 3 above + the first 2045 ties


def test_sample_uniform_is_a_deterministic_hash_of_seed_row_and_step():
    u = synth.sample_uniform(7, 3, 5)
    assert u == synth.sample_uniform(7, 3, 5) and 0.0 < u < 1.0
    assert len({u, synth.sample_uniform(8, 3, 5), synth.sample_uniform(7, 4, 5), synth.sample_uniform(7, 3, 6)}) == 4
    assert synth.sample_uniform(0, 0, 0) != synth.sample_uniform(0, 1, 0) != synth.sample_uniform(0, 0, 1)
    # (hash24 + 0.5) 2^-24: an odd multiple of 2^-25
    assert (u * 2 ** 25) % 2 == 1
    us = np.array([synth.sample_uniform(11, r, s) for r in range(64) for s in range(64)])
    assert us.min() > 0 and us.max() < 1 and np.unique(us).size == us.size
    assert abs(us.mean() - 0.5) < 5 * np.sqrt(1.0 / 12 / us.size)           # 5 sigma of the mean of 4096 uniform draws


def test_inverse_cdf_on_a_known_distribution():
    p = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
    lg = np.log(p).astype(np.float32)
    # descending order of value: 0.3 (col 2), 0.25 (3), 0.2 (1), 0.15 (4), 0.1 (0): cumulative 0.3, 0.55, 0.75, 0.9, 1.0
    for u, col in [(0.01, 2), (0.29, 2), (0.31, 3), (0.54, 3), (0.56, 1), (0.74, 1), (0.76, 4), (0.89, 4), (0.91, 0), (0.999, 0)]:
        assert SR.sample_row(lg, 1.0, 5, 1.0, u)["token"] == col, u
    # top_p = 0.8: tails 1.0, 0.7, 0.45, 0.25, 0.1 against 0.2 -> four ranks stay, renormalised cumulative 0.333, 0.611, 0.833, 1
    for u, col in [(0.30, 2), (0.40, 3), (0.70, 1), (0.90, 4), (0.9999, 4)]:
        r = SR.sample_row(lg, 1.0, 5, 0.8, u)
        assert r["token"] == col and r["kept"].tolist() == [1, 2, 3, 4] and r["scores"][0] == -np.inf
    # no filters: column order, cumulative 0.1, 0.3, 0.6, 0.85, 1.0
    for u, col in [(0.05, 0), (0.2, 1), (0.5, 2), (0.7, 3), (0.9, 4)]:
        assert SR.sample_row(lg, 1.0, 0, 1.0, u)["token"] == col
    assert SR.inverse_cdf([1.0, 1.0], 1.0)[0] == 1                          # rounding left none: the last one
    nxt, fin = SR.bookkeeping([5, 6, 7], [0, 1, 0], [7, 9], 99)
    assert nxt.tolist() == [5, 99, 7] and fin.tolist() == [0, 1, 1]


def test_generation_seed_separates_ranks_and_batches():
    from p2t_hip.loop import generation_seed
    s = {generation_seed(5, r, b) for r in range(4) for b in range(8)}
    assert len(s) == 32 and all(0 <= v < 2 ** 64 for v in s) and generation_seed(5, 1, 2) == generation_seed(5, 1, 2) != generation_seed(6, 1, 2)
