"""CPU: p2t_hip.data.pack_instruct_batch -- stage-2 batches in the reference collater's layout (left pad + bos + prompt with
placeholders + description + eot + right pad) packed into padding-free rows (include/p2t_hip.h "packed rows")."""
import numpy as np
import pytest
import torch

from p2t_hip import pack_instruct_batch

PLACEHOLDER, PAD = 511, 510


def _batch(lens, prot_lens, T=None, seed=0):
    """Reference-layout rows: [left pad | bos, placeholders x prot_len, prompt, description tokens, eot | right pad]."""
    rs = np.random.RandomState(seed)
    T = T or max(lens) + 6
    B = len(lens)
    ids = np.full((B, T), PAD, dtype=np.int64)
    mask = np.zeros((B, T), dtype=np.int64)
    labels = np.full((B, T), -100, dtype=np.int64)
    Tp = max(prot_lens)
    pids = np.ones((B, Tp), dtype=np.int64)
    pmask = np.zeros((B, Tp), dtype=np.int64)
    for i, (n, p) in enumerate(zip(lens, prot_lens)):
        left = rs.randint(0, T - n + 1)
        toks = rs.randint(3, 500, size=n)
        toks[1:1 + p] = PLACEHOLDER
        ids[i, left:left + n] = toks
        mask[i, left:left + n] = 1
        d0 = 1 + p + 2
        labels[i, left + d0:left + n] = toks[d0:]
        pids[i, :p] = 100 + i
        pmask[i, :p] = 1
    return {k: torch.from_numpy(v) for k, v in dict(input_ids=ids, attention_mask=mask, labels=labels, protein_input_ids=pids,
                                                     protein_attention_mask=pmask).items()}


def _samples(batch):
    out = []
    for i in range(batch["input_ids"].shape[0]):
        keep = batch["attention_mask"][i] != 0
        out.append((batch["input_ids"][i, keep], batch["labels"][i, keep]))
    return out


LENS, PROT = [40, 7, 25, 1 + 3 + 2 + 2, 33, 12, 18], [10, 2, 6, 3, 9, 4, 5]


@pytest.mark.parametrize("max_tokens", [40, 64, 200])
def test_conserves_tokens_positions_and_labels(max_tokens):
    b = _batch(LENS, PROT)
    p = pack_instruct_batch(b, max_tokens)
    R, T = p["input_ids"].shape
    assert T <= max_tokens and int(p["attention_mask"].sum(1).max()) <= max_tokens
    assert sorted(i for i, *_ in p["pack_layout"]) == list(range(len(LENS)))
    src = _samples(b)
    for i, r, s, n in p["pack_layout"]:                         # unpacking the rows recovers every sample
        assert torch.equal(p["input_ids"][r, s:s + n], src[i][0])
        assert torch.equal(p["position_ids"][r, s:s + n], torch.arange(n))
        assert int(p["labels"][r, s]) == -100                  # a document start is never a target
        assert torch.equal(p["labels"][r, s + 1:s + n], src[i][1][1:])
        assert bool((p["attention_mask"][r, s:s + n] == 1).all())
    for r in range(R):                                          # right-padded rows, no supervised padding
        n = int(p["attention_mask"][r].sum())
        assert bool((p["attention_mask"][r, :n] == 1).all()) and bool((p["attention_mask"][r, n:] == 0).all())
        assert bool((p["labels"][r, n:] == -100).all()) and bool((p["input_ids"][r, n:] == PAD).all())
    assert "loss_weights" not in p


def test_protein_rows_follow_the_placeholder_order():
    b = _batch(LENS, PROT)
    p = pack_instruct_batch(b, 64)
    # the encoder rows' valid tokens, row-major, pair up with the placeholders, row-major (reference :138)
    enc_rows = [int(p["protein_input_ids"][k, 0]) - 100 for k in range(len(LENS))]
    ph = (p["input_ids"] == PLACEHOLDER)
    owner = []
    for i, r, s, n in sorted(p["pack_layout"], key=lambda x: (x[1], x[2])):
        owner += [i] * int(ph[r, s:s + n].sum())
    expanded = [i for k, i in enumerate(enc_rows) for _ in range(int(p["protein_attention_mask"][k].sum()))]
    assert owner == expanded
    assert int(ph.sum()) == int(p["protein_attention_mask"].sum())


def test_sample_weights_sum_to_one_and_average_documents():
    b = _batch(LENS, PROT)
    p = pack_instruct_batch(b, 64, loss_weighting="sample")
    w = p["loss_weights"]
    assert w.dtype == torch.float32 and w.shape == p["labels"].shape
    assert abs(float(w.sum()) - 1.0) < 1e-6
    assert bool((w[p["labels"] == -100] == 0).all())
    for i, r, s, n in p["pack_layout"]:                         # each document carries 1 / n_docs in total
        assert abs(float(w[r, s:s + n].sum()) - 1.0 / len(LENS)) < 1e-6


def test_first_fit_decreasing_and_refusals():
    b = _batch(LENS, PROT)
    p = pack_instruct_batch(b, 40)
    fill = p["attention_mask"].sum(1).tolist()
    assert sum(fill) == sum(LENS) and len(fill) == 4            # 40 | 33+7 | 25+12 | 18+8
    with pytest.raises(ValueError, match="max_tokens"):
        pack_instruct_batch(b, 39)
    with pytest.raises(ValueError):
        pack_instruct_batch(b, 64, loss_weighting="mean")
