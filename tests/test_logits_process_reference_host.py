"""CPU: tests/logits_process_reference.py (the numpy float32 restatement p2t_logits_process is held to bit for bit) against HF's own
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, MinNewTokensLengthLogitsProcessor and
SuppressTokensLogitsProcessor, chained in the order of GenerationMixin._get_logits_processor on f32 rows, compared bit for bit.

Two things HF does that the comparison has to know about: NoBadWordsLogitsProcessor adds a bias row, which turns a -0.0 score into
+0.0 (the rows here hold +0.0 only), and it skips a word longer than the history, so a word of L > 1 tokens first applies at history
length L although its L - 1 leading tokens fit one step earlier (pinned below)."""
import numpy as np
import pytest

import logits_process_reference as LR

torch = pytest.importorskip("torch")
pytest.importorskip("transformers")

V = 50
EOS = [7, 31]


def _rows(seed, n=4):
    """f32 rows with zeros, negatives, -inf and repeated entries."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(n, V) * 3).astype(np.float32)
    x[:, 3] = 0.0
    x[:, 11] = -np.inf
    x[:, 12] = x[:, 13]                          # repeated entries
    x[0, 20:24] = np.float32(-2.5)
    x[1, :10] = np.abs(x[1, :10])
    x[2, 5] = np.float32(1e-38)                  # the quotient is subnormal
    x[2, 6] = np.float32(-3e38)                  # the product overflows to -inf
    return x


def _hf(x, history, penalty, ngram, min_new, eos_ids, bad_words, suppress):
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor)
    ids = torch.tensor([list(history)] * x.shape[0], dtype=torch.long).reshape(x.shape[0], len(history))
    s = torch.from_numpy(x.copy())
    if penalty is not None and penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=float(penalty))(ids, s)
    if ngram:
        s = NoRepeatNGramLogitsProcessor(ngram)(ids, s)
    if bad_words:
        s = NoBadWordsLogitsProcessor(bad_words, eos_ids or None)(ids, s)
    if min_new and eos_ids:
        s = MinNewTokensLengthLogitsProcessor(0, min_new, eos_ids)(ids, s)
    if suppress:
        s = SuppressTokensLogitsProcessor(suppress)(ids, s)
    return s.numpy()


def _check(x, history, penalty=1.0, ngram=0, min_new=0, eos_ids=(), bad_words=None, suppress=None):
    want = _hf(x, history, penalty, ngram, min_new, list(eos_ids), bad_words, suppress)
    words = LR.words_of(bad_words, suppress, eos_ids)
    got = LR.process(x, [history] * x.shape[0], penalty=penalty, ngram=ngram, min_new=min_new, eos_ids=eos_ids, words=words)
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (history, penalty, ngram, min_new, bad_words, suppress)
    return got


def _histories(n):
    """Empty, one token, n - 2, n - 1 and n tokens, and longer ones with repeated n-grams (and repeated tokens)."""
    base = [5, 9, 5, 9, 2, 5, 9, 5, 4, 4, 4, 17, 5, 9]
    out = [[], [5]] + [base[:k] for k in (n - 2, n - 1, n) if k > 0] + [base[:6], base[:9], base[:11], base, base + [5], base + [5] * 3]
    seen, uniq = set(), []
    for h in out:
        if tuple(h) not in seen:
            seen.add(tuple(h))
            uniq.append(h)
    return uniq


@pytest.mark.parametrize("penalty", [1.3, 0.7, 2.0])
def test_repetition_penalty(penalty):
    x = _rows(0)
    for h in _histories(3):
        y = _check(x, h, penalty=penalty)
        for t in set(h):
            assert np.array_equal(y[:, t], np.where(x[:, t] < 0, x[:, t] * np.float32(penalty), x[:, t] / np.float32(penalty)))
    assert np.array_equal(_check(x, [3, 11, 12, 13, 5, 6], penalty=penalty)[:, 11], x[:, 11])     # -inf stays -inf; zero stays zero


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_no_repeat_ngram(n):
    x = _rows(1)
    banned_any = False
    for h in _histories(n):
        y = _check(x, h, ngram=n)
        banned_any |= bool(np.isneginf(y[0]).sum() > 1)
        if len(h) < n:
            assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
    assert banned_any


def test_bad_words_and_suppress():
    x = _rows(2)
    words = [[9, 5], [5, 9, 2], [4, 4, 4, 8], [8, 9], [21], [9, 5, 30]]
    for h in _histories(3) + [[9], [5, 9], [4, 4, 4], [2, 9, 5]]:
        y = _check(x, h, bad_words=words)
        assert np.isneginf(y[:, 21]).all()
        _check(x, h, suppress=[0, 49, 21])
        _check(x, h, bad_words=words, suppress=[40, 41])
    # prefix matches -> banned; prefix does not match -> untouched
    assert np.isneginf(_check(x, [1, 9], bad_words=words)[:, 5]).all()
    assert np.array_equal(_check(x, [9, 1], bad_words=words)[:, 5], x[:, 5])
    # HF's quirk: [5, 9, 2] against the history [5, 9] (2 tokens, the word has 3) is skipped although its prefix matches
    assert np.array_equal(_check(x, [5, 9], bad_words=[[5, 9, 2]])[:, 2], x[:, 2])
    assert np.isneginf(_check(x, [1, 5, 9], bad_words=[[5, 9, 2]])[:, 2]).all()


def test_an_eos_bad_word_is_dropped():
    x = _rows(3)
    y = _check(x, [9, 5], eos_ids=EOS, bad_words=[[7], [9, 7], [22]])
    assert np.array_equal(y[:, 7], x[:, 7]) and np.isneginf(y[:, 22]).all()
    assert LR.words_of([[7], [9, 7], [22]], [3], EOS) == [[9, 7], [22], [3]]
    assert np.isneginf(_check(x, [5, 9, 9], eos_ids=EOS, bad_words=[[7], [9, 7]])[:, 7]).all()          # [9, 7] is no [eos] word


@pytest.mark.parametrize("min_new", [1, 4])
def test_min_new_tokens(min_new):
    x = _rows(4)
    for h in _histories(3):
        y = _check(x, h, min_new=min_new, eos_ids=EOS)
        assert bool(np.isneginf(y[:, EOS]).all()) == (len(h) < min_new)
    assert np.array_equal(_check(x, [], min_new=min_new, eos_ids=()).view(np.uint32), x.view(np.uint32))   # no eos ids: not installed


@pytest.mark.parametrize("n", [1, 2, 3])
def test_all_processors_chained(n):
    x = _rows(5 + n)
    words = [[9, 5], [5, 9, 2], [21], [7]]
    for h in _histories(n):
        _check(x, h, penalty=1.3, ngram=n, min_new=6, eos_ids=EOS, bad_words=words, suppress=[0, 30])


def test_ids_outside_the_vocabulary_are_ignored():
    """HF would fail on these; the kernel's rule: compared like any other id, never written to."""
    x = _rows(9)
    h = [5, V, -3, 5, V + 7, 5]
    y = LR.process(x, [h] * 4, penalty=1.5, ngram=2, min_new=9, eos_ids=[V, -1, 7], words=[[V], [5, V + 1], [-2]])
    want = x.copy()
    want[:, 5] = np.where(x[:, 5] < 0, x[:, 5] * np.float32(1.5), x[:, 5] / np.float32(1.5))
    want[:, 7] = -np.inf
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    ids, off = LR.pack_words([[1, 2], [3], [4, 5, 6]])
    assert ids.tolist() == [1, 2, 3, 4, 5, 6] and off.tolist() == [0, 2, 3, 6] and off.dtype == np.int32
