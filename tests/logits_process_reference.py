"""numpy float32 restatement of p2t_logits_process (include/p2t_hip.h; csrc/logits_process.hip): HF's RepetitionPenaltyLogitsProcessor ->
NoRepeatNGramLogitsProcessor -> NoBadWordsLogitsProcessor (suppress_tokens as words of one token) -> MinNewTokensLengthLogitsProcessor on
one row, with the generated tokens alone as the history.  Every operation is one IEEE f32 operation, so the kernel is held to it bit
for bit; tests/test_logits_process_reference_host.py holds it to HF's own processors."""
import numpy as np

NINF = np.float32(-np.inf)


def drop_eos_words(bad_words, eos_ids):
    """HF's NoBadWordsLogitsProcessor.__init__: a word equal to [eos] is dropped."""
    return [list(w) for w in (bad_words or ()) if all(list(w) != [int(e)] for e in (eos_ids or ()))]


def words_of(bad_words=None, suppress=None, eos_ids=None):
    """The word list the kernel is handed: the bad words (without [eos]) and every suppressed id as a word of one token."""
    return drop_eos_words(bad_words, eos_ids) + [[int(t)] for t in (suppress or ())]


def process_row(logits, history, penalty=1.0, ngram=0, min_new=0, eos_ids=(), words=()):
    """logits: [V] of any float dtype (up-cast to f32 as the kernel does); history: the row's generated tokens so far (ids outside
    [0, V) are compared like any other and never written to).  -> f32 [V]."""
    x = np.asarray(logits).astype(np.float32)
    V = x.shape[0]
    h = [int(t) for t in history]
    cur = len(h)
    y = x.copy()
    penalty = np.float32(penalty)
    if penalty != np.float32(1.0):
        with np.errstate(all="ignore"):
            for t in h:
                if 0 <= t < V:
                    y[t] = x[t] * penalty if x[t] < 0 else x[t] / penalty
    n = int(ngram)
    if n > 0 and cur >= n:
        last = h[cur - (n - 1):] if n > 1 else []
        for i in range(cur - n + 1):
            if h[i:i + n - 1] == last and 0 <= h[i + n - 1] < V:
                y[h[i + n - 1]] = NINF
    for w in words:
        w = [int(t) for t in w]
        L = len(w)
        if L < 1 or (L > 1 and L > cur):                     # HF skips a word longer than the context
            continue
        if (L == 1 or h[cur - (L - 1):] == w[:-1]) and 0 <= w[-1] < V:
            y[w[-1]] = NINF
    if cur < int(min_new):
        for e in eos_ids:
            if 0 <= int(e) < V:
                y[int(e)] = NINF
    return y


def process(logits, histories, **kw):
    """Rows of logits [R, V] with their histories -> f32 [R, V]."""
    return np.stack([process_row(logits[r], histories[r], **kw) for r in range(len(histories))])


def argmax_first(y):
    """torch.argmax / p2t_greedy_select: the lowest index among equal maxima."""
    return int(np.argmax(y))


def pack_words(words):
    """-> (ids i64 [total], offsets i32 [n + 1]) as p2t_logits_process reads them."""
    ids = np.array([t for w in words for t in w], dtype=np.int64)
    off = np.zeros(len(words) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(w) for w in words])
    return ids, off
