"""numpy reference of prompt-lookup decoding (include/p2t_hip.h "prompt-lookup decoding"; p2t_hip/lookup.py): the draft rule (HF's
PromptLookupCandidateGenerator.get_candidates on a row's own generated tokens), the verify rule, and a simulator that replays a whole
greedy sequence through both and counts (verify steps, drafted tokens, accepted tokens)."""
import numpy as np

EOS_BIT, LIMIT_BIT = 1, 2


def draft(h, k, n):
    """h: the history h[0 .. s] (h[s] = the token chosen last) -> the draft, a list of c <= k tokens.  For m = min(n, s) .. 1: the
    EARLIEST i with h[i : i + m] == h[s - m + 1 : s + 1] and a non-empty continuation h[i + m : min(i + m + k, s + 1)]."""
    h = [int(t) for t in h]
    s = len(h) - 1
    for m in range(min(n, s), 0, -1):
        suffix = h[s - m + 1:]
        for i in range(0, s - m + 1):                    # i + m <= s: at least h[i + m] follows
            if h[i:i + m] == suffix:
                return h[i + m:min(i + m + k, s + 1)]
    return []


def step_tokens(h, k, n, pad):
    """-> (the step's k + 1 tokens: h[s], the draft, pad behind it; c)"""
    d = draft(h, k, n)
    return [int(h[-1])] + d + [int(pad)] * (k - len(d)), len(d)


def argmax_rows(logits, V):
    """lowest index among equal maxima (np.argmax's rule, p2t_greedy_select's)"""
    return np.argmax(np.asarray(logits)[..., :V], axis=-1)


def verify(choice, tokens, c, s, limit, eos_ids, finished=0):
    """choice[j]: the model's token behind the step's token j; tokens: the step's tokens; s: the row's counter; limit: its max_new_tokens.
    -> (new tokens, finished bits, a) -- a: the draft tokens the model agreed with, before the eos / limit cut.  A finished row:
    ([], finished, 0)."""
    if finished:
        return [], finished, 0
    a = 0
    while a < c and s + a + 1 < limit and int(choice[a]) == int(tokens[a + 1]):      # g_a is token s + a + 1: behind the limit it decides nothing
        a += 1
    new, fin = [], 0
    for j in range(a + 1):
        idx = s + 1 + j
        if idx >= limit:
            fin |= LIMIT_BIT
            break
        new.append(int(choice[j]))
        if int(choice[j]) in eos_ids:
            fin |= EOS_BIT
        if idx + 1 >= limit:
            fin |= LIMIT_BIT
        if fin:
            break
    return new, fin, a


def simulate(seq, k, n, eos_ids=(), pad=0, detail=False):
    """seq: ONE row's greedy tokens (its whole sequence; the model's token behind any prefix of it is the next one) -> (verify steps,
    drafted, accepted): the counters of a lookup run that reproduces it.  The row's limit is len(seq); it ends at its first eos (seq
    goes on behind it: what the model would have chosen).  detail: a fourth number, the steps whose draft was not accepted whole."""
    seq = [int(t) for t in seq]
    limit = len(seq)
    s, steps, drafted, accepted, rejected = 0, 0, 0, 0, 0
    fin = (EOS_BIT if seq[0] in eos_ids else 0) | (LIMIT_BIT if limit <= 1 else 0)
    while not fin:
        toks, c = step_tokens(seq[:s + 1], k, n, pad)
        # the model's token behind t_j: the true next token while the fed prefix is the true one, anything else (never compared) behind it
        choice, ok = [], True
        for j in range(k + 1):
            ok = ok and (j == 0 or (s + j < len(seq) and toks[j] == seq[s + j]))
            choice.append(seq[s + 1 + j] if ok and s + 1 + j < len(seq) else -1)
        new, fin, acc = verify(choice, toks, c, s, limit, eos_ids)
        assert new == seq[s + 1:s + 1 + len(new)] and new
        s, steps, drafted, accepted, rejected = s + len(new), steps + 1, drafted + c, accepted + acc, rejected + (acc < c)
    return (steps, drafted, accepted, rejected) if detail else (steps, drafted, accepted)
