"""numpy restatement of the per-row choice kernels of continuous batching (include/p2t_hip.h: p2t_sample_select_rows,
p2t_logits_process_rows; csrc/sample_select.hip, csrc/logits_process.hip, csrc/row_model.h), composed from what the lock-step kernels
are already held to: sampling_reference.sample_row (the warpers and the inverse CDF in fp64, with its decidability margins),
p2t_hip.synth.sample_uniform(seed, key, step) (the draw), logits_process_reference.process_row (the processors, f32 bit for bit) and the
bookkeeping of continuous_reference.greedy_select_rows (row map, finished rows, the eos and limit bits).  numpy only."""
import numpy as np

import logits_process_reference as lpr
import sampling_reference as sref
from p2t_hip.synth import sample_uniform


def logits_process_rows(logits, V, out_tokens, row_step, out, row_map=None, finished=None, **proc):
    """Writes the processed f32 row i of `out` ([n, >= V], in place) for every logits row whose engine row is live; the history of row i is
    out_tokens[r, : clamp(row_step[r], 0, G)].  proc: process_row's keywords (penalty, ngram, min_new, eos_ids, words)."""
    BB, G = out_tokens.shape
    for i in range(logits.shape[0]):
        r = i if row_map is None else int(row_map[i])
        if not 0 <= r < BB or (finished is not None and finished[r]):
            continue                                             # a row the engine does not have, a finished row: nothing is written
        cur = min(max(int(row_step[r]), 0), G)
        out[i, :V] = lpr.process_row(logits[i, :V], out_tokens[r, :cur], **proc)


def sample_select_rows(logits, V, finished, next_tokens, out_tokens, row_step, row_limit, row_key, eos_ids, pad_id, temperature, top_k, top_p, seed,
                       row_map=None, scores=None):
    """Updates finished / next_tokens / out_tokens (and scores [n, >= V], when given) in place as the kernel does -> {i: sample_row's
    result} for the live rows (token, decidable, margins)."""
    BB, G = out_tokens.shape
    results = {}
    for i in range(logits.shape[0]):
        r = i if row_map is None else int(row_map[i])
        if not 0 <= r < BB:
            continue
        if finished[r]:
            next_tokens[r] = pad_id                              # nothing else: not out_tokens, not finished, not the scores row
            continue
        u = sample_uniform(seed, int(row_key[r]), int(row_step[r]))
        res = sref.sample_row(np.asarray(logits[i, :V]), temperature, top_k, top_p, u)
        tok = res["token"]
        st = min(max(int(row_step[r]), 0), G - 1)
        next_tokens[r] = out_tokens[r, st] = tok
        finished[r] |= (1 if tok in eos_ids else 0) | (2 if st + 1 >= int(row_limit[r]) else 0)
        if scores is not None:
            scores[i, :V] = res["scores"]
        results[i] = res
    return results


def rederive(logits, tokens, key, seed, temperature, top_k, top_p, proc=None, eos_ids=()):
    """One request end to end: logits f32 [n, V] (the raw rows the engine returned), tokens [n] -> list of sample_row results, token t
    re-derived from row t, the request's own earlier tokens tokens[:t], its key and its step t."""
    out = []
    for t in range(len(tokens)):
        row = np.asarray(logits[t])
        if proc is not None:
            row = lpr.process_row(row, tokens[:t], penalty=proc["penalty"], ngram=proc["ngram"], min_new=proc["min_new"], eos_ids=eos_ids, words=proc["words"])
        out.append(sref.sample_row(row, temperature, top_k, top_p, sample_uniform(seed, int(key), t)))
    return out
