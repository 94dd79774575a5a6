"""numpy float32 restatement of one p2t_beam_select_logprobs step (include/p2t_hip.h; csrc/beam_select.hip, csrc/beam_merge.h): the beam
step on rows that already hold (processed) log-probabilities.  Given the rows bit for bit, every operation of steps 2 - 6 is one IEEE
f32 operation (an addition, a division, a comparison) and every rank key is the header's, so the kernel is held to this bit for bit:
tokens, src_rows, every table of the written half, flags, done.  The one value that is not an f32 operation is
len_pow = float(pow(double(len), double(length_penalty))): math.pow here, the device's double pow there, rounded to f32 in both.

The state is tests/beam_reference.py's (one half of the kernel's double-buffered tables, numpy arrays); -inf values rank like any other,
ties by position."""
import math

import numpy as np

MASK = np.float32(-1.0e9)
NZERO = np.float32(-0.0)


def _order(v):
    """Positions by (value descending, position ascending); -inf last among themselves by position."""
    return np.argsort(-np.asarray(v, dtype=np.float32), kind="stable")


def _len_pow(n, length_penalty):
    return np.float32(math.pow(n, float(np.float32(length_penalty))))


def es_code(early_stopping) -> int:
    if early_stopping is True or (type(early_stopping) is int and early_stopping == 1):
        return 1
    if (isinstance(early_stopping, str) and early_stopping == "never") or (type(early_stopping) is int and early_stopping == 2):
        return 2
    return 0


def step(lp, st, cur, nb, eos_ids, length_penalty, early_stopping, max_length, pad_id=0):
    """lp f32 [B nb, V] -> dict(state, next_tokens, src_rows, cand_tokens [B, keep], cand_beams [B, keep], cand_acc [B, keep])."""
    lp = np.asarray(lp)
    assert lp.dtype == np.float32
    BB, V = lp.shape
    B = BB // nb
    es = es_code(early_stopping)
    keep = max(2, 1 + len(eos_ids)) * nb
    if st["done"] or cur < 0 or cur >= max_length:
        return dict(state=st, next_tokens=np.full(BB, pad_id, dtype=np.int64), src_rows=np.arange(BB, dtype=np.int64), cand_tokens=None,
                    cand_beams=None, cand_acc=None)
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    next_tokens, src_rows = np.zeros(BB, dtype=np.int64), np.zeros(BB, dtype=np.int64)
    cand_tokens, cand_beams = np.zeros((B, keep), dtype=np.int64), np.zeros((B, keep), dtype=np.int64)
    cand_acc = np.zeros((B, keep), dtype=np.float32)
    len_pow = _len_pow(cur + 1, length_penalty)
    flags = []
    with np.errstate(all="ignore"):
        for b in range(B):
            run = st["running_scores"][b].astype(np.float32)
            c_acc, c_tok, c_beam = [], [], []
            for j in range(nb):
                row = lp[b * nb + j]
                cols = _order(row)[:keep]                              # (lp descending, column ascending)
                c_acc += list(row[cols] + run[j])                      # one f32 addition
                c_tok += list(cols)
                c_beam += [j] * keep
            c_acc = np.array(c_acc, dtype=np.float32)
            top = _order(c_acc)[:keep]                                 # (acc descending, (beam, rank inside the beam) ascending)
            a, tok, beam = c_acc[top], np.array(c_tok)[top], np.array(c_beam)[top]
            cand_tokens[b], cand_beams[b], cand_acc[b] = tok, beam, a
            hit = np.isin(tok, list(eos_ids)) | (cur + 1 >= max_length)
            live = (a + np.where(hit, MASK, NZERO)).astype(np.float32)
            nxt = _order(live)[:nb]
            just = hit & (np.arange(keep) < nb)
            full = bool(st["is_finished"][b].all()) and es == 1
            open_old = bool(st["heuristic_open"][b])
            fin = (a / len_pow).astype(np.float32)
            fin = (fin + (MASK if full else NZERO)).astype(np.float32)
            fin = (fin + (NZERO if open_old else MASK)).astype(np.float32)
            fin = (fin + np.where(just, NZERO, MASK)).astype(np.float32)
            m_sc = np.concatenate([st["beam_scores"][b].astype(np.float32), fin])
            sel = _order(m_sc)[:nb]
            for r in range(nb):
                k = nxt[r]
                new["running"][b, r] = st["running"][b, beam[k]]
                new["running"][b, r, cur] = tok[k]
                new["running_idx"][b, r] = st["running_idx"][b, beam[k]]
                new["running_idx"][b, r, cur] = b * nb + beam[k]
                new["running_scores"][b, r] = live[k]
                next_tokens[b * nb + r], src_rows[b * nb + r] = tok[k], b * nb + beam[k]
                s = sel[r]
                if s < nb:
                    new["sequences"][b, r], new["beam_idx"][b, r] = st["sequences"][b, s], st["beam_idx"][b, s]
                    new["is_finished"][b, r] = st["is_finished"][b, s]
                else:
                    k = s - nb
                    new["sequences"][b, r] = st["running"][b, beam[k]]
                    new["sequences"][b, r, cur] = tok[k]
                    new["beam_idx"][b, r] = st["running_idx"][b, beam[k]]
                    new["beam_idx"][b, r, cur] = b * nb + beam[k]
                    new["is_finished"][b, r] = bool(just[k])
                new["beam_scores"][b, r] = m_sc[s]
            sc, fin_new = new["beam_scores"][b], new["is_finished"][b]
            best_len = max_length if (es == 2 and np.float32(length_penalty) > 0) else cur + 1
            best_running = np.float32(live[nxt[0]] / _len_pow(best_len, length_penalty))
            lo = sc.min()
            better = best_running > np.where(fin_new, lo, MASK)
            new["heuristic_open"][b] = open_old and bool(better.any())
            flags.append((bool(new["heuristic_open"][b]), bool(fin_new.all()), bool(hit.all())))
    go_on = any(f[0] for f in flags) and not (all(f[1] for f in flags) and es == 1) and not all(f[2] for f in flags)
    if not go_on or cur + 1 >= max_length:
        new["done"], new["steps"] = True, cur + 1
    return dict(state=new, next_tokens=next_tokens, src_rows=src_rows, cand_tokens=cand_tokens, cand_beams=cand_beams, cand_acc=cand_acc)


def log_softmax_f32(x):
    """A plain f32 log-softmax of rows (for host tests: NOT the kernel's summation order)."""
    x = np.asarray(x, dtype=np.float32)
    mx = x.max(axis=-1, keepdims=True)
    d = x - mx
    lse = np.log(np.exp(d).sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    return (d - lse).astype(np.float32)
