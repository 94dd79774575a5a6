"""fp64 restatement of one p2t_beam_sample_select step (include/p2t_hip.h; csrc/beam_sample_select.hip), for
tests/test_beam_sample_reference_host.py, tests/test_gpu_beam_sample_select.py and tests/test_gpu_generate_beam_sample.py.

`step` takes the stored logits widened to f32 and a state (beam_reference's: numpy arrays, one half of the kernel's double-buffered
tables) and returns the new state, next_tokens, src_rows, the processed scores and the flags, computed in fp64 with the header's
definitions: log-softmax, y = lp / temperature, the top-k set on the STORED logits (exact: no arithmetic), ranks by (stored logit
descending, column ascending), the top-p cut on the tail mass, acc = y + running, the Gumbel noise g = -log(-log(u)) of
p2t_hip.synth.beam_sample_uniform, key = acc + g, the draw order (key descending, flat index ascending), and then beam_reference's
bookkeeping on the keep draws with a_k = acc.

DECIDABLE.  As in beam_reference: a comparison is decidable when its fp64 gap exceeds the sum of the two sides' f32 error bounds, each
derived from the kernel's formula with u = 2^-24 (one rounding to nearest); nothing is fitted to observed errors.  beam_reference's
docstring derives err(lse) and
  t = fl(fl(x - mx) - lse) = lp:   |err| <= u |d| + err(lse) + u |lp|                                       =: E(lp)
New terms:
  y = fl(lp / T):                  |err| <= E(lp) / T + u |y|             (T is the f32 the kernel gets; an IEEE division)   =: E(y)
  acc = fl(y + run):               |err| <= E(y) + u |acc|                                                  =: E(acc)
  t = -logf(u):                    relative 4 u (two ulp per logf, as beam_reference budgets expf / logf; u is exact in f32)
  g = -logf(t):                    |err| <= 4 u (t's relative error through the logarithm) + 4 u |g|        =: E(g)
  key = fl(acc + g):               |err| <= E(acc) + E(g) + u |key|                                         =: E(key)
Keys of one beam get NO exemption: the noise differs per column, so two candidates of a beam compare like any two.  The same holds for
the later ranks: inside a beam the draws are no longer in stored-logit order, so a tie the rounding creates could fall either way.
The one exemption left: two draws of one beam with the SAME stored logit (bf16 rows have many) have the same acc bit for bit, in f32 as
in fp64, and the position rule decides both alike.
The top-p cut compares tail_j = sum_{i >= j} p_i with 1 - top_p.  p_j = e_j / sum e, e_j = expf(y_j - y_0), and in y_j - y_0 the f32
lse is the same number on both sides, so only the roundings remain:
  |err(y_j - y_0)| <= (u |d_j| + u |lp_j|) / T + u |y_j| + u |y_0| + u |y_j - y_0|                           =: r_j
every p_j is then off by at most r = max_j r_j relatively, a tail (numerator and denominator) by 2 r, on top of
sampling_reference.delta(n) = (n + 8) 2^-23 for the sum of n terms, expf and the threshold's two roundings.  The cut is decidable when
min_j |tail_j - (1 - top_p)| > delta(n) + 2 r.
Flag bit 1 compares a_(keep-1) with best - 100 (best = the prompt's largest acc): decidable when the gap exceeds E(a) + E(best) +
u |best - 100|.  A prompt that is flagged has unspecified results; the tests then check the flag and the index ranges only."""
import math

import numpy as np

import beam_reference as BR
import sampling_reference as SR
from beam_reference import MASK, U, case_eos, case_logits, fresh_state, row_stats, to_dtype, _margin   # noqa: F401  (re-exported)
from p2t_hip import synth

CAP = SR.CAP


def warp_row(x32, temperature, top_k, top_p):
    """One row of f32 logits -> dict(kept (columns, in rank order under top_k), y fp64 [V], e_y [V], scores fp64 [V] (-inf where cut),
    full, p_ok (the top-p cut is decidable), n_survivors)."""
    x32 = np.asarray(x32, dtype=np.float32)
    T = float(np.float32(temperature))
    mx, lse, lp, e_lse = row_stats(x32)
    x = x32.astype(np.float64)
    V = x.shape[0]
    d = x - mx
    y = lp / T
    e_y = (U * np.abs(d) + e_lse + U * np.abs(lp)) / T + U * np.abs(y)
    top_k = 0 if top_k is None else int(top_k)
    top_p = np.float32(1.0 if top_p is None else top_p)
    full, p_ok = False, True
    if top_k <= 0:
        assert top_p >= 1, "top_p without top_k is not a supported combination"
        kept = np.arange(V)
        n = V
    else:
        k = min(top_k, V)
        kth = np.partition(x, V - k)[V - k]
        surv = np.nonzero(x >= kth)[0]
        full = surv.size > CAP
        if full:
            gt = np.nonzero(x > kth)[0]
            surv = np.concatenate([gt, np.nonzero(x == kth)[0][: CAP - gt.size]])
        order = surv[np.lexsort((surv, -x[surv]))]             # stored logit descending, column ascending
        ys = y[order]
        n = m = order.size
        if top_p < 1:
            e = np.exp(ys - ys[0])
            p = e / e.sum()
            tail = np.cumsum(p[::-1])[::-1]
            thr = 1.0 - float(top_p)
            keep_mask = tail > thr
            keep_mask[0] = True
            m = int(keep_mask.sum())
            assert keep_mask[:m].all()
            if n > 1:
                r = float(((U * np.abs(d[order]) + U * np.abs(lp[order])) / T + U * np.abs(ys) + U * abs(ys[0]) + U * np.abs(ys - ys[0])).max())
                p_ok = bool(float(np.min(np.abs(tail[1:] - thr))) > SR.delta(n) + 2 * r)
        kept = order[:m]
    scores = np.full(V, -np.inf)
    scores[kept] = y[kept]
    return dict(kept=kept, y=y, e_y=e_y, scores=scores, full=bool(full), p_ok=p_ok, n_survivors=n)


def prompt_candidates(rows, run, temperature, top_k, top_p):
    """The kept candidates of one prompt: rows f32 [nb, V], run f32 [nb] -> dict(flat, beam, col, acc, e_acc, best, e_best, scores [nb, V],
    e_scores [nb, V], full, p_ok)."""
    nb, V = rows.shape
    flat, beam, col, acc, e_acc, scores, e_scores, xs = [], [], [], [], [], [], [], []
    best, e_best, full, p_ok = -np.inf, 0.0, False, True
    for j in range(nb):
        w = warp_row(rows[j], temperature, top_k, top_p)
        r = float(run[j])
        c = w["kept"]
        a = w["y"][c] + r
        ea = w["e_y"][c] + U * np.abs(a)
        flat.append(j * V + c); beam.append(np.full(c.size, j)); col.append(c); acc.append(a); e_acc.append(ea)
        scores.append(w["scores"]); e_scores.append(w["e_y"]); xs.append(np.asarray(rows[j], dtype=np.float32)[c])
        full |= w["full"]; p_ok &= w["p_ok"]
        i0 = int(np.argmax(w["y"]))
        b0 = w["y"][i0] + r
        if b0 > best:
            best, e_best = b0, w["e_y"][i0] + U * abs(b0)
    cat = np.concatenate
    return dict(flat=cat(flat).astype(np.int64), beam=cat(beam), col=cat(col), acc=cat(acc), e_acc=cat(e_acc), x=cat(xs), best=best, e_best=e_best,
                scores=np.stack(scores), e_scores=np.stack(e_scores), full=full, p_ok=p_ok)


def gumbel(u):
    """g = -log(-log(u)) in fp64 and the bound of its f32 error (docstring)."""
    g = -np.log(-np.log(np.asarray(u, dtype=np.float64)))
    return g, 4 * U + 4 * U * np.abs(g)


def draw(c, seed, prompt, cur, keep):
    """The keep draws of a prompt's candidates `c` in draw order -> dict(top (indices into c's arrays), margin (of the rank decisions),
    flagged (bit 1), flag_margin)."""
    n = c["flat"].size
    g, e_g = gumbel(synth.beam_sample_uniforms(seed, prompt, cur, c["flat"]))
    with np.errstate(invalid="ignore"):
        key = c["acc"] + g
        e_key = c["e_acc"] + e_g + U * np.abs(key)
    order = np.lexsort((c["flat"], -key))
    if n < keep:
        return dict(top=order, margin=np.inf, flagged=True, flag_margin=np.inf, key=key)
    v, e = key[order], e_key[order]
    with np.errstate(invalid="ignore"):
        hi = v + e
        hi = np.where(np.isnan(hi), np.inf, hi)
        suf = np.maximum.accumulate(hi[::-1])[::-1]            # suf[i] = max over j >= i
        later = np.append(suf[1:], -np.inf)[:keep]
        m = float(np.min(v[:keep] - e[:keep] - later))
    if math.isnan(m):
        m = -np.inf
    top = order[:keep]
    a_last, thr = c["acc"][top[-1]], c["best"] - 100.0
    flagged = not (a_last >= thr)
    with np.errstate(invalid="ignore"):
        fm = abs(a_last - thr) - c["e_acc"][top[-1]] - c["e_best"] - U * abs(thr)
    return dict(top=top, margin=m, flagged=bool(flagged), flag_margin=-np.inf if math.isnan(fm) else float(fm), key=key)


def step(logits, st, cur, nb, eos_ids, length_penalty, early_stopping, max_length, pad_id=0, temperature=1.0, top_k=0, top_p=1.0, seed=0,
         prompt0=0, draws=None):
    """logits f32 [B nb, V].  -> dict(state, next_tokens, src_rows, scores fp64 [B nb, V], e_scores, flags (the bits this step raises),
    flagged [B], decidable [B], running_decidable [B], margin [B], running_err, beam_err [B, nb]).  `draws`: per prompt a list of keep
    flat indices that replace the hash's draw (the bookkeeping of somebody else's draws)."""
    logits = np.asarray(logits, dtype=np.float32)
    BB, V = logits.shape
    B = BB // nb
    es = BR.es_code(early_stopping)
    lp_pen = float(np.float32(length_penalty))
    if st["done"] or cur < 0 or cur >= max_length:
        return dict(state=st, next_tokens=np.full(BB, pad_id, dtype=np.int64), src_rows=np.arange(BB, dtype=np.int64), scores=None, e_scores=None,
                    flags=0, flagged=np.zeros(B, dtype=bool), decidable=np.ones(B, dtype=bool), running_decidable=np.ones(B, dtype=bool),
                    margin=np.full(B, np.inf), running_err=np.zeros((B, nb)), beam_err=np.zeros((B, nb)))
    keep = max(2, 1 + len(eos_ids)) * nb
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    next_tokens, src_rows = np.zeros(BB, dtype=np.int64), np.zeros(BB, dtype=np.int64)
    scores, e_scores = np.zeros((BB, V)), np.zeros((BB, V))
    decidable, running_decidable, margins = np.ones(B, dtype=bool), np.ones(B, dtype=bool), np.full(B, np.inf)
    flagged = np.zeros(B, dtype=bool)
    len_pow = float(np.float32((cur + 1) ** lp_pen))
    running_err, beam_err = np.zeros((B, nb)), np.zeros((B, nb))
    stop_flags, bits = [], 0
    for b in range(B):
        c = prompt_candidates(logits[b * nb:(b + 1) * nb], st["running_scores"][b], temperature, top_k, top_p)
        scores[b * nb:(b + 1) * nb], e_scores[b * nb:(b + 1) * nb] = c["scores"], c["e_scores"]
        bits |= 1 if c["full"] else 0
        if draws is not None:
            pos = {int(f): i for i, f in enumerate(c["flat"])}
            top, m1, fm = np.array([pos[int(f)] for f in draws[b]]), np.inf, np.inf
        else:
            dr = draw(c, seed, prompt0 + b, cur, keep)
            top, m1, fm = dr["top"], dr["margin"], dr["flag_margin"]
            flagged[b] = dr["flagged"]
        if flagged[b]:                                          # unspecified from here on: the flag is the result
            bits |= 2
            decidable[b] = bool(c["p_ok"] and fm > 0)
            running_decidable[b] = False
            margins[b] = fm
            stop_flags.append(None)
            continue
        a = c["acc"][top]; e = c["e_acc"][top]; beam = c["beam"][top]; tok = c["col"][top]
        # groups: the same beam and the same stored logit (docstring); everything else compares with a margin
        uniq = np.unique(np.stack([beam.astype(np.float64), c["x"][top].astype(np.float64)]), axis=1, return_inverse=True)[1].reshape(-1)
        hit = np.isin(tok, list(eos_ids)) | (cur + 1 >= max_length)
        live = a + np.where(hit, MASK, 0.0)
        e_live = e + np.where(hit, U * np.abs(live), 0.0)
        o2, m2 = _margin(live, e_live, uniq, nb)
        nxt = o2[:nb]
        just = hit & (np.arange(keep) < nb)
        full = bool(st["is_finished"][b].all()) and es == 1
        open_old = bool(st["heuristic_open"][b])
        fin = a / len_pow
        e_fin = e / len_pow + 2 * U * np.abs(fin)
        elig = np.nonzero(just & open_old & (not full))[0]
        m_val = list(st["beam_scores"][b].astype(np.float64)) + list(fin[elig])
        m_err = [0.0] * nb + list(e_fin[elig])
        m_grp = [-1] * nb + list(uniq[elig])
        o3, m3 = _margin(m_val, m_err, m_grp, nb)
        sel = o3[:nb]
        for r in range(nb):
            k = nxt[r]
            new["running"][b, r] = st["running"][b, beam[k]]
            new["running"][b, r, cur] = tok[k]
            new["running_idx"][b, r] = st["running_idx"][b, beam[k]]
            new["running_idx"][b, r, cur] = b * nb + beam[k]
            new["running_scores"][b, r], running_err[b, r] = live[k], e_live[k] + U * abs(live[k])
            next_tokens[b * nb + r], src_rows[b * nb + r] = tok[k], b * nb + beam[k]
            s = sel[r]
            if s < nb:
                new["sequences"][b, r], new["beam_idx"][b, r] = st["sequences"][b, s], st["beam_idx"][b, s]
                new["beam_scores"][b, r], new["is_finished"][b, r] = st["beam_scores"][b, s], st["is_finished"][b, s]
            else:
                k = elig[s - nb]
                new["sequences"][b, r] = st["running"][b, beam[k]]
                new["sequences"][b, r, cur] = tok[k]
                new["beam_idx"][b, r] = st["running_idx"][b, beam[k]]
                new["beam_idx"][b, r, cur] = b * nb + beam[k]
                new["beam_scores"][b, r], new["is_finished"][b, r], beam_err[b, r] = fin[k], True, e_fin[k] + U * abs(fin[k])
        sc_err = np.array([0.0 if s < nb else e_fin[elig[s - nb]] for s in sel])
        sc = np.array(m_val)[sel]
        fin_new = new["is_finished"][b]
        best_len = max_length if (es == 2 and lp_pen > 0.0) else cur + 1
        bl_pow = float(np.float32(best_len ** lp_pen))
        best = live[nxt[0]] / bl_pow
        e_best = e_live[nxt[0]] / bl_pow + 2 * U * abs(best)
        lo = int(np.argmin(sc))
        worst = np.where(fin_new, sc[lo], MASK)
        e_worst = np.where(fin_new, sc_err[lo], 0.0)
        better = best > worst
        m4 = float(np.min(np.abs(best - worst) - e_best - e_worst)) if open_old else np.inf
        new["heuristic_open"][b] = open_old and bool(better.any())
        all_hits = bool(hit.all())
        stop_flags.append((bool(new["heuristic_open"][b]), bool(fin_new.all()), all_hits))
        running_decidable[b] = m2 > 0 and (m4 > 0 or not open_old)
        decidable[b] = bool(c["p_ok"] and fm > 0 and m1 > 0 and m3 > 0 and (all_hits or running_decidable[b]))
        margins[b] = min(m1, m3, fm, np.inf if all_hits else min(m2, m4))
    if any(f is None for f in stop_flags):                      # a flagged prompt: the stop condition is unspecified with it
        new["done"], new["steps"] = None, None
    else:
        go_on = any(f[0] for f in stop_flags) and not (all(f[1] for f in stop_flags) and es == 1) and not all(f[2] for f in stop_flags)
        if not go_on or cur + 1 >= max_length:
            new["done"], new["steps"] = True, cur + 1
    return dict(state=new, next_tokens=next_tokens, src_rows=src_rows, scores=scores, e_scores=e_scores, flags=bits, flagged=flagged,
                decidable=decidable, running_decidable=running_decidable, margin=margins, running_err=running_err, beam_err=beam_err)


# ---- the synthetic cases of tests/test_gpu_beam_sample_select.py (shared with the host test, which bounds their undecidable share) --------
CASES = [  # (name, V, ld, B0, nb, n_eos, dtype, steps, max_length, length_penalty, early_stopping, temperature, top_k, top_p)
    ("v257_b3_nb3_e1_f32", 257, 320, 3, 3, 1, "f32", 6, 8, 1.0, False, 0.7, 50, 0.9),
    ("v257_b3_nb3_e1_f32_t2", 257, 320, 3, 3, 1, "f32", 6, 8, 1.0, False, 2.0, 50, 0.9),      # the same at a temperature that lets top-p keep enough
    ("v1000_b3_nb5_e2_bf16", 1000, 1024, 3, 5, 2, "bf16", 6, 6, 0.8, True, 1.0, 50, 1.0),
    ("v1000_b3_nb16_e1_bf16", 1000, 1088, 3, 16, 1, "bf16", 5, 8, 1.0, False, 1.3, 200, 1.0),
    ("v1000_b1_nb16_e2_f32", 1000, 1024, 1, 16, 2, "f32", 4, 4, 0.8, True, 1.0, 0, 1.0),
    ("v128256_b1_nb3_e1_bf16", 128256, 128256, 1, 3, 1, "bf16", 4, 6, 1.0, False, 0.7, 50, 0.9),
    ("v128256_b3_nb2_e0_f32", 128256, 128320, 3, 2, 0, "f32", 3, 3, 1.0, False, 1.0, 0, 1.0),
    ("v128256_b1_nb5_e2_bf16", 128256, 128320, 1, 5, 2, "bf16", 3, 8, 0.8, "never", 1.0, 1024, 1.0),
]
SEED = 20260


def case_seed(name):
    return sum(map(ord, name))
