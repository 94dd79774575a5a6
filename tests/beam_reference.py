"""fp64 restatement of one p2t_beam_select step (include/p2t_hip.h; csrc/beam_select.hip), for tests/test_beam_reference_host.py,
tests/test_gpu_beam_select.py and tests/test_gpu_generate_beam.py.

`step` takes the stored logits widened to f32 and a state (numpy arrays, one half of the kernel's double-buffered tables) and returns
the new state, next_tokens, src_rows and the stop flag, computed in fp64 with the header's definitions and its rank keys: candidates
by (acc descending, beam ascending, stored logit descending, column ascending), the later ranks by (value descending, position
ascending).  State values that are f32 in the kernel (run_scores, fin_scores) enter as the exact f32 numbers they are.

DECIDABLE.  The kernel evaluates  acc = fl(fl(fl(x - mx) - lse) + run)  in f32 (header, steps 1-2), the restatement in fp64.  Inside
one beam both orders agree whatever the rounding: x -> acc, acc -> acc + (-1e9) and acc -> acc / len_pow are monotone in f32, equal
stored logits give equal keys, and the position rule then follows the stored-logit order.  The old finished slots compare among
themselves as the exact f32 numbers the state holds.  Every OTHER comparison the rule makes (two candidates of different beams, a
candidate against an old finished slot, the best running score against the worst finished one) is decidable when the fp64 gap exceeds
the sum of the two values' error bounds, derived from the formula with u = 2^-24 (one rounding to nearest):
  d = fl(x - mx):             |err| <= u |d|
  e = expf(d):                relative 4 u (two ulp; the documented accuracy of expf / logf is one) + u |d| from d's own rounding
  S = sum of V terms e <= 1:  relative (depth + 4) u + u mean_p|d|,  depth = ceil(V / 1024) + 8 + 6 + 16 additions on the longest path
                              (a thread's columns, the 64-lane butterfly, the 16 waves); mean_p|d| = entropy - log S <= ln V
  lse = logf(S):              |err| <= (depth + 4 + ln V) u + 4 u |lse|
  t = fl(d - lse):            |err| <= u |d| + err(lse) + u |t|
  acc = fl(t + run):          |err| <= err(t) + u |acc|                                                   =: E(acc)
  live = fl(acc + (-1e9)):    E(acc) + u |live|     (hits only; the others keep acc)
  fin = fl(acc / len_pow):    E(acc) / len_pow + 2 u |fin|   (len_pow = float(pow(cur + 1, length_penalty)): its rounding and the division's)
  run / len_pow (heuristic):  E(run) / len_pow + 2 u |quotient|,  E(run) = the bound of the running score just computed.
Nothing here is fitted to observed errors.  A masked finished candidate (not a hit, rank >= nb, prompt closed, or all slots finished
under early_stopping=True) has a score of at most -1e9 after its masks and a later position than every old slot, whose scores are at
least -1e9: it never enters, in f32 as in fp64, so it is left out of the merge and needs no margin.
When every candidate is a hit (cur + 1 == max_length) all live scores collapse around -1e9 (ulp 64): the order of the new RUNNING rows
and the open flag are then undecidable, but nothing reads them -- the search is done; `running_decidable` says so and the tests
compare the finished side only."""
import math

import numpy as np

U = 2.0 ** -24
MASK = -1.0e9


def depth(V: int) -> int:
    return -(-V // 1024) + 8 + 6 + 16


def fresh_state(B, nb, L, pad_id):
    run_sc = np.zeros((B, nb), dtype=np.float32)
    run_sc[:, 1:] = MASK
    return dict(running=np.full((B, nb, L), pad_id, dtype=np.int64), running_idx=np.full((B, nb, L), -1, dtype=np.int32), running_scores=run_sc,
                sequences=np.full((B, nb, L), pad_id, dtype=np.int64), beam_idx=np.full((B, nb, L), -1, dtype=np.int32),
                beam_scores=np.full((B, nb), MASK, dtype=np.float32), is_finished=np.zeros((B, nb), dtype=bool),
                heuristic_open=np.ones((B,), dtype=bool), done=False, steps=0)


def es_code(early_stopping) -> int:
    """False / True / "never" (or the C ABI's 0 / 1 / 2) -> 0 / 1 / 2."""
    if early_stopping is True or (type(early_stopping) is int and early_stopping == 1):
        return 1
    if (isinstance(early_stopping, str) and early_stopping == "never") or (type(early_stopping) is int and early_stopping == 2):
        return 2
    return 0


def _margin(vals, errs, groups, n_top):
    """Ranks by (value descending, position ascending); -> (order, smallest gap - error sum over the pairs (i in the top n_top, j after
    it) of different groups; inf when there is none).  Group -1 entries are exact among themselves."""
    vals, errs, groups = np.asarray(vals, dtype=np.float64), np.asarray(errs, dtype=np.float64), np.asarray(groups)
    order = np.lexsort((np.arange(len(vals)), -vals))
    v, e, g = vals[order], errs[order], groups[order]
    m = np.inf
    for i in range(min(n_top, len(v))):
        other = g[i + 1:] != g[i]
        if other.any():
            m = min(m, float(np.min((v[i] - v[i + 1:] - e[i] - e[i + 1:])[other])))
    return order, m


def row_stats(x32):
    """One row of f32 logits -> (mx, lse, lp fp64 [V], the bound of lse's f32 error)."""
    x = x32.astype(np.float64)
    mx = x.max()
    lse = math.log(np.exp(x - mx).sum())
    V = x.shape[0]
    return mx, lse, (x - mx) - lse, (depth(V) + 4 + math.log(V)) * U + 4 * U * abs(lse)


def step(logits, st, cur, nb, eos_ids, length_penalty, early_stopping, max_length, pad_id=0):
    """logits f32 [B nb, V].  -> dict(state, next_tokens, src_rows, log_probs, decidable [B] bool, running_decidable [B] bool,
    margin [B], and the f32 error bounds running_err [B, nb], beam_err [B, nb] (0 for a slot carried over), lp_err [B nb] (of a row's
    log-probabilities))."""
    logits = np.asarray(logits, dtype=np.float32)
    BB, V = logits.shape
    B = BB // nb
    es = es_code(early_stopping)
    lp_pen = float(np.float32(length_penalty))
    if st["done"] or cur < 0 or cur >= max_length:
        return dict(state=st, next_tokens=np.full(BB, pad_id, dtype=np.int64), src_rows=np.arange(BB, dtype=np.int64), log_probs=None,
                    decidable=np.ones(B, dtype=bool), running_decidable=np.ones(B, dtype=bool), margin=np.full(B, np.inf),
                    running_err=np.zeros((B, nb)), beam_err=np.zeros((B, nb)), lp_err=np.zeros(BB))
    keep = max(2, 1 + len(eos_ids)) * nb
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    next_tokens, src_rows = np.zeros(BB, dtype=np.int64), np.zeros(BB, dtype=np.int64)
    log_probs = np.zeros((BB, V), dtype=np.float64)
    decidable, running_decidable, margins = np.ones(B, dtype=bool), np.ones(B, dtype=bool), np.full(B, np.inf)
    len_pow = float(np.float32((cur + 1) ** lp_pen))
    running_err, beam_err, lp_err = np.zeros((B, nb)), np.zeros((B, nb)), np.zeros(BB)
    flags = []
    for b in range(B):
        c_acc, c_err, c_beam, c_tok = [], [], [], []
        for j in range(nb):
            x32 = logits[b * nb + j]
            mx, lse, lp, e_lse = row_stats(x32)
            log_probs[b * nb + j] = lp
            lp_err[b * nb + j] = e_lse + 2 * U * float(np.abs(lp).max())
            cols = np.lexsort((np.arange(V), -x32.astype(np.float64)))[:keep]      # stored logit descending, column ascending
            run = float(st["running_scores"][b, j])
            d = x32[cols].astype(np.float64) - mx
            acc = lp[cols] + run
            c_acc += list(acc)
            c_err += list(U * np.abs(d) + e_lse + U * np.abs(lp[cols]) + U * np.abs(acc))
            c_beam += [j] * keep
            c_tok += list(cols)
        order, m1 = _margin(c_acc, c_err, c_beam, keep)                             # positions are (beam, rank inside the beam) already
        top = order[:keep]
        a = np.array(c_acc)[top]; e = np.array(c_err)[top]; beam = np.array(c_beam)[top]; tok = np.array(c_tok)[top]
        hit = np.isin(tok, list(eos_ids)) | (cur + 1 >= max_length)
        live = a + np.where(hit, MASK, 0.0)
        e_live = e + np.where(hit, U * np.abs(live), 0.0)
        o2, m2 = _margin(live, e_live, beam, nb)
        nxt = o2[:nb]
        just = hit & (np.arange(keep) < nb)
        full = bool(st["is_finished"][b].all()) and es == 1
        open_old = bool(st["heuristic_open"][b])
        fin = a / len_pow
        e_fin = e / len_pow + 2 * U * np.abs(fin)
        elig = np.nonzero(just & open_old & (not full))[0]
        m_val = list(st["beam_scores"][b].astype(np.float64)) + list(fin[elig])
        m_err = [0.0] * nb + list(e_fin[elig])
        m_grp = [-1] * nb + list(beam[elig])
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
        # the open / closed heuristic
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
        flags.append((bool(new["heuristic_open"][b]), bool(fin_new.all()), all_hits))
        running_decidable[b] = m2 > 0 and (m4 > 0 or not open_old)
        decidable[b] = m1 > 0 and m3 > 0 and (all_hits or running_decidable[b])
        margins[b] = min(m1, m3, np.inf if all_hits else min(m2, m4))
    go_on = any(f[0] for f in flags) and not (all(f[1] for f in flags) and es == 1) and not all(f[2] for f in flags)
    if not go_on or cur + 1 >= max_length:
        new["done"], new["steps"] = True, cur + 1
    return dict(state=new, next_tokens=next_tokens, src_rows=src_rows, log_probs=log_probs, decidable=decidable,
                running_decidable=running_decidable, margin=margins, running_err=running_err, beam_err=beam_err, lp_err=lp_err)


def score_delta(V, score, steps=1):
    """Bound of a returned score's f32 error after `steps` accumulated steps: every step adds one lse bound, the roundings of d, t and of
    the running sum (|values| <= |score| + ln V + 40), and the final division."""
    per = (depth(V) + 4 + math.log(V)) * U + 4 * U * math.log(V) + 3 * U * (abs(score) + math.log(V) + 40.0)
    return steps * per + 2 * U * abs(score)


# ---- the synthetic cases of tests/test_gpu_beam_select.py (shared with the host test, which bounds their undecidable share) ----------------
def to_dtype(x, dtype):
    """f32 array -> the values a tensor of `dtype` ("f32" | "bf16") stores, as f32 (round to nearest even)."""
    x = np.asarray(x, dtype=np.float32)
    if dtype == "f32":
        return x
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def case_logits(seed, step_no, BB, V, dtype, eos_ids):
    """Gaussian rows (sigma 3) with, on some rows, an eos column lifted next to the row's best: eos hits above and below rank nb."""
    rng = np.random.default_rng([seed, step_no, BB, V])
    x = (rng.standard_normal((BB, V)) * 3.0).astype(np.float32)
    for r in range(BB):
        if eos_ids and rng.random() < 0.5:
            e = eos_ids[int(rng.integers(len(eos_ids)))]
            x[r, e] = np.sort(x[r])[-1 - int(rng.integers(0, 4))] + np.float32(rng.random() * 0.5 - 0.1)
    return to_dtype(x, dtype)


CASES = [  # (name, V, ld, B0, nb, n_eos, dtype, steps, max_length, length_penalty, early_stopping)
    ("v257_b3_nb3_e1_f32", 257, 320, 3, 3, 1, "f32", 6, 8, 1.0, False),
    ("v257_b1_nb1_e0_f32", 257, 257, 1, 1, 0, "f32", 5, 5, 0.0, False),
    ("v1000_b3_nb5_e2_bf16", 1000, 1024, 3, 5, 2, "bf16", 6, 6, 0.8, True),
    ("v1000_b1_nb2_e1_f32", 1000, 1000, 1, 2, 1, "f32", 7, 7, 2.0, "never"),
    ("v1000_b3_nb16_e1_bf16", 1000, 1088, 3, 16, 1, "bf16", 5, 8, 1.0, False),
    ("v1000_b1_nb16_e2_f32", 1000, 1024, 1, 16, 2, "f32", 4, 4, 0.8, True),
    ("v128256_b1_nb3_e1_bf16", 128256, 128256, 1, 3, 1, "bf16", 4, 6, 1.0, False),
    ("v128256_b3_nb2_e0_f32", 128256, 128320, 3, 2, 0, "f32", 3, 3, 1.0, False),
    ("v128256_b1_nb5_e2_bf16", 128256, 128320, 1, 5, 2, "bf16", 3, 8, 0.8, "never"),
]


def case_eos(V, n_eos):
    return [V - 1, 7][:n_eos]
