"""fp64 restatement of p2t_sample_select (include/p2t_hip.h; csrc/sample_select.hip), for tests/test_sampling_reference_host.py,
tests/test_gpu_sample_select.py and tests/test_gpu_generate_sampling.py.

Per row, on the stored logits cast to f32: x = logit / temperature is the f32 quotient (the kernel's scores ARE these values, and
two logits the division makes equal are a tie); everything after that is fp64 with the kernel's definitions:
  * kth = the min(top_k, V)-th largest x; survivors x >= kth; more than CAP of them: all x > kth, then the ties in ascending column
    order until CAP, and the `full` flag;
  * ranks: value descending, column ascending among equal values;
  * p_j = exp(x_j - x_0) / S; rank j kept iff tail_j = sum_{i >= j} p_i > 1 - top_p (top_p as the f32 the kernel gets), rank 0 always;
  * token = the kept rank with the smallest j such that cum_j = sum_{i <= j} e_i > u * S_kept, else the last kept rank;
  * both filters off: the same inverse CDF over all V columns in ascending column order.
Two margins say how far the row's two decisions are from their thresholds: m_p = min_j |tail_j - (1 - top_p)| (j >= 1; rank 0 is
kept whatever its tail), m_u = min_j |cum_j / S_kept - u|.  A row is DECIDABLE when both exceed delta = (n_survivors + 8) * 2^-23:
the worst-case f32 error of a sequential sum of n terms plus the rounding of exp and of u -- an f32 evaluation in any order then
takes the same decisions."""
import numpy as np

CAP = 2048


def delta(n: int) -> float:
    return (n + 8) * 2.0 ** -23


def scaled(logits, temperature):
    """x: the f32 quotients (IEEE division, as the kernel's)."""
    return np.asarray(logits, dtype=np.float32) / np.float32(temperature)


def inverse_cdf(e, u):
    """e: unnormalised masses in draw order -> (position, m_u)."""
    cum = np.cumsum(np.asarray(e, dtype=np.float64))
    S = cum[-1]
    over = np.nonzero(cum > u * S)[0]
    pos = int(over[0]) if over.size else len(cum) - 1
    return pos, float(np.min(np.abs(cum / S - u)))


def sample_row(logits, temperature, top_k, top_p, u):
    """One row -> dict(token, kept (sorted columns), scores f32 [V], n_survivors, full, m_p, m_u, decidable, ties_at_kth,
    ties_at_cut)."""
    x32 = scaled(logits, temperature)
    x = x32.astype(np.float64)
    V = x.shape[0]
    top_k = 0 if top_k is None else int(top_k)
    top_p = np.float32(1.0 if top_p is None else top_p)
    if top_k <= 0:
        assert top_p >= 1, "top_p without top_k is not a supported combination"
        pos, m_u = inverse_cdf(np.exp(x - x.max()), u)
        return dict(token=pos, kept=np.arange(V), scores=x32.copy(), n_survivors=V, full=False, m_p=np.inf, m_u=m_u,
                    decidable=m_u > delta(V), ties_at_kth=0, ties_at_cut=False)
    k = min(top_k, V)
    kth = np.partition(x, V - k)[V - k]
    surv = np.nonzero(x >= kth)[0]
    ties_at_kth = int((x == kth).sum())
    full = surv.size > CAP
    if full:
        gt = np.nonzero(x > kth)[0]
        surv = np.concatenate([gt, np.nonzero(x == kth)[0][: CAP - gt.size]])
    order = surv[np.lexsort((surv, -x[surv]))]             # value descending, column ascending
    xs = x[order]
    n = order.size
    e = np.exp(xs - xs[0])
    m, m_p, ties_at_cut = n, np.inf, False
    if top_p < 1:
        p = e / e.sum()
        tail = np.cumsum(p[::-1])[::-1]
        thr = 1.0 - float(top_p)
        kept = tail > thr
        kept[0] = True
        m = int(kept.sum())
        assert kept[:m].all()
        if n > 1:
            m_p = float(np.min(np.abs(tail[1:] - thr)))
        ties_at_cut = bool(m < n and xs[m - 1] == xs[m])
    pos, m_u = inverse_cdf(e[:m], u)
    scores = np.full(V, -np.inf, dtype=np.float32)
    scores[order[:m]] = x32[order[:m]]
    d = delta(n)
    return dict(token=int(order[pos]), kept=np.sort(order[:m]), scores=scores, n_survivors=n, full=bool(full), m_p=m_p, m_u=m_u,
                decidable=bool(m_p > d and m_u > d), ties_at_kth=ties_at_kth, ties_at_cut=ties_at_cut)


def sample_rows(logits, temperature, top_k, top_p, us):
    """[rows, V] and one u per row -> list of sample_row results."""
    return [sample_row(logits[r], temperature, top_k, top_p, float(us[r])) for r in range(len(logits))]


def bookkeeping(tokens, finished, eos_ids, pad_id):
    """greedy_select_kernel's rule: -> (next, finished after)."""
    tokens, finished = np.asarray(tokens, dtype=np.int64), np.asarray(finished).astype(bool)
    nxt = np.where(finished, pad_id, tokens)
    return nxt, (finished | (~finished & np.isin(nxt, np.asarray(list(eos_ids), dtype=np.int64)))).astype(np.int32)
