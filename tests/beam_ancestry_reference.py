"""numpy restatement of beam search without the cache copy (include/p2t_hip.h, "beam search without the cache copy"; csrc/kv_cache.hip,
csrc/attn_decode.hip): the generated keys stay in the physical row that wrote them, and ancestry[r][i] names the row of r's prompt
(0 .. group - 1) that holds key i of beam row r's history.  numpy only.

* `ancestry_update`: the table after p2t_kv_ancestry_update at counter `step`, out of place;
* `gather`: a beam row's generated segment read through the table -- what p2t_kv_reorder's copies would have materialised;
* `reorder`: p2t_kv_reorder's copy rule (the first `step` keys of row src[r]), for the comparison of the two;
* `decode_attention_beams`: the gather, then continuous_reference.decode_attention_rows on the gathered segment (fp64 operands: the
  fp64 reference)."""
import numpy as np

import continuous_reference as R


def ancestry_update(anc, src_rows, step, group):
    """anc u8 [BB, G] -> the new table: new[r][i] = old[src[r]][i] (i < s), new[r][s] = r % group, columns > s as they were; s =
    clamp(step, 0, G - 1); a source outside r's prompt is clamped into it."""
    BB, G = anc.shape
    s = min(max(int(step), 0), G - 1)
    new = anc.copy()
    for r in range(BB):
        lo = r // group * group
        sr = min(max(int(src_rows[r]), lo), lo + group - 1)
        new[r, :s] = anc[sr, :s]
        new[r, s] = r % group
    return new


def gather(seg, anc, n, group):
    """seg [BB, ..., G, d] (key axis -2) -> the same shape with keys 0 .. n - 1 of row r taken from row r // group * group + anc[r][i];
    keys >= n are zero."""
    out = np.zeros_like(seg)
    for r in range(seg.shape[0]):
        lo = r // group * group
        for i in range(n):
            out[r, ..., i, :] = seg[lo + int(anc[r, i]), ..., i, :]
    return out


def reorder(seg, src_rows, step):
    """p2t_kv_reorder: row r <- the first `step` keys of row src_rows[r]; what lies behind them is not copied (zero here)."""
    out = np.zeros_like(seg)
    for r in range(seg.shape[0]):
        out[r, ..., :step, :] = seg[int(src_rows[r]), ..., :step, :]
    return out


def decode_attention_beams(q, kp, vp, kg, vg, lens, step, anc, group, scale):
    """q [BB, nh, d]; prompt keys / values [B0, nkv, Tp, d]; generated [BB, nkv, G, d] in PHYSICAL rows; lens int [B0]; step: the shared
    counter; anc u8 [BB, G] -> (o, A) of continuous_reference.decode_attention_rows over each beam's own history."""
    BB = q.shape[0]
    n1 = int(step) + 1
    rep = lambda a: np.repeat(a, group, axis=0)
    return R.decode_attention_rows(q, rep(kp), rep(vp), gather(kg, anc, n1, group), gather(vg, anc, n1, group), rep(np.asarray(lens)),
                                   np.full(BB, int(step)), scale)
