"""numpy restatement of what continuous batching's kernels compute (include/p2t_hip.h, "continuous batching"; csrc/llama_decode.hip, csrc/kv_cache.hip, csrc/attn_decode.hip):
every row carries its own step counter.  numpy only.

* `decode_attention_rows`: one query token per row over prompt_len[r] keys of its prompt segment and row_step[r] + 1 keys of its
  generated segment (test_gpu_generate._attn_ref's formula with the counter indexed by row);
* `rotate`: the rotation of one head at one position, HF's rotate_half convention on the pairs (j, j + d / 2), with its error bound
  when the input went through a bf16 rounding;
* `greedy_select_rows`: the state p2t_greedy_select_rows leaves behind;
* `kv_slot_load`: the state p2t_kv_slot_load leaves behind."""
import numpy as np

F32 = np.float32


def decode_attention_rows(q, kp, vp, kg, vg, lens, row_step, scale):
    """q [B, nh, d]; prompt keys / values [B, nkv, Tp, d], generated [B, nkv, G, d]; lens, row_step int [B] -> (o [B, nh, d], A = P |v|:
    the term of gpu_util.attn_o_bound), in the operands' precision (fp64 operands: the fp64 reference)."""
    B, nh, d = q.shape
    nkv = kp.shape[1]
    G = nh // nkv
    out, A = np.zeros((B, nh, d), dtype=q.dtype), np.zeros((B, nh, d), dtype=q.dtype)
    for b in range(B):
        n0, n1 = int(lens[b]), int(row_step[b]) + 1
        for h in range(nh):
            kv = h // G
            k = np.concatenate([kp[b, kv, :n0], kg[b, kv, :n1]], 0)
            v = np.concatenate([vp[b, kv, :n0], vg[b, kv, :n1]], 0)
            s = (k @ q[b, h]) * scale
            p = np.exp(s - s.max())
            out[b, h], A[b, h] = (p / p.sum()) @ v, (p / p.sum()) @ np.abs(v)
    return out, A


def rotate(x, inv_freq, pos):
    """x [..., d] (fp64) at integer position `pos`: the angle is the f32 product pos * inv_freq[j], as the kernels form it -> (rotated
    [..., d], S = |x_j| + |x_{j + d/2}| per element: what an input perturbation is multiplied by at most)."""
    x = np.asarray(x, dtype=np.float64)
    half = x.shape[-1] // 2
    a = (F32(pos) * np.asarray(inv_freq, dtype=F32)).astype(np.float64)
    c, s = np.cos(a), np.sin(a)
    x1, x2 = x[..., :half], x[..., half:]
    S = np.abs(x1) + np.abs(x2)
    return np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], -1), np.concatenate([S, S], -1)


def rotate_bound_bf16(ref, S):
    """|kernel - rotate(bf16(x))| where the kernel rotates the f32 x and rounds once.  bf16 keeps 8 significant bits: round to nearest
    moves a value by at most 2^-8 of itself.  The input's rounding goes through the rotation (at most 2^-8 S), the output's own is 2^-8 of
    the unrounded result (|ref| + 2^-8 S at most); f32 sin / cos / products stay below 2^-16 S."""
    return (2.0 ** -8 + 2.0 ** -15) * S + 2.0 ** -8 * np.abs(ref)


def greedy_select_rows(logits, V, finished, next_tokens, out_tokens, row_step, row_limit, eos_ids, pad_id, row_map=None):
    """Updates finished / next_tokens / out_tokens (numpy arrays, in place) as the kernel does.  logits [n, >= V]."""
    G = out_tokens.shape[1]
    for i in range(logits.shape[0]):
        r = i if row_map is None else int(row_map[i])
        if not 0 <= r < len(finished):                           # a row the engine does not have touches nothing
            continue
        if finished[r]:
            next_tokens[r] = pad_id
            continue
        tok = int(np.argmax(logits[i, :V]))                      # numpy: the first among equal maxima, as torch.argmax
        st = min(max(int(row_step[r]), 0), G - 1)
        next_tokens[r] = out_tokens[r, st] = tok
        finished[r] |= (1 if tok in eos_ids else 0) | (2 if st + 1 >= int(row_limit[r]) else 0)


def kv_slot_load(cache, staging, slots, limits):
    """cache / staging: dicts of numpy arrays -- prompt tensors [L, rows, ...] under "k", "vt" (and "ks", "vs"), counters under "lens"
    (and, cache only, "row_step", "finished", "row_limit").  In place."""
    for i, s in enumerate(slots):
        for name in ("k", "vt", "ks", "vs"):
            if name in cache:
                cache[name][:, s] = staging[name][:, i]
        cache["lens"][s], cache["row_step"][s], cache["finished"][s], cache["row_limit"][s] = staging["lens"][i], 0, 0, limits[i]
