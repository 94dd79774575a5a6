"""numpy reference of the padding-free prefill of ragged prompts (include/p2t_hip.h, "padding-free prefill"; p2t_hip/generation.py,
plan_prompt_rows): the planner's contract, packing and unpacking a prompt batch, and where p2t_kv_store_packed puts every element.
fp8 codes come through tests/kv8_reference.py."""
import numpy as np

import kv8_reference as K8

ROW_MULTIPLE = 64            # Tpk: 64-key tiles of the attention kernels and of the store
TOKENS_MAX = 32768           # the default row capacity (a guard on buffer sizes)


def check_plan(lens, pack_tokens, R, Tpk, place):
    """Every clause of plan_prompt_rows' contract on its own result; raises AssertionError with the clause that fails."""
    lens = [int(n) for n in lens]
    cap = TOKENS_MAX if pack_tokens is None else int(pack_tokens)
    assert len(place) == len(lens), "every prompt placed once, in batch order"
    rows = {}
    for b, (row, start, n) in enumerate(place):
        assert n == lens[b] and 0 <= row < R and start >= 0, f"prompt {b}: placement {row, start, n}"
        rows.setdefault(row, []).append((start, n, b))
    assert sorted(rows) == list(range(R)), "no empty row"
    used = []
    for row in range(R):
        at = 0
        for start, n, b in sorted(rows[row]):
            assert start == at, f"row {row}: prompt {b} starts at {start}, the previous one ends at {at} (back to back, no overlap)"
            at += n
        assert at <= cap, f"row {row} holds {at} tokens, more than {cap}"
        used.append(at)
    assert Tpk % ROW_MULTIPLE == 0 and max(used) <= Tpk < max(used) + ROW_MULTIPLE, f"Tpk {Tpk} is not the fullest row ({max(used)}) rounded up"
    # first-fit decreasing, ties in batch order: replay it
    room, want = [], [None] * len(lens)
    for b in sorted(range(len(lens)), key=lambda i: (-lens[i], i)):
        r = next((r for r in range(len(room)) if room[r] >= lens[b]), None)
        if r is None:
            r = len(room)
            room.append(cap)
        want[b] = (r, cap - room[r], lens[b])
        room[r] -= lens[b]
    assert [tuple(p) for p in place] == want, "first-fit decreasing order"


def prompt_index(mask):
    """p2t_prompt_index: -> (index i32 [B, T]: r for the r-th token under the mask, -1 off it; lens i32 [B])."""
    on = np.asarray(mask) != 0
    idx = np.where(on, np.cumsum(on, axis=1) - 1, -1).astype(np.int32)
    return idx, on.sum(1).astype(np.int32)


def compact_rows(x, mask):
    """p2t_compact_rows: valid tokens first, zeros behind."""
    out = np.zeros_like(x)
    for b in range(x.shape[0]):
        v = x[b][np.asarray(mask[b]) != 0]
        out[b, : len(v)] = v
    return out


def pack_rows(x, mask, R, Tpk, place):
    """p2t_pack_rows: -> (packed [R, Tpk, H], mask i64 [R, Tpk], position_ids i32 [R, Tpk])."""
    out = np.zeros((R, Tpk, x.shape[2]), dtype=x.dtype)
    om, pos = np.zeros((R, Tpk), dtype=np.int64), np.zeros((R, Tpk), dtype=np.int32)
    for b, (row, start, n) in enumerate(place):
        out[row, start:start + n] = x[b][np.asarray(mask[b]) != 0]
        om[row, start:start + n] = 1
        pos[row, start:start + n] = np.arange(n)
    return out, om, pos


def unpack_rows(packed, place, T):
    """The inverse: -> compacted [B, T, H] (prompt b's tokens first, zeros behind)."""
    out = np.zeros((len(place), T, packed.shape[2]), dtype=packed.dtype)
    for b, (row, start, n) in enumerate(place):
        out[b, :n] = packed[row, start:start + n]
    return out


def kv_store(k, v, place, Tp, k_cache, vt_cache):
    """p2t_kv_store_packed on ONE layer's buffers: k, v [R, nkv, Tpk, dp]; k_cache [n, nkv, Tp, dp] and vt_cache [n, nkv, dp, Tp] are
    updated in place (copies of what the cache held): rows / columns 0 .. len - 1 of prompt i, nothing else."""
    for i, (row, start, n) in enumerate(place):
        assert n <= Tp
        k_cache[i, :, :n] = k[row, :, start:start + n]
        vt_cache[i, :, :, :n] = v[row, :, start:start + n].transpose(0, 2, 1)


def kv_store_fp8(k, v, place, d, k_codes, vt_codes, k_scale, v_scale):
    """The fp8 form: k, v bf16-rounded f32 [R, nkv, Tpk, dp]; columns d .. dp count as zero.  Updates codes u8 [n, nkv, Tp, dp] /
    [n, nkv, dp, Tp] and scales u8 [n, nkv, Tp] in place with kv8_reference.quant_keys' bytes."""
    for i, (row, start, n) in enumerate(place):
        for src, codes, scale, tr in ((k, k_codes, k_scale, False), (v, vt_codes, v_scale, True)):
            x = src[row, :, start:start + n].copy()
            x[..., d:] = 0
            c, E, _ = K8.quant_keys(x)
            scale[i, :, :n] = E
            if tr:
                codes[i, :, :, :n] = c.transpose(0, 2, 1)
            else:
                codes[i, :, :n] = c
