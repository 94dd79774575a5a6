"""The attention kernels row by row against fp64: csrc/attn_fwd64.hip (the hand-placed forward the towers run), csrc/attn_mfma.hip (the general MFMA
forward), the fp32-softmax forward, csrc/attn_bwd_mfma.hip and the exact backward, each with and without documents (packed rows).

Every element of every query row, padded rows included, is held to its own bound (gpu_util.check_rows; the bounds' terms come from
encoder_ops_reference.attention_fwd_bwd64(bounds=True), the derivation is in tests/tolerance_changes.md).  The inputs are built in
tests/attention_reference.py so that one wrong key shows: two witnesses (q = 0: every visible probability is exactly 1 / n_visible, and v
names the position, the tile, the kv head and the batch row of every key that was read), peaked random inputs whose diagonal resp. boundary
keys dominate a partner row, and the lazy-rescale cases.  Shapes are the smallest at which each kernel's structure is crossed; lengths and
masks vary over the batch rows of one launch.  Operands are built directly as [B, h, T, dp] tensors (qkv_post and rope are pinned in
test_gpu_gemm_forms.py / test_gpu_kernels.py, and q = 0 stays exact); the backward's o, lse and d_o come from the reference.

The fp64 reference runs once per input set and is shared by the routes (a module cache of the current set: the tests are ordered by set)."""
import numpy as np
import pytest
import torch

import attention_reference as R
from gpu_util import _assert_sentinel, _sentinel, attn_grad_bounds, attn_lse_bound, attn_o_bound, check_rows, to_dev, to_np
from p2t_hip import _lib, ops
from p2t_hip._lib import call
from p2t_hip.ops import ptr, round_up, stream

pytestmark = pytest.mark.gpu
REFUSED = (ValueError, _lib.P2TError)
F32, BF16 = torch.float32, torch.bfloat16

# forward routes: dtype, use_mfma (None: the general kernel -- 2 where the hand-placed one would apply, else 1), log2_scores, lse asked for,
# P rounded to bf16, row sums over the rounded P.  The scale form runs on the same q with scale = ln 2: the same logits, one reference.
FWD = {
    "exact_f32": (F32, 0, False, True, False, False),
    "exact_l2": (BF16, 0, True, True, False, False),
    "exact_sc": (BF16, 0, False, True, False, False),
    "general_l2": (BF16, None, True, True, True, False),
    "general_sc": (BF16, None, False, True, True, False),
    "hand_lse": (BF16, 3, True, True, True, True),
    "hand": (BF16, 3, True, False, True, True),
}
FWD_OF = {"g64": tuple(FWD), "g40": ("exact_f32", "exact_l2", "general_l2", "hand_lse", "hand"), "h64": ("exact_l2", "general_l2", "hand_lse", "hand"),
          "g128": tuple(FWD)[:5], "g24": tuple(FWD)[:5], "doc64": tuple(FWD)[:5], "doc128": tuple(FWD)[:5]}
# backward routes: dtype, use_mfma, log2_scores
BWD = {"exact_f32": (F32, 0, False), "exact_bf16": (BF16, 0, True), "mfma": (BF16, 1, True)}
BWD_OF = lambda c: tuple(BWD) if c.d in (64, 128) else tuple(BWD)[:2]

_BWD_SETS = set(R.backward_cases())
_SETS = sorted(set(R.forward_cases()) | _BWD_SETS, key=lambda c: c.name)
_current = {}


def _set(c):
    """Inputs, fp64 reference (with the backward where the set has one) and device-side mask / documents of one input set."""
    if _current.get("case") != c:
        x = R.inputs(c)
        ref = R.reference(c, x, c in _BWD_SETS)
        R.assert_conditions(c, x, ref)
        mask = c.mask()
        key_mask, kv_info, _ = ops.mask_prepare(to_dev(mask))
        start, pos = c.docs()
        docs = None
        if start is not None:
            docs = ops.doc_prepare(to_dev(np.where(mask != 0, pos, 0)), to_dev(mask))
            want = np.stack([start, np.where(mask != 0, _doc_end(start), np.arange(c.T) + 1)]).astype(np.int32)
            assert docs is not None and np.array_equal(to_np(docs), want)
        _current.clear()
        _current.update(case=c, x=x, ref=ref, mask=mask, key_mask=key_mask, kv_info=kv_info, docs=docs, dev={})
    return _current


def _doc_end(start):
    end = np.empty_like(start)
    for b in range(start.shape[0]):
        edges = np.flatnonzero(np.diff(start[b], append=start.shape[1]) != 0) + 1
        end[b] = np.repeat(edges, np.diff(np.concatenate([[0], edges])))
    return end


def _operands(s, dt, x=None):
    """q, k, v as [B, h, T, dp] device tensors of dtype dt, pad columns [d, dp) zero (x: other inputs than the set's own; not kept)."""
    c = s["case"]
    dp = ops.head_dim_padded(c.d)
    pad = lambda a: to_dev(np.concatenate([a, np.zeros(a.shape[:-1] + (dp - c.d,), np.float32)], -1), dt)
    if x is not None:
        return tuple(pad(x[n]) for n in ("q", "k", "v"))
    if dt not in s["dev"]:
        s["dev"][dt] = tuple(pad(s["x"][n]) for n in ("q", "k", "v"))
    return s["dev"][dt]


def _rows_to_heads(t, B, T, nh, d):
    """[B*T, ld] -> [B, nh, T, d] (numpy)."""
    return to_np(t)[:B * T, :nh * d].reshape(B, T, nh, d).transpose(0, 2, 1, 3)


def _heads_to_rows(a, ld, dt):
    """[B, nh, T, d] -> device [B*T, ld], pad columns zero."""
    B, nh, T, d = a.shape
    out = np.zeros((B * T, ld), np.float32)
    out[:, :nh * d] = a.transpose(0, 2, 1, 3).reshape(B * T, nh * d)
    return to_dev(out, dt)


def _general(c, l2s):
    return 2 if ops.head_dim_padded(c.d) == 64 and c.d % 8 == 0 and l2s else 1


def _forward(s, qkv, dt, use, l2s, want_lse):
    """One p2t_attention / p2t_attention_docs call into a buffer one row longer and 64 columns wider than the contract writes.
    -> out [B*T + 1, ld + 64] (sentinel outside the contract's columns), lse [B, nh, T] or None."""
    c = s["case"]
    B, ld, dp = s["mask"].shape[0], round_up(c.nh * c.d, 64), ops.head_dim_padded(c.d)
    out = _sentinel((B * c.T + 1, ld + 64), dt)
    lse = _sentinel((B, c.nh, c.T), F32) if want_lse else None
    q, k, v = qkv
    scale = 1.0 if l2s else R.LN2
    if s["docs"] is not None:
        call("p2t_attention_docs", ptr(q), ptr(k), ptr(v), ptr(s["key_mask"]), ptr(s["kv_info"]), ptr(s["docs"]), ptr(out), ld + 64, B, c.T, c.nh, c.nkv,
             c.d, dp, scale, ops.dt_of(dt), use, int(l2s), ptr(lse), stream())
    else:
        call("p2t_attention", ptr(q), ptr(k), ptr(v), ptr(s["key_mask"]), ptr(s["kv_info"]), ptr(out), ld + 64, B, c.T, c.nh, c.nkv, c.d, dp, scale,
             int(c.causal), ops.dt_of(dt), use, int(l2s), ptr(lse), stream())
    return out, lse


def _forward_rows(c, route):
    s = _set(c)
    ref = s["ref"]
    dt, use, l2s, want_lse, p_bf16, sum_rounded = FWD[route]
    B, ld = s["mask"].shape[0], round_up(c.nh * c.d, 64)
    out, lse = _forward(s, _operands(s, dt), dt, _general(c, l2s) if use is None else use, l2s, want_lse)
    full = to_np(out)
    assert not full[:B * c.T, c.nh * c.d:ld].any(), "the pad columns of the last head, up to the next multiple of 64, are zeroed"
    _assert_sentinel(out, cols=ld, rows=B * c.T)
    parts = [("o", _rows_to_heads(out, B, c.T, c.nh, c.d), ref["o"], attn_o_bound(ref, p_bf16, dt == BF16, c.witness))]
    if want_lse:
        parts.append(("lse", to_np(lse), ref["lse"], attn_lse_bound(ref, sum_rounded, c.witness)))
    check_rows(f"attn_rows[{c.shape},{route},{'witness' if c.witness else 'peaked'}]", parts)


def _auto_route_is_the_documented_one(c, _route):
    """use_mfma = -1 on bf16 operands (csrc/gemm.hip, attention()): the hand-placed kernel when no lse is asked for and the shape is eligible
    (head_dim padded to 64, d % 8 == 0, log2 scores, no documents), else the general MFMA kernel -- bit for bit.  With documents the
    hand-placed kernel is refused."""
    s = _set(c)
    qkv = _operands(s, BF16)
    eligible = ops.head_dim_padded(c.d) == 64 and c.d % 8 == 0 and s["docs"] is None
    for l2s in (True, False):
        for want_lse in (False, True):
            hand = eligible and l2s and not want_lse
            a, la = _forward(s, qkv, BF16, -1, l2s, want_lse)
            b, lb = _forward(s, qkv, BF16, 3 if hand else _general(c, l2s), l2s, want_lse)
            assert torch.equal(a, b) and (not want_lse or torch.equal(la, lb)), (l2s, want_lse)
            if hand:                                     # and the two kernels are different programs: their outputs differ somewhere
                g, _ = _forward(s, qkv, BF16, 2, True, False)
                assert not torch.equal(a, g)
    if not eligible:
        with pytest.raises(REFUSED):
            _forward(s, qkv, BF16, 3, True, False)


def _backward(s, qkv, dt, use, l2s, ref):
    """One attention_backward call on o (bf16 operands: the reference's o rounded to bf16; fp32: to fp32), lse (fp32) and d_o of the reference."""
    c = s["case"]
    ld = round_up(c.nh * c.d, 64)
    o = _heads_to_rows(ref["o16"] if dt == BF16 else ref["o"].astype(np.float32), ld, dt)
    d_o = _heads_to_rows(s["x"]["d_o"], ld, dt)
    lse = to_dev(ref["lse"].astype(np.float32))
    q, k, v = qkv
    return ops.attention_backward(q, k, v, o, d_o, lse, s["key_mask"], s["kv_info"], c.d, R.LN2, c.causal, log2_scores=l2s, use_mfma=use, docs=s["docs"])


def _backward_rows(c, route):
    """o (rounded to the operands' dtype), lse (fp32) and d_o (non-zero everywhere) come from the reference, so a forward defect cannot fail
    this test.  Rows that see no key carry lse = +inf and get dq = 0; hidden keys get dk = dv = 0: both exactly (their bounds are 0)."""
    s = _set(c)
    dt, use, l2s = BWD[route]
    ref = s["ref"] if dt == BF16 else s["ref"]["f32"]          # D = rowsum(dO o O) from the O this route is handed
    grads = _backward(s, _operands(s, dt), dt, use, l2s, ref)
    bounds = attn_grad_bounds(ref, route == "mfma", c.d)
    parts = []
    for nm, g in zip(("dq", "dk", "dv"), grads):
        gn = to_np(g)
        assert not gn[..., c.d:].any(), (nm, "padded head-dim columns [d, dp) are zero")
        parts.append((nm, gn[..., :c.d], ref[nm], bounds[nm]))
    check_rows(f"attn_rows[{c.shape},bwd_{route},{'witness' if c.witness else 'peaked'}]", parts)


# ---- hidden keys hold anything finite -----------------------------------------------------------------------------------------------
HIDDEN_SETS = [R.Case("g64", "masks", False, "diag"), R.Case("g64", "masks", True, "diag"), R.Case("g64", "lens", True, "diag"),
               R.Case("g128", "masks", True, "diag"), R.Case("g24", "masks", False, "diag"), R.Case("h64", "masks", False, "diag"),
               R.Case("h64", "lens", True, "diag"), R.Case("doc64", "docs", True, "diag"), R.Case("doc128", "docs", True, "diag")]


def _with_hidden(s, value):
    """The set's inputs with the K and V rows of hidden keys (mask = 0; with documents: the padding behind them) holding +-value."""
    x = {n: s["x"][n].copy() for n in ("q", "k", "v")}
    sign = np.where(np.arange(s["case"].T) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for n in ("k", "v"):
        hid = np.broadcast_to((s["mask"] == 0)[:, None, :, None], x[n].shape)
        x[n][hid] = np.broadcast_to((value * sign)[None, None, :, None], x[n].shape)[hid]
    return x


def _hidden_keys_never_reach_a_result(c, _route):
    """K and V rows of hidden keys hold +-2^40 in one run and 0 in another: every forward route's output and lse, and every backward route's dq,
    dk, dv, must be bit-identical.  (Finite values only: Inf or NaN there is outside the kernels' contract, 0 x inf in the PV product.)"""
    s = _set(c)
    assert (s["mask"] == 0).any()
    xs = [_with_hidden(s, 2.0 ** 40), _with_hidden(s, 0.0)]
    assert not np.array_equal(xs[0]["k"], xs[1]["k"])
    for route in FWD_OF[c.shape]:
        dt, use, l2s, want_lse, _, _ = FWD[route]
        a, b = (_forward(s, _operands(s, dt, x), dt, _general(c, l2s) if use is None else use, l2s, want_lse) for x in xs)
        assert torch.equal(a[0], b[0]) and (not want_lse or torch.equal(a[1], b[1])), route
    if c in _BWD_SETS:
        for route in BWD_OF(c):
            dt, use, l2s = BWD[route]
            a, b = (_backward(s, _operands(s, dt, x), dt, use, l2s, s["ref"]) for x in xs)
            for nm, ga, gb in zip(("dq", "dk", "dv"), a, b):
                assert torch.equal(ga, gb), (route, nm)


# ---- the tests, ordered by input set so that each set's reference is computed once --------------------------------------------------
_FWD_SETS = set(R.forward_cases())
_KINDS = {"fwd": _forward_rows, "bwd": _backward_rows, "auto": _auto_route_is_the_documented_one, "hidden": _hidden_keys_never_reach_a_result}
TESTS = []
for _c in _SETS:
    if _c in _FWD_SETS:
        TESTS += [(_c, "fwd", r) for r in FWD_OF[_c.shape]]
        if _c.flavour == "boundary":
            TESTS.append((_c, "auto", "all"))
    if _c in _BWD_SETS:
        TESTS += [(_c, "bwd", r) for r in BWD_OF(_c)]
    if _c in HIDDEN_SETS:
        TESTS.append((_c, "hidden", "all"))


@pytest.mark.parametrize("c,kind,route", TESTS, ids=[f"{c.name}-{k}-{r}" for c, k, r in TESTS])
def test_attention_rows(c, kind, route):
    """fwd / bwd: one route on one input set, row by row against fp64; auto: the default route is the documented one, bit for bit; hidden:
    what hidden keys hold never reaches a result."""
    _KINDS[kind](c, route)
