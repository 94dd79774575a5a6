"""The quantised LM head on its own (include/p2t_hip.h p2t_lm_head_q / p2t_lm_head_logits_q; csrc/llama_decode.hip on the weight stream
of csrc/gemm_skinny.hip): final RMSNorm -> e4m3 rows -> e4m3 / MXFP4 head, both layouts, vocabularies that end inside a 16-row tile and
inside an NT-tile block, an output pitch larger than the vocabulary, hidden sizes whose K is padded to 128 with and without zeros.

* exact-integer witness: normalised rows and head entries exactly representable, every logit an integer below 256 -- equal bit for bit;
* random operands: within lm_head_q_reference.bound of the fp64 product of the returned activation codes and the de-quantised head;
  the returned codes and scale bytes are the fp8 step's row quantiser's rule restated in fp64 (_check_rows_quantised: the step's
  quantiser is not exported and the exported p2t_rmsnorm_fp8 sums the squares in another order, so a code may sit on either side of a
  rounding boundary that the f32 row touches, never further); rows that are normalised already (norm_w = NULL, the prefill's form)
  equal p2t_quant_rows_fp8's codes and scales bit for bit;
* stream order == row-major bit for bit; the head's codes / scales equal the quantiser restatements."""
import numpy as np
import pytest
import torch

import lm_head_q_reference as Q
from gpu_util import bf16r, dev, rnd, to_dev, to_np

pytestmark = pytest.mark.gpu
SENT = -12352.0                                         # exact in bf16
SHAPES = [(M, V, H) for M in (1, 8, 17, 64) for V in (300, 1000) for H in (64, 192, 256)] + [(8, 128256, 4096)]
# two tiles per block (NT = 2: from 384 tiles of 16 rows at 17 .. 64 rows, from 1 024 tiles below that) on an ODD count of tiles whose
# last one is cut after 8 rows: the last block's second tile lies wholly behind the vocabulary.  6 184 -> 387 tiles, 16 392 -> 1 025
SHAPES += [(17, 6184, 192), (64, 6184, 192), (1, 16392, 64), (8, 16392, 64)]
_ids = lambda s: "x".join(str(v) for v in s)


def _heads(fmt, w):
    """bf16 head [V, >= H] on the device -> ((row-major descriptor, stream-order descriptor), codes, scales, keep-alive)."""
    from p2t_hip import _lib, ops
    from p2t_hip.generation import preshuffle, preshuffle_mxfp4
    V, H = w.shape[0], w.shape[1]
    mx = fmt == "mxfp4"
    codes, scales = ops.quant_rows_mxfp4(w, H) if mx else ops.quant_rows_fp8(w, H)
    pre = preshuffle_mxfp4(codes, scales, V) if mx else preshuffle(codes, V)
    f = _lib.LM_HEAD_MXFP4 if mx else _lib.LM_HEAD_E4M3
    rm = _lib.LmHeadQC(format=f, stream_order=0, codes=codes.data_ptr(), scales=scales.data_ptr(), ld=codes.stride(0))
    so = _lib.LmHeadQC(format=f, stream_order=1, codes=pre.data_ptr(), scales=None if mx else scales.data_ptr(), ld=0)
    return (rm, so), codes, scales, pre


def _run(x, nw, eps, head, V, ld):
    from p2t_hip.generation import lm_head_logits_q
    out = torch.full((x.shape[0], ld), SENT, dtype=torch.bfloat16, device=dev())
    return lm_head_logits_q(x, nw, eps, head, V, ld, return_act=True, out=out)


def _witness(M, V, H, seed):
    """x = signs * a power of two per row (mean square = that power squared: the normalised row is the signs), norm weight 2 or 4 per
    column -> activation rows of +-2 / +-4; the head: per vocabulary row up to 20 blocks of 32 columns with ONE non-zero each, +-{0.5, 1,
    1.5} * 2^{0, 1} at a column of its own -- an e2m1 value under the block's own scale and an e4m3 value under the row's.  Every
    logit is a sum of at most 20 integers of magnitude <= 12: an integer below 256 that depends on the row's signs (row), on the
    columns and values picked (vocabulary row, K block) and on the block's scale byte."""
    rs = np.random.RandomState(seed)
    sign = rs.randint(0, 2, size=(M, H)).astype(np.float32) * 2 - 1
    x = sign * np.ldexp(np.float32(1.0), (np.arange(M) % 5 - 2))[:, None].astype(np.float32)
    nw = rs.choice([2.0, 4.0], size=H).astype(np.float32)
    nb = H // 32
    nz = min(nb, 20)
    blocks = np.stack([rs.permutation(nb)[:nz] for _ in range(min(V, 4096))])           # [<= 4096, nz], tiled over the vocabulary
    blocks = blocks[np.arange(V) % blocks.shape[0]]
    cols = (blocks * 32 + rs.randint(0, 32, size=(V, nz))).astype(np.int64)
    vals = (rs.choice([0.5, 1.0, 1.5], size=(V, nz)) * rs.choice([1.0, 2.0], size=(V, nz)) * rs.choice([-1.0, 1.0], size=(V, nz))).astype(np.float32)
    w = torch.zeros((V, H), dtype=torch.bfloat16, device=dev())
    w.scatter_(1, to_dev(cols), to_dev(vals, torch.bfloat16))
    act = sign * nw[None, :]
    ref = (act[:, cols] * vals[None]).sum(-1)                                            # [M, V], exact in f32: integers
    assert np.abs(act[:, cols] * vals[None]).sum(-1).max() < 256 and np.array_equal(ref, np.round(ref))
    return x, nw, w, act, ref


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_integer_witness(shape, fmt):
    M, V, H = shape
    x, nw, w, act, ref = _witness(M, V, H, M * 7919 + V * 31 + H)
    heads, codes, scales, _keep = _heads(fmt, w)
    rows = np.unique(np.concatenate([np.arange(min(V, 64)), np.arange(max(V - 64, 0), V)]))     # the quantised head holds w exactly (sampled rows)
    assert np.array_equal(Q.head_values(fmt, to_np(codes[rows]), to_np(scales[rows]), H), to_np(w[rows]).astype(np.float64))
    ld = (V + 63) // 64 * 64 + 64
    outs = []
    for head in heads:
        out, aq, asc = _run(to_dev(x), to_dev(nw), 0.0, head, V, ld)
        assert np.array_equal(Q.e4m3_values(to_np(aq), to_np(asc), H), act.astype(np.float64))          # the normalised rows are exact in e4m3
        assert (to_np(aq)[:, H:] == 0).all()
        o = to_np(out)
        assert np.array_equal(o[:, :V], ref), f"{int((o[:, :V] != ref).sum())} logits differ from their integers"
        assert (o[:, V:] == SENT).all()                                                                # the pad columns are not written
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def _check_rows_quantised(x, nw, eps, aq, asc):
    """The activation rows the GEMM read are the fp8 step's: RMSNorm in f32, one E8M0 byte per row by p2t_quant_rows_fp8's rule (the
    smallest 2^e with amax / 2^e <= 448), e4m3 codes of y / 2^e, K padded with zeros.  The step's RMSNorm sums the squares in an order of
    its own, so y is known to f32 accuracy only (4e-7 relative here): a code may sit on either side of a rounding boundary that y touches
    within that, never further -- half an e4m3 step (2^-4 relative, 2^-10 2^e under the normal range) plus that slack."""
    from oracle import p2t_oracle as O
    H = x.shape[1]
    x64 = x.astype(np.float64)
    y = x64 / np.sqrt((x64 ** 2).mean(-1, keepdims=True) + eps) * nw.astype(np.float64)
    amax = np.abs(y).max(-1)
    lo, hi = (np.asarray(O.e8m0_of_amax((amax * s).astype(np.float32))).astype(np.int64) for s in (1 - 1e-6, 1 + 1e-6))
    assert ((asc == lo) | (asc == hi)).all(), "row scale bytes"
    got = Q.e4m3_values(aq, asc, H)
    step = np.maximum(2.0 ** -4 * np.abs(y), np.ldexp(2.0 ** -10, asc.astype(np.int64) - 127)[:, None])
    assert (np.abs(got - y) <= step * (1 + 1e-5) + 4e-7 * np.abs(y)).all() and (aq[:, H:] == 0).all()


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_random_operands_within_the_derived_bound(shape, fmt):
    from p2t_hip import ops
    M, V, H = shape
    big = V > 4096
    x = rnd(71, "hq.x", (M, H), 1.0) * np.exp(rnd(71, "hq.xs", (M, 1), 2.0)).astype(np.float32)
    nw = (1.0 + rnd(71, "hq.nw", (H,), 0.5)).astype(np.float32)
    if big:                                              # filled on the device; the reference reads a sample of its rows
        w = ops.fill_hash_(torch.empty((V, H), dtype=torch.bfloat16, device=dev()), 71, "hq.w", 0.02)
        rows = np.unique(np.concatenate([np.arange(96), np.arange(V - 96, V), np.random.RandomState(5).randint(0, V, 320)]))
    else:
        w = to_dev(bf16r(rnd(71, "hq.w", (V, H), 0.5) * np.exp(rnd(71, "hq.ws", (V, 1), 1.0)).astype(np.float32) / np.float32(np.sqrt(H))), torch.bfloat16)
        rows = np.arange(V)
    heads, codes, scales, _keep = _heads(fmt, w)
    wt = Q.head_values(fmt, to_np(codes[rows]), to_np(scales[rows]), H)
    want, want_sc = Q.quantise_head(fmt, to_np(w[rows]))
    assert np.array_equal(wt, want) and np.array_equal(to_np(scales[rows]).reshape(want_sc.shape), want_sc)      # the quantiser restatements
    ld = (V + 63) // 64 * 64 + 64
    eps = 1e-5
    outs, acts = [], []
    for head in heads:
        out, aq, asc = _run(to_dev(x), to_dev(nw), eps, head, V, ld)
        _check_rows_quantised(x, nw, eps, to_np(aq), to_np(asc))
        acts.append((aq, asc))
        ref, abs_sum = Q.logits(Q.e4m3_values(to_np(aq), to_np(asc), H), wt)
        o = to_np(out).astype(np.float64)
        err, bnd = np.abs(o[:, rows] - ref), Q.bound(ref, abs_sum, (H + 127) // 128 * 128)
        assert np.isfinite(o[:, :V]).all() and (err <= bnd).all(), f"{int((err > bnd).sum())} logits off, worst err / bound {float((err / bnd).max()):.3g}"
        assert (o[:, V:] == SENT).all()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(acts[0][0], acts[1][0]) and torch.equal(acts[0][1], acts[1][1])
    # rows that are normalised already (the prefill's form): the same GEMM on p2t_quant_rows_fp8's codes
    y = rnd(71, "hq.y", (M, H), 1.0)
    out, aq, asc = _run(to_dev(y), None, 0.0, heads[0], V, ld)
    qy, sy = ops.quant_rows_fp8(to_dev(y), H)
    assert torch.equal(aq, qy) and torch.equal(asc, sy)
    ref, abs_sum = Q.logits(Q.e4m3_values(to_np(aq), to_np(asc), H), wt)
    assert (np.abs(to_np(out).astype(np.float64)[:, rows] - ref) <= Q.bound(ref, abs_sum, (H + 127) // 128 * 128)).all()


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_more_than_64_rows_run_the_general_gemm_on_e4m3_codes(fmt):
    """80 rows: the e4m3 head's own codes, or the MXFP4 head's e4m3 copy of the same values; within the same bound, and the rows a
    64-row call shares with it agree with the skinny path within the two paths' bounds."""
    from p2t_hip import ops
    M, V, H = 80, 1008, 192                              # the general GEMM takes a vocabulary that is a multiple of 16, as for the bf16 head
    x = rnd(72, "hq.x", (M, H), 1.0)
    nw = (1.0 + rnd(72, "hq.nw", (H,), 0.5)).astype(np.float32)
    w = to_dev(bf16r(rnd(72, "hq.w", (V, H), 0.5) / np.float32(np.sqrt(H))), torch.bfloat16)
    heads, codes, scales, _keep = _heads(fmt, w)
    head = heads[0]
    if fmt == "mxfp4":
        c8, s8 = ops.quant_rows_fp8(ops.dequant_rows_mxfp4(codes, scales, H, 256), H)
        head.codes_e4m3, head.scales_e4m3 = c8.data_ptr(), s8.data_ptr()
        assert np.array_equal(Q.e4m3_values(to_np(c8), to_np(s8), H), Q.head_values(fmt, to_np(codes), to_np(scales), H))
    wt = Q.head_values(fmt, to_np(codes), to_np(scales), H)
    ld = 1024
    out, aq, asc = _run(to_dev(x), to_dev(nw), 1e-5, head, V, ld)
    ref, abs_sum = Q.logits(Q.e4m3_values(to_np(aq), to_np(asc), H), wt)
    o = to_np(out).astype(np.float64)
    assert (np.abs(o[:, :V] - ref) <= Q.bound(ref, abs_sum, 256)).all()
    few, _, _ = _run(to_dev(x[:64]), to_dev(nw), 1e-5, head, V, ld)
    assert (np.abs(to_np(few).astype(np.float64)[:, :V] - o[:64, :V]) <= 2 * Q.bound(ref[:64], abs_sum[:64], 256)).all()
