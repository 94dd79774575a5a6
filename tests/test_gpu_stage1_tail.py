"""The stage-1 (contrastive) tail behind the frozen towers -- readout, L2-normalise, InfoNCE row and column terms, adapter forward /
backward, clip + AdamW -- entry point by entry point against the fp64 references of tests/stage1_tail_reference.py, at the smallest
shapes that reach the code paths a cfg3 step runs and the small-shape tests of tests/test_gpu_kernels.py do not:

  readout_bwd_kernel with blockIdx.x > 0 (D = 4096: 16 column blocks); infonce_fwd_kernel / infonce_bwd_kernel with more than one trip
  of their `j += 256` loops over N (N = 300, 512, 8192), of the forward's `c += 256` dot-product loop and of the backward's `c += 1024`
  loop over D (D = 4100, 8192); the N <= 8192 dynamic-LDS limit of both InfoNCE backwards; adamw_kernel at its 2048-block grid cap with
  a second pass of the grid-stride loop (5.2 M and 8.4 M elements); sumsq_partial_kernel past one stride and its scalar tail
  (n = 4097, 2, 1); the weight-gradient GEMMs of p2t_adapter_backward behind p2t_transpose into Mp = round_up(M, 64) columns with the
  zero K padding live (M = 609) and launch_colsum over thousands of rows (M = 8192).

Every output buffer is larger than the contract writes and pre-filled with the sentinel, which must survive; input regions the contract
does not read (padding columns, the backward's workspace) hold NaN.  fp32 caps are the inline ones of the small-shape tests of the same
kernels; the bf16 adapter goes through observe() against the rounding-matched reference."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stage1_tail_reference as R
from gpu_util import SENT, _assert_sentinel, _check, _sentinel, adapter_forward_case, bf16r, dev, observe, rel, to_dev, to_np
from p2t_hip import _lib
from p2t_hip._lib import P2TError, call
from test_gpu_kernels import ops  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
TAU = 0.05
REFUSED = (ValueError, P2TError)          # _lib.call raises ValueError for the library's argument errors (P2T_ERR_ARG), P2TError for every other code


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _flat_sentinel(n, extra=64):
    """A float32 buffer of n + extra sentinels; the contract owns the first n."""
    return _sentinel((n + extra,), torch.float32)


def _tail_kept(buf, n):
    k = to_np(buf)[n:]
    assert np.all(k == SENT), f"{int(np.sum(k != SENT))} stray writes past the end"


# ---- readout ----------------------------------------------------------------------------------------------------------------
READOUT_SHAPES = {"T1021_D4096": dict(B=3, T=1021, D=4096, ld=4096, lens=[1021, 517, 16]),
                  "T70_D72_ld128": dict(B=4, T=70, D=72, ld=128, lens=[70, 33, 2, 1])}
READOUT_CASES = [(s, k, m) for s, k in (("T1021_D4096", "prefix"), ("T70_D72_ld128", "prefix"), ("T70_D72_ld128", "holes"))
                 for m in ("last", "mean", "std", "mix") if not (k == "holes" and m == "last")]      # "last" reads prefix masks only


@functools.lru_cache(maxsize=None)
def _readout_inputs(shape, dt):
    s = READOUT_SHAPES[shape]
    B, T, D, ld = s["B"], s["T"], s["D"], s["ld"]
    emb = (torch.randn((B, T, D), generator=_gen(21)) * 2 + 0.3).to(dt).float().numpy()            # the stored values
    padded = np.full((B, T, ld), np.nan, dtype=np.float32)                                          # pad columns D .. ld-1: never read
    padded[..., :D] = emb
    prefix = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(s["lens"]):
        prefix[b, :n] = 1
    holes = prefix.copy()
    holes[0, 5:9] = 0
    holes[1, 1::3] = 0
    d_out = torch.randn((B, 2 * D), generator=_gen(22)).numpy()
    return SimpleNamespace(B=B, T=T, D=D, ld=ld, emb=emb, emb_dev=to_dev(padded, dt), masks=dict(prefix=prefix, holes=holes), d_out=d_out)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,kind,mode", READOUT_CASES)
def test_readout_forward_backward_vs_fp64(ops, shape, kind, mode, dt):
    """T1021_D4096: T no multiple of 16 or 32, readout_bwd_kernel with blockIdx.x = 0 .. 15 (D / 256 column blocks).  T70_D72_ld128: a row stride
    larger than D with NaN in the padding columns, rows of 2 and 1 tokens, a mask with holes.  bf16 input: against fp64 of the stored values."""
    c = _readout_inputs(shape, dt)
    B, T, D, ld = c.B, c.T, c.D, c.ld
    mask = c.masks[kind]
    W = 2 * D if mode == "mix" else D
    mid, mask_dev = _lib.READOUT[mode], to_dev(mask)

    def forward(mk):
        out = _flat_sentinel(B * W)
        call("p2t_readout", ops.ptr(c.emb_dev), ops.dt_of(dt), ld, ops.ptr(mk), B, T, D, mid, ops.ptr(out), ops.stream())
        _tail_kept(out, B * W)
        return to_np(out)[:B * W].reshape(B, W)

    for mk_dev, mk in ((mask_dev, mask), (None, None)):
        got, ref = forward(mk_dev), R.readout(c.emb, mk, mode).numpy()
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
        if mode == "last":
            _check(got, ref, torch.float32, what="readout last")
        else:
            e = rel(got, ref)
            print(f"readout {shape} {kind} {mode} {dt} mask={'given' if mk is not None else 'None'}: forward rel {e:.3e}")
            assert e < 3e-6
    pooled = _flat_sentinel(B * 2 * D)
    call("p2t_readout", ops.ptr(c.emb_dev), ops.dt_of(dt), ld, ops.ptr(mask_dev), B, T, D, _lib.READOUT["mix"], ops.ptr(pooled), ops.stream())
    d_out = np.ascontiguousarray(c.d_out[:, :W])
    d_emb, d_out_dev = _flat_sentinel(B * T * D, extra=D), to_dev(d_out)
    call("p2t_readout_backward", ops.ptr(c.emb_dev), ops.dt_of(dt), ld, ops.ptr(mask_dev), B, T, D, mid, ops.ptr(pooled), ops.ptr(d_out_dev),
         ops.ptr(d_emb), ops.stream())
    _tail_kept(d_emb, B * T * D)
    g = to_np(d_emb)[:B * T * D].reshape(B, T, D)
    assert not np.any(g == SENT), "d_emb is not fully written"
    gref = R.readout_backward(c.emb, mask, mode, d_out).numpy()
    # the std of a single token is 0: its gradient is 0 / 0 in the reference and in the kernel alike; nothing else is excluded
    rows = [b for b in range(B) if mask[b].sum() > 1 or mode in ("last", "mean")]
    assert len(rows) >= B - 1 and np.all(np.isfinite(gref[rows]))
    assert np.all(g[rows][mask[rows] == 0] == 0), "d_emb is not exactly 0 at masked tokens"
    if mode == "last":
        _check(g[rows], gref[rows], torch.float32, what="readout last backward")
    else:
        e = rel(g[rows], gref[rows])
        print(f"readout {shape} {kind} {mode} {dt}: backward rel {e:.3e}")
        assert e < 1e-5


# ---- L2-normalise -----------------------------------------------------------------------------------------------------------
def test_l2norm_16x8192_edge_rows_vs_fp64(ops):
    """16 x 8192 (32 trips of the `c += 256` loops per lane): a zero row (output 0, backward finite), a row of norm 1e-20 (under eps: divided by
    eps) and one of norm 1e3, each row compared on its own so that the rows scaled by 1 / eps do not hide the others."""
    rows, cols, eps = 16, 8192, 1e-12
    x = torch.randn((rows, cols), generator=_gen(31), dtype=torch.float64) * 0.7 + 0.1
    x[3] = 0.0
    x[5] *= 1e-20 / float(x[5].norm())
    x[7] *= 1e3 / float(x[7].norm())
    x = x.float().numpy()
    dy = torch.randn((rows, cols), generator=_gen(32)).numpy()
    yr, invr, dxr = R.l2norm(x, eps, dy)
    assert all(bool(torch.isfinite(t).all()) for t in (yr, invr, dxr))
    xd, dyd = to_dev(x), to_dev(dy)
    y, inv, dx = _flat_sentinel(rows * cols), _flat_sentinel(rows), _flat_sentinel(rows * cols)
    call("p2t_l2norm_rows", ops.ptr(xd), ops.ptr(y), ops.ptr(inv), rows, cols, eps, ops.stream())
    call("p2t_l2norm_rows_backward", ops.ptr(xd), ops.ptr(dyd), ops.ptr(dx), rows, cols, eps, ops.stream())
    for buf, n in ((y, rows * cols), (inv, rows), (dx, rows * cols)):
        _tail_kept(buf, n)
    yg, dxg = to_np(y)[:rows * cols].reshape(rows, cols), to_np(dx)[:rows * cols].reshape(rows, cols)
    assert np.all(np.isfinite(yg)) and np.all(np.isfinite(dxg)) and not yg[3].any()
    _check(to_np(inv)[:rows], invr.numpy(), torch.float32, rtol=1e-6, what="inv_norm")
    ef = max(rel(yg[r], yr[r].numpy()) for r in range(rows))
    eb = max(rel(dxg[r], dxr[r].numpy()) for r in range(rows))
    print(f"l2norm 16x8192: worst row forward rel {ef:.3e}, backward rel {eb:.3e}")
    assert ef < 1e-6 and eb < 2e-6


# ---- InfoNCE row term -------------------------------------------------------------------------------------------------------
def _unit(seed, n, d):
    return torch.nn.functional.normalize(torch.randn((n, d), generator=_gen(seed), dtype=torch.float64), dim=-1).float().numpy()


def _rows_inputs(S, N, D, seed):
    """L2-normalised seg [S, D] / batch [N, D], labels = N - S .. N - 1; row 1 of seg IS its positive (logit 1 / tau = 20), row 2 the negative of batch row 0
    (logit -20)."""
    seg, batch = _unit(seed, S, D), _unit(seed + 1, N, D)
    labels = (N - S + np.arange(S)).astype(np.int32)
    seg[1] = batch[labels[1]]
    seg[2 % S] = -batch[0]
    return seg, batch, labels


def _infonce_forward(ops, seg, batch, labels, weight=1.0, loss=None, accumulate=False):
    S, D = seg.shape
    N = batch.shape[0]
    loss = _sentinel((2,), torch.float32) if loss is None else loss
    logits, row_loss = _flat_sentinel(S * N), _flat_sentinel(S)
    sd, bd, ld_ = to_dev(seg), to_dev(batch), to_dev(labels)              # named: a temporary's memory could be handed out again before the launch
    call("p2t_infonce_forward", ops.ptr(sd), ops.ptr(bd), ops.ptr(ld_), S, N, D, TAU, float(weight), int(accumulate),
         ops.ptr(loss), ops.ptr(logits), ops.ptr(row_loss), ops.stream())
    _tail_kept(logits, S * N), _tail_kept(row_loss, S)
    assert float(loss[1]) == SENT
    return loss, logits


def _infonce_backward(ops, batch, labels, logits, S, weight=1.0):
    N, D = batch.shape
    d_seg, bd, ld_ = _flat_sentinel(S * D), to_dev(batch), to_dev(labels)
    call("p2t_infonce_backward", ops.ptr(bd), ops.ptr(ld_), ops.ptr(logits), S, N, D, TAU, float(weight), ops.ptr(d_seg), ops.stream())
    _tail_kept(d_seg, S * D)
    return d_seg


def _close_loss(got, ref):
    assert abs(got - ref) < 2e-6 * max(1.0, abs(ref)), (got, ref)


@pytest.mark.parametrize("S,N,D", [(16, 512, 8192), (5, 300, 4100)])
def test_infonce_rows_vs_fp64(ops, S, N, D):
    """(16, 512, 8192): the cfg3 step on 8 ranks -- two trips of the `j += 256` loops over N of infonce_fwd_kernel and infonce_bwd_kernel, 32 trips of the
    forward's `c += 256` dot-product loop, 8 of the backward's `c += 1024` loop over D.  (5, 300, 4100): N no multiple of 4 or 256, D a partial last
    trip of both D loops.  Loss, logits (one exactly 20, one exactly -20) and d_seg, a weight != 1, two accumulated segment calls."""
    seg, batch, labels = _rows_inputs(S, N, D, 41)
    loss_r, logits_r, dseg_r = R.infonce_rows(seg, batch, labels, TAU)
    assert all(bool(torch.isfinite(t).all()) for t in (loss_r, logits_r, dseg_r))
    loss, logits = _infonce_forward(ops, seg, batch, labels)
    lg = to_np(logits)[:S * N].reshape(S, N)
    _close_loss(float(loss[0]), float(loss_r))
    e_l = rel(lg, logits_r.numpy())
    _check([lg[1, labels[1]], lg[2 % S, 0]], [20.0, -20.0], torch.float32, rtol=1e-6, what="extreme logits")
    d = to_np(_infonce_backward(ops, batch, labels, logits, S))[:S * D].reshape(S, D)
    e_g = rel(d, dseg_r.numpy())
    w = 0.37
    _, _, dseg_w = R.infonce_rows(seg, batch, labels, TAU, w)
    e_w = rel(to_np(_infonce_backward(ops, batch, labels, logits, S, weight=w))[:S * D].reshape(S, D), dseg_w.numpy())
    print(f"infonce rows S={S} N={N} D={D}: logits rel {e_l:.3e}, d_seg rel {e_g:.3e}, weighted d_seg rel {e_w:.3e}, loss {float(loss[0]):.7f} vs {float(loss_r):.7f}")
    assert e_l < 1e-6 and e_g < 2e-6 and e_w < 2e-6
    # two segment calls accumulated into one loss, as the step's segment loop does
    a = S // 2
    acc = _sentinel((2,), torch.float32)
    _infonce_forward(ops, seg[:a], batch, labels[:a], weight=0.5, loss=acc, accumulate=False)
    _infonce_forward(ops, seg[a:], batch, labels[a:], weight=0.5, loss=acc, accumulate=True)
    two = float(R.infonce_rows(seg[:a], batch, labels[:a], TAU, 0.5)[0]) + float(R.infonce_rows(seg[a:], batch, labels[a:], TAU, 0.5)[0])
    _close_loss(float(acc[0]), two)


def test_infonce_backward_lds_limit(ops):
    """The N <= 8192 limit of the backwards' dynamic LDS (N floats of coefficients): N = 8192 is accepted and correct (32 trips of the `j += 256` loops),
    N = 8196 is refused by both backwards before anything is written."""
    S, D = 2, 64
    seg, batch, labels = _rows_inputs(S, 8192, D, 43)
    loss_r, logits_r, dseg_r = R.infonce_rows(seg, batch, labels, TAU)
    loss, logits = _infonce_forward(ops, seg, batch, labels)
    _close_loss(float(loss[0]), float(loss_r))
    assert rel(to_np(logits)[:S * 8192].reshape(S, 8192), logits_r.numpy()) < 1e-6
    e = rel(to_np(_infonce_backward(ops, batch, labels, logits, S))[:S * D].reshape(S, D), dseg_r.numpy())
    print(f"infonce backward N=8192: d_seg rel {e:.3e}")
    assert e < 2e-6
    seg, batch, labels = _rows_inputs(S, 8196, D, 45)
    _, logits = _infonce_forward(ops, seg, batch, labels)                    # the forward has no such limit
    d_seg, col_lse = _flat_sentinel(S * D, extra=0), torch.zeros((8196,), device=dev())
    bd, ld_ = to_dev(batch), to_dev(labels)
    with pytest.raises(REFUSED, match="N <= 8192"):
        call("p2t_infonce_backward", ops.ptr(bd), ops.ptr(ld_), ops.ptr(logits), S, 8196, D, TAU, 1.0, ops.ptr(d_seg), ops.stream())
    with pytest.raises(REFUSED, match="N <= 8192"):
        call("p2t_infonce_col_backward", ops.ptr(bd), ops.ptr(ld_), ops.ptr(logits), ops.ptr(col_lse), S, 8196, D, TAU, 1.0, 0, ops.ptr(d_seg), ops.stream())
    assert np.all(to_np(d_seg) == SENT)


# ---- InfoNCE column term ----------------------------------------------------------------------------------------------------
def test_infonce_columns_n512_d8192_vs_fp64(ops):
    """N = 512, D = 8192 (8 ranks x 64): col_lse, the loss over first / count (this rank's 64 columns) and over an explicit unsorted column list, and
    p2t_infonce_col_backward with accumulate = 1 on top of the row gradient at the scale the trainer passes (cw * weight / Bs)."""
    N, D, first, count = 512, 8192, 448, 64
    p, t = _unit(51, N, D), _unit(52, N, D)
    pd, td = to_dev(p), to_dev(t)

    def col_forward(cols, first, count, weight):
        loss, col_lse = _sentinel((2,), torch.float32), _flat_sentinel(N)
        scratch = _flat_sentinel(N * N + N)
        call("p2t_infonce_col_forward", ops.ptr(pd), ops.ptr(td), N, D, TAU, ops.ptr(cols), first, count, float(weight), 0, ops.ptr(loss), ops.ptr(col_lse),
             ops.ptr(scratch), ops.ptr(scratch[N * N:]), ops.stream())
        _tail_kept(col_lse, N), _tail_kept(scratch, N * N + N)
        assert float(loss[1]) == SENT
        return float(loss[0]), col_lse

    loss_r, lse_r, _ = R.infonce_cols(p, t, TAU, cols=np.arange(first, first + count))
    assert bool(torch.isfinite(lse_r).all())
    loss, col_lse = col_forward(None, first, count, 1.0)
    _close_loss(loss, float(loss_r))
    e_lse = rel(to_np(col_lse)[:N], lse_r.numpy())
    cols = np.random.default_rng(53).permutation(N)[:37].astype(np.int32)     # unsorted, no duplicates
    loss_c, _ = col_forward(to_dev(cols), 0, len(cols), 0.25)
    _close_loss(loss_c, 0.25 * float(R.infonce_cols(p, t, TAU, cols=cols)[0]))
    # this rank's row block: the row gradient, then the column term added to it
    cw, weight, Bs = 0.5, 0.125, count
    rows = np.arange(first, first + count)
    labels = rows.astype(np.int32)
    _, logits = _infonce_forward(ops, p[rows], t, labels, weight=weight * (1 - cw))
    d_seg = _infonce_backward(ops, t, labels, logits, count, weight=weight * (1 - cw))
    scale = cw * weight / Bs
    ld_ = to_dev(labels)
    only = _flat_sentinel(count * D)
    call("p2t_infonce_col_backward", ops.ptr(td), ops.ptr(ld_), ops.ptr(logits), ops.ptr(col_lse), count, N, D, TAU, scale, 0, ops.ptr(only), ops.stream())
    call("p2t_infonce_col_backward", ops.ptr(td), ops.ptr(ld_), ops.ptr(logits), ops.ptr(col_lse), count, N, D, TAU, scale, 1, ops.ptr(d_seg), ops.stream())
    _tail_kept(only, count * D), _tail_kept(d_seg, count * D)
    row_r = R.infonce_rows(p[rows], t, labels, TAU, weight * (1 - cw))[2]
    col_r = R.infonce_cols(p, t, TAU, rows=rows, scale=scale)[2]
    both_r = R.infonce_cols(p, t, TAU, rows=rows, scale=scale, d_seg=row_r)[2]
    e_col = rel(to_np(only)[:count * D].reshape(count, D), col_r.numpy())
    e_both = rel(to_np(d_seg)[:count * D].reshape(count, D), both_r.numpy())
    print(f"infonce columns N=512 D=8192: col_lse rel {e_lse:.3e}, column gradient rel {e_col:.3e}, row + column gradient rel {e_both:.3e}")
    assert e_lse < 1e-6 and e_col < 2e-6 and e_both < 2e-6


# ---- adapter forward + backward ---------------------------------------------------------------------------------------------
ADAPTER = dict(X=2560, I=2048, O=4096)


def test_adapter_gemm_forms_at_the_tested_token_counts():
    """The launch forms the bf16 cases below run, from the lab build's planner on 256 CUs without a split-K workspace (p2t_adapter_backward passes none;
    GELU is planned without dropout): the weight-gradient GEMMs dW2 [4096 x 2048, K = Mp] and dW1 [2048 x 2560, K = Mp] are 256 / 160 whole 128-row
    tiles at either token count -- what M changes for them is K and its zero padding -- while dz1 [M x 2048, K = 4096] goes from 40 per-block tiles
    (M = 609) to one whole round of 256 tiles on the persistent kernel (M = 8192), and the forward's fc1 / fc2 to the four-wave persistent one."""
    from test_gemm_plan import BF16, CUS, F32, _plans
    GELU, STORE_F32, GELU_BWD = 1, 4, 5
    X, I, O = ADAPTER["X"], ADAPTER["I"], ADAPTER["O"]
    want = {609: [("tile128", 256, 256, 0, 0), ("tile128", 40, 40, 0, 0), ("tile128", 160, 160, 0, 0), ("tile128", 40, 40, 0, 0), ("tile128", 80, 80, 0, 0)],
            8192: [("tile128", 256, 256, 0, 0), ("persist", 256, 256, 0, 0), ("tile128", 160, 160, 0, 0), ("w4_persist", 256, 256, 0, 0), ("w4_persist", 256, 512, 0, 0)]}
    for M, rows in want.items():
        Mp = (M + 63) // 64 * 64
        got = _plans([(BF16, O, I, Mp, I, Mp, Mp, STORE_F32, F32, 0, CUS, 0), (BF16, M, I, O, I, O, O, GELU_BWD, BF16, 0, CUS, 0),
                      (BF16, I, X, Mp, X, Mp, Mp, STORE_F32, F32, 0, CUS, 0), (BF16, M, I, X, I, X, X, GELU, BF16, 0, CUS, 0),
                      (BF16, M, O, I, O, I, I, GELU, BF16, 0, CUS, 0)])
        assert got == rows, (M, got)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [609, 8192])
def test_adapter_forward_backward_at_the_real_shape_vs_fp64(ops, M, dt):
    """2560 -> 2048 -> 4096, p = 0.3, weights at fan_in^-1/2, the keep-masks read back from the kernel's own h1 / g2.
    M = 609: Mp = 640, so the three transposes (dz2^T, h1^T / dz1^T, x^T) leave 31 columns of zero K padding in a workspace pre-filled with NaN bytes;
    the weight-gradient GEMMs contract over them.  bf16 forms: dW2 tile128 x 256, dz1 tile128 x 40, dW1 tile128 x 160.
    M = 8192: launch_colsum over 8192 rows (128 per chunk), K = 8192 for the weight gradients; bf16 forms: dW2 tile128 x 256, dz1 `persist` with one whole
    round of 256 tiles, dW1 tile128 x 160 (test_adapter_gemm_forms_at_the_tested_token_counts pins them).  f32 runs the FMA GEMM.
    f32: y and the four gradients against adapter_step(round_bf16=False); bf16: against round_bf16=True through observe(), the unrounded error printed.
    A second call with accumulate = 1 must give twice the gradient within the same bound.  M = 609 also: a workspace one byte short is refused and the
    gradient buffers keep the sentinel."""
    X, I, O = ADAPTER["X"], ADAPTER["I"], ADAPTER["O"]
    c = adapter_forward_case(X, I, O, M, X ** -0.5, I ** -0.5, 0.3, dtype=dt, extra_rows=1)
    _assert_sentinel(c.y, rows=M)
    sizes = dict(dW1=I * X, db1=I, dW2=O * I, db2=O)
    bufs = {k: _flat_sentinel(n) for k, n in sizes.items()}
    nb = call("p2t_adapter_backward_workspace_bytes", C.byref(c.cfg), M)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev())                # NaN in either dtype

    def backward(accumulate, nbytes=nb):
        call("p2t_adapter_backward", C.byref(c.cfg), C.byref(c.wts), ops.ptr(c.xg), c.xg.stride(0), M, C.byref(c.saved), ops.ptr(c.dyg), ops.ptr(bufs["dW1"]),
             ops.ptr(bufs["db1"]), ops.ptr(bufs["dW2"]), ops.ptr(bufs["db2"]), accumulate, ops.ptr(ws), nbytes, ops.stream())

    if M == 609:
        with pytest.raises(REFUSED, match="workspace too small"):
            backward(0, nb - 1)
        assert all(np.all(to_np(b) == SENT) for b in bufs.values())
    backward(0)
    once = {k: to_np(bufs[k])[:n].copy() for k, n in sizes.items()}
    backward(1)
    twice = {k: to_np(bufs[k])[:n].copy() for k, n in sizes.items()}
    for k, n in sizes.items():
        _tail_kept(bufs[k], n)
    bf = dt == torch.bfloat16
    names = ("y", "dW1", "db1", "dW2", "db2")
    ref = dict(zip(names, (t.numpy() for t in R.adapter_step(c.x, c.w1, c.b1, c.w2, c.b2, c.m1, c.m2, c.p, c.dy, round_bf16=bf))))
    assert all(np.all(np.isfinite(v)) for v in ref.values())
    got = dict(once, y=to_np(c.y)[:M, :O])
    assert all(np.all(np.isfinite(v)) for v in got.values()) and all(np.all(np.isfinite(v)) for v in twice.values())
    tag = f"stage1_tail.adapter.M{M}"
    if not bf:
        for k in names:
            e1 = rel(got[k], ref[k].reshape(got[k].shape))
            e2 = rel(twice[k], 2 * ref[k].ravel()) if k != "y" else 0.0
            print(f"{tag}.f32.{k}: rel {e1:.3e}, accumulated twice {e2:.3e}")
            assert e1 < 1e-5 and e2 < 1e-5, k
        return
    plain = dict(zip(names, (t.numpy() for t in R.adapter_step(c.x, c.w1, c.b1, c.w2, c.b2, c.m1, c.m2, c.p, c.dy, round_bf16=False))))
    for k in names:
        print(f"{tag}.bf16.{k}: rel vs the rounding-matched reference {rel(got[k], ref[k].reshape(got[k].shape)):.3e}, vs the unrounded one "
              f"{rel(got[k], plain[k].reshape(got[k].shape)):.3e}")
    for k in names:
        observe(f"{tag}.bf16.{k}", rel(got[k], ref[k].reshape(got[k].shape)), 3e-2)
        if k != "y":
            observe(f"{tag}.bf16.{k}.twice", rel(twice[k], 2 * ref[k].ravel()), 3e-2)


# ---- clip + AdamW -----------------------------------------------------------------------------------------------------------
OPT_GROUPS = {"adapter": [(2048, 2560), (2048,), (4096, 2048), (4096,)],      # 5.2 M and 8.4 M elements: adamw_kernel's grid sits at its 2048-block cap and every
              # thread makes a second trip of the grid-stride loop (n > 2048 * 256 * 8 = 4.19 M); sumsq_partial_kernel makes 20 / 32 trips of its stride
              "small": [(70, 72), (4097,), (2,), (1,)]}                       # shadow ld 128 > 72 columns; n % 4 = 1, 2, 1: the scalar tail of the sum of squares
CALLS = ((1, 1.0), (2, 2.0), (3, 3.0), (10000, 1.5))                          # (step, gradient scale): steps 1, 2, 3, then step 10000 on the evolved state


@functools.lru_cache(maxsize=None)
def _opt_base(group):
    g = _gen(61)
    shapes = OPT_GROUPS[group]
    P = [(torch.randn(s, generator=g) * (s[-1] ** -0.5 if len(s) == 2 else 0.1)).numpy() for s in shapes]
    G = [(torch.randn(s, generator=g) * 0.02).numpy() for s in shapes]
    return P, G


@pytest.mark.parametrize("kind", ["inf", "clip", "hair", "zero_grad"])
@pytest.mark.parametrize("group", list(OPT_GROUPS))
def test_clip_adamw_step_vs_fp64(ops, group, kind):
    """p2t_clip_adamw_step over four calls against torch's clip_grad_norm_ + AdamW in fp64.  max_norm: inf | 0.05 (clipping active) | 1.01 x the fp64 total
    norm of that call (inactive by a hair) | 0.05 with two real steps and then an all-zero gradient (norm 0, coefficient clamped to 1) for step 3 and
    step 10000.  After every call: params (rtol 2e-6, atol 1e-7), exp_avg, exp_avg_sq and the norm against the reference, each bf16 shadow bit for bit
    against the rounded params, and the sentinels past every buffer and in the shadows' padding columns.
    exp_avg = m + (g - m)(1 - beta1) in fp32 is three roundings of quantities bounded by max(|m|, |g|), so it is held to rtol 2e-6 plus 1e-6 of the largest
    clipped gradient entry seen so far (the sum can cancel); exp_avg_sq is a sum of non-negative terms: rtol 2e-6."""
    shapes = OPT_GROUPS[group]
    P0, G0 = _opt_base(group)
    n = [int(np.prod(s)) for s in shapes]

    def owned(arrs):
        bufs = [_flat_sentinel(k) for k in n]
        for b, a, k in zip(bufs, arrs, n):
            b[:k] = to_dev(a).view(-1)
        return bufs, [b[:k].view(s) for b, k, s in zip(bufs, n, shapes)]

    pb, dp = owned(P0)
    mb, dm = owned([np.zeros(s, np.float32) for s in shapes])
    vb, dv = owned([np.zeros(s, np.float32) for s in shapes])
    shadow_buf = [_sentinel((s[0] + 1, (s[1] + 63) // 64 * 64 if group == "adapter" else 128), torch.bfloat16) if len(s) == 2 else None for s in shapes]
    shadows = [b[:s[0]] if b is not None else None for b, s in zip(shadow_buf, shapes)]
    p64, m64, v64 = [R.t64(a) for a in P0], [torch.zeros(s, dtype=torch.float64) for s in shapes], [torch.zeros(s, dtype=torch.float64) for s in shapes]
    gmax = 0.0
    for i, (step, gs) in enumerate(CALLS):
        zero = kind == "zero_grad" and i >= 2
        grads = [np.zeros_like(g) if zero else g * np.float32(gs) for g in G0]
        norm64 = math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads))
        max_norm = {"inf": math.inf, "clip": 0.05, "hair": 1.01 * norm64, "zero_grad": 0.05}[kind]
        gn_ref = R.clip_adamw(p64, grads, m64, v64, step, max_norm=max_norm)
        assert abs(gn_ref - norm64) <= 1e-12 * max(norm64, 1e-300) and all(bool(torch.isfinite(t).all()) for t in p64 + m64 + v64)
        coef = min(1.0, max_norm / (norm64 + 1e-6))
        assert (coef < 1.0) == (kind in ("clip", "zero_grad") and not zero)
        gmax = max([gmax] + [coef * float(np.abs(g).max()) for g in grads])
        gn = _sentinel((2,), torch.float32)
        ops.clip_adamw_step(dp, [to_dev(g) for g in grads], dm, dv, step, max_norm=max_norm, shadows=shadows, grad_norm_out=gn)
        assert float(gn[1]) == SENT and abs(float(gn[0]) - gn_ref) <= 1e-5 * gn_ref, (float(gn[0]), gn_ref)
        for j, s in enumerate(shapes):
            what = f"{group} {kind} step {step} tensor {j}"
            np.testing.assert_allclose(to_np(dp[j]), p64[j].numpy(), rtol=2e-6, atol=1e-7, err_msg="params " + what)
            np.testing.assert_allclose(to_np(dm[j]), m64[j].numpy(), rtol=2e-6, atol=1e-6 * gmax, err_msg="exp_avg " + what)
            np.testing.assert_allclose(to_np(dv[j]), v64[j].numpy(), rtol=2e-6, atol=1e-30, err_msg="exp_avg_sq " + what)
            for b in (pb[j], mb[j], vb[j]):
                _tail_kept(b, n[j])
            if shadows[j] is not None:
                assert np.array_equal(to_np(shadows[j])[:, :s[1]], bf16r(to_np(dp[j]))), "shadow " + what
                _assert_sentinel(shadow_buf[j], cols=s[1] if shadow_buf[j].shape[1] > s[1] else None, rows=s[0])
