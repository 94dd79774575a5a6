"""The entry points of the bf16 stage-2 step (p2t_hip/decoder_train.py) one by one against numpy fp64, at the shapes and edges the
step reaches: p2t_swiglu_gu (forward / backward, interleaved gate / up), p2t_rope_backward_pack (+ _docs), p2t_qkv_post_docs,
p2t_dropout_rows, the shifted cross-entropy (plain / weighted, forward / backward) at real vocabularies, p2t_rmsnorm_backward at
the residual width and in the Qwen3 head-norm form, p2t_scale_by_device_scalar.

fp32 outputs are held to ~1e-6 relative; a bf16 output must be within one rounding step (one bf16 ulp) of the fp64 result.  Every
output buffer is wider than the columns the entry point's contract writes, and the extra columns / rows hold a sentinel that must
survive (a stray write shows up as a failed assertion, not as a fault)."""
import numpy as np
import pytest
import torch

from gpu_util import _assert_sentinel, _check, _q, _sentinel, dev, to_np
from p2t_hip import _lib, ops
from p2t_hip._lib import call
from p2t_hip.decoder_train import _deinterleave, _interleave
from p2t_hip.ops import ptr, round_up, stream

pytestmark = pytest.mark.gpu
DTS = (torch.float32, torch.bfloat16)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [1, 37, 1216])
@pytest.mark.parametrize("F", [32, 96, 1376, 14336])
def test_swiglu_gu_forward_and_backward(F, M, dtype):
    rng = np.random.default_rng(F * 7 + M)
    gate = rng.standard_normal((M, F)) * 4
    gate.ravel()[: min(gate.size, 181)] = np.linspace(-90, 90, 181)[: min(gate.size, 181)]   # the expf overflow range and 0
    up = rng.standard_normal((M, F))
    da = rng.standard_normal((M, F))
    g64, u64, da64 = _q(gate, dtype), _q(up, dtype), _q(da, dtype)
    ld_gu, Fp = 2 * F + 64, round_up(F, 64)
    ld_out = Fp + 64
    gu = _sentinel((M, ld_gu), dtype)
    gu[:, :2 * F] = _interleave(torch.from_numpy(g64).to(dev(), dtype), torch.from_numpy(u64).to(dev(), dtype), F)
    act = _sentinel((M + 1, ld_out), dtype)
    call("p2t_swiglu_gu", ptr(gu), ld_gu, None, 0, ptr(act), ld_out, M, F, ops.dt_of(dtype), stream())
    sg = 1.0 / (1.0 + np.exp(-g64))
    _check(to_np(act)[:M, :F], g64 * sg * u64, dtype, what="act")
    assert np.all(to_np(act)[:M, F:Fp] == 0), "the K padding [F, round_up(F, 64)) is zeroed"
    _assert_sentinel(act, cols=Fp, rows=M)
    # backward: d_gu in the same interleaved layout
    d_act = _sentinel((M, ld_out), dtype)
    d_act[:, :F] = torch.from_numpy(da64).to(dev(), dtype)
    d_gu = _sentinel((M + 1, 2 * F + 64), dtype)
    call("p2t_swiglu_gu", ptr(gu), ld_gu, ptr(d_act), ld_out, ptr(d_gu), d_gu.stride(0), M, F, ops.dt_of(dtype), stream())
    dg, du = _deinterleave(d_gu[:M], F)
    ref_dg = da64 * u64 * sg * (1 + g64 * (1 - sg))
    ref_du = da64 * g64 * sg
    # where expf(-g) overflows (g < -88) sigma is 0 in fp32: both derivatives vanish, as their limits do (|ref| < 1e-35 there);
    # 1 + g (1 - sigma) crosses 0 near g = -1.28: an absolute term at the scale of its summands
    _check(to_np(dg), ref_dg, dtype, atol=2e-6 * np.abs(da64 * u64 * sg) * (1 + np.abs(g64)) + 1e-35, what="d_gate")
    _check(to_np(du), ref_du, dtype, atol=1e-35, what="d_up")
    _assert_sentinel(d_gu, cols=2 * F, rows=M)


# ---------------------------------------------------------------------------------------------
ROW_LENS = ([1, 63, 1, 130, 301, 1, 65, 200, 129], [512, 1, 511])        # as tests/test_gpu_packed_sft.py: row 0 ends in padding
LONG_LENS = ([1, 1000, 2047, 700],)                                     # T = 4096, 348 padding tokens


def _layout(kind, T):
    """(pos [B, T], mask [B, T], docs or None, starts [B, T] as numpy)."""
    if kind == "arange":
        B = 2
        pos = torch.arange(T).expand(B, T).contiguous()
        mask = torch.ones((B, T), dtype=torch.int64)
        mask[1, T - 5:] = 0
        return pos, mask, None, np.zeros((B, T), dtype=np.int64)
    lens = ROW_LENS if T == 1024 else LONG_LENS
    B = len(lens)
    pos = torch.zeros((B, T), dtype=torch.int64)
    mask = torch.zeros((B, T), dtype=torch.int64)
    for b, ls in enumerate(lens):
        t = 0
        for n in ls:
            pos[b, t:t + n] = torch.arange(n)
            mask[b, t:t + n] = 1
            t += n
    docs = ops.doc_prepare(pos.to(dev()), mask.to(dev()))
    assert docs is not None
    starts = to_np(docs[0]).astype(np.int64)
    t = np.arange(T)[None]
    assert np.all((t - starts)[mask.numpy() == 0] == 0), "a padding token has position 0"
    return pos, mask, docs, starts


def _inv_freq(d, kind):
    import stage2_reference as S
    return S.inv_freq_of(d, 500000.0, "llama3") if kind == "llama3" else S.inv_freq_of(d, 10000.0)


def _cs(inv_freq, pt):
    """fp64 cos / sin at the kernels' fp32 angle fp32(pt) * inv_freq: [B, T, d/2]."""
    ang = (pt.astype(np.float32)[..., None] * inv_freq.numpy().astype(np.float32)[None, None]).astype(np.float64)
    return np.cos(ang), np.sin(ang)


ROPE_CASES = [(16, 4, 4, "arange", 4096, "default"), (48, 32, 8, "packed", 1024, "llama3"), (64, 4, 4, "packed", 4096, "llama3"),
              (64, 32, 8, "arange", 1024, "default"), (128, 32, 8, "packed", 1024, "llama3"), (128, 4, 4, "packed", 4096, "default"),
              (48, 4, 4, "arange", 256, "llama3"), (16, 32, 8, "packed", 1024, "default")]


@pytest.mark.parametrize("dtype", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("d,nh,nkv,kind,T,rope", ROPE_CASES)
def test_rope_backward_pack_is_the_transposed_rotation(d, nh, nkv, kind, T, rope, dtype):
    pos, mask, docs, starts = _layout(kind, T)
    B = pos.shape[0]
    dp = ops.head_dim_padded(d)
    inv = _inv_freq(d, rope)
    g = torch.Generator().manual_seed(d + nh + T)
    dq = torch.randn((B, nh, T, dp), generator=g)
    dk = torch.randn((B, nkv, T, dp), generator=g)
    dv = torch.randn((B, nkv, T, dp), generator=g)
    q_scale = d ** -0.5 * 1.4426950408889634
    NQ = (nh + 2 * nkv) * d
    ld = round_up(NQ, 64) + 64
    out = _sentinel((B * T + 1, ld), dtype)
    cs = torch.empty((T, d), dtype=torch.float32, device=dev())
    dqd, dkd, dvd, invd = dq.to(dev()), dk.to(dev()), dv.to(dev()), inv.to(dev())
    if docs is None:
        call("p2t_rope_backward_pack", ptr(dqd), ptr(dkd), ptr(dvd), ptr(invd), ptr(cs), ptr(out), ld, B, T, nh, nkv, d, dp, q_scale,
             ops.dt_of(dtype), stream())
    else:
        call("p2t_rope_backward_pack_docs", ptr(dqd), ptr(dkd), ptr(dvd), ptr(invd), ptr(cs), ptr(docs), ptr(out), ld, B, T, nh, nkv, d, dp,
             q_scale, ops.dt_of(dtype), stream())
    pt = np.arange(T)[None] - starts
    c, s = _cs(inv, pt)
    c, s = c[:, None], s[:, None]                                      # [B, 1, T, d/2]
    h = d // 2

    def tr(x, sc):                                                     # the transposed rotation: (o1 c + o2 s, o2 c - o1 s)
        o1, o2 = x[..., :h].double().numpy() * sc, x[..., h:d].double().numpy() * sc
        return np.concatenate([o1 * c + o2 * s, o2 * c - o1 * s], -1)

    ref = np.concatenate([tr(dq, q_scale).transpose(0, 2, 1, 3).reshape(B * T, nh * d), tr(dk, 1.0).transpose(0, 2, 1, 3).reshape(B * T, nkv * d),
                          dv[..., :d].double().numpy().transpose(0, 2, 1, 3).reshape(B * T, nkv * d)], 1)
    got = to_np(out)[:B * T]
    _check(got[:, :(nh + nkv) * d], ref[:, :(nh + nkv) * d], dtype, rtol=2e-6, atol=1e-6, what="dq / dk")
    vref = _q(ref[:, (nh + nkv) * d:], dtype)
    assert np.array_equal(got[:, (nh + nkv) * d:NQ], vref), "v columns are copied exactly"
    _assert_sentinel(out, cols=NQ, rows=B * T)


LOG2E = 1.4426950408889634
ADJOINT_CASES = [(64, 4, 2, "arange", 512, 0.37, "llama3"), (64, 4, 2, "packed", 1024, 0.37, "llama3"), (128, 8, 2, "packed", 1024, 0.37, "llama3"),
                 (48, 4, 4, "arange", 256, 0.37, "llama3"), (128, 4, 4, "packed", 4096, 0.37, "llama3"),
                 # the ESM2 encoder step: nh == nkv, theta 10000, the query scale folded with log2 e (head_dim 24 / 32 pad to dp = 32)
                 (24, 20, 20, "arange", 130, LOG2E / 24 ** 0.5, "default"), (32, 20, 20, "arange", 300, LOG2E / 32 ** 0.5, "default"),
                 (64, 40, 40, "arange", 512, LOG2E / 64 ** 0.5, "default")]


@pytest.mark.parametrize("d,nh,nkv,kind,T,q_scale,rope", ADJOINT_CASES,
                         ids=["-".join(str(v) for v in c[:5]) + ("" if c[6] == "llama3" else "-esm") for c in ADJOINT_CASES])
def test_rope_backward_is_the_adjoint_of_qkv_post(d, nh, nkv, kind, T, q_scale, rope):
    """<qkv_post(X), Y> = <X, rope_backward(Y)> in fp32: the backward transposes the forward that actually ran (same table, same positions,
    same scale fold, same head / column order)."""
    pos, mask, docs, _ = _layout(kind, T)
    B = pos.shape[0]
    dp = ops.head_dim_padded(d)
    NQ = (nh + 2 * nkv) * d
    g = torch.Generator().manual_seed(11 * d + T)
    X = torch.randn((B * T, round_up(NQ, 64)), generator=g).to(dev())
    inv = _inv_freq(d, rope).to(dev())
    q, k, v = ops.qkv_post(X, inv, B, T, nh, nkv, d, q_scale, docs=docs)
    Y = [torch.randn(t.shape, generator=g).to(dev()) for t in (q, k, v)]
    for y in Y:
        y[..., d:] = 0
    out = torch.zeros((B * T, round_up(NQ, 64)), dtype=torch.float32, device=dev())
    cs = torch.empty((T, d), dtype=torch.float32, device=dev())
    if docs is None:
        call("p2t_rope_backward_pack", ptr(Y[0]), ptr(Y[1]), ptr(Y[2]), ptr(inv), ptr(cs), ptr(out), out.stride(0), B, T, nh, nkv, d, dp, q_scale,
             _lib.F32, stream())
    else:
        call("p2t_rope_backward_pack_docs", ptr(Y[0]), ptr(Y[1]), ptr(Y[2]), ptr(inv), ptr(cs), ptr(docs), ptr(out), out.stride(0), B, T, nh, nkv,
             d, dp, q_scale, _lib.F32, stream())
    lhs = sum(float((a.double() * b.double()).sum()) for a, b in zip((q, k, v), Y))
    rhs = float((X[:, :NQ].double() * out[:, :NQ].double()).sum())
    scale = sum(float(a.double().norm() * b.double().norm()) for a, b in zip((q, k, v), Y))
    assert abs(lhs - rhs) < 1e-6 * scale, (lhs, rhs)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("d,nh,nkv,T", [(64, 4, 2, 1024), (128, 8, 2, 1024), (48, 4, 4, 4096)])
def test_qkv_post_docs_rotates_at_document_positions(d, nh, nkv, T, dtype):
    pos, mask, docs, starts = _layout("packed", T)
    B = pos.shape[0]
    dp = ops.head_dim_padded(d)
    NQ = (nh + 2 * nkv) * d
    g = torch.Generator().manual_seed(d * 3 + T)
    X = torch.randn((B * T, round_up(NQ, 64)), generator=g)
    Xq = X.to(dtype).double().numpy()
    inv = _inv_freq(d, "llama3")
    q_scale = d ** -0.5 * 1.4426950408889634
    qkv = X.to(device=dev(), dtype=dtype)
    q, k, v = ops.qkv_post(qkv, inv.to(dev()), B, T, nh, nkv, d, q_scale, docs=docs)
    c, s = _cs(inv, np.arange(T)[None] - starts)
    h = d // 2

    def rot(cols, heads, sc):
        x = Xq[:, cols].reshape(B, T, heads, d).transpose(0, 2, 1, 3) * sc
        x1, x2 = x[..., :h], x[..., h:]
        return np.concatenate([x1 * c[:, None] - x2 * s[:, None], x2 * c[:, None] + x1 * s[:, None]], -1)

    _check(to_np(q)[..., :d], rot(slice(0, nh * d), nh, q_scale), dtype, rtol=2e-6, atol=1e-6, what="q")
    _check(to_np(k)[..., :d], rot(slice(nh * d, (nh + nkv) * d), nkv, 1.0), dtype, rtol=2e-6, atol=1e-6, what="k")
    assert np.array_equal(to_np(v)[..., :d], Xq[:, (nh + nkv) * d:NQ].reshape(B, T, nkv, d).transpose(0, 2, 1, 3))
    for t in (q, k, v):
        assert np.all(to_np(t)[..., d:] == 0), "columns d .. dp are zero"
    # documents that all start at 0 (docs = 0 everywhere: position = t) give exactly p2t_qkv_post
    zero = torch.zeros((2, B, T), dtype=torch.int32, device=dev())
    a = ops.qkv_post(qkv, inv.to(dev()), B, T, nh, nkv, d, q_scale, docs=zero)
    b = ops.qkv_post(qkv, inv.to(dev()), B, T, nh, nkv, d, q_scale)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------
def _drop(src, dst, M, K, p, seed, acc):
    call("p2t_dropout_rows", ptr(src), ops.dt_of(src), src.stride(0), ptr(dst), ops.dt_of(dst), dst.stride(0), M, K, float(p), int(seed), int(acc),
         stream())


def test_dropout_rows_mask_contract():
    M, K = 300, 1000
    g = torch.Generator().manual_seed(3)
    x = (torch.rand((M, K + 64), generator=g) + 0.5).to(dev())
    # p = 0: an exact converting copy; accumulate adds
    for sd, dd in ((torch.float32, torch.bfloat16), (torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16)):
        src = x.to(sd)
        dst = _sentinel((M + 1, K + 64), dd)
        _drop(src, dst, M, K, 0.0, 5, 0)
        assert torch.equal(dst[:M, :K], src[:, :K].to(dd))
        _assert_sentinel(dst, cols=K, rows=M)
        base = dst[:M, :K].clone()
        _drop(src, dst, M, K, 0.0, 5, 1)
        assert torch.equal(dst[:M, :K], (base.float() + src[:, :K].float()).to(dd))
    # the mask is a function of (seed, m K + c): the same across dtypes and row strides; another seed, another mask
    ones = torch.ones((M, K + 64), device=dev())
    masks = []
    for dd, ld in ((torch.float32, K), (torch.bfloat16, K), (torch.float32, K + 64), (torch.bfloat16, K + 64)):
        src = ones[:, :ld].contiguous() if ld == K else ones
        dst = _sentinel((M + 1, ld), dd)
        _drop(src, dst, M, K, 0.3, 77, 0)
        _assert_sentinel(dst, cols=K, rows=M)
        masks.append(to_np(dst)[:M, :K] != 0)
    for m in masks[1:]:
        assert np.array_equal(m, masks[0])
    other = torch.empty((M, K), device=dev())
    _drop(ones, other, M, K, 0.3, 78, 0)
    assert float(((to_np(other) != 0) != masks[0]).mean()) > 0.3
    # kept values = src / (1 - p) in the destination dtype; the backward (accumulate = 1) applies the same mask
    p = 0.3
    scale = np.float32(1.0) / np.float32(1.0 - np.float32(p))
    for dd in DTS:
        dst = torch.zeros((M, K), dtype=dd, device=dev())
        _drop(x, dst, M, K, p, 77, 0)
        want = np.where(masks[0], x[:, :K].cpu().numpy() * scale, 0).astype(np.float32)
        assert np.array_equal(to_np(dst), to_np(torch.from_numpy(want).to(dd)))
        acc = torch.full((M, K), 2.0, dtype=dd, device=dev())
        _drop(x, acc, M, K, p, 77, 1)
        assert np.array_equal(to_np(acc), to_np(torch.from_numpy((2.0 + want).astype(np.float32)).to(dd)))
    # M = 0 is a no-op
    dst = _sentinel((4, K), torch.float32)
    _drop(x, dst, 0, K, p, 77, 0)
    _assert_sentinel(dst, rows=0)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_rows_keep_rate_and_expectation(p):
    M, K = 4096, 4096                                   # 16.8M draws
    x = torch.rand((M, K), device=dev()) + 0.5
    out = torch.empty_like(x)
    _drop(x, out, M, K, p, 1234, 0)
    n = M * K
    kept = float((out != 0).double().sum()) / n
    assert abs(kept - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n), kept
    mx, md = float(x.double().mean()), float(out.double().mean())
    sigma = float(x.double().pow(2).mean()) ** 0.5 * np.sqrt(p / (1 - p) / n)          # std of the mean of drop(x)
    assert abs(md - mx) < 5 * sigma, (md, mx)


# ---------------------------------------------------------------------------------------------
def _packed_weights(T):
    """loss_weights of a real pack_instruct_batch(..., loss_weighting="sample") batch: rows [2, T]."""
    from p2t_hip.data import pack_instruct_batch
    rs = np.random.RandomState(0)
    lens = [T - 10, 60, 40, T - 110, 7]
    Tb = max(lens) + 4
    B = len(lens)
    ids = np.zeros((B, Tb), dtype=np.int64)
    mask = np.zeros((B, Tb), dtype=np.int64)
    labels = np.full((B, Tb), -100, dtype=np.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = rs.randint(3, 500, size=n)
        mask[i, :n] = 1
        labels[i, 3:n] = ids[i, 3:n]
    batch = {k: torch.from_numpy(v) for k, v in dict(input_ids=ids, attention_mask=mask, labels=labels, protein_input_ids=np.ones((B, 2), np.int64),
                                                     protein_attention_mask=np.ones((B, 2), np.int64)).items()}
    pk = pack_instruct_batch(batch, T, loss_weighting="sample")
    w = pk["loss_weights"].float()
    assert tuple(w.shape)[1] <= T
    out = torch.zeros((w.shape[0], T), dtype=torch.float32)
    out[:, :w.shape[1]] = w
    pos = torch.zeros((w.shape[0], T), dtype=torch.int64)
    pos[:, :w.shape[1]] = pk["position_ids"]
    return out, pos


@pytest.mark.parametrize("dtype", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [128256, 151936])
def test_cross_entropy_shifted_at_real_vocabularies(V, dtype):
    B, T = 2, 128
    M = B * T
    ld = round_up(V, 64) + 64
    g = torch.Generator().manual_seed(V)
    logits = torch.randn((M, V), generator=g) * 3
    labels = torch.randint(0, V, (B, T), generator=g)
    wp, pos = _packed_weights(T)
    assert wp.shape[0] == B
    labels[pos == 0] = -100                              # document starts (and padding) are never targets
    labels[0, 5], labels[1, 9] = V, -5                  # out of range: ignored by the kernels' contract
    for r in (3, 40, 130, 200):
        logits[r, (r * 977) % V] = 40.0                  # one dominant logit
    for r in (10, 77, 150):
        t = (r % T) + 1
        if t < T and 0 <= labels[r // T, t] < V:
            logits[r, labels[r // T, t]] = float(logits[r].min()) - 1.0      # the label's logit is the smallest
    lg = _sentinel((M, ld), dtype)
    lg[:, :V] = logits.to(device=dev(), dtype=dtype)
    x = logits.to(dtype).double().numpy()
    lab_d = labels.to(dev()).contiguous()
    tgt = np.full((B, T), -100, dtype=np.int64)
    tgt[:, :-1] = labels.numpy()[:, 1:]
    tgt = tgt.reshape(M)
    valid = (tgt >= 0) & (tgt < V)
    mx = x.max(1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(1)) + mx[:, 0]
    row_loss = np.where(valid, lse - x[np.arange(M), np.clip(tgt, 0, V - 1)], 0.0)
    sm = np.exp(x - lse[:, None])
    onehot = np.zeros_like(sm)
    onehot[np.arange(M)[valid], tgt[valid]] = 1
    n = int(valid.sum())
    rnd_w = torch.rand((B, T), generator=g)
    for weights in (None, wp, rnd_w):
        if weights is None:
            loss, count = ops.cross_entropy_shifted(lg.view(B, T, ld), lab_d, V)
            ref_loss = row_loss.sum() / n
            wr = np.full(M, 1.0 / n)
        else:
            wd = weights.to(dev()).contiguous()
            loss, count = ops.cross_entropy_shifted(lg.view(B, T, ld), lab_d, V, weights=wd)
            wr = np.zeros(M)
            wr[:-1] = weights.double().numpy().reshape(M)[1:]
            ref_loss = (wr * row_loss).sum()
        assert int(count.item()) == n
        assert abs(float(loss.item()) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss.item()), ref_loss)
        d = _sentinel((M, ld), dtype)
        if weights is None:
            call("p2t_cross_entropy_shifted_backward", ptr(lg), ld, ops.dt_of(dtype), ptr(lab_d), B, T, V, -100, ptr(count), ptr(d), ld, stream())
        else:
            call("p2t_cross_entropy_shifted_weighted_backward", ptr(lg), ld, ops.dt_of(dtype), ptr(lab_d), ptr(wd), B, T, V, -100, ptr(d), ld,
                 stream())
        ref = np.where(valid[:, None], wr[:, None] * (sm - onehot), 0.0)
        got = to_np(d)
        for r0 in range(0, M, 64):                       # (in slices: the fp64 gradient of a full batch is 300 MB)
            sl = slice(r0, r0 + 64)
            _check(got[sl, :V], ref[sl], dtype, rtol=2e-5, atol=1e-12 * wr.max(), what=f"d_logits rows {r0}..")
        assert np.all(got[~valid, :V] == 0), "rows without a counted target get a zero gradient"
        assert np.all(got[:, V:round_up(V, 64)] == 0), "the K padding of the LM-head dX GEMM is zeroed"
        _assert_sentinel(d, cols=round_up(V, 64))
    # every target ignored: the token mean over nothing is NaN, the weighted sum over nothing is 0
    none = torch.full((B, T), -100, dtype=torch.int64, device=dev())
    loss, count = ops.cross_entropy_shifted(lg.view(B, T, ld), none, V)
    assert int(count.item()) == 0 and np.isnan(float(loss.item()))
    loss, count = ops.cross_entropy_shifted(lg.view(B, T, ld), none, V, weights=wp.to(dev()).contiguous())
    assert int(count.item()) == 0 and float(loss.item()) == 0.0


# ---------------------------------------------------------------------------------------------
def _rms_bwd_ref(x, w, dy, eps):
    r = 1.0 / np.sqrt((x * x).mean(1, keepdims=True) + eps)
    wdy = w[None] * dy
    return r * wdy - x * r ** 3 * (wdy * x).mean(1, keepdims=True)


@pytest.mark.parametrize("form", ["resid", "head_norm"])
@pytest.mark.parametrize("acc", [0, 1])
def test_rmsnorm_backward_at_stage2_shapes(form, acc):
    if form == "resid":
        rows, cols, ld = 1216, 4096, 4096 + 64
    else:
        rows, cols, ld = 1216 * 8, 128, 128                 # Qwen3 q / k norm: one row per (token, head)
    eps = 1e-6
    g = torch.Generator().manual_seed(rows + acc)
    x = torch.randn((rows, ld), generator=g) * 2
    w = 1 + 0.2 * torch.randn((cols,), generator=g)
    dy = (torch.randn((rows, ld), generator=g)).to(torch.bfloat16)
    base = torch.randn((rows, ld), generator=g)
    xd, wd, dyd = x.to(dev()), w.to(dev()), dy.to(dev())
    out = _sentinel((rows + 1, ld + 32), torch.float32)
    if acc:
        out[:rows, :cols] = base[:, :cols].to(dev())
    call("p2t_rmsnorm_backward", ptr(xd), ld, ptr(wd), eps, ptr(dyd), ld, 1, ptr(out), out.stride(0), rows, cols, acc, stream())
    ref = _rms_bwd_ref(x[:, :cols].double().numpy(), w.double().numpy(), dy[:, :cols].double().numpy(), eps)
    if acc:
        ref = ref + base[:, :cols].double().numpy()
    got = to_np(out)[:rows, :cols]
    err = np.abs(got - ref).max(1) / np.abs(ref).max(1)
    assert float(err.max()) < 2e-6, float(err.max())
    _assert_sentinel(out, cols=cols, rows=rows)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 1023, 4097])
def test_scale_by_device_scalar(n):
    x = torch.randn((n + 8,), generator=torch.Generator().manual_seed(n)).to(dev())
    keep = x[n:].clone()
    want = (x[:n].cpu().numpy() * np.float32(-0.731)).astype(np.float32)
    s = torch.tensor([-0.731], dtype=torch.float32, device=dev())
    call("p2t_scale_by_device_scalar", ptr(x), n, ptr(s), stream())
    assert np.array_equal(x[:n].cpu().numpy(), want)
    assert torch.equal(x[n:], keep), "nothing beyond n is written"
