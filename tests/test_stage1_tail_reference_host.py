"""tests/stage1_tail_reference.py on its own, on the CPU: every reference against an independent statement of the same operation
(closed-form gradients against its autograd, torch.nn.functional composed directly, the fp32 numpy oracle at the toy shapes of the
older tests), its bf16-rounded adapter variant against its unrounded one, and finiteness on the kinds of inputs
tests/test_gpu_stage1_tail.py feeds it (a zero row, rows of norm 1e-20 and 1e3, logits of exactly +-1 / tau, an all-zero gradient)."""
import math

import numpy as np
import pytest
import torch

import stage1_tail_reference as R
from oracle import p2t_oracle as O

F64 = torch.float64


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _masks(B, T, lens, holes):
    mask = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    if holes:
        mask[0, 3:6] = 0
        mask[1, 1::3] = 0
    return mask


# ---- readout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("holes", [False, True])
def test_readout_closed_form_gradients_against_autograd(holes):
    B, T, D = 4, 19, 12
    emb = torch.randn((B, T, D), generator=_gen(1), dtype=F64) * 2 + 0.3
    mask = _masks(B, T, [19, 11, 2, 1], holes)
    m = torch.from_numpy(mask).to(F64)
    cnt = m.sum(1)[:, None, None]
    mean = (emb * m[..., None]).sum(1, keepdim=True) / cnt
    std = (((emb - mean) ** 2 * m[..., None]).sum(1, keepdim=True) / cnt).sqrt()
    np.testing.assert_allclose(R.readout(emb, mask, "mean"), mean[:, 0], rtol=1e-14)
    np.testing.assert_allclose(R.readout(emb, mask, "std"), std[:, 0], rtol=1e-14, atol=1e-300)
    np.testing.assert_allclose(R.readout(emb, mask, "mix"), torch.cat([mean[:, 0], std[:, 0]], 1), rtol=1e-14)
    np.testing.assert_allclose(R.readout(emb, None, "mean"), emb.mean(1), rtol=1e-13)
    np.testing.assert_allclose(R.readout(emb, None, "std"), emb.std(1, unbiased=False), rtol=1e-12)
    g = torch.randn((B, 2 * D), generator=_gen(2), dtype=F64)
    rows = [0, 1, 2]                                          # row 3 is one token: std = 0, its gradient 0 / 0
    d_mean = m[..., None] * g[:, None, :D] / cnt
    d_std = m[..., None] * g[:, None, D:] * (emb - mean) / (cnt * std)
    assert rel(R.readout_backward(emb, mask, "mean", g[:, :D]), d_mean) < 1e-14
    assert rel(R.readout_backward(emb, mask, "std", g[:, D:])[rows], d_std[rows]) < 1e-12
    assert rel(R.readout_backward(emb, mask, "mix", g)[rows], (d_mean + d_std)[rows]) < 1e-12
    assert not bool(torch.isfinite(R.readout_backward(emb, mask, "std", g[:, D:])[3]).all())           # documented: 0 / 0
    assert bool(torch.isfinite(R.readout_backward(emb, mask, "mix", g)[rows]).all())
    if not holes:
        last = R.readout(emb, mask, "last")
        idx = mask.sum(1) - 1
        assert torch.equal(last, emb[torch.arange(B), torch.from_numpy(idx)])
        d_last = R.readout_backward(emb, mask, "last", g[:, :D])
        want = torch.zeros_like(emb)
        want[torch.arange(B), torch.from_numpy(idx)] = g[:, :D]
        assert torch.equal(d_last, want)
    # the fp32 numpy oracle (hand-written backward) says the same to fp32 accuracy
    e32 = emb.float().numpy()
    for mode in ("mean", "std", "mix"):
        assert rel(O.readout_embeddings(e32, mask, mode), R.readout(e32, mask, mode)) < 1e-6


# ---- L2-normalise -----------------------------------------------------------------------------------------------------------
def test_l2norm_closed_form_and_edge_rows():
    rows, cols, eps = 6, 64, 1e-12
    x = torch.randn((rows, cols), generator=_gen(3), dtype=F64)
    x[1] = 0.0
    x[2] *= 1e-20 / float(x[2].norm())
    x[3] *= 1e3 / float(x[3].norm())
    dy = torch.randn((rows, cols), generator=_gen(4), dtype=F64)
    y, inv, dx = R.l2norm(x, eps, dy)
    assert all(bool(torch.isfinite(t).all()) for t in (y, inv, dx))
    n = x.norm(dim=-1, keepdim=True)
    big = (n > eps)[:, 0]
    yy = x / n.clamp_min(eps)
    np.testing.assert_allclose(y, yy, rtol=1e-14, atol=0)
    np.testing.assert_allclose(inv, 1.0 / n.clamp_min(eps)[:, 0], rtol=1e-14)
    closed = (dy - yy * (dy * yy).sum(-1, keepdim=True)) / n.clamp_min(eps)
    assert rel(dx[big], closed[big]) < 1e-13
    assert torch.equal(y[1], torch.zeros(cols, dtype=F64)) and rel(dx[1], dy[1] / eps) < 1e-15
    # under eps the divisor is the constant eps: dx = dy / eps; the projection term of the closed form is 1e-16 of it
    assert rel(dx[2], dy[2] / eps) < 1e-15 and rel(closed[2], dy[2] / eps) < 1e-12
    assert abs(float(y[3].norm()) - 1.0) < 1e-14 and abs(float(inv[3]) - 1e-3) < 1e-17


# ---- InfoNCE ----------------------------------------------------------------------------------------------------------------
def _unit(seed, n, d):
    return torch.nn.functional.normalize(torch.randn((n, d), generator=_gen(seed), dtype=F64), dim=-1)


def test_infonce_rows_closed_form_and_extreme_logits():
    S, N, D, tau, w = 5, 9, 16, 0.05, 0.7
    seg, batch = _unit(5, S, D), _unit(6, N, D)
    labels = np.arange(N - S, N)
    seg[1] = batch[labels[1]]                                 # the positive logit is exactly 1 / tau
    seg[2] = -batch[0]                                        # a logit of exactly -1 / tau
    loss, logits, d_seg = R.infonce_rows(seg, batch, labels, tau, w)
    assert abs(float(logits[1, labels[1]]) - 20.0) < 1e-12 and abs(float(logits[2, 0]) + 20.0) < 1e-12
    assert all(bool(torch.isfinite(t).all()) for t in (loss, logits, d_seg))
    sm = torch.softmax(seg @ batch.T / tau, 1)
    sm[torch.arange(S), torch.from_numpy(labels)] -= 1.0
    assert rel(d_seg, w * (sm @ batch) / (S * tau)) < 1e-12
    lse = torch.logsumexp(logits, 1)
    assert abs(float(loss) - w * float((lse - logits[torch.arange(S), torch.from_numpy(labels)]).mean())) < 1e-13
    l32, g32, lg32 = O.infonce_segmented(seg.float().numpy(), batch.float().numpy(), labels, tau, return_grad=True)
    s32, b32 = seg.float().numpy(), batch.float().numpy()
    loss1, logits1, d1 = R.infonce_rows(s32, b32, labels, tau, 1.0)
    assert abs(float(l32) - float(loss1)) < 2e-6 * max(1.0, float(loss1)) and rel(lg32, logits1) < 1e-6 and rel(g32, d1) < 2e-6


def test_infonce_cols_closed_form_and_row_block():
    N, D, tau = 8, 16, 0.05
    p, t = _unit(7, N, D), _unit(8, N, D)
    loss, col_lse, g = R.infonce_cols(p, t, tau)
    logits = p @ t.T / tau
    np.testing.assert_allclose(col_lse, torch.log(torch.exp(logits).sum(0)), rtol=1e-13)
    assert abs(float(loss) - float(torch.nn.functional.cross_entropy(logits.T, torch.arange(N)))) < 1e-13
    coef = torch.exp(logits - col_lse[None, :]) - torch.eye(N, dtype=F64)
    assert rel(g, coef @ t / tau) < 1e-12                     # the formula include/p2t_hip.h gives p2t_infonce_col_backward, scale 1
    cols = np.array([6, 1, 4])
    loss_c, _, g_blk = R.infonce_cols(p, t, tau, cols=cols, rows=np.arange(2, 5), scale=0.25, d_seg=np.ones((3, D)))
    assert abs(float(loss_c) - float((col_lse - torch.diagonal(logits))[torch.from_numpy(cols)].mean())) < 1e-13
    assert rel(g_blk, 0.25 * (coef @ t / tau)[2:5] + 1.0) < 1e-12
    assert bool(torch.isfinite(g).all())
    l32, g32 = O.infonce_columns(p.float().numpy(), t.float().numpy(), cols, tau, return_grad=True)
    loss1, _, g1 = R.infonce_cols(p.float().numpy(), t.float().numpy(), tau, cols=cols)
    assert abs(float(l32) - float(loss1)) < 2e-6 * max(1.0, float(loss1)) and rel(g32, g1) < 3e-6


# ---- adapter ----------------------------------------------------------------------------------------------------------------
def _adapter_inputs(M=23, X=32, I=48, O_=16, seed=9):
    g = _gen(seed)
    w1, b1 = torch.randn((I, X), generator=g) * X ** -0.5, torch.randn(I, generator=g) * 0.1
    w2, b2 = torch.randn((O_, I), generator=g) * I ** -0.5, torch.randn(O_, generator=g) * 0.1
    x, dy = torch.randn((M, X), generator=g), torch.randn((M, O_), generator=g)
    m1, m2 = torch.rand((M, I), generator=g) > 0.3, torch.rand((M, O_), generator=g) > 0.3
    return x, w1, b1, w2, b2, m1, m2, dy


def test_adapter_step_against_functional_composed_directly():
    x, w1, b1, w2, b2, m1, m2, dy = _adapter_inputs()
    p = 0.3
    y, dW1, db1, dW2, db2 = R.adapter_step(x, w1, b1, w2, b2, m1, m2, p, dy)
    F = torch.nn.functional
    sc = R.drop_scale(p)
    assert abs(sc - 1.0 / 0.7) < 1e-7 and R.drop_scale(0.0) == 1.0
    lin1, lin2 = torch.nn.Linear(32, 48).double(), torch.nn.Linear(48, 16).double()
    with torch.no_grad():
        lin1.weight.copy_(w1), lin1.bias.copy_(b1), lin2.weight.copy_(w2), lin2.bias.copy_(b2)
    yy = F.normalize(F.gelu(lin2(F.gelu(lin1(x.double())) * m1 * sc)) * m2 * sc, p=2, dim=-1)
    (yy * dy.double()).sum().backward()
    assert rel(y, yy.detach()) < 1e-14
    for got, want in ((dW1, lin1.weight.grad), (db1, lin1.bias.grad), (dW2, lin2.weight.grad), (db2, lin2.bias.grad)):
        assert rel(got, want) < 1e-13 and bool(torch.isfinite(got).all())
    # the hand-written chain of csrc/adapter.hip's header comment
    xd, W1, W2 = x.double(), w1.double(), w2.double()
    z1 = xd @ W1.T + b1.double()
    h1 = F.gelu(z1) * m1 * sc
    z2 = h1 @ W2.T + b2.double()
    g2 = F.gelu(z2) * m2 * sc
    n = g2.norm(dim=-1, keepdim=True)
    dg2 = (dy.double() - yy.detach() * (dy.double() * yy.detach()).sum(-1, keepdim=True)) / n
    gp = lambda z: 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    dz2 = dg2 * m2 * sc * gp(z2)
    dz1 = (dz2 @ W2) * m1 * sc * gp(z1)
    assert rel(dW2, dz2.T @ h1) < 1e-13 and rel(db2, dz2.sum(0)) < 1e-13
    assert rel(dW1, dz1.T @ xd) < 1e-13 and rel(db1, dz1.sum(0)) < 1e-13


def test_adapter_step_bf16_rounding_points():
    """round_bf16=True: y is a bf16 value, the result moves by bf16 roundings (1e-3 .. 3e-2) and not more, and on operands for which
    every stored tensor is already exact in bf16 nothing moves at all."""
    x, w1, b1, w2, b2, m1, m2, dy = _adapter_inputs()
    q = lambda t: t.bfloat16().float()
    args = (q(x), q(w1), b1, q(w2), b2, m1, m2, 0.3, dy)
    plain, rounded = R.adapter_step(*args), R.adapter_step(*args, round_bf16=True)
    assert torch.equal(rounded[0], R.bf16(rounded[0])) and not torch.equal(plain[0], R.bf16(plain[0]))
    for a, b in zip(rounded, plain):
        assert bool(torch.isfinite(a).all()) and 1e-4 < rel(a, b) < 3e-2
    # _RoundValue / _RoundGrad / _GeluAtStoredZ are the identity on bf16-exact values
    z = q(torch.randn((5, 7), generator=_gen(10))).double().requires_grad_(True)
    w = torch.tensor([0.5, 2.0, -1.0, 4.0, 0.25, 1.0, -8.0], dtype=F64)
    out = R._RoundGrad.apply(R._RoundValue.apply(R._GeluAtStoredZ.apply(z)))
    g_r = torch.autograd.grad(out, z, w.expand(5, 7))[0]
    z2 = z.detach().clone().requires_grad_(True)
    g_p = torch.autograd.grad(torch.nn.functional.gelu(z2), z2, w.expand(5, 7))[0]
    assert rel(g_r, g_p) < 1e-15 and rel(out.detach(), torch.nn.functional.gelu(z2).detach()) < 4e-3


# ---- clip + AdamW -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [math.inf, 0.05])
def test_clip_adamw_against_the_fp32_oracle_at_the_toy_shapes(max_norm):
    names, shapes = ["w1", "b1", "w2", "b2"], [(48, 32), (48,), (64, 48), (64,)]
    rng = np.random.default_rng(11)
    P = {n: (rng.standard_normal(s) * 0.5).astype(np.float32) for n, s in zip(names, shapes)}
    G = {n: (rng.standard_normal(s) * 0.02).astype(np.float32) for n, s in zip(names, shapes)}
    m = {n: np.zeros(s, np.float32) for n, s in zip(names, shapes)}
    v = {n: np.zeros(s, np.float32) for n, s in zip(names, shapes)}
    p64, m64, v64 = ([R.t64(d[n]) for n in names] for d in (P, m, v))
    for step in (1, 2, 3, 10000):
        gs = {n: G[n] * np.float32(min(step, 4)) for n in names}
        if step == 10000 and max_norm == 0.05:
            gs = {n: np.zeros_like(G[n]) for n in names}                             # an all-zero gradient: norm 0, coef clamped to 1
        gn32 = O.clip_and_adamw(P, gs, m, v, step, max_norm=max_norm)
        gn64 = R.clip_adamw(p64, [gs[n] for n in names], m64, v64, step, max_norm=max_norm)
        assert abs(float(gn32) - gn64) <= 1e-6 * max(gn64, 1e-30)
        for i, n in enumerate(names):
            np.testing.assert_allclose(P[n], p64[i].numpy(), rtol=2e-6, atol=1e-7)
            np.testing.assert_allclose(m[n], m64[i].numpy(), rtol=2e-6, atol=1e-9)
            np.testing.assert_allclose(v[n], v64[i].numpy(), rtol=2e-6, atol=1e-12)
            assert all(bool(torch.isfinite(t[i]).all()) for t in (p64, m64, v64))


def test_clip_adamw_is_clip_grad_norm_then_one_adamw_step_by_hand():
    p0 = torch.randn((7, 5), generator=_gen(12), dtype=F64)
    g = torch.randn((7, 5), generator=_gen(13), dtype=F64) * 0.1
    m0, v0 = torch.rand((7, 5), generator=_gen(14), dtype=F64) * 0.01, torch.rand((7, 5), generator=_gen(15), dtype=F64) * 1e-4
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    total = R.clip_adamw([p], [g], [m], [v], 4, max_norm=0.05)
    assert abs(total - float(g.norm())) < 1e-15
    gc = g * min(1.0, 0.05 / (total + 1e-6))
    mm, vv = 0.9 * m0 + 0.1 * gc, 0.999 * v0 + 0.001 * gc * gc
    want = p0 * (1 - 2e-4 * 0.01) - 2e-4 / (1 - 0.9 ** 4) * mm / (vv.sqrt() / math.sqrt(1 - 0.999 ** 4) + 1e-6)
    assert rel(p, want) < 1e-14 and rel(m, mm) < 1e-14 and rel(v, vv) < 1e-14
    p2 = p0.clone()
    assert R.clip_adamw([p2], [g], [m0.clone()], [v0.clone()], 4, max_norm=1.01 * total) == total        # inactive by a hair
    p3 = p0.clone()
    R.clip_adamw([p3], [g], [m0.clone()], [v0.clone()], 4)
    assert torch.equal(p2, p3)
