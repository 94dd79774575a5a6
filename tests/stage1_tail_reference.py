"""fp64 references of the stage-1 (contrastive) tail behind the frozen towers -- adapter forward / backward, readout, L2-normalise, the
InfoNCE row and column terms, clip + AdamW -- plain torch on the CPU, gradients by torch.autograd: the other side of
tests/test_gpu_stage1_tail.py, checked on their own in tests/test_stage1_tail_reference_host.py.  Independent of oracle/p2t_oracle.py
(fp32 numpy with hand-written backwards), which the older small-shape tests compare against.

Every function takes numpy arrays or torch tensors and computes on float64 copies; what it returns is float64 torch."""
from __future__ import annotations

import math

import numpy as np
import torch

F64 = torch.float64


def t64(a) -> torch.Tensor:
    """A float64 torch copy of a numpy array or a tensor of any float / integer dtype (a bf16 tensor: its stored values, widened)."""
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(F64).clone()
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64).clone()


def bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 through fp32 (what a kernel's fp32 result stored as bf16 is), back in the input dtype."""
    return x.float().bfloat16().to(x.dtype)


# ---- readout ----------------------------------------------------------------------------------------------------------------
def readout(emb, mask, mode: str):
    """readout_embeddings of the reference project's contrastive script: emb [B, T, D], mask [B, T] of 0 / 1 (None: all ones);
    "last" = the token at index sum(mask) - 1, "mean" = sum(emb * mask) / sum(mask), "std" = sqrt(sum((emb - mean)^2 * mask) / sum(mask))
    (population, no eps), "mix" = cat(mean, std).  The argument may carry requires_grad (the backward differentiates through it)."""
    e = emb if isinstance(emb, torch.Tensor) and emb.dtype == F64 else t64(emb)
    B, T, _ = e.shape
    m = torch.ones((B, T), dtype=F64) if mask is None else t64(mask)
    if mode == "last":
        return e[torch.arange(B), m.sum(1).long() - 1, :]
    cnt = m.sum(1, keepdim=True)
    mean = (e * m[..., None]).sum(1) / cnt
    if mode == "mean":
        return mean
    std = (((e - mean[:, None, :]) ** 2 * m[..., None]).sum(1) / cnt).sqrt()
    if mode == "std":
        return std
    if mode == "mix":
        return torch.cat([mean, std], 1)
    raise ValueError(mode)


def readout_backward(emb, mask, mode: str, d_out):
    """d_emb [B, T, D] = (d readout / d emb)^T d_out by autograd (a batch row of one token has std = 0: its std gradient is 0 / 0 = NaN)."""
    e = t64(emb).requires_grad_(True)
    return torch.autograd.grad(readout(e, mask, mode), e, t64(d_out))[0]


# ---- L2-normalise -----------------------------------------------------------------------------------------------------------
def l2norm(x, eps: float = 1e-12, dy=None):
    """torch.nn.functional.normalize(x, p=2, dim=-1, eps) = x / max(||x||, eps).  -> (y, inv_norm = 1 / max(||x||, eps), dx or None);
    dx by autograd: a row whose norm is under eps is divided by the constant eps, so its dx = dy / eps (a zero row included)."""
    xd = t64(x).requires_grad_(dy is not None)
    y = torch.nn.functional.normalize(xd, p=2.0, dim=-1, eps=eps)
    inv = 1.0 / torch.linalg.vector_norm(xd.detach(), dim=-1).clamp_min(eps)
    dx = torch.autograd.grad(y, xd, t64(dy))[0] if dy is not None else None
    return y.detach(), inv, dx


# ---- InfoNCE ----------------------------------------------------------------------------------------------------------------
def infonce_rows(seg, batch, labels, tau: float = 0.05, weight: float = 1.0):
    """weight * F.cross_entropy(seg @ batch.T / tau, labels) (mean over the rows of seg) -> (loss, logits [S, N], d_seg = d loss / d seg)."""
    s = t64(seg).requires_grad_(True)
    logits = s @ t64(batch).T / tau
    loss = weight * torch.nn.functional.cross_entropy(logits, torch.as_tensor(np.asarray(labels)).long())
    return loss.detach(), logits.detach(), torch.autograd.grad(loss, s)[0]


def infonce_cols(p_all, t_all, tau: float = 0.05, cols=None, rows=None, scale: float = 1.0, d_seg=None):
    """The column (text -> protein) term: F.cross_entropy(logits.T, arange) restricted to the columns `cols` (default all), logits =
    p_all @ t_all.T / tau.  -> (loss = mean over cols of (col_lse_j - l_jj), col_lse [N] = logsumexp over the ROWS of every column,
    grad).  grad is what p2t_infonce_col_backward produces for the row block `rows` (indices into p_all, default all):
    scale * d( sum over ALL columns j of (col_lse_j - l_jj) ) / d p_all[rows], added to `d_seg` when that is given (accumulate)."""
    p = t64(p_all).requires_grad_(True)
    logits = p @ t64(t_all).T / tau
    col_lse = torch.logsumexp(logits, 0)
    per_col = col_lse - torch.diagonal(logits)
    N = p.shape[0]
    cols = torch.arange(N) if cols is None else torch.as_tensor(np.asarray(cols)).long()
    chosen = torch.nn.functional.cross_entropy(logits.T[cols], cols)              # the statement itself: the mean over the chosen columns
    assert abs(float(chosen.detach()) - float(per_col.detach()[cols].mean())) <= 1e-12 * max(1.0, abs(float(chosen.detach())))
    g = torch.autograd.grad(per_col.sum(), p)[0] * scale
    rows = torch.arange(N) if rows is None else torch.as_tensor(np.asarray(rows)).long()
    g = g[rows]
    if d_seg is not None:
        g = g + t64(d_seg)
    return chosen.detach(), col_lse.detach(), g


# ---- ModalityAdapter --------------------------------------------------------------------------------------------------------
class _RoundValue(torch.autograd.Function):
    """forward: bf16(x); backward: the gradient as it is (the kernels differentiate at the value they stored)."""

    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """forward: x as it is; backward: bf16(gradient) (a gradient the backward materialises in bf16)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


class _GeluAtStoredZ(torch.autograd.Function):
    """forward: gelu(z) of the GEMM's own (unrounded) accumulator, as the P2T_EPI_GELU epilogue evaluates it; backward: g * gelu'(bf16(z)),
    the derivative at the pre-activation the forward STORED (z1 / z2 are bf16 tensors that only the backward reads)."""

    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(bf16(z))
        return torch.nn.functional.gelu(z)

    @staticmethod
    def backward(ctx, g):
        (zs,) = ctx.saved_tensors
        return g * (0.5 * (1.0 + torch.erf(zs / math.sqrt(2.0))) + zs * torch.exp(-0.5 * zs * zs) / math.sqrt(2.0 * math.pi))


def drop_scale(p: float) -> float:
    """1 / (1 - p) as the kernels hold it: an fp32 division of fp32 operands."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def adapter_step(x, w1, b1, w2, b2, m1, m2, p: float, dy, round_bf16: bool = False):
    """y = normalize(drop(gelu(fc2(drop(gelu(fc1(x))))))) with the keep-masks m1 [M, I], m2 [M, O] given (kept activations are scaled by
    drop_scale(p)), and the gradients of sum(y * dy) by autograd -> (y, dW1, db1, dW2, db2).
    round_bf16: a bf16 rounding exactly where csrc/adapter.hip stores a bf16 tensor -- forward values z1, h1, z2, g2, y; gradients dz2, dz1.
    The GELU is taken of the unrounded pre-activation (the GEMM epilogue's accumulator), its derivative at the stored bf16 one; the
    L2-normalisation is differentiated at the stored g2, and y's own rounding does not enter the backward.  x, w1, w2 are taken as stored."""
    R = _RoundValue.apply if round_bf16 else (lambda t: t)
    G = _RoundGrad.apply if round_bf16 else (lambda t: t)
    gelu = _GeluAtStoredZ.apply if round_bf16 else torch.nn.functional.gelu
    sc = drop_scale(p)
    xd = t64(x)
    W1, B1, W2, B2 = (t64(t).requires_grad_(True) for t in (w1, b1, w2, b2))
    k1 = torch.as_tensor(np.asarray(m1)).to(F64) * sc
    k2 = torch.as_tensor(np.asarray(m2)).to(F64) * sc
    z1 = G(xd @ W1.T + B1)                                     # dz1 is a bf16 tensor
    h1 = R(gelu(z1) * k1)
    z2 = G(h1 @ W2.T + B2)                                     # dz2 is a bf16 tensor
    g2 = R(gelu(z2) * k2)
    y = R(torch.nn.functional.normalize(g2, p=2.0, dim=-1, eps=1e-12))
    grads = torch.autograd.grad(y, [W1, B1, W2, B2], t64(dy))
    return (y.detach(),) + tuple(grads)


# ---- clip_grad_norm_ + AdamW ------------------------------------------------------------------------------------------------
def clip_adamw(params, grads, m, v, step: int, lr=2e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, max_norm=math.inf):
    """torch.nn.utils.clip_grad_norm_(max_norm) followed by torch.optim.AdamW.step() as its `step`-th step, on the float64 tensors
    params / m (exp_avg) / v (exp_avg_sq), which are updated IN PLACE; grads are left as given.  -> the total norm (before clipping)."""
    assert all(t.dtype == F64 for t in list(params) + list(m) + list(v))
    ps = [torch.nn.Parameter(q.clone()) for q in params]
    for q, g in zip(ps, grads):
        q.grad = t64(g)
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    for q, mm, vv in zip(ps, m, v):
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": mm.clone(), "exp_avg_sq": vv.clone()}
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm=max_norm if max_norm is not None else math.inf)
    opt.step()
    for q, pp, mm, vv in zip(ps, params, m, v):
        pp.copy_(q.detach())
        mm.copy_(opt.state[q]["exp_avg"])
        vv.copy_(opt.state[q]["exp_avg_sq"])
    return float(total)
