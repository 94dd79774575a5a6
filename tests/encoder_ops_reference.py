"""fp64 (and, for the embeddings, torch fp32) references of the entry points the encoder LoRA step runs (p2t_hip/encoder_train.py), plain
numpy / torch on the CPU: used by tests/test_gpu_encoder_ops.py and tests/test_gpu_sft_backward.py, and checked on their own against
torch autograd in tests/test_encoder_ops_reference_host.py."""
from __future__ import annotations

import math

import numpy as np
import torch

SQRT1_2 = 0.70710678118654752440


# ---- erf GELU ---------------------------------------------------------------------------------------------------------------
def erf64(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def gelu64(z):
    """z / 2 (1 + erf(z / sqrt 2)) in fp64."""
    z = np.asarray(z, dtype=np.float64)
    return 0.5 * z * (1.0 + erf64(z * SQRT1_2))


def gelu_grad64(z):
    """d gelu / dz = Phi(z) + z phi(z) in fp64."""
    z = np.asarray(z, dtype=np.float64)
    return 0.5 * (1.0 + erf64(z * SQRT1_2)) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 numbers is exact in fp64, so one fp64 add and one rounding to fp32 remain."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def erf_as_f32(a):
    """csrc/common.h erf_as (Abramowitz-Stegun 7.1.26) restated in fp32 with IEEE division and exp in place of the hardware rcp / exp."""
    f = np.float32
    a = np.asarray(a, dtype=np.float32)
    ax = np.abs(a)
    t = (f(1.0) / _fma32(np.full_like(ax, f(0.3275911)), ax, np.full_like(ax, f(1.0)))).astype(np.float32)
    c = lambda v: np.full_like(ax, f(v))
    p = _fma32(c(1.061405429), t, c(-1.453152027))
    p = _fma32(p, t, c(1.421413741))
    p = _fma32(p, t, c(-0.284496736))
    p = _fma32(p, t, c(0.254829592))
    e = np.exp((-ax * ax).astype(np.float64)).astype(np.float32)          # expf, correctly rounded
    r = (f(1.0) - ((p * t).astype(np.float32) * e).astype(np.float32)).astype(np.float32)
    return np.copysign(r, a)


def erf_as_error(z):
    """E of the bf16-output GELU bound: max |erf_as_f32(fp32(z * fp32(1 / sqrt 2))) - erf(z / sqrt 2)| over the fp32 inputs z (the argument's
    rounding included), from the restatement and fp64 alone."""
    z = np.asarray(z, dtype=np.float32)
    a = (z * np.float32(SQRT1_2)).astype(np.float32)
    return float(np.max(np.abs(erf_as_f32(a).astype(np.float64) - erf64(z.astype(np.float64) * SQRT1_2))))


def gelu_grid(n: int, seed: int) -> np.ndarray:
    """n pre-activations: linspace(-40, 40) (the erf tails on both sides, where 1 + erf cancels), +-0, and randn * 3."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal(n) * 3).astype(np.float32)
    k = min(801, max(n - 2, 0))
    z[:k] = np.linspace(-40, 40, k, dtype=np.float32)
    if n >= 2:
        z[k], z[k + 1] = 0.0, -0.0
    return z


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------------
def layernorm_bwd64(x, w, dy, eps):
    """dX of torch.nn.functional.layer_norm (frozen weight / bias) by fp64 autograd; x, dy [rows, cols], w [cols] as numpy."""
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).requires_grad_(True)
    y = torch.nn.functional.layer_norm(xd, (xd.shape[-1],), torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)), None, eps)
    return torch.autograd.grad(y, xd, torch.from_numpy(np.ascontiguousarray(dy, dtype=np.float64)))[0].numpy()


def layernorm_bwd_terms(x, w, dy, eps):
    """The quantities the error bound of an fp32 evaluation of r (w dy - mean(w dy) - xhat mean(w dy xhat)) is built from, per row:
    dict(r, xhat, gw, m1, c2, a1, a2, ax) with gw = w dy, m1 = mean gw, c2 = mean gw xhat, a1 = mean |gw|, a2 = mean |gw xhat|, ax = mean |x|."""
    x, w, dy = (np.asarray(t, dtype=np.float64) for t in (x, w, dy))
    mu = x.mean(1, keepdims=True)
    r = 1.0 / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + eps)
    xhat = (x - mu) * r
    gw = w[None] * dy
    return dict(r=r, xhat=xhat, gw=gw, m1=gw.mean(1, keepdims=True), c2=(gw * xhat).mean(1, keepdims=True), a1=np.abs(gw).mean(1, keepdims=True),
                a2=np.abs(gw * xhat).mean(1, keepdims=True), ax=np.abs(x).mean(1, keepdims=True))


# ---- ESM2 embeddings --------------------------------------------------------------------------------------------------------
def esm_embed_f32(ids, mask, table, mask_id: int, token_dropout: bool):
    """HF EsmEmbeddings.forward (rotary checkpoints: no position embeddings, no emb_layer_norm_before) in torch fp32 on the CPU, in
    HF's order of operations: gather, masked_fill(<mask>, 0), * (1 - 0.15 * 0.8) / (1 - observed ratio), * attention_mask.
    ids, mask int64 [B, T]; table fp32 [vocab, H] (a bf16 table: its values, widened).  -> fp32 [B, T, H]."""
    e = table.float()[ids]
    if token_dropout:
        e = e.masked_fill((ids == mask_id).unsqueeze(-1), 0.0)
        mask_ratio_train = 0.15 * 0.8
        src_lengths = mask.sum(-1)
        mask_ratio_observed = (ids == mask_id).sum(-1).float() / src_lengths
        e = (e * (1 - mask_ratio_train) / (1 - mask_ratio_observed)[:, None, None]).to(e.dtype)
    return (e * mask.unsqueeze(-1)).to(e.dtype)


# ---- attention --------------------------------------------------------------------------------------------------------------
def attention_fwd_bwd64(q, k, v, d_o, mask, causal: bool, c_s: float, o_stored=None, docs=None, bounds: bool = False):
    """Textbook attention in fp64 on stored operands, one (batch, head) at a time (B * heads * T^2 doubles never exist at once).
    q [B, nh, T, d], k / v [B, nkv, T, d], d_o [B, nh, T, d] (or None: forward only), mask [B, T] (1 = valid key), logits = c_s q k^T.
    o_stored [B, nh, T, d]: the output D = rowsum(dO o O) is taken from (the kernel's stored one, as torch does); None: the fp64 one;
    a callable: applied to the fp64 output of each (batch, head), e.g. its rounding to the stored dtype.
    docs int [B, T] (or None): the start of each token's document; key j is visible to query i iff docs[b, i] <= j <= i and the mask allows it.
    -> dict(lse [B, nh, T] (+inf where a row sees no key), o, rows (bool [B, nh, T]: the row sees a key), dq, dk, dv).
    bounds: also n_visible [B, nh, T], p_diag [B, nh, T] (P[i, i]) and the per-element terms a rounding bound is built from:
    A = P |v| (o); dq_abs = c_s |dS| |k|, dk_abs = c_s |dS|^T |q|, dv_abs = P^T |dO|; and with F = P o (|dO| |v|^T + rowsum(|dO| o |O|)) (what an
    fp32 evaluation of dO v^T - D is rounded against) dq_F = c_s F |k|, dk_F = c_s F^T |q| (dv does not pass through dS: no F term)."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    B, nh, T, d = q.shape
    nkv = k.shape[1]
    rep = nh // nkv
    out = dict(lse=np.full((B, nh, T), np.inf), o=np.zeros((B, nh, T, d)), rows=np.zeros((B, nh, T), bool))
    if bounds:
        out.update(A=np.zeros((B, nh, T, d)), n_visible=np.zeros((B, nh, T), np.int64), p_diag=np.zeros((B, nh, T)))
    if d_o is not None:
        d_o = np.asarray(d_o, dtype=np.float64)
        out.update(dq=np.zeros((B, nh, T, d)), dk=np.zeros((B, nkv, T, d)), dv=np.zeros((B, nkv, T, d)))
        if bounds:
            out.update(dq_abs=np.zeros((B, nh, T, d)), dk_abs=np.zeros((B, nkv, T, d)), dv_abs=np.zeros((B, nkv, T, d)),
                       dq_F=np.zeros((B, nh, T, d)), dk_F=np.zeros((B, nkv, T, d)))
    tri = np.tril(np.ones((T, T), bool)) if causal or docs is not None else None
    for b in range(B):
        allowed = np.broadcast_to(np.asarray(mask[b] != 0)[None, :], (T, T))
        if causal or docs is not None:
            allowed = allowed & tri
        if docs is not None:
            allowed = allowed & (np.arange(T)[None, :] >= np.asarray(docs[b])[:, None])
        for h in range(nh):
            kk, vv = k[b, h // rep], v[b, h // rep]
            S = np.where(allowed, (q[b, h] @ kk.T) * c_s, -np.inf)
            m = S.max(-1, keepdims=True)
            m = np.where(np.isfinite(m), m, 0.0)
            E = np.exp(S - m)
            l = E.sum(-1, keepdims=True)
            P = np.divide(E, l, out=np.zeros_like(E), where=l > 0)
            seen = l[:, 0] > 0
            out["rows"][b, h] = seen
            out["lse"][b, h] = np.where(seen, m[:, 0] + np.log(np.where(l > 0, l, 1.0))[:, 0], np.inf)
            O = P @ vv
            out["o"][b, h] = O
            if bounds:
                out["A"][b, h] = P @ np.abs(vv)
                out["n_visible"][b, h] = allowed.sum(-1)
                out["p_diag"][b, h] = np.diagonal(P)
            if d_o is None:
                continue
            dO = d_o[b, h]
            Ost = O if o_stored is None else np.asarray(o_stored(O) if callable(o_stored) else o_stored[b, h], dtype=np.float64)
            D = (dO * Ost).sum(-1, keepdims=True)
            dS = P * (dO @ vv.T - D)
            out["dq"][b, h] = (dS @ kk) * c_s
            out["dk"][b, h // rep] += (dS.T @ q[b, h]) * c_s
            out["dv"][b, h // rep] += P.T @ dO
            if bounds:
                aS, aq, ak, adO = np.abs(dS), np.abs(q[b, h]), np.abs(kk), np.abs(dO)
                F = P * (adO @ np.abs(vv).T + (adO * np.abs(Ost)).sum(-1, keepdims=True))
                out["dq_abs"][b, h] = (aS @ ak) * c_s
                out["dk_abs"][b, h // rep] += (aS.T @ aq) * c_s
                out["dv_abs"][b, h // rep] += P.T @ adO
                out["dq_F"][b, h] = (F @ ak) * c_s
                out["dk_F"][b, h // rep] += (F.T @ aq) * c_s
    return out
