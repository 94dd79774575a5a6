"""The LM head of the stage-2 steps, written once: final RMSNorm -> LM-head GEMM -> shifted cross-entropy and its backward, for the
frozen-decoder step (p2t_hip/modeling.py `_DecoderLossFn`) and the per-layer LoRA step (p2t_hip/decoder_train.py `DecoderLoraLossFn`).

    reference  scripts/train_instruct.py:192-213, 313-349   the train and eval loops read `model(**batch).loss` only
               transformers loss_utils.ForCausalLMLoss      position (b, t) predicts labels[b, t+1]; -100 is ignored

Two forms of the same head:

`head_loss` / `head_backward` -- the unfused head both steps always had: every one of the M = B T rows goes through the norm, the
GEMM and p2t_cross_entropy_shifted; the forward keeps `logits [M, ld(V)]`, the backward allocates a `d_logits` of the same size.
This is the form that returns `CausalLMOutput.logits`.

`lm_head_loss` / `lm_head_backward` -- the opt-in fused head (`LlamaDecoder.fused_lm_loss()`): p2t_lm_target_rows lists the rows with a
counted target, their fp32 residual rows are gathered into a compact [capacity, H] buffer, and the norm, the GEMM and the loss run on
those rows alone, `chunk_rows` at a time.  p2t_lm_loss_grad_rows turns each chunk of logits into its own gradient in place and the
dX GEMM consumes it at once (Liger-style), so one [chunk, ld(V)] buffer is all the head ever holds; the forward keeps the unscaled
gradient of the compact post-norm rows (f32 [capacity, H]), the row list, the count and the compact inputs, and the backward is a
scale by the upstream gradient, the RMSNorm backward and a scatter into a zeroed [M, H].  Under `torch.no_grad()` the dX GEMM and
everything kept are skipped.  torch allocates and slices; no torch op computes on the path.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from ._lib import call
from .ops import ptr, round_up, stream

ROW_ALIGN = 128                                      # the compact row count is a multiple of this (whole MFMA GEMM row tiles)


def _norm_weight(decoder) -> torch.Tensor:
    return decoder.model.norm.weight.detach().float().contiguous()


def _rms_bwd(decoder, x: torch.Tensor, dy: torch.Tensor, out: torch.Tensor) -> None:
    call("p2t_rmsnorm_backward", ptr(x), x.stride(0), ptr(_norm_weight(decoder)), float(decoder.spec.rms_norm_eps), ptr(dy), dy.stride(0),
         0 if dy.dtype == torch.float32 else 1, ptr(out), out.stride(0), x.shape[0], x.shape[1], 0, stream())


# ---------------------------------------------------------------------------------------------------------------------------
# the unfused head (all M rows; keeps the logits)
# ---------------------------------------------------------------------------------------------------------------------------
def head_loss(decoder, x: torch.Tensor, labels: torch.Tensor, *, weights: Optional[torch.Tensor] = None, norm: bool = True):
    """x f32 [M, H]: the residual stream before the final RMSNorm (norm = True, the per-layer step) or the post-norm states
    (norm = False: p2t_llama_train_forward has applied it).  labels int64 [B, T] on the device.
    -> (loss f32 [1], logits `dtype` [B, T, ld(V)], saved for head_backward)."""
    s, dt = decoder.spec, decoder.model.dtype
    B, T = labels.shape
    H = s.hidden_size
    if norm:
        a = ops.rmsnorm(x, _norm_weight(decoder), s.rms_norm_eps, out_dtype=dt)
    else:
        a = x if dt == torch.float32 else ops.cast(x, dt)
    logits = ops.gemm_nt(a, decoder._lm_head_padded(), None, n=s.vocab_size, k=H, out_dtype=dt).view(B, T, -1)
    loss, count = ops.cross_entropy_shifted(logits, labels, s.vocab_size, weights=weights)
    return loss, logits, dict(x=x if norm else None, logits=logits, labels=labels, count=count, weights=weights, norm=norm)


def head_backward(decoder, saved: dict) -> torch.Tensor:
    """d loss / d x of head_loss for an upstream gradient of 1 (the callers scale at the end of their chains): f32 [M, H]."""
    s = decoder.spec
    logits = saved["logits"]
    B, T, ld = logits.shape
    H, V = s.hidden_size, s.vocab_size
    d_logits = ops.cross_entropy_shifted_backward(logits, saved["labels"], V, saved["count"], weights=saved["weights"])
    d_h = ops.gemm_nt(d_logits.view(B * T, ld), decoder._lm_head_transposed(), None, n=H, k=round_up(V, 64), epilogue=_lib.EPI_STORE_F32)   # [M, H] f32
    if not saved["norm"]:
        return d_h
    g = torch.empty((B * T, H), dtype=torch.float32, device=d_h.device)
    _rms_bwd(decoder, saved["x"], d_h, g)
    return g


def head_saved_tensors(saved: dict) -> tuple:
    """What a head's `saved` keeps alive (either form), for `last_tape_bytes`."""
    return tuple(v for v in saved.values() if isinstance(v, torch.Tensor))


# ---------------------------------------------------------------------------------------------------------------------------
# the fused head (target rows only; keeps no logits)
# ---------------------------------------------------------------------------------------------------------------------------
def select_targets(labels: torch.Tensor, V: int, num_targets: Optional[int] = None) -> dict:
    """The target rows of `labels` (int64 [B, T], device) for lm_head_loss.  num_targets: a host upper bound on their number --
    nothing is read back, and a bound that is too small makes the loss NaN (p2t_lm_loss_reduce) instead of training on a subset.
    None: the 4-byte count is read here (one host sync; call this before the towers are enqueued, so that the wait is only for
    earlier work).  The capacity of the compact buffers is the bound, or the count, rounded up to 128."""
    B, T = labels.shape
    if num_targets is None:
        rows, targets, count = ops.lm_target_rows(labels, V, B * T, size=round_up(B * T, ROW_ALIGN))
        n = int(count[0].item())
        bound = max(n, 1)
        capacity = round_up(bound, ROW_ALIGN)
        rows, targets = rows[:capacity], targets[:capacity]      # entries n .. are -1 already
    else:
        bound = max(int(num_targets), 1)
        capacity = round_up(bound, ROW_ALIGN)
        rows, targets, count = ops.lm_target_rows(labels, V, bound, size=capacity)
    dev = labels.device
    return dict(rows=rows, targets=targets, count=count, capacity=capacity,
                limit=torch.full((1,), bound, dtype=torch.int32, device=dev),      # the listed entries: min(count, limit)
                iota=torch.arange(capacity, dtype=torch.int32, device=dev))


def lm_head_loss(decoder, x_last: torch.Tensor, labels: torch.Tensor, *, weights: Optional[torch.Tensor] = None,
                 capacity: Optional[int] = None, chunk_rows: int = 1024, norm: bool = True, targets: Optional[dict] = None,
                 with_grad: Optional[bool] = None):
    """LM loss of the rows with a counted target.  x_last f32 [M, H] as `head_loss`'s x (norm = False: post-norm states, the
    frozen-decoder chain); labels int64 [B, T] on the device; weights f32 [B, T] or None; capacity: a host bound on the number of
    target rows (see select_targets; None reads the count), or pass `targets` = select_targets(...) made earlier.
    with_grad: None = torch.is_grad_enabled(); an autograd.Function's forward runs with gradients disabled and says what it needs.
    -> (loss f32 [1], saved): saved is None without gradients (eval: the dX GEMM and everything kept are skipped), else what
    lm_head_backward reads -- no logits."""
    s, dt = decoder.spec, decoder.model.dtype
    H, V = s.hidden_size, s.vocab_size
    M = x_last.shape[0]
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be positive")
    sel = targets if targets is not None else select_targets(labels, V, capacity)
    cap, rows, count = sel["capacity"], sel["rows"], sel["count"]
    dev = x_last.device
    with_grad = torch.is_grad_enabled() if with_grad is None else bool(with_grad)
    xc = torch.zeros((cap, H), dtype=torch.float32, device=dev)          # pad rows are zero: zero norm, zero logits, no loss, no gradient
    call("p2t_gather_rows_f32", ptr(xc), xc.stride(0), ptr(sel["iota"]), ptr(x_last), x_last.stride(0), ptr(rows), ptr(count), ptr(sel["limit"]),
         cap, H, stream())
    if norm:
        a = ops.rmsnorm(xc, _norm_weight(decoder), s.rms_norm_eps, out_dtype=dt)
    else:
        a = xc if dt == torch.float32 else ops.cast(xc, dt)
    chunk = min(round_up(int(chunk_rows), ROW_ALIGN), cap)
    ld = round_up(V, 64)
    buf = torch.empty((chunk, ld), dtype=dt, device=dev)                  # the one logits buffer, overwritten by its own gradient
    row_loss = torch.empty((cap,), dtype=torch.float32, device=dev)
    d_a = torch.empty((cap, H), dtype=torch.float32, device=dev) if with_grad else None
    w, wT = decoder._lm_head_padded(), (decoder._lm_head_transposed() if with_grad else None)
    for c0 in range(0, cap, chunk):
        r = min(chunk, cap - c0)
        ops.gemm_nt(a[c0:c0 + r], w, None, n=V, k=H, out=buf[:r])
        ops.lm_loss_grad_rows(buf[:r], V, rows, sel["targets"], count, row_loss, first=c0, weights=weights, with_grad=with_grad)
        if with_grad:
            ops.gemm_nt(buf[:r], wT, None, n=H, k=ld, epilogue=_lib.EPI_STORE_F32, out=d_a[c0:c0 + r])
    loss = ops.lm_loss_reduce(row_loss, rows, count, weights=weights)
    if not with_grad:
        return loss, None
    return loss, dict(d_a=d_a, xc=xc if norm else None, rows=rows, count=count, limit=sel["limit"], iota=sel["iota"], norm=norm, M=M)


def lm_head_backward(decoder, saved: dict, g_loss: Optional[torch.Tensor]) -> torch.Tensor:
    """d loss / d x_last, f32 [M, H], zero outside the target rows.  g_loss: the upstream gradient as a device scalar (1 / GA under
    gradient accumulation), multiplied in here (p2t_scale_by_device_scalar); None leaves the result unscaled for a caller that
    scales at the end of its own chain.  Consumes `saved` (the kept gradient is scaled in place)."""
    d_a, rows = saved["d_a"], saved["rows"]
    cap, H = d_a.shape
    if g_loss is not None:
        call("p2t_scale_by_device_scalar", ptr(d_a), d_a.numel(), ptr(g_loss.float().reshape(1).contiguous()), stream())
    if saved["norm"]:
        d_x = torch.empty((cap, H), dtype=torch.float32, device=d_a.device)
        _rms_bwd(decoder, saved["xc"], d_a, d_x)
    else:
        d_x = d_a
    out = torch.zeros((saved["M"], H), dtype=torch.float32, device=d_a.device)
    call("p2t_gather_rows_f32", ptr(out), out.stride(0), ptr(rows), ptr(d_x), d_x.stride(0), ptr(saved["iota"]), ptr(saved["count"]),
         ptr(saved["limit"]), cap, H, stream())
    return out
