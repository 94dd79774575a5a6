"""The LoRA branch of the stage-2 per-layer steps, shared by both towers (p2t_hip/decoder_train.py, p2t_hip/encoder_train.py):

    resolve_targets which projections of the two towers a peft `target_modules` list selects
    LoraPairs       the trainable A [r, in] / B [out, r] pairs of one tower: init, hyper-parameters, dropout seeds, the GEMM-layout
                    operands an optimizer may keep for them, peft's key layout.  A tower states only data (class attributes).
    LoraLinear      one frozen projection W [N, K] (+ bias) of one layer with its branch: y = W x + b + s B (A drop(x)), and its backward
    _transposed     the cached [K, N padded] copy of a frozen weight for the dX GEMMs
    tape_bytes      the bytes a pass keeps for its backward (`last_tape_bytes` of a tower)
    scaled_grads    the collected (buffer, rows, columns, factor) gradients, scaled and cut for autograd

Every product is p2t_gemm_nt, but dA / dB of the checkpointed backward (p2t_lora_wgrad: the token axis summed in place); the branch's input
dropout is p2t_dropout_rows (a counter-hash mask, regenerated in the backward).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib, ops
from ._lib import call
from .ops import ptr, round_up, stream

DECODER_TARGETS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
ENCODER_TARGETS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "intermediate.dense", "output.dense")


def _matches(name: str, target: str) -> bool:
    """peft's suffix rule (tuners_utils.check_target_module_exists): the module key equals the target or ends in "." + target."""
    return name == target or name.endswith("." + target)


def resolve_targets(target_modules: Sequence[str]) -> Tuple[Tuple[str, ...], Tuple[str, ...]]:
    """-> (decoder targets, encoder targets) selected by `target_modules`, as per-layer module names.
    Every name must select at least one module of this model (the decoder's seven projections, ESM2's six linears)."""
    if isinstance(target_modules, str):
        target_modules = [target_modules]
    dec, enc = [], []
    for t in target_modules:                            # the order of `target_modules` (parameter order), each module once
        dec += [n for n in DECODER_TARGETS if _matches(n, t) and n not in dec]
        enc += [n for n in ENCODER_TARGETS if _matches(n, t) and n not in enc]
    bad = [t for t in target_modules if not any(_matches(n, t) for n in DECODER_TARGETS + ENCODER_TARGETS)]
    if bad:
        raise ValueError(f"unsupported LoRA targets {bad}; decoder targets are {DECODER_TARGETS}, ESM2 encoder targets are {ENCODER_TARGETS} "
                         "(a target selects every module whose name is it or ends in '.' + it)")
    return tuple(dec), tuple(enc)


class LoraPairs(nn.Module):
    """`LoraConfig(r, lora_alpha, lora_dropout, target_modules)` on one tower: fp32 masters initialised as peft does
    (`init_lora_weights=True`: A ~ kaiming-uniform(a = sqrt 5), B = 0), drawn from one CPU generator in layer-major, then target, order.
    A subclass names its tower: TARGETS, WEIGHT (layer i's weight of target t in the parameter owner), MODULE (peft's module path),
    SEED_OFFSET (keeps the towers' dropout masks apart)."""

    TOWER: str
    TARGETS: Tuple[str, ...]
    WEIGHT: str
    MODULE: str
    SEED_OFFSET: int

    def __init__(self, owner: nn.Module, n_layers: int, r: int, lora_alpha: Optional[float], lora_dropout: float, target_modules: Sequence[str],
                 seed: int):
        super().__init__()
        if r < 1:
            raise ValueError("LoRA rank must be >= 1")
        bad = [t for t in target_modules if t not in self.TARGETS]
        if bad:
            raise ValueError(f"unsupported {self.TOWER} LoRA targets {bad}; its targets are {self.TARGETS}")
        self.r, self.alpha, self.p, self.targets = int(r), float(2 * r if lora_alpha is None else lora_alpha), float(lora_dropout), tuple(target_modules)
        self.seed, self.step_count = int(seed), 0
        self.rank = 0                                   # data-parallel rank: ranks > 0 draw their own dropout masks (rank 0: unchanged)
        self.n_layers = int(n_layers)
        self._operands, self._operand_key = {}, {}
        P = dict(owner.named_parameters())
        gen = torch.Generator(device="cpu").manual_seed(seed)
        for i in range(self.n_layers):
            for t in self.targets:
                w = P[self.WEIGHT.format(i=i, t=t)]
                a = torch.empty((r, w.shape[1]), dtype=torch.float32)
                bound = 1.0 / math.sqrt(w.shape[1])                    # kaiming_uniform_(a = sqrt(5)) on [r, in]
                a.uniform_(-bound, bound, generator=gen)
                self.register_parameter(self._name(i, t, "A"), nn.Parameter(a.to(w.device)))
                self.register_parameter(self._name(i, t, "B"), nn.Parameter(torch.zeros((w.shape[0], r), dtype=torch.float32, device=w.device)))

    @staticmethod
    def _name(i: int, target: str, which: str) -> str:
        return f"l{i}_{target.replace('.', '_')}_{which}"

    @property
    def scale(self) -> float:
        return self.alpha / self.r

    def get(self, i: int, target: str) -> Optional[Tuple[nn.Parameter, nn.Parameter]]:
        if target not in self.targets:
            return None
        return getattr(self, self._name(i, target, "A")), getattr(self, self._name(i, target, "B"))

    def pairs(self) -> List[tuple]:
        """[(layer, target, A, B)] in parameter order."""
        return [(i, t, *self.get(i, t)) for i in range(self.n_layers) for t in self.targets]

    def seed_for(self, i: int, target: str) -> int:
        """The dropout mask seed of one projection at the current step (p2t_dropout_rows)."""
        s = (self.seed * 1000003 + self.step_count * 7919 + i * 131 + self.SEED_OFFSET + self.TARGETS.index(target)
             + self.rank * 0x9E3779B97F4A7C15)
        return s & 0x7FFFFFFFFFFFFFFF

    def zero_operands(self, i: int, target: str, dt) -> Tuple[torch.Tensor, torch.Tensor]:
        """Zeroed GEMM-layout operands of one projection in `dt`: a16 holds A as [rp, K padded to 8] and bs16 holds (alpha / r) B as
        [N, rp padded to 64], rp = r padded to 16 (p2t_gemm_nt wants N % 16 == 0: the rank axis is zero padded to rp everywhere)."""
        a, b = self.get(i, target)
        rp = round_up(self.r, 16)
        return (torch.zeros((rp, round_up(a.shape[1], 8)), dtype=dt, device=a.device),
                torch.zeros((b.shape[0], round_up(rp, 64)), dtype=dt, device=a.device))

    def set_operands(self, operands: Optional[Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]]]):
        """Register GEMM-layout operands {(layer, target): (a16, bs16)} (`zero_operands`' layout) that an optimizer keeps equal to what
        LoraLinear would build from the masters; None drops them.  They count as current for the masters' `_version` at this call:
        `mark_operands_current()` after every write of the owner."""
        self._operands = dict(operands) if operands else {}
        self.mark_operands_current()

    def mark_operands_current(self):
        self._operand_key = {k: (a._version, b._version) for k in self._operands for a, b in (self.get(*k),)}

    def operands(self, i: int, target: str, dt) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """The registered (a16, bs16) of one projection, or None when there are none or a master changed since the owner's last
        write (load_state_dict, copy_, ...: anything that bumps the parameter's version)."""
        hit = self._operands.get((i, target))
        if hit is None or hit[0].dtype != dt:
            return None
        a, b = self.get(i, target)
        return hit if self._operand_key.get((i, target)) == (a._version, b._version) else None

    def peft_items(self, prefix: str = "base_model.model.") -> List[Tuple[str, nn.Parameter]]:
        """[(peft key, parameter)] in parameter order: `{prefix}{MODULE}.lora_A.weight`, then lora_B, of every pair."""
        return [(f"{prefix}{self.MODULE.format(i=i, t=t)}.lora_{w}.weight", q) for i, t, a, b in self.pairs() for w, q in (("A", a), ("B", b))]

    def peft_state_dict(self, prefix: str = "base_model.model.") -> Dict[str, torch.Tensor]:
        """The adapter in the key layout p2t_hip/lora.py reads (peft's, restated without the library: unverified against it)."""
        return {k: q.detach().clone() for k, q in self.peft_items(prefix)}


def _transposed(owner: nn.Module, name: str, w: torch.Tensor) -> torch.Tensor:
    """[in, out padded to 64] copy of the frozen weight `name` for the dX GEMMs, built once per weight version and kept on the owner
    (`_lora_wT`): a second copy of the frozen projections, about 5 GB for ESM2-3B's six linears per layer in bf16 (tools/sft_bench.py
    `encoder` reports it).  The encoder drops its copies when its engine is invalidated (p2t_hip.lora.merge_lora_state_dict does)."""
    cache = owner.__dict__.setdefault("_lora_wT", {})
    key = (w.data_ptr(), w._version)
    hit = cache.get(name)
    if hit is None or hit[0] != key:
        cache[name] = (key, ops.transpose(w.detach(), round_up(w.shape[0], 64)))
    return cache[name][1]


def _zero_tail(t: torch.Tensor, m: int):
    if t.shape[1] > m:
        t[:, m:].zero_()


class LoraLinear:
    """One projection `name` of a parameter dict P (built once per pass from `owner`): frozen W [N, K], the bias when P has one, and the
    pair of (lora, i, target) when there is one.  Without a bias the output is f32 [M, N] (EPI_STORE_F32), with one f32 [M, N padded to
    64] (EPI_STORE); either may instead accumulate into the fp32 residual stream."""

    def __init__(self, owner: nn.Module, P: Dict[str, torch.Tensor], name: str, lora: Optional[LoraPairs], i: int, target: str, dt,
                 dropout: float):
        self.owner, self.name, self.dt = owner, name, dt
        self.w = P[name + ".weight"].detach()
        bias = P.get(name + ".bias")
        self.bias = bias.detach().float().contiguous() if bias is not None else None
        self.N, self.K = self.w.shape
        self.ab = lora.get(i, target) if lora is not None else None
        if self.ab is None:
            return
        a, b = self.ab
        self.r, self.s, self.rp = a.shape[0], lora.scale, round_up(a.shape[0], 16)
        self.p, self.seed = float(dropout), lora.seed_for(i, target)
        # operands of the low-rank products in the model dtype (the masters stay fp32): the ones an optimizer registered
        # (InstructTrainer: written by its AdamW step), else built here from the masters
        hit = lora.operands(i, target, dt)
        if hit is None:
            hit = lora.zero_operands(i, target, dt)
            hit[0][:self.r, :self.K] = a.detach().to(dt)
            hit[1][:, :self.r] = (b.detach() * self.s).to(dt)
        self.a16, self.bs16 = hit

    def transposed(self) -> torch.Tensor:
        return _transposed(self.owner, self.name, self.w)

    # -- forward: f32 y, or accumulated into the fp32 residual stream `resid`
    def forward(self, x: torch.Tensor, resid: Optional[torch.Tensor] = None, keep_u: bool = True):
        """-> (y, or None when accumulated into `resid`; u = drop(x) A^T [M, rp padded to 64] or None)."""
        y = None
        if resid is not None:
            ops.gemm_nt(x, self.w, self.bias, n=self.N, k=self.K, epilogue=_lib.EPI_RESID, out=resid)
        elif self.bias is None:
            y = ops.gemm_nt(x, self.w, None, n=self.N, k=self.K, epilogue=_lib.EPI_STORE_F32)
        else:
            y = ops.gemm_nt(x, self.w, self.bias, n=self.N, k=self.K, epilogue=_lib.EPI_STORE, out_dtype=torch.float32)
        if self.ab is None:
            return y, None
        u = self.branch_input(x)
        if resid is not None:
            ops.gemm_nt(u, self.bs16, None, n=self.N, k=self.rp, epilogue=_lib.EPI_RESID, out=resid)
        else:
            ops.gemm_nt(u, self.bs16, None, n=self.N, k=self.rp, epilogue=_lib.EPI_STORE_F32, out=y, accumulate=True)
        return y, (u if keep_u else None)

    def branch_input(self, x: torch.Tensor) -> Optional[torch.Tensor]:
        """u = drop(x) A^T [M, rp padded to 64] of the branch, None without a pair (the checkpointed backward asks for it alone where it
        does not redo the projection)."""
        if self.ab is None:
            return None
        return ops.gemm_nt(self.dropped(x), self.a16, None, n=self.rp, k=self.K, epilogue=_lib.EPI_STORE, out_dtype=self.dt)

    def dropped(self, x: torch.Tensor) -> torch.Tensor:
        if self.p <= 0.0:
            return x
        xd = torch.empty((x.shape[0], round_up(self.K, 64)), dtype=self.dt, device=x.device)
        if xd.shape[1] != self.K:
            xd.zero_()
        call("p2t_dropout_rows", ptr(x), ops.dt_of(x), x.stride(0), ptr(xd), ops.dt_of(xd), xd.stride(0), x.shape[0], self.K, self.p, int(self.seed), 0,
             stream())
        return xd

    # -- backward: dy `dt` [M, >= N] -> dX; the pair's gradients into `grads`
    def backward(self, dy: torch.Tensor, x: torch.Tensor, u: Optional[torch.Tensor], out: Optional[torch.Tensor], out_f32: bool, accumulate: bool,
                 grads: dict, token_axis: bool = False) -> torch.Tensor:
        """dX (+)= dy W (+ the branch's share); x: the projection's input as the forward saw it (before the dropout).
        token_axis: dB and dA by p2t_lora_wgrad, which sums over the token rows of dy, u, x and du as they lie in memory (the dropout of
        x applied on the fly), instead of p2t_gemm_nt over four transposed copies and a dropped copy of x.  The two differ in the order
        of the fp32 sum over tokens, nothing else."""
        wT = self.transposed()                                                                      # [K, N padded]
        if out_f32:
            dx = ops.gemm_nt(dy, wT, None, n=self.K, k=self.N, epilogue=_lib.EPI_STORE_F32, out=out, accumulate=accumulate)
        else:
            assert not accumulate
            dx = ops.gemm_nt(dy, wT, None, n=self.K, k=self.N, epilogue=_lib.EPI_STORE, out=out, out_dtype=self.dt)
        if self.ab is None:
            return dx
        a, b = self.ab
        r, rp, M = self.r, self.rp, dy.shape[0]
        # du = dy (s B)  [M, rp]; dB = s dy^T u; dA = du^T drop(x); dX += drop'(du A)
        bsT = ops.transpose(self.bs16[:, :rp].contiguous(), round_up(self.N, 64))                   # [rp, N]
        du = ops.gemm_nt(dy, bsT, None, n=rp, k=self.N, epilogue=_lib.EPI_STORE, out_dtype=self.dt) # [M, 64]
        if token_axis:
            dB = ops.lora_wgrad(dy, u, c=self.N, r=rp)                                              # [N, rp] = dy^T u
            dA = ops.lora_wgrad(x, du, c=self.K, r=rp, transposed=True, p=self.p, seed=self.seed)   # [rp, K] = du^T drop(x)
        else:
            dA, dB = self._wgrad_transposed(dy, x, u, du)
        grads[id(a)] = (dA, r, self.K, 1.0)           # (buffer, rows, columns, factor on top of the upstream gradient)
        grads[id(b)] = (dB, self.N, r, self.s)
        aT = ops.transpose(self.a16[:, :self.K], round_up(rp, 8))                                   # [K, rp] = A^T
        t = ops.gemm_nt(du, aT, None, n=self.K, k=rp, epilogue=_lib.EPI_STORE_F32)                  # [M, K] f32
        call("p2t_dropout_rows", ptr(t), _lib.F32, t.stride(0), ptr(dx), ops.dt_of(dx), dx.stride(0), M, self.K, self.p, int(self.seed), 1, stream())
        return dx

    def _wgrad_transposed(self, dy: torch.Tensor, x: torch.Tensor, u: torch.Tensor, du: torch.Tensor):
        """(dA [rp, K], dB [N, rp]) by p2t_gemm_nt: the token axis made contiguous (p2t_transpose) and zero padded to 64."""
        rp, M = self.rp, dy.shape[0]
        xd = self.dropped(x)
        dyT, uT = ops.transpose(dy[:, :self.N]), ops.transpose(u[:, :rp])                           # [N, Mp], [rp, Mp] (token axis contiguous, zero padded)
        _zero_tail(dyT, M), _zero_tail(uT, M)
        dB = torch.zeros((self.N, rp), dtype=torch.float32, device=dy.device)
        ops.gemm_nt(dyT, uT, None, n=rp, k=round_up(M, 64), epilogue=_lib.EPI_STORE_F32, out=dB)    # [N, rp] = dy^T u
        duT, xdT = ops.transpose(du[:, :rp]), ops.transpose(xd[:, :self.K])
        _zero_tail(duT, M), _zero_tail(xdT, M)
        dA = ops.gemm_nt(duT, xdT, None, n=self.K, k=round_up(M, 64), epilogue=_lib.EPI_STORE_F32)  # [rp, K] = du^T drop(x)
        return dA, dB


def tape_bytes(tape: Sequence[dict], extra: Sequence[Optional[torch.Tensor]] = ()) -> int:
    """Bytes of the distinct tensors a pass keeps for its backward: every tensor of the per-layer records `tape` and of `extra` (what
    the head of the pass keeps); the LoraLinear objects of a record hold weights and operands, no activations, and count nothing."""
    seen, total = set(), 0
    for t in [v for rec in tape for v in rec.values()] + list(extra):
        if isinstance(t, torch.Tensor) and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            total += t.numel() * t.element_size()
    return total


def scaled_grads(params: Sequence[nn.Parameter], grads: dict, g_loss: Optional[torch.Tensor] = None) -> list:
    """The gradients LoraLinear.backward collected, one per parameter (None without one), each buffer scaled in place by its factor
    (dB carries alpha / r) and, when given, by the upstream gradient g_loss (device f32 [1]), then cut to [rows, cols]."""
    out = []
    for prm in params:
        gp = grads.get(id(prm))
        if gp is None:
            out.append(None)
            continue
        buf, rows, cols, factor = gp
        if g_loss is not None:
            call("p2t_scale_by_device_scalar", ptr(buf), buf.numel(), ptr(g_loss if factor == 1.0 else (g_loss * factor).contiguous()), stream())
        elif factor != 1.0:
            call("p2t_scale_by_device_scalar", ptr(buf), buf.numel(), ptr(torch.full((1,), factor, dtype=torch.float32, device=buf.device)), stream())
        out.append(buf[:rows, :cols].to(prm.dtype))
    return out
