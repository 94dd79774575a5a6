"""The stage-2 (instruction tuning) trainer: host-side mirror of what scripts/train_instruct.py does after `loss.backward()`.

    optimizer       train_instruct.py:431-447   AdamW(lr 2e-4, betas (0.9, 0.999), eps 1e-6, weight_decay 0.01) over the LoRA matrices
                                                + adapter.fc1 / fc2 (modules_to_save), cosine warmup (6 %) stepped per optimizer step
    train_epoch     :234-300                    loss / GA -> backward; every GA batches clip_grad_norm_ -> step -> scheduler.step()
    eval_epoch      :303-335                    model.eval(): peft's LoRA dropout is the identity
    checkpoints     :448-455, :489-512          adapter_checkpoint_{e}/ (peft save_pretrained) + optimizer_scheduler_checkpoint_{e}.pt

`InstructTrainer` keeps the fp32 masters, gradients and Adam moments of every trained tensor in ONE flat buffer each (segments
aligned to 16 elements): the LoRA parameters' `.data` / `.grad` ARE views of those buffers, so autograd accumulates the 448 LoRA
gradients in place, the data-parallel exchange is one all-reduce, and the optimizer is two launches (`p2t_clip_adamw_flat`: the
norm, then clip + AdamW over a host-built chunk table).  The same update writes the bf16 GEMM operands of the next forward
(A as `a16`, (alpha / r) B as `bs16`), which `DecoderLora.set_operands` hands to the per-layer LoRA path instead of rebuilding them.

The epoch drivers of the contrastive stage work unchanged on this trainer: `P.train_epoch(trainer, loader)` /
`P.eval_epoch(trainer, loader)`; `run_instruct_epochs` is `P.run_epochs` with the stage-2 checkpoint files.

`peft` is not importable here: the checkpoint layout (adapter_config.json + adapter_model.safetensors, keys as
`DecoderLora.peft_state_dict`) is peft's published one restated, and the optimizer state is indexed over the trainer's tensors
(LoRA matrices in `peft_state_dict` order, then adapter fc1.weight, fc1.bias, fc2.weight, fc2.bias).  Compatibility with files a
real peft run wrote (the parameter order of a `PeftModel`) is UNPINNED, as in p2t_hip/lora.py.
"""
from __future__ import annotations

import json
import math
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops, sharding
from ._lib import call
from .ops import ptr, stream

ALIGN = 16                                           # segment offsets: float4 access is legal everywhere
ADAPTER_KEYS = ("adapter.fc1.weight", "adapter.fc1.bias", "adapter.fc2.weight", "adapter.fc2.bias")
_PEFT_PREFIX = "base_model.model."

SEGMENT_DTYPE = np.dtype([("offset", "<i8"), ("numel", "<i8"), ("shadow", "<u8"), ("rows", "<i8"), ("cols", "<i8"), ("ld", "<i8"),
                          ("scale", "<f4"), ("shadow_dtype", "<i4")])                  # p2t_flat_segment
CHUNK_DTYPE = np.dtype([("start", "<i8"), ("segment", "<i4"), ("count", "<i4")])        # p2t_flat_chunk


# ---------------------------------------------------------------------------------------------------------------------------
# host planning (pure numpy)
# ---------------------------------------------------------------------------------------------------------------------------
def plan_segments(numels: Sequence[int], align: int = ALIGN) -> Tuple[np.ndarray, int]:
    """Offsets of tensors of `numels` elements packed in order into one flat buffer, each at a multiple of `align`;
    -> (offsets int64 [n], buffer length: the last segment's end rounded up to `align`)."""
    n = np.asarray(list(numels), dtype=np.int64)
    if n.ndim != 1 or len(n) == 0 or (n <= 0).any():
        raise ValueError("every trained tensor needs at least one element")
    padded = (n + align - 1) // align * align
    offsets = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    return offsets, int(padded.sum())


def plan_chunks(offsets: np.ndarray, numels: Sequence[int], chunk: int = _lib.FLAT_CHUNK) -> np.ndarray:
    """The chunk table of p2t_clip_adamw_flat: every segment cut into pieces of at most `chunk` elements, in flat order;
    -> structured array (start, segment, count), CHUNK_DTYPE."""
    n = np.asarray(list(numels), dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    if len(n) >= 2 ** 31:
        raise ValueError("too many segments")
    per = (n + chunk - 1) // chunk
    seg = np.repeat(np.arange(len(n), dtype=np.int64), per)
    first = np.concatenate([[0], np.cumsum(per)[:-1]])
    k = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(first, per)          # index of the chunk inside its segment
    out = np.empty(len(seg), dtype=CHUNK_DTYPE)
    out["start"] = offsets[seg] + k * chunk
    out["segment"] = seg
    out["count"] = np.minimum(chunk, n[seg] - k * chunk)
    return out


class FlatAdamW:
    """clip_grad_norm_ + torch's AdamW over tensors kept in flat f32 buffers (`flat_p`, `flat_g`, `flat_m`, `flat_v`), one
    `p2t_clip_adamw_flat` call per step.  shadows[i]: None or (tensor, rows, cols, scale): after every step the 2-D `tensor`
    (bf16 / f32, unit column stride) holds RNE(scale * p_i) viewed as [rows, cols] in its leading rows / columns."""

    def __init__(self, numels: Sequence[int], device, shadows: Optional[Sequence[Optional[tuple]]] = None):
        self.numels = [int(v) for v in numels]
        self.offsets, self.total = plan_segments(self.numels)
        dev = torch.device(device)
        z = lambda: torch.zeros((self.total,), dtype=torch.float32, device=dev)
        self.flat_p, self.flat_g, self.flat_m, self.flat_v = z(), z(), z(), z()
        shadows = list(shadows) if shadows is not None else [None] * len(self.numels)
        if len(shadows) != len(self.numels):
            raise ValueError("one shadow entry (or None) per tensor")
        seg = np.zeros(len(self.numels), dtype=SEGMENT_DTYPE)
        seg["offset"], seg["numel"], seg["scale"], seg["cols"], seg["ld"], seg["rows"] = self.offsets, self.numels, 1.0, 1, 1, 1
        self.shadows = shadows
        for i, sh in enumerate(shadows):
            if sh is None:
                continue
            t, rows, cols, scale = sh
            if t.dim() != 2 or t.stride(1) != 1 or t.dtype not in (torch.float32, torch.bfloat16) or t.device != dev:
                raise ValueError(f"shadow {i}: a 2-D bf16 / f32 tensor on {dev} with unit column stride")
            if rows * cols != self.numels[i] or rows > t.shape[0] or cols > t.shape[1]:
                raise ValueError(f"shadow {i}: [{rows}, {cols}] does not hold {self.numels[i]} elements inside {tuple(t.shape)}")
            for f, val in (("shadow", t.data_ptr()), ("rows", rows), ("cols", cols), ("ld", t.stride(0)), ("scale", scale),
                           ("shadow_dtype", _lib.BF16 if t.dtype == torch.bfloat16 else _lib.F32)):
                seg[f][i] = val
        chunks = plan_chunks(self.offsets, self.numels)
        self.n_chunks = len(chunks)
        self.segment_table = torch.from_numpy(seg.view(np.uint8).copy()).to(dev)
        self.chunk_table = torch.from_numpy(chunks.view(np.uint8).copy()).to(dev)
        self.scratch = torch.empty((_lib.FLAT_NORM_BLOCKS,), dtype=torch.float32, device=dev)
        self.grad_norm = torch.zeros((1,), dtype=torch.float32, device=dev)

    def view(self, flat: torch.Tensor, i: int, shape=None) -> torch.Tensor:
        v = flat[int(self.offsets[i]): int(self.offsets[i]) + self.numels[i]]
        return v.view(shape) if shape is not None else v

    def step(self, step: int, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.01,
             max_norm: Optional[float] = None) -> torch.Tensor:
        """Optimizer step number `step` (1-based: the bias corrections) at learning rate `lr`; -> grad_norm (device f32 [1])."""
        mn = 0.0 if (max_norm is None or math.isinf(max_norm)) else float(max_norm)
        call("p2t_clip_adamw_flat", ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), ptr(self.flat_v), self.total,
             ptr(self.segment_table), ptr(self.chunk_table), self.n_chunks, int(step), float(lr), float(betas[0]), float(betas[1]),
             float(eps), float(weight_decay), mn, ptr(self.grad_norm), ptr(self.scratch), stream())
        return self.grad_norm

    @torch.no_grad()
    def refresh_shadows(self):
        """Shadows from the current masters with torch ops (after a load): the same RNE(scale * p) the step writes."""
        for i, sh in enumerate(self.shadows):
            if sh is not None:
                t, rows, cols, scale = sh
                p = self.view(self.flat_p, i, (rows, cols))
                t[:rows, :cols].copy_((p * scale).to(t.dtype) if scale != 1.0 else p.to(t.dtype))

    def bytes_per_step(self) -> int:
        """HBM bytes one step moves: g read twice (norm + update), p, m, v read and written, the shadows written."""
        sh = sum(self.numels[i] * (2 if s[0].dtype == torch.bfloat16 else 4) for i, s in enumerate(self.shadows) if s is not None)
        return self.total * 4 * 8 + sh


def instruct_schedule(base_lr: float, num_epochs: int, batches_per_epoch: int, gradient_accumulation_steps: int = 1):
    """`get_cosine_schedule_with_warmup(optimizer, int(0.06 * total), total)` with total = len(train_loader) * num_epochs // GA
    (train_instruct.py:436-447; note the order: the contrastive stage computes num_epochs * (len // GA))."""
    from .training_state import CosineWarmupSchedule
    total = batches_per_epoch * num_epochs // gradient_accumulation_steps
    return CosineWarmupSchedule(base_lr, int(0.06 * total), total)


# ---------------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------------
class InstructTrainer:
    """Stage-2 step of Esm2LlamaInstructForCausalLM with LoRA (`model.add_lora(...)` first): `model(..., labels=...)` ->
    backward of loss / GA -> at every GA boundary one all-reduce of the flat gradient (world > 1), the fused clip + AdamW, one
    `schedule.step()`, zeroing.  Same protocol as ContrastiveTrainer (`step`, `evaluate`, `grad_norm`, `step_count`, `hp`,
    `schedule`, `dev`, `group`, `train_mode`), so `loop.train_epoch` / `eval_epoch` drive it.

    train_adapter=False is the reference's --fix_modality_adapter (no modules_to_save).  An fp32 adapter's parameters become views of
    the flat buffers like the LoRA matrices; a bf16 adapter keeps its module tensors, which the optimizer writes as shadows of the
    fp32 masters, and its bf16 gradients are folded into the flat buffer after every micro-batch.
    The step adds no host synchronisation of its own (the model's placeholder-count check reads one count, as torch's boolean
    assignment in the reference does).
    fused_lm_loss=True switches the decoder to the LM loss over the target rows only (`model.fused_lm_loss()`, p2t_hip/lm_head.py) for
    `step` and `evaluate`; a batch's `num_targets` (p2t_hip.data.pack_instruct_batch) is passed through as the host bound, without it
    the head reads the 4-byte target count once per forward.  False (the default) leaves the model as it is."""

    def __init__(self, model, *, lr=2e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, max_norm=None,
                 gradient_accumulation_steps: int = 1, schedule=None, process_group=None, train_adapter: bool = True,
                 fused_lm_loss: bool = False):
        lora = getattr(model.llama_decoder, "lora", None)
        enc_lora = getattr(getattr(model, "esm_encoder", None), "lora", None)     # LoRA on the ESM2 encoder (p2t_hip/encoder_train.py)
        if lora is None and enc_lora is None:
            raise ValueError("InstructTrainer trains LoRA adapters: call model.add_lora(...) first")
        if int(gradient_accumulation_steps) != gradient_accumulation_steps or gradient_accumulation_steps < 1:
            raise ValueError("gradient_accumulation_steps must be an integer >= 1")
        if not lr > 0 or not eps > 0 or weight_decay < 0:
            raise ValueError("need lr > 0, eps > 0 and weight_decay >= 0")
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError("betas must be two values in [0, 1)")
        if max_norm is not None and not max_norm > 0:
            raise ValueError("max_norm must be positive (None: no clipping)")
        self.model, self.lora, self.enc_lora = model, lora, enc_lora
        if fused_lm_loss:
            model.fused_lm_loss(True)
        self.hp = dict(lr=float(lr), betas=tuple(float(b) for b in betas), eps=float(eps), weight_decay=float(weight_decay),
                       max_norm=math.inf if max_norm is None else float(max_norm))
        self.schedule, self.group = schedule, process_group
        self.gradient_accumulation_steps, self._micro, self._dirty = int(gradient_accumulation_steps), 0, False
        self.step_count, self.train_mode, self.train_adapter = 0, True, bool(train_adapter)
        dec = model.llama_decoder
        self.dt = dec.model.dtype
        dev = next((lora if lora is not None else enc_lora).parameters()).device
        self.dev = dev
        rank, world = sharding.world_info(process_group)
        # ---- trained tensors: decoder LoRA, encoder LoRA (each in peft_state_dict order), then the adapter
        self.names: List[str] = []
        self.params: List[torch.nn.Parameter] = []
        shadows, self._operands, self._enc_operands = [], {}, {}
        towers = [(lora, self._operands, self.dt), (enc_lora, self._enc_operands, model.esm_encoder.dtype if enc_lora is not None else None)]
        for lo, operands, dt in towers:
            if lo is None:
                continue
            lo.rank = rank if world > 1 else 0        # each rank its own dropout masks; a single process keeps the old sequence
            for i, t, a, b in lo.pairs():
                a16, bs16 = operands[(i, t)] = lo.zero_operands(i, t, dt)
                shadows += [(a16, lo.r, a.shape[1], 1.0), (bs16, b.shape[0], lo.r, lo.scale)]
            for name, q in lo.peft_items(prefix=""):
                self.names.append(name)
                self.params.append(q)
        ad = model.adapter
        ad_params = (ad.fc1.weight, ad.fc1.bias, ad.fc2.weight, ad.fc2.bias)
        self._adapter_views = self.train_adapter and ad.fc1.weight.dtype == torch.float32
        if self.train_adapter:
            ad.requires_grad_(True)
            for n, q in zip(ADAPTER_KEYS, ad_params):
                self.names.append(n)
                self.params.append(q)
                shadows.append(None if self._adapter_views else (q.data.view(-1, q.shape[-1]), q.numel() // q.shape[-1], q.shape[-1], 1.0))
        else:
            ad.requires_grad_(False)
        self.n_lora = 2 * (len(self._operands) + len(self._enc_operands))
        self.opt = FlatAdamW([q.numel() for q in self.params], dev, shadows)
        with torch.no_grad():
            for k, q in enumerate(self.params):
                self.opt.view(self.opt.flat_p, k).copy_(q.detach().reshape(-1).float())
        for k, q in enumerate(self.params):
            if k < self.n_lora or self._adapter_views:
                q.data = self.opt.view(self.opt.flat_p, k, q.shape)
                q.grad = self.opt.view(self.opt.flat_g, k, q.shape)
        self.opt.refresh_shadows()
        for lo, ops_ in ((lora, self._operands), (enc_lora, self._enc_operands)):
            if lo is not None:
                lo.set_operands(ops_)
        self.grad_norm = self.opt.grad_norm

    @property
    def loras(self):
        """The LoRA modules this trainer optimises (decoder, encoder), those that exist."""
        return [lo for lo in (self.lora, self.enc_lora) if lo is not None]

    def _mark_operands_current(self):
        for lo in self.loras:
            lo.mark_operands_current()

    # ---- protocol of loop.train_epoch / eval_epoch
    @property
    def flat_p(self):
        return self.opt.flat_p

    @property
    def flat_g(self):
        return self.opt.flat_g

    def _fold_adapter_grads(self):
        """bf16 adapter: its module gradients (this micro-batch) into the flat fp32 buffer."""
        if not self.train_adapter or self._adapter_views:
            return
        for k in range(self.n_lora, len(self.params)):
            q = self.params[k]
            if q.grad is not None:
                self.opt.view(self.opt.flat_g, k).add_(q.grad.reshape(-1).float())
                q.grad = None

    def step(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """One micro-batch of train_instruct.py's train_epoch: forward with labels, backward of loss / GA (gradients accumulate in
        the flat buffer); every `gradient_accumulation_steps` calls the optimizer step.  -> this batch's unscaled loss (device f32 [1])."""
        _, _, _, do_step = sharding.micro_step_plan(self._micro, self.gradient_accumulation_steps)
        if self._micro == 0 and self._dirty:        # a window restarted (train_epoch resets _micro: the reference's zero_grad, :245)
            self.opt.flat_g.zero_()
        self._dirty = True
        out = self.model(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"],
                         protein_input_ids=batch["protein_input_ids"], protein_attention_mask=batch["protein_attention_mask"],
                         position_ids=batch.get("position_ids"), loss_weights=batch.get("loss_weights"),
                         num_targets=batch.get("num_targets"))
        loss = out.loss
        (loss / self.gradient_accumulation_steps).backward()
        self._fold_adapter_grads()
        self._micro += 1
        if do_step:
            self.optimizer_step()
            self._micro = 0
        return loss.detach().reshape(1)

    def optimizer_step(self) -> torch.Tensor:
        """clip_grad_norm_ -> AdamW.step -> scheduler.step() -> zero_grad (train_instruct.py:282-294): one gradient all-reduce
        across ranks, two launches for the update, the shadows / GEMM operands rewritten on the way."""
        sharding.average_gradients(self.opt.flat_g, self.group)
        self.step_count += 1
        hp = dict(self.hp)
        if self.schedule is not None:
            hp["lr"] = self.schedule.lr()
        self.opt.step(self.step_count, **hp)
        self._mark_operands_current()
        if self.schedule is not None:
            self.schedule.step()
        self.opt.flat_g.zero_()
        self._dirty = False
        return self.grad_norm

    def zero_grad(self):
        """Drop accumulated gradients (start of an epoch: `optimizer.zero_grad()`, :245).  The .grad views stay in place."""
        self.opt.flat_g.zero_()
        self._micro, self._dirty = 0, False

    def end_epoch(self):
        """No-op: stage 2 steps its schedule once per optimizer step (run_epochs calls this after every epoch)."""

    @torch.no_grad()
    def evaluate(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """Forward-only loss with no activation tape, as under the reference's model.eval(): LoRA branches without dropout (peft's
        eval mode), adapter without dropout.  The LoRA mask counters do not move."""
        from .decoder_train import lora_lm_loss
        m = self.model
        was = m.adapter.training
        m.adapter.train(False)
        enc_was = self.enc_lora.training if self.enc_lora is not None else None
        if self.enc_lora is not None:
            self.enc_lora.train(False)               # encoder branches: dropout 0 and no mask step in eval mode (encoder_lora_forward)
        try:
            embeds, mask = m(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], protein_input_ids=batch["protein_input_ids"],
                             protein_attention_mask=batch["protein_attention_mask"], position_ids=batch.get("position_ids"),
                             return_decoder_inputs=True)
        finally:
            m.adapter.train(was)
            if self.enc_lora is not None:
                self.enc_lora.train(enc_was)
        labels = batch["labels"]
        if tuple(labels.shape) != tuple(embeds.shape[:2]):
            raise ValueError(f"labels shape {tuple(labels.shape)} != {tuple(embeds.shape[:2])}")
        if m.llama_decoder.model.gemm_fp8:
            raise ValueError("stage-2 training runs the decoder GEMMs in the model dtype (set_gemm_dtype('model'))")
        docs, weights, pos = None, batch.get("loss_weights"), batch.get("position_ids")
        if pos is not None:                         # packed rows (p2t_hip.data.pack_instruct_batch): as LlamaDecoder.forward
            docs = ops.doc_prepare(pos, mask.to(torch.int64).contiguous())
            if docs is not None:
                labels = labels.masked_fill(pos.to(labels.device) == 0, -100)
        if weights is not None:
            weights = weights.to(device=embeds.device, dtype=torch.float32).contiguous()
        fused = getattr(m.llama_decoder, "_fused_lm_loss", None)
        if fused is not None:                        # as LlamaDecoder.forward: the target rows are listed before the decoder is enqueued
            from . import lm_head
            lab = labels.to(embeds.device).to(torch.int64).contiguous()
            fused = dict(fused, targets=lm_head.select_targets(lab, m.llama_decoder.spec.vocab_size, batch.get("num_targets")))
        loss, _ = lora_lm_loss(m.llama_decoder, self.lora, embeds, mask, labels, dropout=0.0, docs=docs, loss_weights=weights, fused=fused)
        return loss.reshape(1)

    def global_loss(self, loss: torch.Tensor) -> torch.Tensor:
        return sharding.average_loss(loss, self.group)

    # ---- state
    @torch.no_grad()
    def sync_from_masters(self):
        """After the trainer wrote flat_p itself (a load): shadows, bf16 adapter tensors and the registered operands."""
        self.opt.refresh_shadows()
        self._mark_operands_current()

    def adapter_state(self) -> Dict[str, torch.Tensor]:
        """The four adapter tensors (the fp32 masters when trained, the module's otherwise), checkpoint keys."""
        ad = self.model.adapter
        if self.train_adapter:
            return {n: self.opt.view(self.opt.flat_p, self.n_lora + j, q.shape) for j, (n, q) in
                    enumerate(zip(ADAPTER_KEYS, (ad.fc1.weight, ad.fc1.bias, ad.fc2.weight, ad.fc2.bias)))}
        return {"adapter.fc1.weight": ad.fc1.weight, "adapter.fc1.bias": ad.fc1.bias, "adapter.fc2.weight": ad.fc2.weight,
                "adapter.fc2.bias": ad.fc2.bias}


# ---------------------------------------------------------------------------------------------------------------------------
# checkpoints (train_instruct.py:489-512, resume :448-455)
# ---------------------------------------------------------------------------------------------------------------------------
def checkpoint_paths(save_checkpoint_dir: str, epoch_idx: int) -> Tuple[str, str]:
    return (os.path.join(save_checkpoint_dir, f"adapter_checkpoint_{epoch_idx}"),
            os.path.join(save_checkpoint_dir, f"optimizer_scheduler_checkpoint_{epoch_idx}.pt"))


def adapter_config(lora, train_adapter: bool = True, encoder_lora=None) -> Dict[str, Any]:
    """adapter_config.json of `LoraConfig(r, lora_alpha, lora_dropout, target_modules, modules_to_save)` (the keys p2t_hip/lora.py reads);
    target_modules lists the decoder's targets, then the encoder's (either LoRA may be None)."""
    los = [lo for lo in (lora, encoder_lora) if lo is not None]
    lo = los[0]
    return {"peft_type": "LORA", "task_type": None, "r": lo.r, "lora_alpha": lo.alpha, "lora_dropout": lo.p, "bias": "none",
            "target_modules": [t for x in los for t in x.targets], "modules_to_save": ["adapter.fc1", "adapter.fc2"] if train_adapter else None,
            "init_lora_weights": True, "use_rslora": False, "fan_in_fan_out": False, "inference_mode": True}


def adapter_tensors(lora, adapter: Optional[Dict[str, torch.Tensor]], encoder_lora=None) -> Dict[str, torch.Tensor]:
    """adapter_model.safetensors: DecoderLora.peft_state_dict() (+ EncoderLora's) + base_model.model.adapter.fc1 / fc2.weight / bias
    (CPU, contiguous)."""
    out = {k: v.detach().cpu().contiguous() for lo in (lora, encoder_lora) if lo is not None for k, v in lo.peft_state_dict().items()}
    for k, v in (adapter or {}).items():
        out[_PEFT_PREFIX + k] = v.detach().cpu().contiguous()
    return out


def optimizer_state_dict(trainer) -> Dict[str, Any]:
    """`torch.optim.AdamW.state_dict()` over the trainer's tensors (param index = position in `trainer.names`)."""
    from .training_state import _adamw_group_template
    hp = trainer.hp
    group = _adamw_group_template()
    group.update(lr=trainer.schedule.lr() if trainer.schedule is not None else hp["lr"], betas=tuple(hp["betas"]), eps=hp["eps"],
                 weight_decay=hp["weight_decay"])
    if trainer.schedule is not None:
        group["initial_lr"] = trainer.schedule.base_lr
    group["params"] = list(range(len(trainer.params)))
    state = {}
    if trainer.step_count > 0:
        for k, q in enumerate(trainer.params):
            state[k] = {"step": torch.tensor(float(trainer.step_count)), "exp_avg": trainer.opt.view(trainer.opt.flat_m, k, q.shape).cpu().clone(),
                        "exp_avg_sq": trainer.opt.view(trainer.opt.flat_v, k, q.shape).cpu().clone()}
    return {"state": state, "param_groups": [group]}


def save_instruct_checkpoint(trainer: InstructTrainer, save_checkpoint_dir: str, epoch_idx: int) -> List[str]:
    """`model.module.save_pretrained(adapter_checkpoint_{e})` + `torch.save({"optimizer_state_dict", "scheduler_state_dict"},
    optimizer_scheduler_checkpoint_{e}.pt)`; the .pt also carries the dropout counters ("p2t_dropout_state") so that a resume
    draws the same masks.  -> [adapter dir, optimizer file]."""
    from safetensors.torch import save_file
    adir, opath = checkpoint_paths(save_checkpoint_dir, epoch_idx)
    os.makedirs(adir, exist_ok=True)
    with open(os.path.join(adir, "adapter_config.json"), "w") as f:
        json.dump(adapter_config(trainer.lora, trainer.train_adapter, trainer.enc_lora), f, indent=2)
    save_file(adapter_tensors(trainer.lora, trainer.adapter_state() if trainer.train_adapter else None, trainer.enc_lora),
              os.path.join(adir, "adapter_model.safetensors"), metadata={"format": "pt"})
    sched = trainer.schedule.state_dict() if trainer.schedule is not None else None
    ds = {"adapter_calls": int(trainer.model.adapter._calls)}
    if trainer.lora is not None:
        ds["lora_step_count"] = int(trainer.lora.step_count)
    if trainer.enc_lora is not None:
        ds["encoder_lora_step_count"] = int(trainer.enc_lora.step_count)
    torch.save({"optimizer_state_dict": optimizer_state_dict(trainer), "scheduler_state_dict": sched, "p2t_dropout_state": ds}, opath)
    return [adir, opath]


@torch.no_grad()
def load_instruct_checkpoint(trainer: InstructTrainer, adapter_dir: str, opt_path: Optional[str] = None) -> None:
    """Resume (train_instruct.py:148-153, 448-455): LoRA matrices and adapter from `adapter_dir`, Adam moments, step count,
    hyper-parameters, schedule and dropout counters from `opt_path` (optional)."""
    from safetensors.torch import load_file
    tensors = load_file(os.path.join(adapter_dir, "adapter_model.safetensors"))
    index = {(_PEFT_PREFIX + n if n.startswith("adapter.") else "base_model.model." + n): k for k, n in enumerate(trainer.names)}
    for key, t in tensors.items():
        k = index.get(key.replace(".default.", "."))
        if k is None:
            if key.startswith(_PEFT_PREFIX + "adapter.") and not trainer.train_adapter:
                continue
            raise KeyError(f"checkpoint tensor {key} is not a tensor of this trainer")
        q = trainer.params[k]
        if tuple(t.shape) != tuple(q.shape):
            raise ValueError(f"{key}: shape {tuple(t.shape)} != {tuple(q.shape)}")
        trainer.opt.view(trainer.opt.flat_p, k).copy_(t.reshape(-1).to(device=trainer.dev, dtype=torch.float32))
    if opt_path is not None:
        sd = torch.load(opt_path, weights_only=True, map_location="cpu")
        osd = sd["optimizer_state_dict"]
        steps = set()
        for k, q in enumerate(trainer.params):
            st = osd["state"].get(k, osd["state"].get(str(k)))
            m, v = trainer.opt.view(trainer.opt.flat_m, k), trainer.opt.view(trainer.opt.flat_v, k)
            if st is None:
                m.zero_(), v.zero_()
                continue
            if st["exp_avg"].numel() != m.numel():
                raise ValueError(f"optimizer state of tensor {k}: {st['exp_avg'].numel()} elements != {m.numel()}")
            m.copy_(st["exp_avg"].reshape(-1).to(m.device, torch.float32))
            v.copy_(st["exp_avg_sq"].reshape(-1).to(v.device, torch.float32))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"tensors disagree on the Adam step count: {sorted(steps)}")
        trainer.step_count = steps.pop() if steps else 0
        group = osd["param_groups"][0]
        trainer.hp.update(betas=tuple(group["betas"]), eps=float(group["eps"]), weight_decay=float(group["weight_decay"]),
                          lr=float(group.get("initial_lr", group["lr"])))
        if trainer.schedule is not None and sd.get("scheduler_state_dict") is not None:
            trainer.schedule.load_state_dict(sd["scheduler_state_dict"])
        ds = sd.get("p2t_dropout_state") or {}
        if trainer.lora is not None:
            trainer.lora.step_count = int(ds.get("lora_step_count", trainer.lora.step_count))
        if trainer.enc_lora is not None:
            trainer.enc_lora.step_count = int(ds.get("encoder_lora_step_count", trainer.enc_lora.step_count))
        trainer.model.adapter._calls = int(ds.get("adapter_calls", trainer.model.adapter._calls))
    trainer.sync_from_masters()


def run_instruct_epochs(trainer: InstructTrainer, train_loader, eval_loader=None, *, num_epochs: int, rank: int = 0, start_epoch: int = 1,
                        checkpoint_dir: Optional[str] = None, save_every_epochs: int = 1, train_sampler=None, check_every: int = 50,
                        log=print) -> list:
    """The epoch loop of train_instruct.py:457-512: set_epoch -> train_epoch -> barrier -> eval_epoch -> barrier -> on rank 0 the
    stage-2 checkpoint files at epoch 1, the last epoch and every `save_every_epochs`."""
    import torch.distributed as dist
    from .loop import eval_epoch, train_epoch
    world = sharding.world_info(trainer.group)[1]
    history = []
    for epoch in range(start_epoch, num_epochs + 1):
        if train_sampler is not None and hasattr(train_sampler, "set_epoch"):
            train_sampler.set_epoch(epoch)
        trainer.zero_grad()
        rec = {"epoch": epoch}
        rec.update(train_epoch(trainer, train_loader, rank=rank, current_epoch=epoch, num_epochs=num_epochs, check_every=check_every, log=log))
        if world > 1:
            dist.barrier(group=trainer.group)
        if eval_loader is not None:
            rec.update(eval_epoch(trainer, eval_loader, rank=rank, current_epoch=epoch, num_epochs=num_epochs, check_every=check_every, log=log))
        if world > 1:
            dist.barrier(group=trainer.group)
        if checkpoint_dir is not None and rank == 0 and (epoch == 1 or epoch == num_epochs or epoch % save_every_epochs == 0):
            rec["checkpoint"] = save_instruct_checkpoint(trainer, checkpoint_dir, epoch)
        if world > 1:
            dist.barrier(group=trainer.group)
        history.append(rec)
    return history
