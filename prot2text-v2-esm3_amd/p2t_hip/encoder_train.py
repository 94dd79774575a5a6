"""Stage-2 step through the ESM2 encoder with LoRA adapters on its projections (the protein half of the stage-2 recipe):

    reference  scripts/train_instruct.py:155-183                   LoraConfig(target_modules = [...]) -- peft matches every module
                                                                   whose name equals a target or ends in "." + target
               models/modeling_esm2llama_instruct.py:174-193       the ESM2 encoder runs under autograd (no no_grad, no detach), so
                                                                   LoRA pairs on its modules are trained by loss.backward()

`p2t_esm2_forward` runs the FROZEN encoder as fused blocks and keeps no tape.  With a LoRA branch y = W x + b + s B (A drop(x)) on
`attention.self.{query,key,value}`, `attention.output.dense`, `intermediate.dense` or `output.dense`, this module drives the C ABI
layer by layer instead, as p2t_hip/decoder_train.py does for the decoder (HF EsmLayer, transformers/models/esm/modeling_esm.py):

    h  = LayerNorm(x)                   p2t_layernorm                 backward p2t_layernorm_backward
    q, k, v = W h + b (+ branch)        p2t_gemm_nt (+ low-rank)      dX GEMMs on W^T, dA / dB
    rotate-half rotary, q * d^-1/2      p2t_qkv_post                  p2t_rope_backward_pack
    attention (bidirectional, lse)      p2t_attention                 p2t_attention_backward (causal = 0)
    x += o(attn) + b (+ branch)         p2t_gemm_nt (RESID)
    h2 = LayerNorm(x)
    Z = fc1 h2 + b (+ branch), gelu(Z)  P2T_EPI_GELU (no branch) or   P2T_EPI_GELU_BWD on the fc2 dX GEMM, or p2t_gelu_rows
                                        p2t_gemm_nt + p2t_gelu_rows   (backward) when fc2 carries a branch
    x += fc2 gelu(Z) + b (+ branch)
    out = emb_layer_norm_after(x)

The tape keeps x at the layer's input and after the attention (fp32), q / k / v, the log-sum-exps, the attention output, Z and the
branches' u = drop(x) A^T; the backward stops at layer 0's input (the embeddings are frozen).  Dropout masks are the counter hash of
p2t_dropout_rows, regenerated in the backward.  torch allocates, slices and wires autograd; no torch op computes on the path.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._lib import call
from .decoder_train import TARGETS as DECODER_TARGETS
from .decoder_train import DecoderLora, _zero_tail
from .ops import ptr, round_up, stream

TARGETS = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "intermediate.dense", "output.dense")


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
        enc += [n for n in TARGETS if _matches(n, t) and n not in enc]
    bad = [t for t in target_modules if not any(_matches(n, t) for n in DECODER_TARGETS + TARGETS)]
    if bad:
        raise ValueError(f"unsupported LoRA targets {bad}; decoder targets are {DECODER_TARGETS}, ESM2 encoder targets are {TARGETS} "
                         "(a target selects every module whose name is it or ends in '.' + it)")
    return tuple(dec), tuple(enc)


class EncoderLora(DecoderLora):
    """The trainable A [r, in] / B [out, r] pairs of a LoraConfig on the ESM2 encoder's linears: the initialisation (A kaiming-uniform
    with a = sqrt 5, B = 0), fp32 masters, dropout seeding (`seed`, `rank`, `step_count`) and operand registry of DecoderLora."""

    def __init__(self, encoder, r: int, lora_alpha: Optional[float] = None, lora_dropout: float = 0.1, target_modules: Sequence[str] = TARGETS,
                 seed: int = 0):
        torch.nn.Module.__init__(self)
        if r < 1:
            raise ValueError("LoRA rank must be >= 1")
        bad = [t for t in target_modules if t not in TARGETS]
        if bad:
            raise ValueError(f"unsupported ESM2 LoRA targets {bad}; encoder targets are {TARGETS}")
        self.r, self.alpha, self.p, self.targets = int(r), float(2 * r if lora_alpha is None else lora_alpha), float(lora_dropout), tuple(target_modules)
        self.seed, self.step_count = int(seed), 0
        self.rank = 0
        self._operands, self._operand_key = {}, {}
        s = encoder.spec
        self.n_layers = s.num_hidden_layers
        P = dict(encoder.named_parameters())
        dev = P["embeddings.word_embeddings.weight"].device
        gen = torch.Generator(device="cpu").manual_seed(seed)
        for i in range(s.num_hidden_layers):
            for t in self.targets:
                w = P[f"encoder.layer.{i}.{t}.weight"]
                a = torch.empty((r, w.shape[1]), dtype=torch.float32)
                bound = 1.0 / math.sqrt(w.shape[1])
                a.uniform_(-bound, bound, generator=gen)
                self.register_parameter(self._name(i, t, "A"), torch.nn.Parameter(a.to(dev)))
                self.register_parameter(self._name(i, t, "B"), torch.nn.Parameter(torch.zeros((w.shape[0], r), dtype=torch.float32, device=dev)))

    def pairs(self):
        """[(layer, target, A, B)] in parameter order."""
        return [(i, t, *self.get(i, t)) for i in range(self.n_layers) for t in self.targets]

    def peft_state_dict(self, prefix: str = "base_model.model.esm_encoder.") -> Dict[str, torch.Tensor]:
        out = {}
        for i, t, a, b in self.pairs():
            out[f"{prefix}encoder.layer.{i}.{t}.lora_A.weight"] = a.detach().clone()
            out[f"{prefix}encoder.layer.{i}.{t}.lora_B.weight"] = b.detach().clone()
        return out


def _transposed(encoder, w: torch.Tensor, name: str) -> torch.Tensor:
    """[in, out padded to 64] copy of a frozen linear for the dX GEMMs, built once per weight version and kept on the encoder (as the
    decoder's are): a second copy of the six frozen linears of every layer, about 5 GB for ESM2-3B in bf16 -- tools/sft_bench.py
    `encoder` reports it.  Dropped when the encoder LoRA is merged (p2t_hip.lora.merge_lora_state_dict invalidates the engines)."""
    cache = encoder.__dict__.setdefault("_et_wT", {})
    key = (w.data_ptr(), w._version)
    hit = cache.get(name)
    if hit is None or hit[0] != key:
        cache[name] = (key, ops.transpose(w.detach(), round_up(w.shape[0], 64)))
    return cache[name][1]


class _Lin:
    """One linear of one ESM2 layer: frozen W [N, K] and bias (+ LoRA A, B): y = W x + b + s B A drop(x), and its backward."""

    def __init__(self, encoder, P, lora: Optional[EncoderLora], i: int, target: str, dt, dropout: float):
        self.name = f"encoder.layer.{i}.{target}"
        self.encoder, self.dt = encoder, dt
        self.w = P[self.name + ".weight"].detach()
        self.b = P[self.name + ".bias"].detach().float().contiguous()
        self.N, self.K = self.w.shape
        ab = lora.get(i, target) if lora is not None else None
        self.lora = None
        if ab is not None:
            a, b = ab
            s, r = lora.scale, a.shape[0]
            rp = round_up(r, 16)
            hit = lora.operands(i, target, dt)
            if hit is not None:
                self.a16, self.bs16 = hit
            else:
                a16 = torch.zeros((rp, round_up(self.K, 8)), dtype=dt, device=a.device)
                a16[:r, :self.K] = a.detach().to(dt)
                bs = torch.zeros((self.N, round_up(rp, 64)), dtype=dt, device=a.device)
                bs[:, :r] = (b.detach() * s).to(dt)
                self.a16, self.bs16 = a16, bs
            self.rp = rp
            seed = (lora.seed * 1000003 + lora.step_count * 7919 + i * 131 + 64 + TARGETS.index(target) + lora.rank * 0x9E3779B97F4A7C15)
            self.lora = (a, b, r, s, float(dropout), seed & 0x7FFFFFFFFFFFFFFF)

    def forward(self, x: torch.Tensor, resid: Optional[torch.Tensor] = None, keep_u: bool = True):
        """-> (y f32 [M, N] or None when accumulated into the fp32 residual stream `resid`, u)."""
        if resid is not None:
            ops.gemm_nt(x, self.w, self.b, n=self.N, k=self.K, epilogue=_lib.EPI_RESID, out=resid)
            y = None
        else:
            y = ops.gemm_nt(x, self.w, self.b, n=self.N, k=self.K, epilogue=_lib.EPI_STORE, out_dtype=torch.float32)
        u = None
        if self.lora is not None:
            xd = self.dropped(x)
            u = ops.gemm_nt(xd, self.a16, None, n=self.rp, k=self.K, epilogue=_lib.EPI_STORE, out_dtype=self.dt)
            if resid is not None:
                ops.gemm_nt(u, self.bs16, None, n=self.N, k=self.rp, epilogue=_lib.EPI_RESID, out=resid)
            else:
                ops.gemm_nt(u, self.bs16, None, n=self.N, k=self.rp, epilogue=_lib.EPI_STORE_F32, out=y, accumulate=True)
        return y, (u if keep_u else None)

    def dropped(self, x: torch.Tensor) -> torch.Tensor:
        _, _, _, _, p, seed = self.lora
        if p <= 0.0:
            return x
        xd = torch.empty((x.shape[0], round_up(self.K, 64)), dtype=self.dt, device=x.device)
        if xd.shape[1] != self.K:
            xd.zero_()
        call("p2t_dropout_rows", ptr(x), ops.dt_of(x), x.stride(0), ptr(xd), ops.dt_of(xd), xd.stride(0), x.shape[0], self.K, float(p), int(seed), 0, stream())
        return xd

    def backward_branch(self, dy: torch.Tensor, x: torch.Tensor, u: torch.Tensor, dx: torch.Tensor, grads: dict):
        """The branch's share: dA, dB into `grads`, drop'(du A) added to dx (f32 or `dt`)."""
        a, b, r, s, p, seed = self.lora
        rp, M = self.rp, dy.shape[0]
        xd = self.dropped(x)
        bsT = ops.transpose(self.bs16[:, :rp].contiguous(), round_up(self.N, 64))                   # [rp, N]
        du = ops.gemm_nt(dy, bsT, None, n=rp, k=self.N, epilogue=_lib.EPI_STORE, out_dtype=self.dt) # [M, 64] = dy (s B)
        dyT, uT = ops.transpose(dy[:, :self.N]), ops.transpose(u[:, :rp])
        _zero_tail(dyT, M), _zero_tail(uT, M)
        dB = torch.zeros((self.N, rp), dtype=torch.float32, device=dy.device)
        ops.gemm_nt(dyT, uT, None, n=rp, k=round_up(M, 64), epilogue=_lib.EPI_STORE_F32, out=dB)    # [N, rp] = dy^T u
        duT, xdT = ops.transpose(du[:, :rp]), ops.transpose(xd[:, :self.K])
        _zero_tail(duT, M), _zero_tail(xdT, M)
        dA = ops.gemm_nt(duT, xdT, None, n=self.K, k=round_up(M, 64), epilogue=_lib.EPI_STORE_F32)  # [rp, K] = du^T drop(x)
        grads[id(a)] = (dA, r, self.K, 1.0)
        grads[id(b)] = (dB, self.N, r, s)
        aT = ops.transpose(self.a16[:, :self.K], round_up(rp, 8))
        t = ops.gemm_nt(du, aT, None, n=self.K, k=rp, epilogue=_lib.EPI_STORE_F32)                  # [M, K] f32
        call("p2t_dropout_rows", ptr(t), _lib.F32, t.stride(0), ptr(dx), ops.dt_of(dx), dx.stride(0), M, self.K, float(p), int(seed), 1, stream())

    def backward(self, dy: torch.Tensor, x: torch.Tensor, u: Optional[torch.Tensor], out: Optional[torch.Tensor], out_f32: bool, accumulate: bool,
                 grads: dict) -> torch.Tensor:
        """dX (+)= dy W (+ the branch's share); x: the linear's input as the forward saw it (before the dropout)."""
        wT = _transposed(self.encoder, self.w, self.name)
        if out_f32:
            dx = ops.gemm_nt(dy, wT, None, n=self.K, k=self.N, epilogue=_lib.EPI_STORE_F32, out=out, accumulate=accumulate)
        else:
            assert not accumulate
            dx = ops.gemm_nt(dy, wT, None, n=self.K, k=self.N, epilogue=_lib.EPI_STORE, out=out, out_dtype=self.dt)
        if self.lora is not None:
            self.backward_branch(dy, x, u, dx, grads)
        return dx


def _gelu_rows(z: torch.Tensor, dy: Optional[torch.Tensor], n: int, out_dtype) -> torch.Tensor:
    M = z.shape[0]
    out = torch.empty((M, round_up(n, 64)), dtype=out_dtype, device=z.device)
    call("p2t_gelu_rows", ptr(z), ops.dt_of(z), z.stride(0), ptr(dy), ops.dt_of(dy) if dy is not None else 0, dy.stride(0) if dy is not None else 0,
         ptr(out), ops.dt_of(out), out.stride(0), M, n, stream())
    return out


class EncoderLoraFn(torch.autograd.Function):
    """last_hidden_state of the ESM2 encoder ([B, T, Hp] in the model dtype, zero padded as `EsmEncoder.encode` returns it) as a
    function of the LoRA parameters (frozen base weights and embeddings)."""

    @staticmethod
    def forward(ctx, input_ids, attention_mask, encoder, lora, opts, *params):
        s, dt = encoder.spec, encoder.dtype
        B, T = input_ids.shape
        M, H, F = B * T, s.hidden_size, s.intermediate_size
        nh, d, L = s.num_attention_heads, s.head_dim, s.num_hidden_layers
        Hp = round_up(H, 64)
        if H % 8 or F % 8:
            raise ValueError("the encoder LoRA step needs hidden_size and intermediate_size multiples of 8")
        P = dict(encoder.named_parameters())
        dev = P["embeddings.word_embeddings.weight"].device
        f32v = lambda n: P[n].detach().float().contiguous()
        ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
        mask = attention_mask.to(device=dev, dtype=torch.int64).contiguous()
        key_mask, kv_info, emb_scale = ops.mask_prepare(mask, ids, s.mask_token_id, s.token_dropout)
        x = torch.empty((M, H), dtype=torch.float32, device=dev)
        call("p2t_esm2_embed", ptr(ids), ptr(mask), ptr(P["embeddings.word_embeddings.weight"]), ops.dt_of(dt), ptr(emb_scale), B, T, H, s.vocab_size,
             s.mask_token_id, int(s.token_dropout), ptr(x), stream())
        inv_freq = encoder.rotary_embeddings.inv_freq.detach().float().contiguous()
        l2s = dt == torch.bfloat16                      # as p2t_esm2_forward: q carries d^-1/2 * log2 e, the logits are ln 2 * q.k
        q_fold = (1.4426950408889634 if l2s else 1.0) / math.sqrt(d)
        eps = s.layer_norm_eps
        keep = opts["keep_tape"]
        tape = []
        for i in range(L):
            p = f"encoder.layer.{i}."
            lin = {t: _Lin(encoder, P, lora, i, t, dt, opts["dropout"]) for t in TARGETS}
            rec = dict(lin=lin, x_in=x.clone() if keep else None)
            h = ops.layernorm(x, f32v(p + "attention.LayerNorm.weight"), f32v(p + "attention.LayerNorm.bias"), eps, out_dtype=dt)
            parts = []
            for t in TARGETS[:3]:
                y, rec["u_" + t] = lin[t].forward(h, keep_u=keep)
                parts.append(y)
            qkv = torch.cat([y[:, :H] for y in parts], 1)
            qkv = ops.cast(qkv, dt) if dt != torch.float32 else qkv
            q4, k4, v4 = ops.qkv_post(qkv, inv_freq, B, T, nh, nh, d, q_fold)
            lse = torch.empty((B, nh, T), dtype=torch.float32, device=dev) if keep else None
            ao = ops.attention(q4, k4, v4, key_mask, kv_info, d, 1.0, False, log2_scores=l2s, lse=lse)
            if keep:
                rec.update(q=q4, k=k4, v=v4, lse=lse, ao=ao)
            _, rec["u_attention.output.dense"] = lin["attention.output.dense"].forward(ao, resid=x, keep_u=keep)
            rec["x_mid"] = x.clone() if keep else None
            h2 = ops.layernorm(x, f32v(p + "LayerNorm.weight"), f32v(p + "LayerNorm.bias"), eps, out_dtype=dt)
            fc1 = lin["intermediate.dense"]
            if fc1.lora is None:                        # the fused bias + GELU epilogue, keeping Z
                z = torch.empty((M, round_up(F, 64)), dtype=dt, device=dev)
                act = ops.gemm_nt(h2, fc1.w, fc1.b, n=F, k=H, epilogue=_lib.EPI_GELU, out_dtype=dt, z=z)
            else:                                       # the branch lands BEFORE the GELU: Z assembled in fp32, then p2t_gelu_rows
                zf, rec["u_intermediate.dense"] = fc1.forward(h2, keep_u=keep)
                act = _gelu_rows(zf, None, F, dt)
                z = ops.cast(zf, dt) if dt != torch.float32 else zf
            rec["z"] = z if keep else None
            _, rec["u_output.dense"] = lin["output.dense"].forward(act, resid=x, keep_u=keep)
            if keep:
                tape.append(rec)
        out = ops.layernorm(x, f32v("encoder.emb_layer_norm_after.weight"), f32v("encoder.emb_layer_norm_after.bias"), eps, out_dtype=dt, ld_out=Hp)
        ctx.state = dict(encoder=encoder, tape=tape, x_last=x, key_mask=key_mask, kv_info=kv_info, inv_freq=inv_freq, l2s=l2s, q_fold=q_fold,
                         shape=(B, T), params=params) if keep else None
        return out.view(B, T, Hp)

    @staticmethod
    def backward(ctx, d_out):
        st = ctx.state
        enc = st["encoder"]
        s, dt = enc.spec, enc.dtype
        B, T = st["shape"]
        M, H, F = B * T, s.hidden_size, s.intermediate_size
        nh, d = s.num_attention_heads, s.head_dim
        dp = ops.head_dim_padded(d)
        eps = s.layer_norm_eps
        P = dict(enc.named_parameters())
        dev = st["x_last"].device
        f32v = lambda n: P[n].detach().float().contiguous()
        to_dt = lambda t: ops.cast(t, dt) if t.dtype != dt else t
        c_s = 0.6931471805599453 if st["l2s"] else 1.0

        def ln_bwd(x, name, dy, out, acc):
            call("p2t_layernorm_backward", ptr(x), x.stride(0), ptr(f32v(name)), float(eps), ptr(dy), dy.stride(0), ops.dt_of(dy), ptr(out), out.stride(0),
                 M, H, int(acc), stream())

        dy = d_out.reshape(M, -1)
        if dy.dtype not in (torch.float32, torch.bfloat16) or dy.stride(1) != 1 or dy.stride(0) % 4:
            dy = dy.float().contiguous()
        g = torch.empty((M, H), dtype=torch.float32, device=dev)
        ln_bwd(st["x_last"], "encoder.emb_layer_norm_after.weight", dy, g, 0)
        grads: dict = {}
        for i in range(len(st["tape"]) - 1, -1, -1):
            rec = st["tape"][i]
            lin = rec["lin"]
            p = f"encoder.layer.{i}."
            # ---- FFN: x2 = x1 + fc2(gelu(Z)) + b
            g16 = to_dt(g)
            z, fc2 = rec["z"], lin["output.dense"]
            if fc2.lora is None:                        # dZ = (dy W2) * gelu'(Z) in the dX GEMM's epilogue
                dz = ops.gemm_nt(g16, _transposed(enc, fc2.w, fc2.name), None, n=F, k=H, epilogue=_lib.EPI_GELU_BWD, out_dtype=dt, z=z)
            else:                                       # gelu(Z) recomputed: the branch's dA needs fc2's input
                d_act = fc2.backward(g16, _gelu_rows(z, None, F, dt), rec["u_output.dense"], None, True, False, grads)
                dz = _gelu_rows(z, d_act, F, dt)
            h2 = ops.layernorm(rec["x_mid"], f32v(p + "LayerNorm.weight"), f32v(p + "LayerNorm.bias"), eps, out_dtype=dt)
            d_h2 = lin["intermediate.dense"].backward(dz, h2, rec["u_intermediate.dense"] if "u_intermediate.dense" in rec else None, None, True, False, grads)
            ln_bwd(rec["x_mid"], p + "LayerNorm.weight", d_h2, g, 1)
            # ---- attention: x1 = x + o(attn(rope(q), rope(k), v)) + b
            g16 = to_dt(g)
            d_ao = lin["attention.output.dense"].backward(g16, rec["ao"], rec["u_attention.output.dense"], None, False, False, grads)
            dq, dk, dv = ops.attention_backward(rec["q"], rec["k"], rec["v"], rec["ao"], d_ao, rec["lse"], st["key_mask"], st["kv_info"], d, c_s, False,
                                                log2_scores=st["l2s"])
            d_qkv = torch.zeros((M, round_up(3 * H, 64)), dtype=dt, device=dev)
            cs = torch.empty((T, d), dtype=torch.float32, device=dev)
            call("p2t_rope_backward_pack", ptr(dq), ptr(dk), ptr(dv), ptr(st["inv_freq"]), ptr(cs), ptr(d_qkv), d_qkv.stride(0), B, T, nh, nh, d, dp,
                 float(st["q_fold"]), ops.dt_of(dt), stream())
            h1 = ops.layernorm(rec["x_in"], f32v(p + "attention.LayerNorm.weight"), f32v(p + "attention.LayerNorm.bias"), eps, out_dtype=dt)
            d_h1 = None
            for j, t in enumerate(TARGETS[:3]):
                d_h1 = lin[t].backward(d_qkv[:, j * H:(j + 1) * H], h1, rec["u_" + t], d_h1, True, j > 0, grads)
            ln_bwd(rec["x_in"], p + "attention.LayerNorm.weight", d_h1, g, 1)
            st["tape"][i] = None
        out_params = []
        for prm in st["params"]:
            gp = grads.get(id(prm))
            if gp is None:
                out_params.append(None)
                continue
            buf, rows, cols, factor = gp                # dB carries alpha / r
            if factor != 1.0:
                call("p2t_scale_by_device_scalar", ptr(buf), buf.numel(), ptr(torch.full((1,), factor, dtype=torch.float32, device=dev)), stream())
            out_params.append(buf[:rows, :cols].to(prm.dtype))
        ctx.state = None
        return (None, None, None, None, None, *out_params)


def encoder_lora_forward(encoder, lora: EncoderLora, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor],
                         dropout: Optional[float] = None) -> torch.Tensor:
    """last_hidden_state [B, T, Hp] of the encoder with the LoRA branches in the graph (what `EsmEncoder.encode` returns otherwise).
    dropout: None = `lora.p` in train mode (one mask step per call), 0 in eval mode (peft's nn.Dropout, no mask step -- what
    InstructTrainer.evaluate sets); a value overrides both and leaves the mask counter where it is.  Without gradients to compute, no activation tape is kept."""
    if input_ids is None or input_ids.dim() != 2:
        raise ValueError("protein_input_ids must be a [batch, seq_len] tensor of token ids")
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    if tuple(attention_mask.shape) != tuple(input_ids.shape):
        raise ValueError(f"protein_attention_mask shape {tuple(attention_mask.shape)} != input ids {tuple(input_ids.shape)}")
    if encoder.gemm_fp8:
        raise ValueError("stage-2 training runs the encoder GEMMs in the model dtype (set_gemm_dtype('model'))")
    params = tuple(lora.parameters())
    if dropout is None:
        if lora.training:
            lora.step_count += 1                        # a fresh dropout mask per step
        dropout = lora.p if lora.training else 0.0
    keep = torch.is_grad_enabled() and any(q.requires_grad for q in params)
    opts = dict(dropout=float(dropout), keep_tape=keep)
    return EncoderLoraFn.apply(input_ids, attention_mask, encoder, lora, opts, *params)
