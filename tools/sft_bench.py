"""Stage-2 (SFT) step of Esm2LlamaInstructForCausalLM at cfg3 sizes: ESM2-3B encode -> adapter -> placeholder
scatter -> 32-layer Llama-3.1-8B -> LM head -> shifted CE, once forward only and once as the training step `loss.backward()`
(frozen towers, adapter trainable: training forward with the activation tape + the dX chain of csrc/llama_train.hip (cross-entropy: csrc/lm_loss.hip; norm / SwiGLU backwards: csrc/norm.hip, csrc/activations.hip) + adapter
backward), with a per-kernel-family breakdown of the backward from the torch profiler-free HIP-event brackets below.
python tools/sft_bench.py [B] [lora] [trainer] [encoder] [packed] [checkpoint] [fused] [targets=F] > sft_bench.log
`fused`: every training leg once more with `model.fused_lm_loss()` (p2t_hip/lm_head.py: the LM loss over the target rows only), the
modes alternating with the unfused ones in the same process: ms per step, peak memory and the number of target rows.
`targets=F`: the fraction of the T decoder positions of every sample whose label is supervised (the tail of the row; default
128 / T ~ 0.105, the description of the synthetic sample; 1.0 supervises every position).
`checkpoint` (with `lora` / `encoder`): the same step again under gradient_checkpointing_enable() (per-layer recompute, dA / dB by
p2t_lora_wgrad), the two modes alternating in one process: ms per step, `last_tape_bytes` and peak memory of each.
`encoder`: InstructTrainer with LoRA r = 16 on the decoder's seven projections AND ESM2's six linears of every layer
(p2t_hip/encoder_train.py: the encoder runs layer by layer with a tape and a HIP backward): ms per step and peak memory.
`trainer`: the stage-2 InstructTrainer (LoRA r = 16 + adapter, GA 1): ms per full step, the flat clip + AdamW tail alone (bytes,
fraction of HBM bandwidth) and the host time per step that the optimizer-written LoRA operands save.
`packed`: InstructTrainer (r = 16) on ragged samples (tools/ragged_sweep.py's protein length draws) as padded micro-batches of 1 (the
reference's default) and 4, and packed into rows of <= 4 x 1216 tokens (p2t_hip.data.pack_instruct_batch): samples/s and real
(unpadded) decoder tokens/s; then the attention forward / backward of one packed row against one full causal row of the same T."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prot2text-v2-esm3_amd"))
import p2t_hip as P                                             # noqa: E402
from p2t_hip import specs, synth                                # noqa: E402


def main():
    dev = torch.device("cuda:0")
    if sys.argv[1:2] == ["packed"]:
        return packed_leg(dev)
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    esm_name, llama_name, _, _, Tp, _ = specs.CONFIGS["cfg3"]
    esm, llama = specs.esm_spec(esm_name), specs.llama_spec(llama_name)
    ad = specs.adapter_spec(esm, llama)
    model = P.Esm2LlamaInstructForCausalLM.from_specs(esm, llama, ad, dtype=torch.bfloat16, device=dev, seed=0)
    model.eval()
    n_prompt, n_desc = 64, 128
    T = Tp + n_prompt + n_desc                                      # placeholders (one per residue token) + prompt + description
    ph = model.config.placeholder_id
    rs = np.random.RandomState(0)
    ids = rs.randint(0, 128000, size=(B, T)).astype(np.int64)
    ids[:, 16:16 + Tp] = ph                                         # chat template: system text, <protein placeholders>, question, answer
    labels = ids.copy()
    frac = next((float(a.split("=", 1)[1]) for a in sys.argv if a.startswith("targets=")), None)
    n_sup = n_desc if frac is None else max(1, min(T, int(round(frac * T))))
    labels[:, :T - n_sup] = -100
    labels[labels == ph] = 0                                       # (a supervised placeholder position: any real token id)
    n_targets = int((labels[:, 1:] != -100).sum())
    fused_modes = (False, True) if "fused" in sys.argv else (False,)
    pid, pmask = synth.protein_batch(5, B, Tp)
    t = lambda a: torch.from_numpy(a).to(dev)
    kw = dict(input_ids=t(ids), attention_mask=torch.ones((B, T), dtype=torch.int64, device=dev), labels=t(labels),
              protein_input_ids=t(pid), protein_attention_mask=t(pmask))
    with torch.no_grad():
        out = model(**kw)
        torch.cuda.synchronize()
        n = 3
        t0 = time.perf_counter()
        for _ in range(n):
            out = model(**kw)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
    He, Fe, Le = esm.hidden_size, esm.intermediate_size, esm.num_hidden_layers
    Hl, Fl, Ll = llama.hidden_size, llama.intermediate_size, llama.num_hidden_layers
    kv = llama.num_key_value_heads * llama.head_dim
    f_esm = Le * Tp * (2 * (4 * He * He + 2 * He * Fe) + 4 * Tp * He)
    f_ad = 2 * Tp * (He * ad.intermediate_dim + ad.intermediate_dim * Hl)
    f_llama = Ll * T * (2 * (2 * Hl * Hl + 2 * Hl * kv + 3 * Hl * Fl) + 2 * (T + 1) * Hl) + 2 * T * Hl * llama.vocab_size
    f = f_esm + f_ad + f_llama
    # ---- training step: frozen towers, adapter trainable
    model.requires_grad_(False)
    model.adapter.requires_grad_(True)

    def step():
        model.zero_grad(set_to_none=True)
        o = model(**kw)
        o.loss.backward()
        return o
    for rnd in range(2 if len(fused_modes) > 1 else 0):            # frozen step, unfused / fused alternating
        for fz in fused_modes:
            model.fused_lm_loss(fz)
            step()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(2):
                of = step()
            torch.cuda.synchronize()
            print(f"sft frozen train step cfg3 (fused LM loss {'on' if fz else 'off'}, round {rnd}): B={B}, {n_targets} target rows of {B * T}: "
                  f"{(time.perf_counter() - t0) / 2 * 1e3:.1f} ms/batch; loss {float(of.loss):.4f}; |grad fc2.weight| "
                  f"{float(model.adapter.fc2.weight.grad.float().norm()):.3e}; peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
            del of
    model.fused_lm_loss(False)
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(2):
        o2 = step()
    torch.cuda.synchronize()
    dt_train = (time.perf_counter() - t0) / 2
    gn = float(model.adapter.fc2.weight.grad.float().norm())
    # the dX chain costs the decoder's linear FLOPs once more (no weight gradients) + attention backward (2.5 x its forward)
    f_bwd = Ll * T * (2 * (2 * Hl * Hl + 2 * Hl * kv + 3 * Hl * Fl) + 2.5 * 2 * (T + 1) * Hl) + 2 * T * Hl * llama.vocab_size + 2 * f_ad
    print(f"sft train step cfg3: B={B}: {dt_train * 1e3:.1f} ms/batch = {B / dt_train:.2f} samples/s, {(f + f_bwd) * B / dt_train / 1e12:.0f} TFLOP/s algorithmic "
          f"(forward {f / 1e12:.2f} + backward {f_bwd / 1e12:.2f} TF/sample); backward alone ~{(dt_train - dt) * 1e3:.1f} ms; loss {float(o2.loss):.4f}, "
          f"|grad fc2.weight| {gn:.3e}", flush=True)
    print(f"sft forward cfg3: B={B}, {Tp} residues, {T} decoder tokens ({n_sup} supervised): {dt * 1e3:.1f} ms/batch = {B / dt:.2f} samples/s, "
          f"{B * T / dt:.0f} decoder tokens/s, {f * B / dt / 1e12:.0f} TFLOP/s algorithmic ({f / 1e12:.2f} TF/sample: ESM {f_esm / 1e12:.2f}, "
          f"decoder + LM head {f_llama / 1e12:.2f}); loss {float(out.loss):.4f}", flush=True)
    if "lora" in sys.argv:
        # the reference's stage-2 recipe: LoRA (r = 16, alpha = 32, dropout 0.1) on the seven decoder projections + the adapter trainable
        # (scripts/train_instruct.py:146-183); per-layer path of p2t_hip/decoder_train.py (correctness first, not tuned)
        del o2, out
        torch.cuda.empty_cache()
        lora = model.add_lora(r=16, lora_alpha=32, lora_dropout=0.1)
        model.train()

        def lstep():
            model.zero_grad(set_to_none=True)
            lora.zero_grad(set_to_none=True)
            o = model(**kw)
            o.loss.backward()
            return o
        ga_n, n_l = None, sum(q.numel() for q in lora.parameters())
        for rnd in range(2 if ("checkpoint" in sys.argv or "fused" in sys.argv) else 1):      # the modes alternate
            for on, fz in [(on, fz) for on in ((False, True) if "checkpoint" in sys.argv else (False,)) for fz in fused_modes]:
                model.gradient_checkpointing_enable() if on else model.gradient_checkpointing_disable()
                model.fused_lm_loss(fz)
                o3 = lstep()
                del o3
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                for _ in range(2):
                    o3 = lstep()
                torch.cuda.synchronize()
                dt_l = (time.perf_counter() - t0) / 2
                ga = [q.grad for q in lora.parameters() if q.grad is not None]
                print(f"sft LoRA train step cfg3 (checkpointing {'on' if on else 'off'}, fused LM loss {'on' if fz else 'off'}, {n_targets} target rows "
                      f"of {B * T}, round {rnd}): B={B}, r=16 on {len(ga)} of "
                      f"{len(list(lora.parameters()))} matrices with a gradient ({n_l / 1e6:.1f} M LoRA parameters): "
                      f"{dt_l * 1e3:.1f} ms/batch = {B / dt_l:.2f} samples/s; loss {float(o3.loss):.4f}; |grad| of the first B matrix "
                      f"{float([q.grad for n, q in lora.named_parameters() if n.endswith('B')][0].float().norm()):.3e}; "
                      f"tape {model.llama_decoder.last_tape_bytes / 2**30:.2f} GiB; peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB",
                      flush=True)
                del o3
        model.gradient_checkpointing_disable()
        model.fused_lm_loss(False)
    if "trainer" in sys.argv:
        trainer_leg(model, kw, B)
    if "encoder" in sys.argv:
        encoder_leg(model, kw, B)


def encoder_leg(model, kw, B):
    """InstructTrainer at cfg3 sizes with LoRA r = 16 on both towers: 7 x 32 decoder projections + 6 x 36 ESM2 linears, + the adapter."""
    from p2t_hip.decoder_train import TARGETS
    from p2t_hip.encoder_train import TARGETS as ENC
    torch.cuda.empty_cache()
    model.add_lora(r=16, lora_alpha=32, lora_dropout=0.1, target_modules=list(TARGETS) + list(ENC))
    model.train()
    tr = P.InstructTrainer(model)
    n_p = sum(tr.opt.numels)
    modes = (False, True, False, True) if "checkpoint" in sys.argv else (False,)
    for on in modes:                                                # the modes alternate in one process
        model.gradient_checkpointing_enable() if on else model.gradient_checkpointing_disable()
        tr.step(kw)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        n = 3
        t0 = time.perf_counter()
        for _ in range(n):
            loss = tr.step(kw)
        torch.cuda.synchronize()
        dt_step = (time.perf_counter() - t0) / n
        enc_cache = sum(t.numel() * t.element_size() for _, t in model.esm_encoder.__dict__.get("_lora_wT", {}).values())
        print(f"sft InstructTrainer step cfg3 with encoder LoRA (checkpointing {'on' if on else 'off'}): B={B}, r=16 on {len(tr.params) - 4} LoRA "
              f"matrices of both towers + adapter ({n_p / 1e6:.1f} M parameters), GA 1: {dt_step * 1e3:.1f} ms/step = {B / dt_step:.2f} samples/s; "
              f"loss {float(loss):.4f}; tape decoder {model.llama_decoder.last_tape_bytes / 2**30:.2f} + encoder "
              f"{model.esm_encoder.last_tape_bytes / 2**30:.2f} GiB; peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB (resident before "
              f"the step {base / 2**30:.1f} GiB, of which {enc_cache / 2**30:.1f} GiB are the encoder's transposed frozen weights for its dX GEMMs)",
              flush=True)
    model.gradient_checkpointing_disable()


def trainer_leg(model, kw, B):
    """InstructTrainer at cfg3 sizes: LoRA r = 16 (alpha 32, dropout 0.1) on the 7 x 32 projections + the adapter, GA 1."""
    from p2t_hip.decoder_train import TARGETS
    from p2t_hip.lora_linear import LoraLinear
    torch.cuda.empty_cache()
    lora = getattr(model.llama_decoder, "lora", None) or model.add_lora(r=16, lora_alpha=32, lora_dropout=0.1)
    model.train()
    tr = P.InstructTrainer(model)
    n_p = sum(tr.opt.numels)
    tr.step(kw)
    torch.cuda.synchronize()
    n = 3
    t0 = time.perf_counter()
    for _ in range(n):
        loss = tr.step(kw)
    torch.cuda.synchronize()
    dt_step = (time.perf_counter() - t0) / n
    # the optimizer tail alone: norm + update over the flat buffers (gradients of the last step are zero by now: refill)
    tr.opt.flat_g.normal_(0.0, 1e-3)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 20
    tr.opt.step(tr.step_count + 1, lr=2e-4)
    ev0.record()
    for k in range(reps):
        tr.opt.step(tr.step_count + 2 + k, lr=2e-4)
    ev1.record()
    torch.cuda.synchronize()
    dt_opt = ev0.elapsed_time(ev1) / reps * 1e-3
    nbytes = tr.opt.bytes_per_step()
    # host cost of the LoRA operands per step: every LoraLinear of the forward built from the masters vs taken from the trainer
    dec, dt = model.llama_decoder, model.llama_decoder.model.dtype
    L = dec.spec.num_hidden_layers

    def build_all():
        torch.cuda.synchronize()
        t = time.perf_counter()
        P = dict(dec.model.named_parameters())             # once per pass, as the step builds it
        for i in range(L):
            for tg in TARGETS:
                LoraLinear(dec.model, P, f"layers.{i}.{tg}", lora, i, tg, dt, lora.p)
        torch.cuda.synchronize()
        return time.perf_counter() - t
    build_all()
    t_reg = min(build_all() for _ in range(3))
    saved = lora._operands, lora._operand_key
    lora._operands, lora._operand_key = {}, {}
    t_fresh = min(build_all() for _ in range(3))
    lora._operands, lora._operand_key = saved
    print(f"sft InstructTrainer step cfg3: B={B}, r=16 LoRA + adapter ({len(tr.params)} tensors, {n_p / 1e6:.1f} M parameters, "
          f"{tr.opt.n_chunks} chunks), GA 1: {dt_step * 1e3:.1f} ms/step = {B / dt_step:.2f} samples/s; loss {float(loss):.4f}; "
          f"peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)
    print(f"flat clip + AdamW (p2t_clip_adamw_flat, 2 launches): {dt_opt * 1e3:.3f} ms, {nbytes / 1e9:.3f} GB moved = "
          f"{nbytes / dt_opt / 1e12:.2f} TB/s = {nbytes / dt_opt / 8.0e12:.2f} of the 8.0 TB/s HBM peak "
          f"({nbytes / dt_opt / 6.29e12:.2f} of the 6.29 TB/s float4 copy rate)", flush=True)
    print(f"LoRA operands per step ({L * len(TARGETS)} projections): rebuilt from the masters {t_fresh * 1e3:.1f} ms, "
          f"registered by the trainer {t_reg * 1e3:.1f} ms: {(t_fresh - t_reg) * 1e3:.1f} ms saved per step", flush=True)


def packed_leg(dev, N=48, max_tokens=4 * 1216):
    esm_name, llama_name, _, _, Tp, _ = specs.CONFIGS["cfg3"]
    esm, llama = specs.esm_spec(esm_name), specs.llama_spec(llama_name)
    ad = specs.adapter_spec(esm, llama)
    model = P.Esm2LlamaInstructForCausalLM.from_specs(esm, llama, ad, dtype=torch.bfloat16, device=dev, seed=0)
    ph = model.config.placeholder_id
    rs = np.random.RandomState(0)
    plen = np.clip(np.round(rs.lognormal(5.75, 0.6, N)), 16, Tp).astype(int)           # ragged_sweep.py's draws
    dlen = np.clip(np.round(rs.lognormal(4.0, 0.5, N)), 4, 256).astype(int)
    pid, pm = synth.protein_batch(77, N, Tp, plen.tolist())
    samples = []
    for i in range(N):                  # [bos, placeholders, 16 prompt tokens, description, eot]; the description is supervised
        ids = np.concatenate([[1], np.full(plen[i], ph), rs.randint(2, 128000, 16), rs.randint(2, 128000, dlen[i]), [2]]).astype(np.int64)
        lab = np.full_like(ids, -100)
        lab[-dlen[i] - 1:] = ids[-dlen[i] - 1:]
        samples.append((ids, lab))
    real = int(sum(len(x) for x, _ in samples))

    def padded(idx):                    # right-padded micro-batch of samples idx, protein rows trimmed to their longest
        T = max(len(samples[i][0]) for i in idx)
        ids = np.zeros((len(idx), T), np.int64); mask = np.zeros_like(ids); lab = np.full_like(ids, -100)
        for r, i in enumerate(idx):
            n = len(samples[i][0])
            ids[r, :n], mask[r, :n], lab[r, :n] = samples[i][0], 1, samples[i][1]
        tp = int(plen[idx].max())
        return dict(input_ids=ids, attention_mask=mask, labels=lab, protein_input_ids=pid[idx, :tp], protein_attention_mask=pm[idx, :tp])

    t = lambda b: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v.to(dev) for k, v in b.items()
                   if k != "pack_layout"}
    setups = {"padded B=1": [t(padded(np.array([i]))) for i in range(N)],
              "padded B=4": [t(padded(np.arange(i, min(i + 4, N)))) for i in range(0, N, 4)]}
    host = {k: torch.from_numpy(v) for k, v in padded(np.arange(N)).items()}
    pk = P.pack_instruct_batch(host, max_tokens)
    rows = []
    for r in range(pk["input_ids"].shape[0]):
        members = [i for i, rr, _, _ in pk["pack_layout"] if rr == r]
        n = int(pk["attention_mask"][r].sum())
        tp = int(plen[members].max())
        rows.append(t(dict(input_ids=pk["input_ids"][r:r + 1, :n], attention_mask=pk["attention_mask"][r:r + 1, :n], labels=pk["labels"][r:r + 1, :n],
                           position_ids=pk["position_ids"][r:r + 1, :n], protein_input_ids=torch.from_numpy(pid[members, :tp]),
                           protein_attention_mask=torch.from_numpy(pm[members, :tp]))))
    setups[f"packed rows <= {max_tokens}"] = rows
    lora = model.add_lora(r=16, lora_alpha=32, lora_dropout=0.1)
    model.train()
    tr = P.InstructTrainer(model)
    print(f"packed leg cfg3: {N} samples, protein length mean {plen.mean():.0f} (max {plen.max()}), {real} real decoder tokens "
          f"(mean {real / N:.0f} per sample); InstructTrainer r=16, GA 1", flush=True)
    res = {}
    for name, mbs in setups.items():
        tr.step(mbs[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in mbs:
            tr.step(b)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        slots = sum(int(b["input_ids"].numel()) for b in mbs)
        res[name] = N / dt
        print(f"  {name:>22}: {len(mbs)} micro-batches, {slots} decoder slots ({real / slots:.2f} real): {dt * 1e3:.0f} ms = {N / dt:.2f} samples/s, "
              f"{real / dt:.0f} real decoder tokens/s", flush=True)
    names = list(res)
    print(f"  packed / padded B=4 = {res[names[2]] / res[names[1]]:.2f}x, packed / padded B=1 = {res[names[2]] / res[names[0]]:.2f}x", flush=True)
    # attention of the longest packed row against one full causal row of the same T (cfg3 heads), HIP events
    from p2t_hip import ops
    b = max(rows, key=lambda x: x["input_ids"].shape[1])
    T = b["input_ids"].shape[1]
    nh, nkv, d = llama.num_attention_heads, llama.num_key_value_heads, llama.head_dim
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = [(torch.randn((1, h, T, d), generator=g) * 0.3).to(dev, torch.bfloat16) for h in (nh, nkv, nkv)]
    mask = torch.ones((1, T), dtype=torch.int64, device=dev)
    key_mask, kv_info, _ = ops.mask_prepare(mask)
    docs = ops.doc_prepare(b["position_ids"], mask)
    d_o = (torch.randn((T, ops.round_up(nh * d, 64)), generator=g) * 0.3).to(dev, torch.bfloat16)
    lse = torch.empty((1, nh, T), dtype=torch.float32, device=dev)

    def timed(fn, reps=10):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    for name, dc in (("full causal row", None), ("packed row", docs)):
        fwd = lambda: ops.attention(q, k, v, key_mask, kv_info, d, 1.0, True, use_mfma=2, log2_scores=True, lse=lse, docs=dc)
        out = fwd()
        bwd = lambda: ops.attention_backward(q, k, v, out, d_o, lse, key_mask, kv_info, d, 0.6931471805599453, True, log2_scores=True, use_mfma=1, docs=dc)
        print(f"  attention {name}, T={T}, {nh}/{nkv} heads x {d}: forward {timed(fwd):.3f} ms, backward {timed(bwd):.3f} ms", flush=True)
    lens = [int(x) for x in torch.unique_consecutive(torch.cumsum((b["position_ids"][0] == 0).long(), 0), return_counts=True)[1]]
    print(f"  packed row documents: {lens}; sum len^2 / T^2 = {sum(x * x for x in lens) / T / T:.3f}", flush=True)


if __name__ == "__main__":
    main()
