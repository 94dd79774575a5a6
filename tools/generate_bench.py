"""`generate` at cfg3 sizes (reference scripts/generate_instruct.py: ESM2-3B -> adapter -> placeholder scatter -> Llama-3.1-8B, greedy
decoding): B prompts of 1024 residues + 64 prompt tokens, N new tokens.  Prints the prefill time, the time per decode step and the
HBM roofline of the step: every decoder weight is read once per step (bf16: 2 bytes x (32 layers x (qkv + o + gate/up + down) + LM
head)) plus the keys / values of the cache -- the algorithmic bytes of a step; frac = (bytes / step time) / 8 TB/s.
python tools/generate_bench.py [B] [N] [beams] [fp8] > gpurun_out/generate_bench.log      (fp8: set_gemm_dtype("fp8"): e4m3 decoder weights,
half the projection bytes of a step; the LM head stays bf16)
python tools/generate_bench.py [B] [N] [beams] mxfp4: the same with set_gemm_dtype("mxfp4"): MXFP4 decoder weights, 4.25 bits per projection
weight in the decode step
python tools/generate_bench.py [B] [N] sample: the three ways of choosing a token in one process, top_k=50, top_p=0.9, temperature=0.7: ms per
decode step of greedy decoding, of sampling with torch ops on the logits (`generator=`: no graph) and of the device sampler (`seed=`: graph
replay), and p2t_sample_select's own time on [B, vocab] bf16 logits (HIP events around 200 launches).
python tools/generate_bench.py [B] [N] [beams > 1]: beam search three ways, interleaved, three runs each (median and min .. max): the torch
bookkeeping (`beam_select="torch"`: one host read per token), p2t_beam_select with eager launches and under replay of the two-step graph;
then B * beams greedy rows under replay, p2t_beam_select's two launches alone, and p2t_kv_reorder at 30 and at 250 generated tokens.
python tools/generate_bench.py [B] [N] [beams > 1] sample: beam sampling (top_k=50, top_p=0.9, temperature=0.7) four ways, interleaved, three
runs each: beam search with p2t_beam_select under graph replay (the yardstick: the same work without the noise), torch beam sampling
(`beam_select="torch"`, `generator=`), p2t_beam_sample_select with eager launches and under graph replay; then the two select entry
points' launches alone, back to back.
python tools/generate_bench.py [B] [N] process: the logits processors (repetition_penalty 1.3, no_repeat_ngram_size 3; then those plus
min_new_tokens, bad_words_ids and suppress_tokens) in front of the greedy choice, under graph replay, against plain greedy decoding,
interleaved, three runs each; then p2t_logits_process alone on [B, vocab] bf16 logits at histories of 0, 64 and 255 tokens.
python tools/generate_bench.py [B] [N] [beams > 1] process: the logits processors under beam search (`beam_select="device"`), under replay of
the two-step graph, interleaved, three runs each: plain beam search (p2t_beam_select: nothing new is launched or allocated), the same with
repetition_penalty 1.3 + no_repeat_ngram_size 3, the same with all five processors; then p2t_beam_logprobs_process alone on
[B * beams, vocab] bf16 logits at histories of 0 and 64 tokens, p2t_beam_select_logprobs alone on its rows, and p2t_beam_select alone.
python tools/generate_bench.py [B] [N] [beams] kv8 [fp8 | mxfp4]: the step with the bf16 and with the fp8 prompt segment of the KV cache
(`prompt_kv_dtype="fp8"`), interleaved in one process, three runs each under graph replay, each next to a run of its prompt phase (beams > 1: beam_select="device", the beams of a
prompt share its prompt segment): median and min .. max, and the cache bytes a step reads either way.
python tools/generate_bench.py [B] [N] [beams > 1] ancestry [kv8] [fp8 | mxfp4]: the device beam search with the per-step cache copy and with
`beam_cache="ancestry"` (the ancestry table read by the attention), interleaved in one process, three runs each under graph replay.
python tools/generate_bench.py [B] [N] [beams] head [fp8 | mxfp4] [kv8] [fp8 | mxfp4]: the step with the bf16 LM head (off) and with the
quantised one (`lm_head_dtype=`; both formats when none is named), interleaved in one process, three runs each under graph replay, each
next to a run of its prompt phase; `kv8`: the same again over the fp8 prompt segment; last: the tower GEMM dtype.
python tools/generate_bench.py [slots] [Tnew] continuous [fp8 | mxfp4] [kv8] [head fp8 | head mxfp4]: continuous batching (p2t_hip/continuous.py)
against lock-step decoding on one queue of 8 x slots requests at the bench's prompt shape, whose limits are drawn once from a seeded
log-normal clipped to 1 .. Tnew (random weights have no natural eos: the limit is what ends a row).  (a) batches of `slots` through the
decoder's plain `generate` with max_new_tokens = the batch's longest limit -- what lock-step decoding with an eos costs; (b) the same
requests through ContinuousDecoder.  Interleaved, three runs each, on the decoder alone (the prompt embeddings are computed once and
shared): useful tokens/s (sum of limits / wall time) and the fraction of row-steps spent on finished rows, for both; then ms per step of
p2t_llama_decode_step_rows against the lock-step step at equal counters, under graph replay.
python tools/generate_bench.py [slots] [Tnew] continuous sample | process: the continuous leg with `choice="device"` -- `sample`: the
device sampler (top_k=50, top_p=0.9, temperature=0.7, seed=1; p2t_sample_select_rows), `process`: all five logits processors in front of
the greedy choice (p2t_logits_process_rows) -- against the greedy continuous leg on the same queue, interleaved, three runs each: ms per
step and useful tokens/s; then the whole step {embed, step, [processors], choice} under graph replay at equal rows, the per-row engine
against the lock-step engine with the SAME choice rule (the yardstick: what `generate(seed=)` / `generate(processors)` replays), three
interleaved runs each, and whether the per-row step exceeds it by more than the runs' own min .. max spread.  Random weights have no eos:
the limit ends a row, and nothing is claimed about the quality of what is decoded.
python tools/generate_bench.py [B] [N] ragged [uniform]: the padded prompt phase against the padding-free one (`prefill="packed"`) on B prompts
whose protein lengths are drawn once from bench.py's lognormal(5.75, 0.6) clipped to [16, 1024] (seed 0) + 64 chat tokens, left-padded to
the longest as the collater does (`uniform`: 1024 residues each -- packing can win nothing there and pays for the unfused rotation).
Interleaved in one process, three runs each, medians: (a) the decoder's share alone (compact + prefill | pack + prefill_packed, first-token
head included), (b) the whole prompt phase with the still-padded ESM2 + adapter, (c) a whole generate of N tokens; and padded / valid
tokens, the bound on (a).
python tools/generate_bench.py 8 [N] lookup [fp8 | mxfp4] [kv8]: prompt-lookup decoding (`prompt_lookup_num_tokens`, p2t_hip/lookup.py): ms per
multi-token step at 1 / 2 / 4 / 8 prompts x k = 1 / 3 / 7 next to the one-token step at the same prompts and at 32 rows, one process,
interleaved, three runs each under graph replay, the break-even acceptance per step, and the random-weight run's observed tokens per
step (labelled synthetic)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prot2text-v2-esm3_amd"))
import p2t_hip as P                                             # noqa: E402
from p2t_hip import generation, specs, synth                    # noqa: E402
from p2t_hip._lib import call                                   # noqa: E402
from p2t_hip.ops import ptr, stream                             # noqa: E402


def sampler_alone(B: int, V: int, dev, iters: int = 200) -> float:
    """-> microseconds per p2t_sample_select launch on randn * 3 bf16 logits (top_k 50, top_p 0.9, temperature 0.7)."""
    from p2t_hip import _lib
    from p2t_hip.ops import ptr, stream
    ld = (V + 63) // 64 * 64
    lg = (torch.randn((B, ld), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 3).to(torch.bfloat16)
    fin, nxt = torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int64, device=dev)
    out, flags, step = torch.zeros((B, 64), dtype=torch.int64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    go = lambda: _lib.call("p2t_sample_select", ptr(lg), _lib.BF16, ld, V, B, None, 0, 0, ptr(fin), ptr(nxt), ptr(out), 64, ptr(step), 64, 0.7, 50, 0.9, 1, 0,
                           None, 0, ptr(flags), stream())
    for _ in range(10):
        go()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        go()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def sample_mode(model, kw, B: int, N: int, V: int, dev):
    gen = torch.Generator(device=dev)
    sampling = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.7)
    cases = [("greedy (graph replay)", dict(do_sample=False)),
             ("sampling, torch ops on the logits (generator=; eager launches)", dict(**sampling, generator=gen.manual_seed(1))),
             ("sampling, p2t_sample_select (seed=; graph replay)", dict(**sampling, seed=1))]
    for _, extra in cases:                                       # warm-up of each path
        model.generate(**{**kw, **extra, "max_new_tokens": 4})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(**{**kw, "max_new_tokens": 1})
    torch.cuda.synchronize()
    t_prompt = time.perf_counter() - t0
    for name, extra in cases:
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            model.generate(**{**kw, **extra})
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0 - t_prompt) / (N - 1)
            best = dt if best is None else min(best, dt)
        print(f"generate cfg3: B={B}, {N} new tokens, {name}: {best * 1e3:.3f} ms/step", flush=True)
    print(f"p2t_sample_select alone, [{B}, {V}] bf16 logits, top_k=50 top_p=0.9 temperature=0.7: {sampler_alone(B, V, dev):.1f} us per launch", flush=True)


def _events(go, iters: int) -> float:
    """-> microseconds per call of go(), HIP events around `iters` calls after 10 warm-up calls."""
    for _ in range(10):
        go()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        go()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def beam_mode(model, kw, B: int, N: int, beams: int, V: int, dev):
    cases = [("torch bookkeeping (beam_select=\"torch\"; eager launches, one host read per token)", dict(beam_select="torch")),
             ("p2t_beam_select, eager launches", dict(beam_select="device", use_graph=False)),
             ("p2t_beam_select, two-step graph replay", dict(beam_select="device", use_graph=True))]
    for _, extra in cases:
        model.generate(**{**kw, **extra, "max_new_tokens": 6})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(**{**kw, "max_new_tokens": 1, "beam_select": "device"})
    torch.cuda.synchronize()
    t_prompt = time.perf_counter() - t0
    runs = {name: [] for name, _ in cases}
    for _ in range(3):                                           # interleaved: a drift of the box hits all three alike
        for name, extra in cases:
            t0 = time.perf_counter()
            model.generate(**{**kw, **extra})
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0 - t_prompt) / (N - 1) * 1e3)
    for name, r in runs.items():
        print(f"generate cfg3: B={B} beams={beams}, {N} new tokens, {name}: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)
    # the same number of rows, greedy, under replay
    rows = B * beams
    gkw = {k: (v.repeat_interleave(beams, dim=0) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    gkw["num_beams"] = 1
    model.generate(**{**gkw, "max_new_tokens": 4})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(**{**gkw, "max_new_tokens": 1})
    torch.cuda.synchronize()
    tg = time.perf_counter() - t0
    r = []
    for _ in range(3):
        t0 = time.perf_counter()
        model.generate(**gkw)
        torch.cuda.synchronize()
        r.append((time.perf_counter() - t0 - tg) / (N - 1) * 1e3)
    print(f"generate cfg3: {rows} greedy rows, {N} new tokens, graph replay: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)
    # the two select launches alone: a fresh state at step 0, nothing finishes, so every call does the full work
    ld = (V + 63) // 64 * 64
    lg = (torch.randn((rows, ld), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 3).to(torch.bfloat16)
    st = generation.BeamState(B, beams, 256, 0, dev)
    step, nxt, src = (torch.zeros((n,), dtype=dt, device=dev) for n, dt in ((1, torch.int32), (rows, torch.int64), (rows, torch.int64)))
    eos = torch.zeros((0,), dtype=torch.int64, device=dev)
    us = _events(lambda: generation.beam_select(lg, V, st, eos, 0, 1.0, False, 256, step, nxt, src), 200)
    print(f"p2t_beam_select alone (both launches), [{rows}, {V}] bf16 logits, {beams} beams: {us:.1f} us per call", flush=True)
    # the beam re-ordering copy of the generated cache segment at two lengths
    eng = generation.DecodeEngine(model.llama_decoder, B, beams, 64, 256)
    ident = torch.arange(rows, dtype=torch.int64, device=dev)
    for at in (30, 250):
        eng.step.fill_(at)
        print(f"p2t_kv_reorder, {rows} rows, {at} generated tokens: {_events(lambda: eng.reorder(ident), 50):.1f} us per call", flush=True)


def process_mode(model, kw, B: int, N: int, V: int, dev):
    rp = dict(repetition_penalty=1.3, no_repeat_ngram_size=3)
    every = dict(rp, min_new_tokens=N // 2, eos_token_id=[128001, 128009], bad_words_ids=[[11, 12], [13, 14, 15], [16]] * 8, suppress_tokens=list(range(100, 132)))
    cases = [("greedy (graph replay)", dict()),
             ("greedy + repetition_penalty 1.3, no_repeat_ngram_size 3 (p2t_logits_process in the graph)", rp),
             ("greedy + penalty, n-gram, min_new_tokens, 24 bad words, 32 suppressed ids (two eos ids: a host read per 16 tokens)", every)]
    for _, extra in cases:
        model.generate(**{**kw, **extra, "max_new_tokens": 4})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(**{**kw, "max_new_tokens": 1})
    torch.cuda.synchronize()
    t_prompt = time.perf_counter() - t0
    runs = {name: [] for name, _ in cases}
    for _ in range(3):                                           # interleaved: a drift of the box hits all three alike
        for name, extra in cases:
            t0 = time.perf_counter()
            out = model.generate(**{**kw, **extra})
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0 - t_prompt) / (out.shape[1] - 1) * 1e3)
    for name, r in runs.items():
        print(f"generate cfg3: B={B}, {N} new tokens, {name}: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)
    # the kernel alone: every processor on, random histories from 1000 ids (repeats for certain)
    eng = generation.DecodeEngine(model.llama_decoder, B, 1, 64, 256, processors=generation._processor_args(
        V, [128001, 128009], 1.3, 3, 256, every["bad_words_ids"], every["suppress_tokens"]), eos_ids=[128001, 128009])
    g = torch.Generator(device=dev).manual_seed(0)
    eng.logits.copy_((torch.randn(eng.logits.shape, device=dev, generator=g) * 3).to(torch.bfloat16))
    eng.out_tokens.copy_(torch.randint(0, 1000, eng.out_tokens.shape, device=dev, generator=g))
    for at in (0, 64, 255):
        eng.step.fill_(at)
        us = _events(lambda: eng.process(eng.logits), 200)
        print(f"p2t_logits_process alone, [{B}, {V}] bf16 logits -> f32, every processor on, {at} history tokens: {us:.1f} us per launch "
              f"({B * V * 6 / us / 1e6:.2f} TB/s of row traffic)", flush=True)


def beam_process_mode(model, kw, B: int, N: int, beams: int, V: int, dev):
    rp = dict(repetition_penalty=1.3, no_repeat_ngram_size=3)
    every = dict(rp, min_new_tokens=N // 2, eos_token_id=[128001, 128009], bad_words_ids=[[11, 12], [13, 14, 15], [16]] * 8, suppress_tokens=list(range(100, 132)))
    cases = [("beam search, p2t_beam_select, two-step graph replay", dict()),
             ("beam search + repetition_penalty 1.3, no_repeat_ngram_size 3 (p2t_beam_logprobs_process + p2t_beam_select_logprobs in the graph)", rp),
             ("beam search + penalty, n-gram, min_new_tokens, 24 bad words, 32 suppressed ids (two eos ids)", every)]
    kw = {**kw, "beam_select": "device"}
    for _, extra in cases:
        model.generate(**{**kw, **extra, "max_new_tokens": 6})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(**{**kw, "max_new_tokens": 1})
    torch.cuda.synchronize()
    t_prompt = time.perf_counter() - t0
    runs = {name: [] for name, _ in cases}
    for _ in range(3):                                           # interleaved: a drift of the box hits all three alike
        for name, extra in cases:
            t0 = time.perf_counter()
            out = model.generate(**{**kw, **extra})
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0 - t_prompt) / (N - 1) * 1e3)
            assert out.shape[1] == N, (name, out.shape)          # nothing finished early: every run is N steps
    for name, r in runs.items():
        print(f"generate cfg3: B={B} beams={beams}, {N} new tokens, {name}: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)
    # the entry points alone: every processor on, random histories from 1000 ids (repeats for certain); the selections on a fresh state at
    # step 0, where nothing finishes, so every call does the full work
    rows = B * beams
    eng = generation.DecodeEngine(model.llama_decoder, B, beams, 64, 256, processors=generation._processor_args(
        V, [128001, 128009], 1.3, 3, 256, every["bad_words_ids"], every["suppress_tokens"]), eos_ids=[128001, 128009])
    g = torch.Generator(device=dev).manual_seed(0)
    eng.logits.copy_((torch.randn(eng.logits.shape, device=dev, generator=g) * 3).to(torch.bfloat16))
    hist = generation.BeamState(B, beams, 256, 0, dev)
    hist.run_seq.copy_(torch.randint(0, 1000, hist.run_seq.shape, device=dev, generator=g))
    for at in (0, 64):
        eng.step.fill_(at)
        us = _events(lambda: eng.beam_process(eng.logits, hist, 256, eng.processed), 200)
        print(f"p2t_beam_logprobs_process alone, [{rows}, {V}] bf16 logits -> f32, every processor on, {at} history tokens: {us:.1f} us per launch",
              flush=True)
    st = generation.BeamState(B, beams, 256, 0, dev)
    step, nxt, src = (torch.zeros((n,), dtype=dt, device=dev) for n, dt in ((1, torch.int32), (rows, torch.int64), (rows, torch.int64)))
    eos = torch.zeros((0,), dtype=torch.int64, device=dev)
    us = _events(lambda: generation.beam_select_logprobs(eng.processed, V, st, eos, 0, 1.0, False, 256, step, nxt, src), 200)
    print(f"p2t_beam_select_logprobs alone (both launches), [{rows}, {V}] f32 processed log-probabilities, {beams} beams: {us:.1f} us per call", flush=True)
    st = generation.BeamState(B, beams, 256, 0, dev)
    us = _events(lambda: generation.beam_select(eng.logits, V, st, eos, 0, 1.0, False, 256, step, nxt, src), 200)
    print(f"p2t_beam_select alone (both launches), [{rows}, {V}] bf16 logits, {beams} beams: {us:.1f} us per call", flush=True)


def beam_sample_mode(model, kw, B: int, N: int, beams: int, V: int, dev):
    sampling = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.7)
    gen = torch.Generator(device=dev).manual_seed(1)
    cases = [("beam search, p2t_beam_select, two-step graph replay", dict(beam_select="device")),
             ("beam sampling, torch (beam_select=\"torch\", generator=; eager launches, one host read per token)",
              dict(**sampling, beam_select="torch", generator=gen)),
             ("beam sampling, p2t_beam_sample_select, eager launches", dict(**sampling, beam_select="device", seed=1, use_graph=False)),
             ("beam sampling, p2t_beam_sample_select, two-step graph replay", dict(**sampling, beam_select="device", seed=1))]
    for _, extra in cases:
        model.generate(**{**kw, **extra, "max_new_tokens": 6})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(**{**kw, "max_new_tokens": 1, "beam_select": "device"})
    torch.cuda.synchronize()
    t_prompt = time.perf_counter() - t0
    runs = {name: [] for name, _ in cases}
    for _ in range(3):                                           # interleaved: a drift of the box hits all four alike
        for name, extra in cases:
            t0 = time.perf_counter()
            model.generate(**{**kw, **extra})
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0 - t_prompt) / (N - 1) * 1e3)
    for name, r in runs.items():
        print(f"generate cfg3: B={B} beams={beams}, {N} new tokens, {name}: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)
    # the select launches alone, back to back: a fresh state at step 0, nothing finishes, so every call does the full work
    rows, ld = B * beams, (V + 63) // 64 * 64
    lg = (torch.randn((rows, ld), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 3).to(torch.bfloat16)
    step, nxt, src = (torch.zeros((n,), dtype=dt, device=dev) for n, dt in ((1, torch.int32), (rows, torch.int64), (rows, torch.int64)))
    eos = torch.zeros((0,), dtype=torch.int64, device=dev)
    st, sst = generation.BeamState(B, beams, 256, 0, dev), generation.BeamState(B, beams, 256, 0, dev, sample=True)
    live = generation.BeamState(B, beams, 256, 0, dev, sample=True)        # every beam live, as from the second step on: a fresh state's beams 1 ..
    live.run_scores[:] = -1.0 - 0.25 * torch.arange(beams, device=dev)     # score -1e9, and with both filters off all V keys of such a row tie
    for _ in range(2):
        us = _events(lambda: generation.beam_select(lg, V, st, eos, 0, 1.0, False, 256, step, nxt, src), 200)
        print(f"p2t_beam_select alone (both launches), [{rows}, {V}] bf16 logits, {beams} beams: {us:.1f} us per call", flush=True)
        us = _events(lambda: generation.beam_sample_select(lg, V, sst, eos, 0, 1.0, False, 256, step, nxt, src, 0.7, 50, 0.9, 1), 200)
        print(f"p2t_beam_sample_select alone (both launches), top_k=50 top_p=0.9 temperature=0.7: {us:.1f} us per call", flush=True)
        us = _events(lambda: generation.beam_sample_select(lg, V, sst, eos, 0, 1.0, False, 256, step, nxt, src, 1.0, 0, 1.0, 1), 200)
        print(f"p2t_beam_sample_select alone (both launches), both filters off, fresh state (3 of 4 beams at -1e9): {us:.1f} us per call", flush=True)
        us = _events(lambda: generation.beam_sample_select(lg, V, live, eos, 0, 1.0, False, 256, step, nxt, src, 0.7, 50, 0.9, 1), 200)
        print(f"p2t_beam_sample_select alone (both launches), top_k=50 top_p=0.9 temperature=0.7, every beam live: {us:.1f} us per call", flush=True)
        us = _events(lambda: generation.beam_sample_select(lg, V, live, eos, 0, 1.0, False, 256, step, nxt, src, 1.0, 0, 1.0, 1), 200)
        print(f"p2t_beam_sample_select alone (both launches), both filters off, every beam live: {us:.1f} us per call", flush=True)
    print(f"flags after these calls: {int(sst.flags.item())} (fresh state), {int(live.flags.item())} (every beam live)", flush=True)


def kv8_mode(model, kw, B: int, N: int, beams: int, T: int, llama, gemm_dtype: str):
    cases = [("bf16 prompt segment", dict()), ("fp8 prompt segment (prompt_kv_dtype=\"fp8\")", dict(prompt_kv_dtype="fp8"))]
    if beams > 1:
        kw = {**kw, "beam_select": "device"}
    for _, extra in cases:                                       # warm-up of each path
        model.generate(**{**kw, **extra, "max_new_tokens": 6})
    torch.cuda.synchronize()

    def timed(**over):
        t0 = time.perf_counter()
        model.generate(**{**kw, **over})
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    runs, t_prompt = {name: [] for name, _ in cases}, {name: [] for name, _ in cases}
    for _ in range(3):                                           # interleaved: a drift of the box hits both alike
        for name, extra in cases:
            # the prompt phase (one new token) next to every full run: at 32 prompts it is longer than the 63 steps it is subtracted from
            t1 = timed(**extra, max_new_tokens=1)
            runs[name].append((timed(**extra) - t1) / (N - 1) * 1e3)
            t_prompt[name].append(t1 * 1e3)
    L, nkv, d = llama.num_hidden_layers, llama.num_key_value_heads, llama.head_dim
    rows = B * beams
    gen_bytes = 2 * 2 * L * nkv * d * rows * N / 2               # the generated segment: bf16 either way, at the mean generated length
    # every row streams its prompt's segment (the beams of a prompt read the same bytes: rows * T keys pass the CUs, B * T are distinct)
    for (name, _), per_key in zip(cases, (2 * 2 * d, 2 * d + 2)):
        r = runs[name]
        print(f"generate cfg3{' ' + gemm_dtype + ' GEMMs' if gemm_dtype != 'model' else ''}: B={B} beams={beams} prompt {T} tokens, {N} new tokens, graph replay, "
              f"{name}: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs); cache bytes read per step "
              f"{(L * nkv * per_key * rows * T + gen_bytes) / 1e9:.2f} GB ({L * nkv * per_key * B * T / 1e9:.2f} GB distinct prompt bytes); "
              f"prompt phase {np.median(t_prompt[name]):.1f} ms", flush=True)


def ancestry_mode(model, kw, B: int, N: int, beams: int, T: int, gemm_dtype: str, with_kv8: bool):
    """The device beam search with the per-step cache copy (beam_cache=None: p2t_kv_reorder + the (row, kv head) attention) and without it
    (beam_cache="ancestry": p2t_kv_ancestry_update + the (prompt, kv head) attention), interleaved in one process, three runs each under
    graph replay, each next to a run of its prompt phase -- kv8_mode's method."""
    cases = [("copy (beam_cache=None)", dict()), ("ancestry table (beam_cache=\"ancestry\")", dict(beam_cache="ancestry"))]
    kw = {**kw, "beam_select": "device", **({"prompt_kv_dtype": "fp8"} if with_kv8 else {})}
    for _, extra in cases:                                       # warm-up of each path
        model.generate(**{**kw, **extra, "max_new_tokens": 6})
    torch.cuda.synchronize()

    def timed(**over):
        t0 = time.perf_counter()
        model.generate(**{**kw, **over})
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    runs = {name: [] for name, _ in cases}
    for _ in range(3):                                           # interleaved: a drift of the box hits both alike
        for name, extra in cases:
            t1 = timed(**extra, max_new_tokens=1)
            runs[name].append((timed(**extra) - t1) / (N - 1) * 1e3)
    for name, _ in cases:
        r = runs[name]
        print(f"generate cfg3{' ' + gemm_dtype + ' GEMMs' if gemm_dtype != 'model' else ''}{' kv8' if with_kv8 else ''}: B={B} beams={beams} prompt {T} tokens, "
              f"{N} new tokens, graph replay, {name}: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)
    a, c = np.median(runs[cases[1][0]]), np.median(runs[cases[0][0]])
    print(f"  ancestry / copy = {a / c:.4f} (copy - ancestry = {(c - a) * 1e3:+.0f} us per step; ranges {max(runs[cases[0][0]]) - min(runs[cases[0][0]]):.3f} and "
          f"{max(runs[cases[1][0]]) - min(runs[cases[1][0]]):.3f} ms)", flush=True)


def head_mode(model, kw, B: int, N: int, beams: int, T: int, llama, gemm_dtype: str, fmts, with_kv8: bool):
    """The step with the bf16 LM head (off: the parent's arithmetic) and with the quantised one (`lm_head_dtype=`), interleaved in one
    process, three runs each under graph replay, each next to a run of its prompt phase -- kv8_mode's method; with `kv8` the same again
    over the fp8 prompt segment of the KV cache."""
    if beams > 1:
        kw = {**kw, "beam_select": "device"}
    H, V = llama.hidden_size, llama.vocab_size
    head_bytes = {None: 2.0 * V * H, "fp8": 1.0 * V * H + V, "mxfp4": V * H * 17.0 / 32.0}

    def timed(**over):
        t0 = time.perf_counter()
        model.generate(**{**kw, **over})
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for kv in ((None, "fp8") if with_kv8 else (None,)):
        cases = [("bf16 LM head (off)", None)] + [(f"{f} LM head (lm_head_dtype=\"{f}\")", f) for f in fmts]
        extra = lambda f: dict(lm_head_dtype=f, prompt_kv_dtype=kv)
        for _, f in cases:                                       # warm-up of each path: engines, the quantised head and its stream copy
            model.generate(**{**kw, **extra(f), "max_new_tokens": 6})
        torch.cuda.synchronize()
        runs = {name: [] for name, _ in cases}
        for _ in range(3):                                       # interleaved: a drift of the box hits every case alike
            for name, f in cases:
                t1 = timed(**extra(f), max_new_tokens=1)
                runs[name].append((timed(**extra(f)) - t1) / (N - 1) * 1e3)
        off = np.median(runs[cases[0][0]])
        for name, f in cases:
            r = runs[name]
            print(f"generate cfg3{' ' + gemm_dtype + ' GEMMs' if gemm_dtype != 'model' else ''}{' kv8' if kv else ''}: B={B} beams={beams} prompt {T} tokens, "
                  f"{N} new tokens, graph replay, {name}: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs), "
                  f"{np.median(r) - off:+.3f} ms vs off; head bytes per step {head_bytes[f] / 1e9:.3f} GB", flush=True)


def continuous_mode(model, kw, slots: int, Tnew: int, T: int, gemm_dtype: str, extra: dict):
    from p2t_hip.continuous import ContinuousDecoder, ContinuousEngine
    dec = model.llama_decoder
    n_req = 8 * slots
    rs = np.random.RandomState(1)
    limits = np.clip(np.rint(np.exp(rs.normal(np.log(Tnew / 4.0), 0.8, size=n_req))), 1, Tnew).astype(int).tolist()
    with torch.no_grad():
        emb, mask = model(input_ids=kw["inputs"], attention_mask=kw["attention_mask"], protein_input_ids=kw["protein_input_ids"],
                          protein_attention_mask=kw["protein_attention_mask"], return_decoder_inputs=True)
    pad = kw["pad_token_id"]
    batches = [limits[i:i + slots] for i in range(0, n_req, slots)]
    useful_steps = sum(l - 1 for l in limits)                    # the first token of a request comes out of its prefill

    def lock_step():
        for lim in batches:
            out = dec.generate(inputs_embeds=emb, attention_mask=mask, max_new_tokens=max(lim), eos_token_id=None, pad_token_id=pad, do_sample=False, **extra)
            assert out.shape[1] == max(lim)
        return sum(slots * (max(lim) - 1) for lim in batches)

    def continuous():
        cd = ContinuousDecoder(dec, slots, T, Tnew, eos_token_id=None, pad_token_id=pad, sync_every=8, **extra)
        for i in range(0, n_req, slots):
            cd.submit(emb, mask, max_new_tokens=limits[i:i + slots])
        got = {rid: int(toks.numel()) for rid, toks in cd.run()}
        assert [got[i] for i in range(n_req)] == limits
        return cd.engine().steps_run * slots

    cases = [("(a) lock-step batches of `slots` through generate, max_new_tokens = the batch's longest limit", lock_step),
             ("(b) ContinuousDecoder, sync_every 8", continuous)]
    for _, f in cases:                                           # warm-up of each path: engines, stream copies, lazy initialisation
        f()
    torch.cuda.synchronize()
    wall, row_steps = {n: [] for n, _ in cases}, {}
    for _ in range(3):                                           # interleaved: a drift of the box hits both alike
        for name, f in cases:
            t0 = time.perf_counter()
            row_steps[name] = f()
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    tag = f"generate cfg3{' ' + gemm_dtype + ' GEMMs' if gemm_dtype != 'model' else ''}{''.join(' ' + k + '=' + str(v) for k, v in extra.items())}"
    print(f"{tag}: {n_req} requests through {slots} slots, prompt {T} tokens, limits log-normal (median {int(np.median(limits))}, mean {np.mean(limits):.1f}, "
          f"max {max(limits)}, clipped to 1 .. {Tnew}; synthetic lengths: no claim about real descriptions), decoder only", flush=True)
    tps = {}
    for name, _ in cases:
        w = wall[name]
        tps[name] = sum(limits) / np.median(w)
        print(f"{tag}: {name}: median {np.median(w) * 1e3:.0f} ms (min {min(w) * 1e3:.0f}, max {max(w) * 1e3:.0f}; 3 runs) = {tps[name]:.0f} useful tokens/s; "
              f"{row_steps[name]} row-steps, {1 - useful_steps / row_steps[name]:.3f} of them on finished rows", flush=True)
    (na, _), (nb, _) = cases
    print(f"{tag}: (b) / (a) useful tokens/s = {tps[nb] / tps[na]:.2f}; the ratio of live row-step fractions bounds it at "
          f"{(useful_steps / row_steps[nb]) / (useful_steps / row_steps[na]):.2f} (the rest: refill prefills between replays and sync_every slack)", flush=True)
    # the step alone at equal counters: the lock-step entry point against p2t_llama_decode_step_rows, a graph of {embed, step} each
    e1 = generation.DecodeEngine(dec, slots, 1, T, 256, **extra)
    e1.prefill(*e1.compact(emb, mask))
    e2 = ContinuousEngine(dec, slots, T, 256, [], pad, use_graph=False, **extra)
    e2.load(list(range(slots)), [(emb[b], mask[b]) for b in range(slots)], [256] * slots)
    tok = torch.full((slots,), 11, dtype=torch.int64, device=emb.device)
    steps = {"lock-step step (p2t_llama_decode_step[_q])": (e1, lambda: (e1.feed(tok), e1.decode_step()), lambda: e1.step.zero_()),
             "p2t_llama_decode_step_rows": (e2, lambda: (e2.feed(tok), e2._step_rows(frozen=False)), lambda: e2.row_step.zero_())}
    graphs = {}
    for name, (_, go, reset) in steps.items():
        go(); go()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], capture_error_mode="thread_local"):
            go()
        reset()
    ms = {name: [] for name in steps}
    for _ in range(3):
        for name, (_, _, reset) in steps.items():
            reset()
            ms[name].append(_events(graphs[name].replay, 100) / 1e3)
    for name, r in ms.items():
        print(f"{tag}: {slots} rows, counters 0 .. 110, graph replay, {name}: median {np.median(r):.3f} ms/step (min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)


def lookup_mode(model, kw, B: int, N: int, T: int, gemm_dtype: str, extra: dict):
    """[B] [N] lookup [fp8 | mxfp4] [kv8]: prompt-lookup decoding (generate(prompt_lookup_num_tokens=k)) at 1 / 2 / 4 / 8 prompts x k = 1 / 3 / 7.
    (1) the step alone, one process, interleaved, three runs each under graph replay: {embed, p2t_llama_decode_step_multi} of rows x (k + 1)
    tokens next to {embed, p2t_llama_decode_step_rows} of the same rows (and of 32 rows), every counter held at 64 generated tokens (the rows
    are marked finished: nothing advances, the work is that of live rows) -> the break-even acceptance t_multi / t_plain - 1 tokens per step;
    (2) generate with the switch on this random-weight model: tokens per verify step as observed -- SYNTHETIC: random-weight greedy text
    loops, so this says nothing about real descriptions."""
    from p2t_hip.continuous import ContinuousEngine
    from p2t_hip.lookup import LookupEngine
    dec = model.llama_decoder
    with torch.no_grad():
        emb, mask = model(input_ids=kw["inputs"], attention_mask=kw["attention_mask"], protein_input_ids=kw["protein_input_ids"],
                          protein_attention_mask=kw["protein_attention_mask"], return_decoder_inputs=True)
    pad, S = kw["pad_token_id"], 64
    tag = f"generate cfg3{' ' + gemm_dtype + ' GEMMs' if gemm_dtype != 'model' else ''}{''.join(' ' + k + '=' + str(v) for k, v in extra.items())} lookup"
    rep = lambda t, rows: t.repeat((rows + t.shape[0] - 1) // t.shape[0], *([1] * (t.dim() - 1)))[:rows].contiguous()
    graphs, keep = {}, []
    for rows in (1, 2, 4, 8, 32):
        e = ContinuousEngine(dec, rows, T, 256, [], pad, use_graph=False, **extra)
        x, m = rep(emb, rows), rep(mask, rows)
        e.load(list(range(rows)), [(x[b], m[b]) for b in range(rows)], [256] * rows)
        e.row_step.fill_(S)
        e.finished.fill_(2)
        tok = torch.full((rows,), 11, dtype=torch.int64, device=emb.device)
        graphs[(rows, 0)] = (e, tok, lambda e=e, tok=tok: (e.feed(tok), e._step_rows(frozen=True)))
    for rows in (1, 2, 4, 8):
        for k in (1, 3, 7):
            e = LookupEngine(dec, rows, T, 256, k, 2, [], pad, use_graph=False, **extra)
            e.first(e.prompt(rep(emb, rows), rep(mask, rows)))
            e.row_step.fill_(S)
            e.finished.fill_(2)
            e.step_tokens.fill_(11)
            graphs[(rows, k)] = (e, None, lambda e=e: (call("p2t_llama_embed_tokens", C.byref(e.e["cfg"]), C.byref(e.e["w"]), ptr(e.step_tokens),
                                                            e.BB * e.Q, ptr(e.x), stream()), e.step_multi()))
    for key, (e, tok, go) in graphs.items():
        go(); go()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            go()
        graphs[key] = (e, tok, g)
    ms = {key: [] for key in graphs}
    for _ in range(3):
        for key, (_, _, g) in graphs.items():
            ms[key].append(_events(g.replay, 100) / 1e3)
    med = {key: float(np.median(r)) for key, r in ms.items()}
    for (rows, k), r in ms.items():
        if k == 0:
            print(f"{tag}: {rows} rows, {T}+{S + 1} keys, graph replay, one-token step (p2t_llama_decode_step_rows): median {med[(rows, 0)]:.3f} ms/step "
                  f"(min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)
    for (rows, k), r in ms.items():
        if k:
            print(f"{tag}: {rows} rows x {k + 1} tokens (k = {k}), graph replay, p2t_llama_decode_step_multi: median {med[(rows, k)]:.3f} ms/step (min {min(r):.3f}, "
                  f"max {max(r):.3f}; 3 runs) = {med[(rows, k)] / med[(rows, 0)]:.3f} x the one-token step, {med[(rows, k)] / ((k + 1) * med[(rows, 0)]):.3f} x "
                  f"{k + 1} of them; break-even at {med[(rows, k)] / med[(rows, 0)] - 1:.3f} accepted tokens per step", flush=True)
    print(f"{tag}: 8 rows x 4 tokens {med[(8, 3)]:.3f} ms against the 32-row one-token step {med[(32, 0)]:.3f} ms", flush=True)
    del graphs
    torch.cuda.empty_cache()
    # (2) the whole call, random weights: SYNTHETIC acceptance
    for rows in (1, 8):
        sub = {k2: (v[:rows] if isinstance(v, torch.Tensor) else v) for k2, v in kw.items()}
        for k in (0, 3, 7):
            over = dict(prompt_lookup_num_tokens=k) if k else {}
            model.generate(**{**sub, **extra, **over, "max_new_tokens": 6})
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(**{**sub, **extra, **over}, return_dict_in_generate=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = out.lookup_stats
            note = (f"verify steps per row {st[:, 0].tolist()}, tokens per step {((N - 1) / st[:, 0].float()).mean().item():.2f} (SYNTHETIC: random weights)"
                    if st is not None else "one token per step")
            print(f"{tag}: generate, {rows} prompts, {N} new tokens, k = {k}: {dt * 1e3:.0f} ms wall with the prompt phase; {note}", flush=True)


CHOICE_LEGS = {"sample": dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.7, seed=1),
               # every processor on; the eos ids end no row: they are banned for the first tokens by min_new_tokens and suppressed throughout
               "process": dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=8, eos_token_id=[128001, 128009],
                               bad_words_ids=[[11, 12], [13, 14, 15], [16]] * 8, suppress_tokens=list(range(100, 132)) + [128001, 128009])}


def continuous_choice_mode(model, kw, slots: int, Tnew: int, T: int, leg: str):
    from p2t_hip.continuous import ContinuousDecoder, ContinuousEngine, device_choice
    dec, rule = model.llama_decoder, CHOICE_LEGS[leg]
    V = dec.spec.vocab_size
    n_req = 8 * slots
    rs = np.random.RandomState(1)
    limits = np.clip(np.rint(np.exp(rs.normal(np.log(Tnew / 4.0), 0.8, size=n_req))), 1, Tnew).astype(int).tolist()
    with torch.no_grad():
        emb, mask = model(input_ids=kw["inputs"], attention_mask=kw["attention_mask"], protein_input_ids=kw["protein_input_ids"],
                          protein_attention_mask=kw["protein_attention_mask"], return_decoder_inputs=True)
    pad = kw["pad_token_id"]

    def continuous(**choice):
        cd = ContinuousDecoder(dec, slots, T, Tnew, pad_token_id=pad, sync_every=8, **{"eos_token_id": None, **choice})
        for i in range(0, n_req, slots):
            cd.submit(emb, mask, max_new_tokens=limits[i:i + slots])
        got = {item[0]: int(item[1].numel()) for item in cd.run()}
        assert [got[i] for i in range(n_req)] == limits
        return cd.engine().steps_run

    cases = [("(b) ContinuousDecoder, greedy", lambda: continuous()),
             (f"(c) ContinuousDecoder, choice='device', {leg}", lambda: continuous(choice="device", **rule))]
    for _, f in cases:
        f()
    torch.cuda.synchronize()
    wall, steps_run = {n: [] for n, _ in cases}, {}
    for _ in range(3):                                           # interleaved: a drift of the box hits both alike
        for name, f in cases:
            t0 = time.perf_counter()
            steps_run[name] = f()
            torch.cuda.synchronize()
            wall[name].append(time.perf_counter() - t0)
    tag = f"generate cfg3 continuous {leg}"
    print(f"{tag}: {n_req} requests through {slots} slots, prompt {T} tokens, limits log-normal (median {int(np.median(limits))}, mean {np.mean(limits):.1f}, "
          f"max {max(limits)}, clipped to 1 .. {Tnew}; synthetic lengths, random weights without an eos: no claim about real descriptions or their quality), "
          f"decoder only; rule: {', '.join(k + '=' + (str(v) if not isinstance(v, list) else '[' + str(len(v)) + ' entries]') for k, v in rule.items())}", flush=True)
    for name, _ in cases:
        w = wall[name]
        print(f"{tag}: {name}: median {np.median(w) * 1e3:.0f} ms (min {min(w) * 1e3:.0f}, max {max(w) * 1e3:.0f}; 3 runs) = {sum(limits) / np.median(w):.0f} useful "
              f"tokens/s; {steps_run[name]} steps, {np.median(w) * 1e3 / steps_run[name]:.3f} ms per step (prefills of the refills included)", flush=True)
    # the whole step at equal rows under graph replay: the lock-step engine with the same choice rule against the per-row engine
    eos_ids = rule.get("eos_token_id") or []
    choice = device_choice(V, eos_ids, **{k: v for k, v in rule.items() if k != "eos_token_id"})
    proc, sm = choice["processors"], choice["sampling"]
    eos = torch.tensor(eos_ids, dtype=torch.int64, device=emb.device)
    e1 = generation.DecodeEngine(dec, slots, 1, T, 256, processors=proc, eos_ids=eos_ids)
    e1.prefill(*e1.compact(emb, mask))
    e1.next_tokens.fill_(11)
    e2 = ContinuousEngine(dec, slots, T, 256, eos_ids, pad, use_graph=False, choice=choice)
    e2.load(list(range(slots)), [(emb[b], mask[b]) for b in range(slots)], [256] * slots, list(range(slots)))

    def lock_step():
        e1.feed(e1.next_tokens)
        e1.decode_step()
        lg = e1.process(e1.logits) if proc is not None else e1.logits
        if sm is not None:
            e1.sample_select(lg, eos, pad, sm["temperature"], sm["top_k"], sm["top_p"], sm["seed"])
        else:
            e1.greedy_select(lg, eos, pad)

    def reset2():
        e2.row_step.zero_()
        e2.finished.zero_()

    steps = {f"lock-step engine ({'p2t_logits_process + ' if proc else ''}{'p2t_sample_select' if sm else 'p2t_greedy_select'})": (lock_step, lambda: e1.step.zero_()),
             f"per-row engine ({'p2t_logits_process_rows + ' if proc else ''}{'p2t_sample_select_rows' if sm else 'p2t_greedy_select_rows'})": (e2._advance, reset2)}
    graphs = {}
    for name, (go, reset) in steps.items():
        go(); go()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], capture_error_mode="thread_local"):
            go()
        reset()
    ms = {name: [] for name in steps}
    for _ in range(3):
        for name, (_, reset) in steps.items():
            reset()
            ms[name].append(_events(graphs[name].replay, 100) / 1e3)
    for name, r in ms.items():
        print(f"{tag}: {slots} rows, counters 0 .. 110, graph replay of {{embed, step, choice}}, {name}: median {np.median(r):.3f} ms/step "
              f"(min {min(r):.3f}, max {max(r):.3f}; 3 runs)", flush=True)
    (la, ra), (lb, rb) = ms.items()
    spread = max(max(ra) - min(ra), max(rb) - min(rb))
    over = np.median(rb) - np.median(ra)
    print(f"{tag}: per-row - lock-step = {over * 1e3:+.1f} us per step; the runs' min .. max spread is {spread * 1e3:.1f} us: "
          f"{'within' if over <= spread else 'BEYOND'} the spread", flush=True)
    assert not bool(e2.finished.any().item()) and int(e2.sample_flags.item()) == 0


def ragged_mode(model, B: int, N: int, dev, uniform: bool):
    """The padded prompt phase (compact + p2t_llama_prefill over B x longest tokens) against the packed one (generate(prefill="packed")),
    interleaved in one process, three runs each: (a) the decoder's share alone on shared prompt embeddings, first-token head included,
    (b) the whole prompt phase (ESM2 + adapter + scatter included: the encoder stays padded), (c) a whole generate of N tokens."""
    Tp, n_chat = 1024, 64
    rs = np.random.RandomState(0)
    plens = [Tp] * B if uniform else np.clip(np.round(rs.lognormal(5.75, 0.6, B)), 16, Tp).astype(int).tolist()
    Tl = int(max(plens))
    T = Tl + n_chat
    ids = rs.randint(0, 128000, size=(B, T)).astype(np.int64)
    mask = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(plens):                                # left-padded as the collater does: [pad .. | 16 chat ids | n placeholders | 48 chat ids]
        at = T - n - n_chat
        ids[b, :at], mask[b, at:] = 128002, 1
        ids[b, at + 16:at + 16 + n] = model.config.placeholder_id
    pid, pmask = synth.protein_batch(5, B, Tl, plens)
    t = lambda a: torch.from_numpy(a).to(dev)
    kw = dict(inputs=t(ids), attention_mask=t(mask), protein_input_ids=t(pid), protein_attention_mask=t(pmask), eos_token_id=None, pad_token_id=128002,
              do_sample=False, num_beams=1)
    valid = int(mask.sum())
    bound = B * T / valid
    R, Tpk, _ = generation.plan_prompt_rows(mask.sum(1).tolist())
    tag = f"generate cfg3 ragged{' (uniform 1024 residues)' if uniform else ''}: B={B}"
    print(f"{tag}: protein lengths {'1024 each' if uniform else 'lognormal(5.75, 0.6) clipped to [16, 1024], seed 0'} + {n_chat} chat tokens: "
          f"mean {valid / B:.1f}, longest {T}; padded {B} x {T} = {B * T} tokens, valid {valid}, packed {R} x {Tpk} = {R * Tpk}; "
          f"padded / valid tokens = {bound:.3f} (the bound on the decoder's share)", flush=True)
    with torch.no_grad():
        emb, dmask = model(input_ids=kw["inputs"], attention_mask=kw["attention_mask"], protein_input_ids=kw["protein_input_ids"],
                           protein_attention_mask=kw["protein_attention_mask"], return_decoder_inputs=True)
    dec = model.llama_decoder
    eng = generation.DecodeEngine(dec, B, 1, T, 64)

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    legs = [("(a) decoder share: compact + prefill | pack + prefill_packed, first-token head included",
             lambda: eng.prefill(*eng.compact(emb, dmask)), lambda: eng.prefill_packed(eng.pack(emb, dmask))),
            ("(b) whole prompt phase (ESM2 + adapter + scatter + prefill + first token)",
             lambda: model.generate(**kw, max_new_tokens=1), lambda: model.generate(**kw, max_new_tokens=1, prefill="packed")),
            (f"(c) generate, {N} new tokens", lambda: model.generate(**kw, max_new_tokens=N), lambda: model.generate(**kw, max_new_tokens=N, prefill="packed"))]
    for name, padded, packed in legs:
        padded(); packed()                                       # warm-up of each path
        runs = {"padded": [], "packed": []}
        for _ in range(3):                                       # interleaved: a drift of the box hits both alike
            runs["padded"].append(clock(padded))
            runs["packed"].append(clock(packed))
        a, b = np.median(runs["padded"]), np.median(runs["packed"])
        spread = max(max(r) - min(r) for r in runs.values())
        line = (f"{tag}: {name}: padded median {a:.1f} ms (min {min(runs['padded']):.1f}, max {max(runs['padded']):.1f}), packed median {b:.1f} ms "
                f"(min {min(runs['packed']):.1f}, max {max(runs['packed']):.1f}); 3 runs each; padded / packed = {a / b:.3f}; padded - packed = {a - b:+.1f} ms, "
                f"the runs' min .. max spread is {spread:.1f} ms: {'beyond' if abs(a - b) > spread else 'within'} the spread")
        if name.startswith("(a)"):
            line += f"; achieved / bound = {a / b:.3f} / {bound:.3f} = {a / b / bound:.3f}"
        print(line, flush=True)


def main():
    dev = torch.device("cuda:0")
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    sample = len(sys.argv) > 3 and sys.argv[3] == "sample"        # (after `continuous`, sample / process name that leg's choice rule)
    process = len(sys.argv) > 3 and sys.argv[3] == "process"
    head = "head" in sys.argv[3:5]                               # [B] [N] [beams] head [fp8 | mxfp4] [kv8] [fp8 | mxfp4 weights]
    kv8 = "kv8" in sys.argv[3:5] and not head
    continuous = len(sys.argv) > 3 and sys.argv[3] == "continuous"   # [slots] [Tnew] continuous [fp8 | mxfp4] [kv8] [head fp8 | head mxfp4]
    ragged = len(sys.argv) > 3 and sys.argv[3] == "ragged"           # [B] [N] ragged [uniform]
    lookup = len(sys.argv) > 3 and sys.argv[3] == "lookup"           # [B >= 8] [N] lookup [fp8 | mxfp4] [kv8]
    beams = int(sys.argv[3]) if len(sys.argv) > 3 and not sample and not process and sys.argv[3] not in ("kv8", "head", "continuous", "ragged", "lookup") else 1
    gemm_dtype = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] in ("fp8", "mxfp4") else "model"
    cont_extra = {}
    choice_leg = None
    if continuous:
        after = sys.argv[4:]
        choice_leg = after[0] if after and after[0] in CHOICE_LEGS else None
        gemm_dtype = after[0] if after and after[0] in ("fp8", "mxfp4") else "model"
        if "kv8" in after:
            cont_extra["prompt_kv_dtype"] = "fp8"
        if "head" in after:
            cont_extra["lm_head_dtype"] = after[after.index("head") + 1]
        head = kv8 = False
    if lookup:
        after = sys.argv[4:]
        gemm_dtype = after[0] if after and after[0] in ("fp8", "mxfp4") else "model"
        if "kv8" in after:
            cont_extra["prompt_kv_dtype"] = "fp8"
        head = kv8 = False
    if kv8:                                                      # [B] [N] [beams] kv8 [fp8 | mxfp4]
        after = sys.argv[sys.argv.index("kv8") + 1:]
        gemm_dtype = after[0] if after and after[0] in ("fp8", "mxfp4") else "model"
    head_fmts, head_kv8 = ("fp8", "mxfp4"), False
    if head:
        after = sys.argv[sys.argv.index("head") + 1:]
        if after and after[0] in ("fp8", "mxfp4"):
            head_fmts, after = (after[0],), after[1:]
        if after and after[0] == "kv8":
            head_kv8, after = True, after[1:]
        gemm_dtype = after[0] if after and after[0] in ("fp8", "mxfp4") else "model"
    fp8 = gemm_dtype != "model"
    ancestry = beams > 1 and len(sys.argv) > 4 and sys.argv[4] == "ancestry"      # [B] [N] [beams] ancestry [kv8] [fp8 | mxfp4]
    if ancestry:
        after = sys.argv[5:]
        gemm_dtype = after[-1] if after and after[-1] in ("fp8", "mxfp4") else "model"
        fp8 = gemm_dtype != "model"
    beam_sample = beams > 1 and len(sys.argv) > 4 and sys.argv[4] == "sample"
    beam_process = beams > 1 and len(sys.argv) > 4 and sys.argv[4] == "process"
    esm_name, llama_name, _, _, Tp, _ = specs.CONFIGS["cfg3"]
    esm, llama = specs.esm_spec(esm_name), specs.llama_spec(llama_name)
    ad = specs.adapter_spec(esm, llama)
    model = P.Esm2LlamaInstructForCausalLM.from_specs(esm, llama, ad, dtype=torch.bfloat16, device=dev, seed=0)
    model.eval()
    if fp8:
        model.set_gemm_dtype(gemm_dtype)
    if ragged:
        return ragged_mode(model, B, N, dev, "uniform" in sys.argv[4:])
    n_prompt = 64
    T = Tp + n_prompt
    rs = np.random.RandomState(0)
    ids = rs.randint(0, 128000, size=(B, T)).astype(np.int64)
    ids[:, 16:16 + Tp] = model.config.placeholder_id
    pid, pmask = synth.protein_batch(5, B, Tp)
    t = lambda a: torch.from_numpy(a).to(dev)
    kw = dict(inputs=t(ids), attention_mask=torch.ones((B, T), dtype=torch.int64, device=dev), protein_input_ids=t(pid),
              protein_attention_mask=t(pmask), max_new_tokens=N, eos_token_id=None, pad_token_id=128002, do_sample=False, num_beams=beams)
    if lookup:
        return lookup_mode(model, kw, B, N, T, gemm_dtype, cont_extra)
    if continuous and choice_leg:
        return continuous_choice_mode(model, kw, B, N, T, choice_leg)
    if continuous:
        return continuous_mode(model, kw, B, N, T, gemm_dtype, cont_extra)
    if ancestry:
        return ancestry_mode(model, kw, B, N, beams, T, gemm_dtype, "kv8" in sys.argv[5:])
    if head:
        return head_mode(model, kw, B, N, beams, T, llama, gemm_dtype, head_fmts, head_kv8)
    if kv8:
        return kv8_mode(model, kw, B, N, beams, T, llama, gemm_dtype)
    if sample:
        return sample_mode(model, kw, B, N, llama.vocab_size, dev)
    if process:
        return process_mode(model, kw, B, N, llama.vocab_size, dev)
    if beam_process:
        return beam_process_mode(model, kw, B, N, beams, llama.vocab_size, dev)
    if beam_sample:
        return beam_sample_mode(model, kw, B, N, beams, llama.vocab_size, dev)
    if beams > 1:
        return beam_mode(model, kw, B, N, beams, llama.vocab_size, dev)
    out = model.generate(**{**kw, "max_new_tokens": 4})          # warm-up: engines, workspaces, lazy initialisation
    torch.cuda.synchronize()
    # prompt phase alone
    t0 = time.perf_counter()
    out1 = model.generate(**{**kw, "max_new_tokens": 1})
    torch.cuda.synchronize()
    t_prompt = time.perf_counter() - t0
    res = {}
    for graph in ((True, False) if beams == 1 else (False,)):
        t0 = time.perf_counter()
        out = model.generate(**kw, use_graph=graph)
        torch.cuda.synchronize()
        res[graph] = (time.perf_counter() - t0 - t_prompt) / (N - 1)
    H, F, L, V = llama.hidden_size, llama.intermediate_size, llama.num_hidden_layers, llama.vocab_size
    nh, nkv, d = llama.num_attention_heads, llama.num_key_value_heads, llama.head_dim
    per_weight = {"model": 2.0, "fp8": 1.0, "mxfp4": 17.0 / 32.0}[gemm_dtype]       # mxfp4: 4 bits + one scale byte per 32 weights
    w_bytes = per_weight * L * ((nh + 2 * nkv) * d * H + nh * d * H + 3 * H * F) + 2 * V * H
    BB = B * beams
    kv_bytes = 2 * 2 * L * nkv * d * (B * T + BB * N / 2)       # keys + values, bf16, at the mean generated length
    step_bytes = w_bytes + kv_bytes
    for graph, dt in res.items():
        print(f"generate cfg3{' ' + gemm_dtype + ' GEMMs' if fp8 else ''}: B={B} beams={beams} prompt {T} tokens, {N} new tokens, {'HIP graph' if graph else 'eager launches'}: "
              f"{dt * 1e3:.3f} ms/step = {BB / dt:.0f} tokens/s ({1 / dt:.1f} steps/s); step bytes {step_bytes / 1e9:.2f} GB (weights {w_bytes / 1e9:.2f}, "
              f"cache {kv_bytes / 1e9:.2f}) -> {step_bytes / dt / 1e12:.2f} TB/s = {step_bytes / dt / 8e12:.3f} of 8 TB/s", flush=True)
    print(f"prompt phase (ESM2-3B + adapter + scatter + compaction + prefill of {B} x {T} tokens + first token): {t_prompt * 1e3:.1f} ms; "
          f"first ids {out[0, :6].tolist()}", flush=True)


if __name__ == "__main__":
    main()
