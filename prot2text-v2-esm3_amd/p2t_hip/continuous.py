"""Continuous batching for `generate` (greedy; with `choice="device"` also seeded sampling, the logits processors and output_scores): a fixed number of row SLOTS decode together, every row on its own device-side step
counter, and a slot whose request finished (eos, or the request's own limit) is loaded with the next waiting prompt while the other
rows go on.  `generation.generate` decodes a batch in lock-step until its longest row is done; here no slot waits for another.

What runs where (csrc/llama_decode.hip, csrc/kv_cache.hip, csrc/attn_decode.hip; include/p2t_hip.h "continuous batching"):
  * p2t_llama_decode_step_rows: the decode step with row r at position prompt_len[r] + row_step[r]; `frozen = finished`, so a finished
    (or never loaded) slot re-appends at its own index and stays where it is;
  * p2t_greedy_select_rows: the greedy choice per row, its eos bit (1) and limit bit (2) into `finished`;
  * choice="device" (csrc/sample_select.hip, csrc/logits_process.hip over csrc/row_model.h): p2t_logits_process_rows in front of the
    choice -- the five processors on the row's OWN history out_tokens[r, : row_step[r]] -- and p2t_sample_select_rows in the greedy choice's
    place: row r draws synth.sample_uniform(seed, row_key[r], row_step[r]), so a request's tokens depend on (seed, its key, its own
    logits) and not on its slot, `slots`, `sync_every`, graph or eager, or what else is queued;
  * p2t_kv_slot_load: the k waiting prompts are prefilled TOGETHER into a staging cache (p2t_llama_prefill wants a cache of exactly its
    batch), then one launch copies each row's prompt segment into its slot and resets the slot's counters.
The graph of {embed, step, [processors], choice} is captured once and replayed `sync_every` times between two host reads of (finished, row_step);
refills do not invalidate it: every pointer stays and every length lives on the device.

Two layers: ContinuousScheduler is the queue / slot bookkeeping over anything with the engine's four methods (tests drive it with a
stub, without a GPU); ContinuousEngine is the device state; ContinuousDecoder puts them together for a decoder, and
ContinuousGenerator (Esm2LlamaInstructForCausalLM.continuous_generator) runs the encoder + adapter per submitted batch in front."""
from __future__ import annotations

import ctypes as C
import numbers
import warnings
from collections import deque
from typing import Iterator, List, Optional, Sequence

import torch

from . import _lib, ops
from ._lib import call
from .generation import _FLAG_WARNINGS, DecodeEngine, _as_id_list, _processor_args, _sampler_args
from .ops import ptr, stream

EOS_BIT, LIMIT_BIT = 1, 2          # p2t_greedy_select_rows' bits in `finished`


def refuse_unsupported(num_beams=1, do_sample=False, output_scores=False, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None,
                       bad_words_ids=None, suppress_tokens=None, num_return_sequences=1, **rest) -> None:
    """The keywords of generate() this path does not serve, each refused by name; greedy decoding's neutral ones pass."""
    if num_beams is not None and int(num_beams) > 1:
        raise NotImplementedError("continuous batching: num_beams > 1 is out of scope (beams of a prompt move together; rows here do not)")
    if do_sample:
        raise NotImplementedError("continuous batching: do_sample is out of scope (greedy only; seeded sampling is keyed by (seed, row, step) and can follow)")
    if output_scores:
        raise NotImplementedError("continuous batching: output_scores is out of scope (ask for output_logits: the raw LM-head rows)")
    if (repetition_penalty not in (None, 1.0) or no_repeat_ngram_size not in (None, 0) or min_new_tokens not in (None, 0) or bad_words_ids is not None
            or suppress_tokens is not None):
        raise NotImplementedError("continuous batching: logits processors (repetition_penalty / no_repeat_ngram_size / min_new_tokens / bad_words_ids / "
                                  "suppress_tokens) are out of scope")
    if num_return_sequences not in (None, 1):
        raise NotImplementedError("continuous batching: num_return_sequences > 1 is out of scope")
    neutral = ("temperature", "top_k", "top_p", "length_penalty", "early_stopping", "return_dict_in_generate", "use_cache", "seed", "generator",
               "beam_select", "output_attentions", "output_hidden_states", "synced_gpus")
    bad = [k for k, v in rest.items() if k not in neutral and v is not None]
    if bad:
        raise NotImplementedError(f"continuous batching: unsupported arguments {bad}")


def device_choice(V: int, eos_ids: Sequence[int], num_beams=1, do_sample=False, output_scores=False, temperature=1.0, top_k=50, top_p=1.0, seed=None,
                  generator=None, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, bad_words_ids=None, suppress_tokens=None,
                  num_return_sequences=1, **rest) -> dict:
    """choice="device": generate()'s choice keywords -> dict(processors: _processor_args' settings or None, sampling: dict(temperature,
    top_k, top_p, seed) or None, output_scores), checked by the helpers `generate` uses (the same ValueErrors).  Beams, several
    sequences per prompt and unknown keywords stay refused; sampling needs `seed` (there is no torch path here)."""
    refuse_unsupported(num_beams=num_beams, num_return_sequences=num_return_sequences, **rest)
    proc = _processor_args(V, eos_ids, repetition_penalty, no_repeat_ngram_size, min_new_tokens, bad_words_ids, suppress_tokens)
    sampling = None
    if do_sample:
        if generator is not None:
            raise NotImplementedError("continuous batching: generator= is out of scope (the draws are made on the device, keyed by (seed, key, step): pass seed=)")
        if seed is None or isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError("continuous batching: do_sample=True with choice='device' needs an integer `seed` (the device sampler's; got %r)" % (seed,))
        t, k, p = _sampler_args(temperature, top_k, top_p, seed, None)
        sampling = dict(temperature=t, top_k=k, top_p=p, seed=int(seed))
    return dict(processors=proc, sampling=sampling, output_scores=bool(output_scores))


class ContinuousScheduler:
    """Requests wait in a queue; free slots take them in order; every `sync_every` steps the finished slots are harvested.

    `engine` provides: load(slots, payloads, limits) -- the payloads' prompts into those slots, first token chosen (`keyed`: load(slots,
    payloads, limits, keys) with each request's draw key, by default its request id);
    steps(n) -- n decode steps of every slot; poll() -> (finished [slots], row_step [slots]) as host ints, ONE host read;
    harvest(slot, n) -> a tuple: the slot's first n tokens (and whatever else the engine returns per request)."""

    def __init__(self, engine, slots: int, sync_every: int = 8, keyed: bool = False):
        if slots < 1 or sync_every < 1:
            raise ValueError("slots >= 1 and sync_every >= 1")
        self.engine, self.slots, self.sync_every, self.keyed = engine, int(slots), int(sync_every), bool(keyed)
        self.queue = deque()                               # (request id, payload, limit, key)
        self.owner: List[Optional[int]] = [None] * self.slots
        self.limit = [0] * self.slots                      # the live request's limit per slot
        self.next_id = 0

    def submit(self, payload, limit: int, key: Optional[int] = None) -> int:
        rid, self.next_id = self.next_id, self.next_id + 1
        self.queue.append((rid, payload, int(limit), rid if key is None else int(key)))
        return rid

    def pending(self) -> bool:
        return bool(self.queue) or any(o is not None for o in self.owner)

    def run(self) -> Iterator[tuple]:
        """(request id, *engine.harvest(...)) as requests finish, until the queue is empty and every slot is finished."""
        while self.pending():
            free = [s for s in range(self.slots) if self.owner[s] is None]
            if free and self.queue:
                take = [self.queue.popleft() for _ in range(min(len(free), len(self.queue)))]
                where = free[: len(take)]
                keys = ([k for _, _, _, k in take],) if self.keyed else ()
                self.engine.load(where, [p for _, p, _, _ in take], [l for _, _, l, _ in take], *keys)
                for s, (rid, _, l, _) in zip(where, take):
                    self.owner[s], self.limit[s] = rid, l
            # (requests that all end at their first token -- limit 1 -- are harvested without a step)
            if any(self.owner[s] is not None and self.limit[s] > 1 for s in range(self.slots)):
                self.engine.steps(self.sync_every)
            fin, steps = self.engine.poll()
            for s in range(self.slots):
                if self.owner[s] is not None and fin[s]:
                    rid, self.owner[s] = self.owner[s], None
                    yield (rid,) + tuple(self.engine.harvest(s, int(steps[s]) + 1))


class ContinuousEngine(DecodeEngine):
    """DecodeEngine's buffers for `slots` rows (group 1) + the per-row counters, the rows' limits and a staging cache of the prompt
    segment's shape.  A slot that was never loaded is finished (frozen) with an empty prompt."""

    def __init__(self, decoder, slots: int, max_prompt_tokens: int, max_new_tokens: int, eos_ids: Sequence[int], pad_id: int, use_graph: bool = True,
                 stream_copy: bool = True, prompt_kv_dtype: Optional[str] = None, lm_head_dtype: Optional[str] = None, output_logits: bool = False,
                 choice: Optional[dict] = None):
        """choice: device_choice's dict (None: the greedy choice alone).  Its processors bring DecodeEngine's processed f32 buffer [slots, ld]
        and the word / eos device arrays, built once; its sampler the draw keys row_key and DecodeEngine's flags word."""
        choice = choice or dict(processors=None, sampling=None, output_scores=False)
        super().__init__(decoder, slots, 1, max_prompt_tokens, max_new_tokens, stream_copy, True, processors=choice["processors"], eos_ids=eos_ids,
                         prompt_kv_dtype=prompt_kv_dtype, lm_head_dtype=lm_head_dtype)
        i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=self.dev)
        self.row_step, self.row_limit = i32(slots, 0), i32(slots, 1)
        self.finished.fill_(LIMIT_BIT)
        self.stage = [torch.zeros_like(t) if t is not None else None for t in (self.k_prompt, self.vt_prompt, self.k_prompt_scale, self.v_prompt_scale)]
        self.stage_lens = torch.zeros((slots,), dtype=torch.int32, device=self.dev)
        self.eos = torch.tensor(list(eos_ids), dtype=torch.int64, device=self.dev)
        self.pad_id, self.use_graph, self.graph, self.steps_run = int(pad_id), bool(use_graph), None, 0
        V = self.spec.vocab_size
        # output_logits: row r's f32 logits of its token n at [r, n]; row G takes what finished rows compute
        self.logit_log = torch.zeros((slots, self.G + 1, V), dtype=torch.float32, device=self.dev) if output_logits else None
        self.all_rows = torch.arange(slots, device=self.dev)
        self.sampling = choice["sampling"]
        self.row_key = torch.zeros((slots,), dtype=torch.int64, device=self.dev)      # the draw key of the request in each slot
        self.warned = set()                                # the flags word's bits already reported
        # output_scores: generate()'s rule -- the sampler's scores, else the processed rows, else the raw logits -- in logit_log's shape,
        # at logit_log's indices; the sampler writes its rows into score_rows first
        self.score_log = torch.zeros((slots, self.G + 1, V), dtype=torch.float32, device=self.dev) if choice["output_scores"] else None
        self.score_rows = torch.zeros((slots, V), dtype=torch.float32, device=self.dev) if (self.score_log is not None and self.sampling) else None

    def _stage_cache(self, k: int):
        """The staging buffers as a cache of exactly k rows (p2t_llama_prefill: cache->B0 == B)."""
        kp, vtp, ks, vs = self.stage
        return _lib.KvCacheC(k_prompt=kp.data_ptr(), vt_prompt=vtp.data_ptr(), k_gen=self.k_gen.data_ptr(), vt_gen=self.vt_gen.data_ptr(),
                             prompt_len=self.stage_lens.data_ptr(), step=self.step.data_ptr(), B0=k, group=1, Tp=self.Tp, G=self.G,
                             k_prompt_scale=ks.data_ptr() if ks is not None else None, v_prompt_scale=vs.data_ptr() if vs is not None else None)

    def _select(self, logits: torch.Tensor, row_map: Optional[torch.Tensor]) -> torch.Tensor:
        """[processors ->] the greedy or the sampled choice of the n logits rows (engine rows row_map, None: all of them, in order) -> the
        rows' scores f32 [n, >= V] in generate()'s sense (read them before the next choice)."""
        n, V, rmap = logits.shape[0], self.spec.vocab_size, ptr(row_map) if row_map is not None else None
        eos = (ptr(self.eos) if self.eos.numel() else None, self.eos.numel(), self.pad_id)
        scores = logits
        if self.processors is not None:
            pr, opt = self.processors, lambda t: ptr(t) if t.numel() else None
            call("p2t_logits_process_rows", ptr(logits), ops.dt_of(logits), logits.stride(0), V, n, ptr(self.out_tokens), self.out_tokens.stride(0),
                 ptr(self.row_step), rmap, ptr(self.finished), self.BB, self.G, ptr(self.processed), self.processed.stride(0), pr["penalty"], pr["ngram"],
                 pr["min_new"], opt(self.proc_eos), self.proc_eos.numel(), opt(self.word_ids), opt(self.word_offsets), len(pr["words"]),
                 self.word_ids.numel(), stream())
            logits = scores = self.processed[:n]
        rows = (ptr(self.finished), ptr(self.next_tokens), ptr(self.out_tokens), self.out_tokens.stride(0), ptr(self.row_step), ptr(self.row_limit), rmap)
        if self.sampling is None:
            call("p2t_greedy_select_rows", ptr(logits), ops.dt_of(logits), logits.stride(0), V, n, *eos, *rows, self.BB, self.G, stream())
            return scores
        sm, sc = self.sampling, self.score_rows
        call("p2t_sample_select_rows", ptr(logits), ops.dt_of(logits), logits.stride(0), V, n, *eos, *rows, ptr(self.row_key), self.BB, self.G,
             sm["temperature"], sm["top_k"], sm["top_p"], sm["seed"] & (2 ** 64 - 1), ptr(sc) if sc is not None else None,
             sc.stride(0) if sc is not None else 0, ptr(self.sample_flags), stream())
        return sc[:n] if sc is not None else scores

    def load(self, slots: Sequence[int], payloads: Sequence[tuple], limits: Sequence[int], keys: Optional[Sequence[int]] = None):
        """payloads: (embeds f32 [T_i, H], mask [T_i]) per request; keys: the requests' draw keys into row_key[slots] (any i64; None: the
        slots keep theirs -- nothing draws).  Compaction + ONE prefill of the k prompts into the staging cache, the
        slot load, the first token's logits on the head the steps use (DecodeEngine.prefill's rule; returned, [k, ld]) and its choice for those rows."""
        k, H = len(slots), self.spec.hidden_size
        T = max(e.shape[0] for e, _ in payloads)
        x = torch.zeros((k, T, H), dtype=torch.float32, device=self.dev)
        m = torch.zeros((k, T), dtype=torch.int64, device=self.dev)
        for i, (e, mk) in enumerate(payloads):
            x[i, : e.shape[0]], m[i, : e.shape[0]] = e.to(device=self.dev, dtype=torch.float32), mk.to(device=self.dev, dtype=torch.int64)
        lens = self.stage_lens[:k]
        embeds, mask = self.compact(x, m, lens=lens)
        stage = self._stage_cache(k)
        logits = self.prefill(embeds, mask, cache=stage)
        call("p2t_kv_slot_load", C.byref(self.e["cfg"]), C.byref(stage), C.byref(self.cache), (C.c_int32 * k)(*[int(s) for s in slots]),
             (C.c_int32 * k)(*[int(l) for l in limits]), k, ptr(self.row_step), ptr(self.finished), ptr(self.row_limit), stream())
        where = torch.tensor([int(s) for s in slots], dtype=torch.int32, device=self.dev)
        if keys is not None:
            self.row_key[where.long()] = torch.tensor([int(v) for v in keys], dtype=torch.int64, device=self.dev)
        if self.logit_log is not None:
            self.logit_log[where.long(), 0] = logits[:, : self.spec.vocab_size].float()
        scores = self._select(logits, where)
        if self.score_log is not None:
            self.score_log[where.long(), 0] = scores[:, : self.spec.vocab_size].float()
        return logits

    def _step_rows(self, frozen: bool = True):
        """One token per row at its own counter; `frozen`: the finished rows stay where they are (False: every row advances)."""
        call("p2t_llama_decode_step_rows", C.byref(self.e["cfg"]), C.byref(self.e["w"]), *self.step_weights(), C.byref(self.cache), ptr(self.x),
             ptr(self.logits), self.ld_logits, self.flags, ptr(self.ws), self.ws.numel(), ptr(self.row_step), ptr(self.finished) if frozen else None, stream())

    def _advance(self):
        self.feed(self.next_tokens)
        self._step_rows()
        if self.logit_log is not None or self.score_log is not None:
            # a live row's logits at its new index (the step advanced it), a finished row's to row G; taken BEFORE the choice sets its bits
            idx = torch.where(self.finished != 0, self.G, self.row_step).long()
        if self.logit_log is not None:
            self.logit_log[self.all_rows, idx] = self.logits[:, : self.spec.vocab_size].float()
        scores = self._select(self.logits, None)
        if self.score_log is not None:                     # (a finished row's scores are not written by the per-row kernels: stale rows, to row G)
            self.score_log[self.all_rows, idx] = scores[:, : self.spec.vocab_size].float()

    def steps(self, n: int):
        for _ in range(n):
            if self.use_graph and self.steps_run >= 1:     # the first step ran eagerly (lazy one-time initialisation inside the library)
                if self.graph is None:
                    self.graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                        self._advance()
                self.graph.replay()
            else:
                self._advance()
            self.steps_run += 1

    def poll(self):
        n = self.BB
        if self.sampling is None:
            both = torch.stack([self.finished, self.row_step]).cpu()  # the one host read per `sync_every` steps
            return both[0].tolist(), both[1].tolist()
        word = torch.cat([self.finished, self.row_step, self.sample_flags]).cpu().tolist()      # ... the sampler's flags word in the same read
        for bit, message in _FLAG_WARNINGS:
            if word[2 * n] & bit and bit not in self.warned:
                self.warned.add(bit)
                warnings.warn(message, RuntimeWarning, stacklevel=2)
        return word[:n], word[n: 2 * n]

    def harvest(self, slot: int, n: int):
        """-> (tokens i64 [n], [logits f32 [n, V]], [scores f32 [n, V]])"""
        out = (self.out_tokens[slot, :n].clone(),)
        if self.logit_log is not None:
            out += (self.logit_log[slot, :n].clone(),)
        if self.score_log is not None:
            out += (self.score_log[slot, :n].clone(),)
        return out


class ContinuousDecoder:
    """Decoding of a queue of prompts over `slots` rows that refill as they finish: greedy, and with `choice="device"` every choice rule
    `generate` serves on the device for one sequence per prompt.

    submit(inputs_embeds [B, T, H], attention_mask [B, T], max_new_tokens=None) -> request ids (one per row; the limit: an int or one
    per row, 1 .. the constructor's max_new_tokens, which is the default).  run() / results() yield (request id, tokens i64 [n]) -- with
    `output_logits` also the f32 logits [n, vocab] -- as requests finish, until none is left; a request's tokens end with its eos when
    one was hit.  Prompts with more than `max_prompt_tokens` tokens under their mask raise ValueError.

    choice=None (default): beam search, sampling, logits processors and output_scores raise NotImplementedError.  choice="device" serves,
    with generate()'s keywords and argument checks: the five logits processors (repetition_penalty, no_repeat_ngram_size, min_new_tokens,
    bad_words_ids, suppress_tokens; the history is the request's own generated tokens), `do_sample=True` with `seed=int` (temperature /
    top_k 1 .. 1024 / top_p, or both filters off; seed=None: ValueError, generator=: NotImplementedError) and `output_scores=True`
    (generate()'s scores -- the sampler's, else the processed rows, else the logits -- f32 [n, vocab], yielded after the logits).  The
    draw of a request's token t is synth.sample_uniform(seed, key, t): submit(..., sample_keys=) gives one integer key per row (any
    i64), by default the request id, and the request's tokens depend on (seed, key, its own logits) alone.  num_beams > 1 and
    num_return_sequences > 1 stay refused."""

    def __init__(self, decoder, slots: int, max_prompt_tokens: int, max_new_tokens: int, eos_token_id=None, pad_token_id: Optional[int] = None,
                 sync_every: int = 8, use_graph: bool = True, stream_copy: bool = True, prompt_kv_dtype: Optional[str] = None,
                 lm_head_dtype: Optional[str] = None, output_logits: bool = False, choice: Optional[str] = None, prefill: Optional[str] = None,
                 pack_tokens: Optional[int] = None, **generate_kwargs):
        if prefill not in (None, "padded") or pack_tokens is not None:
            # generate(prefill="packed"): the refills prefill one to three prompts at a time, so there is little padding to remove
            raise NotImplementedError(f"continuous batching prefills its refills padded: prefill={prefill!r} / pack_tokens={pack_tokens!r} are generate()'s "
                                      "(prefill='packed' is not served here)")
        if choice not in (None, "device"):
            raise ValueError(f"choice must be None or 'device' (got {choice!r})")
        if choice is None:
            refuse_unsupported(**generate_kwargs)
        if slots < 1 or max_prompt_tokens < 1 or max_new_tokens < 1:
            raise ValueError("slots, max_prompt_tokens and max_new_tokens must be >= 1")
        self.decoder, self.slots = decoder, int(slots)
        self.max_prompt_tokens, self.max_new_tokens = int(max_prompt_tokens), int(max_new_tokens)
        self.eos_ids = _as_id_list(eos_token_id)
        self.pad_id = int(pad_token_id) if pad_token_id is not None else (self.eos_ids[0] if self.eos_ids else 0)
        self.choice = device_choice(decoder.spec.vocab_size, self.eos_ids, **generate_kwargs) if choice == "device" else None
        self._engine_args = dict(use_graph=use_graph, stream_copy=stream_copy, prompt_kv_dtype=prompt_kv_dtype, lm_head_dtype=lm_head_dtype,
                                 output_logits=output_logits, choice=self.choice)
        self.scheduler = ContinuousScheduler(_LazyEngine(self), self.slots, sync_every, keyed=self.choice is not None)

    def engine(self) -> ContinuousEngine:
        """The device state, built on first use (submit() checks its arguments without it)."""
        if getattr(self, "_engine", None) is None:
            self._engine = ContinuousEngine(self.decoder, self.slots, self.max_prompt_tokens, self.max_new_tokens, self.eos_ids, self.pad_id,
                                            **self._engine_args)
        return self._engine

    def submit(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, max_new_tokens=None, sample_keys=None) -> List[int]:
        H = self.decoder.spec.hidden_size
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[2] != H:
            raise ValueError(f"inputs_embeds must be [batch, seq_len, {H}]")
        B, T, _ = inputs_embeds.shape
        if attention_mask is None:
            attention_mask = torch.ones((B, T), dtype=torch.int64, device=inputs_embeds.device)
        if tuple(attention_mask.shape) != (B, T):
            raise ValueError(f"attention_mask shape {tuple(attention_mask.shape)} != inputs {(B, T)}")
        lens = attention_mask.ne(0).sum(1).tolist()
        if max(lens) > self.max_prompt_tokens:
            raise ValueError(f"a prompt of {max(lens)} tokens exceeds max_prompt_tokens = {self.max_prompt_tokens}")
        if min(lens) < 1:
            raise ValueError("every prompt row needs at least one token under its attention mask")
        limits = [self.max_new_tokens] * B if max_new_tokens is None else ([int(max_new_tokens)] * B if isinstance(max_new_tokens, int) else
                                                                              [int(v) for v in max_new_tokens])
        if len(limits) != B or any(l < 1 or l > self.max_new_tokens for l in limits):
            raise ValueError(f"max_new_tokens: one limit per row, each in 1 .. {self.max_new_tokens}")
        keys = [None] * B
        if sample_keys is not None:
            if self.choice is None:
                raise ValueError("sample_keys are the draw keys of choice='device'; this decoder chooses greedily")
            keys = list(sample_keys.tolist() if isinstance(sample_keys, torch.Tensor) else sample_keys)
            if len(keys) != B or any(isinstance(k, bool) or not isinstance(k, numbers.Integral) or not -2 ** 63 <= k < 2 ** 63 for k in keys):
                raise ValueError(f"sample_keys: one integer per row ({B}), each a signed 64-bit value")
        return [self.scheduler.submit((inputs_embeds[b], attention_mask[b]), limits[b], keys[b]) for b in range(B)]

    def run(self) -> Iterator[tuple]:
        return self.scheduler.run()

    results = run


class _LazyEngine:
    """The scheduler's engine: the decoder's ContinuousEngine, built when the first load needs it."""

    def __init__(self, owner: ContinuousDecoder):
        self.owner = owner

    def __getattr__(self, name):
        return getattr(self.owner.engine(), name)


class ContinuousGenerator:
    """ContinuousDecoder behind Esm2LlamaInstructForCausalLM: `submit` takes the four tensors `generate` takes and turns them into
    prompt embeddings with `forward(return_decoder_inputs=True)`, per submitted batch."""

    def __init__(self, model, slots: int, max_prompt_tokens: int, max_new_tokens: int, **kwargs):
        self.model = model
        self.decoder = ContinuousDecoder(model.llama_decoder, slots, max_prompt_tokens, max_new_tokens, **kwargs)

    def submit(self, inputs: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, protein_input_ids: Optional[torch.Tensor] = None,
               protein_attention_mask: Optional[torch.Tensor] = None, max_new_tokens=None, protein_inputs_embeds: Optional[torch.Tensor] = None,
               sample_keys=None) -> List[int]:
        with torch.no_grad():
            embeds, mask = self.model(input_ids=inputs, attention_mask=attention_mask, protein_input_ids=protein_input_ids,
                                      protein_attention_mask=protein_attention_mask, protein_inputs_embeds=protein_inputs_embeds, use_cache=False,
                                      output_attentions=False, output_hidden_states=False, return_dict=False, return_decoder_inputs=True)
        return self.decoder.submit(embeds, mask, max_new_tokens, sample_keys)

    def run(self) -> Iterator[tuple]:
        return self.decoder.run()

    results = run
