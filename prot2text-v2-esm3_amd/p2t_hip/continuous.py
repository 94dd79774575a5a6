"""Continuous batching for greedy `generate`: a fixed number of row SLOTS decode together, every row on its own device-side step
counter, and a slot whose request finished (eos, or the request's own limit) is loaded with the next waiting prompt while the other
rows go on.  `generation.generate` decodes a batch in lock-step until its longest row is done; here no slot waits for another.

What runs where (csrc/llama_decode.hip, csrc/kv_cache.hip, csrc/attn_decode.hip; include/p2t_hip.h "continuous batching"):
  * p2t_llama_decode_step_rows: the decode step with row r at position prompt_len[r] + row_step[r]; `frozen = finished`, so a finished
    (or never loaded) slot re-appends at its own index and stays where it is;
  * p2t_greedy_select_rows: the greedy choice per row, its eos bit (1) and limit bit (2) into `finished`;
  * p2t_kv_slot_load: the k waiting prompts are prefilled TOGETHER into a staging cache (p2t_llama_prefill wants a cache of exactly its
    batch), then one launch copies each row's prompt segment into its slot and resets the slot's counters.
The graph of {embed, step, choice} is captured once and replayed `sync_every` times between two host reads of (finished, row_step);
refills do not invalidate it: every pointer stays and every length lives on the device.

Two layers: ContinuousScheduler is the queue / slot bookkeeping over anything with the engine's four methods (tests drive it with a
stub, without a GPU); ContinuousEngine is the device state; ContinuousDecoder puts them together for a decoder, and
ContinuousGenerator (Esm2LlamaInstructForCausalLM.continuous_generator) runs the encoder + adapter per submitted batch in front."""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Iterator, List, Optional, Sequence

import torch

from . import _lib, ops
from ._lib import call
from .generation import DecodeEngine, _as_id_list
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


class ContinuousScheduler:
    """Requests wait in a queue; free slots take them in order; every `sync_every` steps the finished slots are harvested.

    `engine` provides: load(slots, payloads, limits) -- the payloads' prompts into those slots, first token chosen;
    steps(n) -- n decode steps of every slot; poll() -> (finished [slots], row_step [slots]) as host ints, ONE host read;
    harvest(slot, n) -> a tuple: the slot's first n tokens (and whatever else the engine returns per request)."""

    def __init__(self, engine, slots: int, sync_every: int = 8):
        if slots < 1 or sync_every < 1:
            raise ValueError("slots >= 1 and sync_every >= 1")
        self.engine, self.slots, self.sync_every = engine, int(slots), int(sync_every)
        self.queue = deque()                               # (request id, payload, limit)
        self.owner: List[Optional[int]] = [None] * self.slots
        self.limit = [0] * self.slots                      # the live request's limit per slot
        self.next_id = 0

    def submit(self, payload, limit: int) -> int:
        rid, self.next_id = self.next_id, self.next_id + 1
        self.queue.append((rid, payload, int(limit)))
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
                self.engine.load(where, [p for _, p, _ in take], [l for _, _, l in take])
                for s, (rid, _, l) in zip(where, take):
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
                 stream_copy: bool = True, prompt_kv_dtype: Optional[str] = None, lm_head_dtype: Optional[str] = None, output_logits: bool = False):
        super().__init__(decoder, slots, 1, max_prompt_tokens, max_new_tokens, stream_copy, True, prompt_kv_dtype=prompt_kv_dtype, lm_head_dtype=lm_head_dtype)
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

    def _stage_cache(self, k: int):
        """The staging buffers as a cache of exactly k rows (p2t_llama_prefill: cache->B0 == B)."""
        kp, vtp, ks, vs = self.stage
        return _lib.KvCacheC(k_prompt=kp.data_ptr(), vt_prompt=vtp.data_ptr(), k_gen=self.k_gen.data_ptr(), vt_gen=self.vt_gen.data_ptr(),
                             prompt_len=self.stage_lens.data_ptr(), step=self.step.data_ptr(), B0=k, group=1, Tp=self.Tp, G=self.G,
                             k_prompt_scale=ks.data_ptr() if ks is not None else None, v_prompt_scale=vs.data_ptr() if vs is not None else None)

    def _select(self, logits: torch.Tensor, row_map: Optional[torch.Tensor]):
        call("p2t_greedy_select_rows", ptr(logits), ops.dt_of(logits), logits.stride(0), self.spec.vocab_size, logits.shape[0],
             ptr(self.eos) if self.eos.numel() else None, self.eos.numel(), self.pad_id, ptr(self.finished), ptr(self.next_tokens), ptr(self.out_tokens),
             self.G, ptr(self.row_step), ptr(self.row_limit), ptr(row_map) if row_map is not None else None, self.BB, self.G, stream())

    def load(self, slots: Sequence[int], payloads: Sequence[tuple], limits: Sequence[int]):
        """payloads: (embeds f32 [T_i, H], mask [T_i]) per request.  Compaction + ONE prefill of the k prompts into the staging cache, the
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
        if self.logit_log is not None:
            self.logit_log[where.long(), 0] = logits[:, : self.spec.vocab_size].float()
        self._select(logits, where)
        return logits

    def _step_rows(self, frozen: bool = True):
        """One token per row at its own counter; `frozen`: the finished rows stay where they are (False: every row advances)."""
        call("p2t_llama_decode_step_rows", C.byref(self.e["cfg"]), C.byref(self.e["w"]), *self.step_weights(), C.byref(self.cache), ptr(self.x),
             ptr(self.logits), self.ld_logits, self.flags, ptr(self.ws), self.ws.numel(), ptr(self.row_step), ptr(self.finished) if frozen else None, stream())

    def _advance(self):
        self.feed(self.next_tokens)
        self._step_rows()
        if self.logit_log is not None:                     # a live row's logits at its new index (the step advanced it), a finished row's to row G
            idx = torch.where(self.finished != 0, self.G, self.row_step).long()
            self.logit_log[self.all_rows, idx] = self.logits[:, : self.spec.vocab_size].float()
        self._select(self.logits, None)

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
        both = torch.stack([self.finished, self.row_step]).cpu()      # the one host read per `sync_every` steps
        return both[0].tolist(), both[1].tolist()

    def harvest(self, slot: int, n: int):
        toks = self.out_tokens[slot, :n].clone()
        return (toks, self.logit_log[slot, :n].clone()) if self.logit_log is not None else (toks,)


class ContinuousDecoder:
    """Greedy decoding of a queue of prompts over `slots` rows that refill as they finish.

    submit(inputs_embeds [B, T, H], attention_mask [B, T], max_new_tokens=None) -> request ids (one per row; the limit: an int or one
    per row, 1 .. the constructor's max_new_tokens, which is the default).  run() / results() yield (request id, tokens i64 [n]) -- with
    `output_logits` also the f32 logits [n, vocab] -- as requests finish, until none is left; a request's tokens end with its eos when
    one was hit.  Prompts with more than `max_prompt_tokens` tokens under their mask raise ValueError.  Beam search, sampling, logits
    processors and output_scores are out of scope: NotImplementedError."""

    def __init__(self, decoder, slots: int, max_prompt_tokens: int, max_new_tokens: int, eos_token_id=None, pad_token_id: Optional[int] = None,
                 sync_every: int = 8, use_graph: bool = True, stream_copy: bool = True, prompt_kv_dtype: Optional[str] = None,
                 lm_head_dtype: Optional[str] = None, output_logits: bool = False, **generate_kwargs):
        refuse_unsupported(**generate_kwargs)
        if slots < 1 or max_prompt_tokens < 1 or max_new_tokens < 1:
            raise ValueError("slots, max_prompt_tokens and max_new_tokens must be >= 1")
        self.decoder, self.slots = decoder, int(slots)
        self.max_prompt_tokens, self.max_new_tokens = int(max_prompt_tokens), int(max_new_tokens)
        self.eos_ids = _as_id_list(eos_token_id)
        self.pad_id = int(pad_token_id) if pad_token_id is not None else (self.eos_ids[0] if self.eos_ids else 0)
        self._engine_args = dict(use_graph=use_graph, stream_copy=stream_copy, prompt_kv_dtype=prompt_kv_dtype, lm_head_dtype=lm_head_dtype,
                                 output_logits=output_logits)
        self.scheduler = ContinuousScheduler(_LazyEngine(self), self.slots, sync_every)

    def engine(self) -> ContinuousEngine:
        """The device state, built on first use (submit() checks its arguments without it)."""
        if getattr(self, "_engine", None) is None:
            self._engine = ContinuousEngine(self.decoder, self.slots, self.max_prompt_tokens, self.max_new_tokens, self.eos_ids, self.pad_id,
                                            **self._engine_args)
        return self._engine

    def submit(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, max_new_tokens=None) -> List[int]:
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
        return [self.scheduler.submit((inputs_embeds[b], attention_mask[b]), limits[b]) for b in range(B)]

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
               protein_attention_mask: Optional[torch.Tensor] = None, max_new_tokens=None, protein_inputs_embeds: Optional[torch.Tensor] = None) -> List[int]:
        with torch.no_grad():
            embeds, mask = self.model(input_ids=inputs, attention_mask=attention_mask, protein_input_ids=protein_input_ids,
                                      protein_attention_mask=protein_attention_mask, protein_inputs_embeds=protein_inputs_embeds, use_cache=False,
                                      output_attentions=False, output_hidden_states=False, return_dict=False, return_decoder_inputs=True)
        return self.decoder.submit(embeds, mask, max_new_tokens)

    def run(self) -> Iterator[tuple]:
        return self.decoder.run()

    results = run
