"""Prompt-lookup decoding for `generate` (HF's `prompt_lookup_num_tokens`; greedy): a decode step reads every weight byte once whatever
the number of rows, and at 1 - 8 prompts most of the 16 MFMA columns of the weight-streaming GEMM compute nothing.  Here a step carries
Q = k + 1 tokens per row -- the token chosen last and a draft of up to k tokens that followed the row's trailing n-gram earlier in its
own generated text -- and keeps the longest prefix of the draft the model agrees with, plus the model's own next token.  The tokens are
greedy decoding's; only the number of steps changes.

What runs where (csrc/lookup.hip, csrc/llama_decode.hip, csrc/attn_decode.hip; include/p2t_hip.h "prompt-lookup decoding"):
  * p2t_lookup_draft_rows: the draft, HF's PromptLookupCandidateGenerator.get_candidates on the row's history out_tokens[r, 0 .. row_step[r]];
  * p2t_llama_embed_tokens on the batch x Q step tokens, then p2t_llama_decode_step_multi: the decode step of batch x Q rows whose rotation
    and cache append run at (row, token) and whose attention is causal among the step's own tokens (p2t_attention_decode_multi);
  * p2t_lookup_verify_rows: the greedy token behind every step token, the accepted prefix, out_tokens / row_step / finished / next_tokens.
A rejected draft token leaves a stale cache entry behind the row's counter: nothing reads it and the next step overwrites it.  The graph
of {draft, embed, step, [logit log], verify} is captured once and replayed; the host reads `finished` every `sync_every` steps.

The row model is ContinuousEngine's (per-row counters row_step, finished bits 1 = eos and 2 = limit, row_limit); the generated segment
holds max_new_tokens + k tokens, so a row near its limit appends its whole step without clamping."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import ops
from ._lib import call
from .generation import DecodeEngine, GenerateOutput, _trim
from .ops import ptr, stream

NUM_TOKENS_MAX, NGRAM_MAX, NGRAM_DEFAULT, STEP_ROWS_MAX = 7, 4, 2, 64


def refuse_unsupported(num_beams, do_sample, processors, output_scores, num_return_sequences) -> None:
    """The modes of generate() that prompt-lookup decoding does not serve, each by name."""
    if num_beams is not None and int(num_beams) > 1:
        raise NotImplementedError("generate(prompt_lookup_num_tokens=): num_beams > 1 is out of scope (the draft is verified against the greedy choice)")
    if do_sample:
        raise NotImplementedError("generate(prompt_lookup_num_tokens=): do_sample is out of scope (speculative sampling is not served; greedy only)")
    if processors is not None:
        raise NotImplementedError("generate(prompt_lookup_num_tokens=): logits processors (repetition_penalty / no_repeat_ngram_size / min_new_tokens / "
                                  "bad_words_ids / suppress_tokens) are out of scope")
    if output_scores:
        raise NotImplementedError("generate(prompt_lookup_num_tokens=): output_scores is out of scope (ask for output_logits: the raw LM-head rows)")
    if num_return_sequences not in (None, 1):
        raise ValueError("greedy decoding returns one sequence per prompt: num_return_sequences > 1 needs do_sample=True or num_beams > 1")


def check_args(spec, batch: int, k, n) -> tuple:
    """-> (k, n) as ints, n defaulted; ValueError outside what the step serves."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= NUM_TOKENS_MAX:
        raise ValueError(f"prompt_lookup_num_tokens must be an integer in 1 .. {NUM_TOKENS_MAX} (got {k!r})")
    n = NGRAM_DEFAULT if n is None else n
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= NGRAM_MAX:
        raise ValueError(f"max_matching_ngram_size must be an integer in 1 .. {NGRAM_MAX} (got {n!r})")
    if batch * (k + 1) > STEP_ROWS_MAX:
        raise ValueError(f"prompt_lookup_num_tokens={k}: {batch} prompts x {k + 1} tokens per step exceed the {STEP_ROWS_MAX} rows of one weight-streaming step")
    if spec.num_attention_heads // spec.num_key_value_heads > 16:
        raise ValueError("prompt_lookup_num_tokens: the multi-token attention serves at most 16 query heads per kv head")
    return k, n


class LookupEngine(DecodeEngine):
    """DecodeEngine's cache for B rows (group 1) with a step of B x (k + 1) rows, the per-row counters and the lookup state."""

    def __init__(self, decoder, B: int, T: int, max_new_tokens: int, k: int, n: int, eos_ids: Sequence[int], pad_id: int, use_graph: bool = True,
                 stream_copy: bool = True, fuse_rope: bool = True, prompt_kv_dtype: Optional[str] = None, lm_head_dtype: Optional[str] = None,
                 output_logits: bool = False):
        k, n = check_args(decoder.spec, B, k, n)
        self.k, self.n, self.Q = k, n, k + 1
        # the generated segment's capacity: a row one short of its limit still appends Q tokens
        super().__init__(decoder, B, 1, T, max_new_tokens + k, stream_copy, fuse_rope, eos_ids=eos_ids, prompt_kv_dtype=prompt_kv_dtype,
                         lm_head_dtype=lm_head_dtype, step_rows=B * self.Q)
        i32 = lambda shape, v: torch.full(shape, v, dtype=torch.int32, device=self.dev)
        self.row_step, self.row_limit = i32((B,), 0), i32((B,), int(max_new_tokens))
        self.eos = torch.tensor(list(eos_ids), dtype=torch.int64, device=self.dev)
        self.pad_id, self.use_graph, self.graph, self.steps_run = int(pad_id), bool(use_graph), None, 0
        self.out_tokens.fill_(self.pad_id)                 # a finished row writes nothing more: what lies behind its last token is pad
        self.step_tokens = torch.full((B, self.Q), self.pad_id, dtype=torch.int64, device=self.dev)
        self.draft_len, self.stats, self.choice = i32((B,), 0), i32((B, 3), 0), i32((B * self.Q,), 0)
        V = self.spec.vocab_size
        # output_logits: the f32 logits that chose row r's token i at [r, i]; rows G + Q .. take what finished rows compute
        self.logit_log = torch.zeros((B, self.G + 2 * self.Q, V), dtype=torch.float32, device=self.dev) if output_logits else None
        self.all_rows = torch.arange(B, device=self.dev)[:, None]
        self.token_offsets = torch.arange(self.Q, device=self.dev)[None, :]

    def first(self, logits: torch.Tensor):
        """The prefill's logits [B, ld] -> token 0 of every row (p2t_greedy_select_rows at row_step 0: its eos and limit bits too)."""
        if self.logit_log is not None:
            self.logit_log[:, 0] = logits[:, : self.spec.vocab_size].float()
        call("p2t_greedy_select_rows", ptr(logits), ops.dt_of(logits), logits.stride(0), self.spec.vocab_size, self.BB,
             ptr(self.eos) if self.eos.numel() else None, self.eos.numel(), self.pad_id, ptr(self.finished), ptr(self.next_tokens), ptr(self.out_tokens),
             self.out_tokens.stride(0), ptr(self.row_step), ptr(self.row_limit), None, self.BB, self.G, stream())

    def draft(self):
        call("p2t_lookup_draft_rows", ptr(self.out_tokens), self.out_tokens.stride(0), ptr(self.row_step), ptr(self.finished), self.BB, self.G, self.k, self.n,
             self.pad_id, ptr(self.step_tokens), ptr(self.draft_len), stream())

    def step_multi(self):
        """Q tokens per row from self.x [B * Q, H] -> self.logits [B * Q, ld]; row_step is read only."""
        call("p2t_llama_decode_step_multi", C.byref(self.e["cfg"]), C.byref(self.e["w"]), *self.step_weights(), C.byref(self.cache), ptr(self.x),
             ptr(self.logits), self.ld_logits, self.flags, ptr(self.ws), self.ws.numel(), ptr(self.row_step), self.Q, stream())

    def verify(self):
        call("p2t_lookup_verify_rows", ptr(self.logits), ops.dt_of(self.logits), self.logits.stride(0), self.spec.vocab_size, self.BB, self.Q,
             ptr(self.step_tokens), ptr(self.draft_len), ptr(self.eos) if self.eos.numel() else None, self.eos.numel(), self.pad_id, ptr(self.finished),
             ptr(self.next_tokens), ptr(self.out_tokens), self.out_tokens.stride(0), ptr(self.row_step), ptr(self.row_limit), self.G, ptr(self.stats),
             ptr(self.choice), stream())

    def _advance(self):
        self.draft()
        call("p2t_llama_embed_tokens", C.byref(self.e["cfg"]), C.byref(self.e["w"]), ptr(self.step_tokens), self.BB * self.Q, ptr(self.x), stream())
        self.step_multi()
        if self.logit_log is not None:
            # logits row (r, j) chooses token row_step[r] + 1 + j; a later step overwrites what a rejected draft left behind.  BEFORE the
            # verification moves the counters; a finished row's rows go behind the segment
            base = torch.where(self.finished != 0, self.G + self.Q, self.row_step + 1).long()
            self.logit_log[self.all_rows, base[:, None] + self.token_offsets] = self.logits.view(self.BB, self.Q, -1)[:, :, : self.spec.vocab_size].float()
        self.verify()

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


def generate_lookup(decoder, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, o):
    """generate()'s greedy loop over LookupEngine; `o`: the call's settings (generation.generate fills them)."""
    B, T, _ = inputs_embeds.shape
    eng = LookupEngine(decoder, B, T, o.max_new_tokens, o.k, o.n, o.eos_ids, o.pad_id, o.use_graph, o.stream_copy, o.fuse_rope, o.prompt_kv_dtype,
                       o.lm_head_dtype, output_logits=bool(o.return_dict and o.output_logits))
    eng.first(eng.prompt(inputs_embeds, attention_mask, o.prefill, o.pack_tokens))
    done, sync = 0, max(int(o.sync_every), 1)
    while done < o.max_new_tokens - 1:                     # every step gives a live row at least one token
        if bool(eng.finished.all().item()):                # the one host read per `sync_every` steps
            break
        todo = min(sync, o.max_new_tokens - 1 - done)
        eng.steps(todo)
        done += todo
    n = int(eng.row_step.max().item()) + 1
    seqs = _trim(eng.out_tokens, o.eos_ids, n)
    if not o.return_dict:
        return seqs
    logits = tuple(eng.logit_log[:, i].clone() for i in range(seqs.shape[1])) if eng.logit_log is not None else None
    return GenerateOutput(seqs, logits=logits, lookup_stats=eng.stats.to(torch.int64).clone())
