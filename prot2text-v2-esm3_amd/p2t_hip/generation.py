"""`generate` for the decoder half of Esm2LlamaInstructForCausalLM (reference models/modeling_esm2llama_instruct.py:217-251:
prompt embeddings from `forward(return_decoder_inputs=True)`, then `llama_decoder.generate(inputs_embeds=, attention_mask=,
**kwargs)`; call sites scripts/generate_instruct.py:72-87: max_new_tokens, eos_token_id, pad_token_id, num_beams, length_penalty,
temperature, do_sample, top_p, top_k, return_dict_in_generate=False).

What runs where: the prompt compaction, the prefill (all decoder layers + KV-cache write), every decode step (RMSNorm, the
projections, rotation + cache append, single-query attention over the cache, LM head) and the greedy choice are kernels of
libp2t_hip (csrc/llama_decode.hip: the step; csrc/kv_cache.hip, csrc/attn_decode.hip: its cache and attention).  After the first step the greedy loop replays ONE captured HIP graph per token (every length
lives in device memory), and the host looks at the finished flags only every `sync_every` tokens.  Sampling with `seed=` is the same
loop with p2t_sample_select (csrc/sample_select.hip: temperature / top-k / top-p and a counter-hashed draw per row and step) in the
place of the greedy choice, captured and replayed alike.  Beam search selects with p2t_beam_select (csrc/beam_select.hip: log-softmax,
the cut to max(2, 1 + n_eos) * beams candidates, the finished slots, the stop condition and the token tables, all in device memory)
and replays a graph of two steps, since the beam re-ordering swaps two cache buffers (`beam_cache="ancestry"`: no re-ordering copy --
p2t_kv_ancestry_update keeps a table of where each beam's keys lie and p2t_llama_decode_step_beams' attention reads it).  Beam sampling (`num_beams > 1, do_sample=True`
with `seed=` and `beam_select="device"`) is that loop with p2t_beam_sample_select (csrc/beam_sample_select.hip: the warpers on the
log-probabilities and keep draws without replacement as the descending order of score + counter-hashed Gumbel noise).  The logits
processors of `num_beams == 1` (repetition penalty, n-gram, bad-word / suppressed-token and min-new-token bans) are p2t_logits_process
(csrc/logits_process.hip), one launch in front of the greedy / sampled choice inside the same graph: it reads the step's logits and the
rows' own generated history on the device and writes the f32 scores the selector then reads.  Under beam search (opt-in:
`beam_select="device"`) HF runs them on the log-softmax inside the beam step with the beam's running sequence as the history:
p2t_beam_logprobs_process (csrc/beam_process.hip) writes those processed log-probabilities and p2t_beam_select_logprobs ranks them as they
stand, both inside the two-step graph.  Sampling with a torch `generator` (temperature /
top-k / top-p filters + multinomial) and the beam bookkeeping under `beam_select="torch"` or outside the kernel's range (log-softmax,
top-k over beams x vocabulary, gathers of the token tables) are torch device ops on the [rows, vocab] logits -- selection bookkeeping,
restated from transformers/generation/utils.py (`_sample`, `_beam_search` and its helpers) and transformers/generation/
logits_process.py; the decoder arithmetic never goes through torch.

Like HF with `inputs_embeds` only, the returned ids hold the NEW tokens only ([batch, <= max_new_tokens])."""
from __future__ import annotations

import ctypes as C
import warnings
from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from . import _lib, ops
from ._lib import call
from .ops import ptr, round_up, stream


class GenerateOutput:
    """`return_dict_in_generate=True`: the fields of HF's GenerateDecoderOnlyOutput / GenerateBeamDecoderOnlyOutput this path fills."""

    def __init__(self, sequences, scores=None, logits=None, sequences_scores=None, beam_indices=None, lookup_stats=None):
        self.sequences, self.scores, self.logits = sequences, scores, logits
        self.sequences_scores, self.beam_indices = sequences_scores, beam_indices
        self.lookup_stats = lookup_stats                   # prompt_lookup_num_tokens: i64 [batch, 3] = (verify steps, drafted, accepted) per row
        self.past_key_values = None

    def __getitem__(self, k):
        return getattr(self, k)


def _as_id_list(v) -> list:
    if v is None:
        return []
    if isinstance(v, torch.Tensor):
        return [int(x) for x in v.reshape(-1).tolist()]
    if isinstance(v, (list, tuple)):
        return [int(x) for x in v]
    return [int(v)]


# ---------------------------------------------------------------------------------------------------------------------------
# logits filters of the sampling mode (transformers/generation/logits_process.py: TemperatureLogitsWarper, TopKLogitsWarper,
# TopPLogitsWarper; applied in that order by GenerationMixin._get_logits_processor)
# ---------------------------------------------------------------------------------------------------------------------------
def filter_logits(scores: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                  min_tokens_to_keep: int = 1) -> torch.Tensor:
    """f32 [rows, vocab] -> filtered scores (removed entries = -inf)."""
    if temperature is not None and temperature != 1.0:
        if not temperature > 0:
            raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float")
        scores = scores / temperature
    if top_k is not None and top_k > 0:
        k = min(max(int(top_k), min_tokens_to_keep), scores.shape[-1])
        kth = torch.topk(scores, k)[0][..., -1, None]
        scores = scores.masked_fill(scores < kth, -float("inf"))
    if top_p is not None and top_p < 1.0:
        if top_p < 0:
            raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        cumulative = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        remove = cumulative <= (1 - top_p)
        remove[..., -min_tokens_to_keep:] = False
        scores = scores.masked_fill(remove.scatter(1, sorted_indices, remove), -float("inf"))
    return scores


def _sampler_args(temperature, top_k, top_p, seed, generator, device: bool = True):
    """generate()'s (temperature, top_k, top_p) -> the (temperature, k, p) of p2t_sample_select / p2t_beam_sample_select (k = 0 and
    p = 1.0: off), checked up front; `device`: held to the device sampler's range."""
    if seed is not None and generator is not None:
        raise ValueError("generate: pass `seed` (the device sampler) or `generator` (the torch path), not both")
    temperature = 1.0 if temperature is None else float(temperature)
    k = 0 if top_k is None or int(top_k) <= 0 else int(top_k)
    p = 1.0 if top_p is None or float(top_p) >= 1.0 else float(top_p)
    if not (temperature > 0 and temperature < float("inf")):
        raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float")
    if not p > 0:
        raise ValueError(f"`top_p` has to be a float > 0 and < 1, but is {top_p}")
    if device and (k > 1024 or (k == 0 and p < 1.0)):
        raise ValueError(f"generate(seed=): the device sampler serves top_k 1 .. 1024 with top_p on or off, and both filters off (got top_k={top_k}, "
                         f"top_p={top_p}); sample with `generator=` for anything else")
    return temperature, k, p


def _processor_args(V: int, eos_ids: Sequence[int], repetition_penalty, no_repeat_ngram_size, min_new_tokens, bad_words_ids, suppress_tokens):
    """generate()'s logits-processor keywords -> the settings of p2t_logits_process (None: no processor is active), checked up front with
    HF's wording where HF has one (transformers/generation/logits_process.py).  Words: the bad words without any equal to [eos] (HF drops
    them), then every suppressed id as a word of one token."""
    penalty = 1.0 if repetition_penalty is None else repetition_penalty
    if isinstance(penalty, bool) or not isinstance(penalty, (int, float)) or not (penalty > 0 and penalty < float("inf")):
        raise ValueError(f"`penalty` has to be a strictly positive float, but is {repetition_penalty}")
    ngram = 0 if no_repeat_ngram_size is None else no_repeat_ngram_size
    if isinstance(ngram, bool) or not isinstance(ngram, int) or ngram < 0:
        raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {no_repeat_ngram_size}")
    min_new = 0 if min_new_tokens is None else min_new_tokens
    if isinstance(min_new, bool) or not isinstance(min_new, int) or min_new < 0:
        raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {min_new_tokens}")
    words = []
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, list) or len(bad_words_ids) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
        if any(not isinstance(w, list) for w in bad_words_ids):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad_words_ids}.")
        if any(len(w) == 0 or any(isinstance(t, bool) or not isinstance(t, int) or t < 0 for t in w) for w in bad_words_ids):
            raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of positive integers, but is {bad_words_ids}.")
        beyond = [t for w in bad_words_ids for t in w if t >= V]
        if beyond:
            raise ValueError(f"The model vocabulary size is {V}, but the following tokens were being biased: {beyond}")
        words = [list(w) for w in bad_words_ids if all(list(w) != [e] for e in eos_ids)]
    words += [[t] for t in _as_id_list(suppress_tokens)]          # ids outside the vocabulary name no column (HF: torch.isin over arange(V))
    min_new = min_new if eos_ids else 0                           # HF installs MinNewTokensLengthLogitsProcessor only with an eos id
    if float(penalty) == 1.0 and ngram == 0 and min_new == 0 and not words:
        return None
    return dict(penalty=float(penalty), ngram=int(ngram), min_new=int(min_new), words=words)


_FLAG_WARNINGS = ((1, "generate(seed=): more than 2048 logits tied at the top-k boundary of a row; the ties beyond the table were dropped in "
                      "ascending column order (HF would keep them all)"),
                  (2, "generate(seed=): a prompt ran out of continuations with positive probability under beam sampling (HF's torch.multinomial "
                      "fails there); its results are unspecified"))


def _warn_flags(flags: torch.Tensor, warned: set, stacklevel: int) -> None:
    """One host read of a device sampler's flags word; each bit's warning at most once per generate() call (`warned`: the bits already
    reported).  stacklevel: the caller of generate(), counted from the function that calls this one as 2."""
    bits = int(flags.item())
    for bit, message in _FLAG_WARNINGS:
        if bits & bit and bit not in warned:
            warned.add(bit)
            warnings.warn(message, RuntimeWarning, stacklevel=stacklevel)


# ---------------------------------------------------------------------------------------------------------------------------
def preshuffle(w: torch.Tensor, n: int) -> torch.Tensor:
    """bf16 [>= n, K] (or e4m3 bytes as uint8, K % 128 == 0) -> the stream order of the decode GEMM (p2t_preshuffle_w[_fp8]): the
    1 KB one MFMA consumes is contiguous, whole-line loads."""
    K = w.shape[1]
    out = torch.empty((round_up(n, 16) * K,), dtype=w.dtype, device=w.device)
    call("p2t_preshuffle_w_fp8" if w.dtype == torch.uint8 else "p2t_preshuffle_w", ptr(w), w.stride(0), n, K, ptr(out), stream())
    return out


def preshuffle_mxfp4(codes: torch.Tensor, scales: torch.Tensor, n: int) -> torch.Tensor:
    """MXFP4 codes [>= n, K / 2] + block scales [>= n, K / 32] -> the interleaved stream copy of the decode GEMM (p2t_preshuffle_w_mxfp4):
    per 16-row tile and 128-column step the 1 KB of codes one MFMA consumes, then its 64 scale bytes."""
    K = codes.shape[1] * 2
    out = torch.empty((round_up(n, 16) // 16 * (K // 128) * 1088,), dtype=torch.uint8, device=codes.device)
    call("p2t_preshuffle_w_mxfp4", ptr(codes), codes.stride(0), ptr(scales), n, K, ptr(out), stream())
    return out


def mxfp4_layers(e, stream_order: bool):
    """(host array of p2t_llama_layer_mxfp4, tensors to keep alive) from the engine's MXFP4 codes / block scales: row-major, or their
    stream copies."""
    layers, keep = (_lib.LlamaLayerMxfp4C * len(e["mx"]))(), []
    for i, t in enumerate(e["mx"]):
        for name in ("qkv", "o", "gu", "down"):
            codes, bs = t[name + "_w"], t[name + "_bs"]
            if stream_order:
                codes = preshuffle_mxfp4(codes, bs, codes.shape[0])
            keep.append(codes)
            setattr(layers[i], name + "_w", codes.data_ptr())
            setattr(layers[i], name + "_bs", None if stream_order else bs.data_ptr())
        layers[i].stream_order = int(stream_order)
    return layers, keep


def stream_weights(decoder, lm_head: bool = True):
    """Second copies of every decoder projection + the LM head in the stream order, built once per model (dropped with the engine
    when weights are loaded): Llama-3.1-8B: 15 GB next to the 15 GB the prefill reads -- HBM is sized for it.
    lm_head=False (a quantised head serves the steps: generate(lm_head_dtype=)): the bf16 head's copy, 1.05 GB there, is not built --
    st["lm_head"] stays None until a call with lm_head=True wants it."""
    m, s = decoder.model, decoder.spec
    e = m.ensure_engine(s.num_hidden_layers)
    lm = decoder._lm_head_padded()
    # (the engine object is rebuilt when weights are loaded; _version catches an in-place update of the LM head that kept the engine)
    fmt = "mxfp4" if m.gemm_mxfp4 else ("fp8" if m.gemm_fp8 else "model")
    key = (id(e), lm.data_ptr(), lm._version, decoder.model.embed_tokens.weight._version, fmt)
    st = getattr(m, "_stream_engine", None)
    if st is not None and st["key"] == key:
        if lm_head and st["lm_head"] is None:
            st["lm_head"] = preshuffle(lm, s.vocab_size)
        return st
    d, nh, nkv = s.head_dim, s.num_attention_heads, s.num_key_value_heads
    rows = dict(qkv_w=(nh + 2 * nkv) * d, o_w=s.hidden_size, gu_w=2 * s.intermediate_size, down_w=s.hidden_size)
    if m.gemm_mxfp4:       # the stream copies serve the decode step alone (<= 64 rows), and that step reads the 4-bit form: no e4m3 copies
        layers, keep = mxfp4_layers(e, True)
    else:
        layers, keep = (_lib.LlamaLayerStreamC * s.num_hidden_layers)(), []
        for i in range(s.num_hidden_layers):
            t = e["keep"][i]
            for name, n in rows.items():
                w = preshuffle(t[name], n)
                keep.append(w)
                setattr(layers[i], name, w.data_ptr())
    st = dict(key=key, layers=layers, keep=keep, lm_head=preshuffle(lm, s.vocab_size) if lm_head else None)
    m._stream_engine = st
    return st


def lm_head_q(decoder, fmt: str) -> dict:
    """The quantised LM head of generate(lm_head_dtype=fmt), built once per model and kept beside the bf16 head (which still serves
    lm_head_dtype=None, training and, with tied embeddings, the embedding lookup): "fp8" = p2t_quant_rows_fp8 of the padded bf16 head
    (e4m3 codes + one E8M0 byte per vocabulary row), "mxfp4" = p2t_quant_rows_mxfp4 of it (e2m1 codes + one E8M0 byte per 32 columns).
    Keyed like stream_weights: a weight load (new engine) or an in-place update of the head rebuilds it.  The stream-order copy and, for
    "mxfp4", the e4m3 copy of the same values W~ that more than 64 rows read are made on first use (head_q_struct)."""
    m, s = decoder.model, decoder.spec
    e = m.ensure_engine(s.num_hidden_layers)
    lm = decoder._lm_head_padded()
    key = (id(e), lm.data_ptr(), lm._version, decoder.lm_head.weight._version, fmt)
    cache = getattr(m, "_lm_head_q", None)
    if cache is None:
        cache = m._lm_head_q = {}
    st = cache.get(fmt)
    if st is not None and st["key"] == key:
        return st
    H = s.hidden_size
    if fmt == "fp8":
        codes, scales = ops.quant_rows_fp8(lm, H)
    else:
        codes, scales = ops.quant_rows_mxfp4(lm, H)
    st = cache[fmt] = dict(key=key, fmt=fmt, codes=codes, scales=scales, stream=None, e4m3=None)
    return st


def head_q_struct(decoder, st: dict, stream_order: bool, rows: int):
    """(p2t_lm_head_q, what it points to) over lm_head_q's tensors: the stream-order copy (at most 64 rows, never the general GEMM) or
    the row-major codes, plus, for an MXFP4 head read by more than 64 rows, the e4m3 codes of the dequantised head."""
    V, H = decoder.spec.vocab_size, decoder.spec.hidden_size
    mx = st["fmt"] == "mxfp4"
    d = _lib.LmHeadQC(format=_lib.LM_HEAD_MXFP4 if mx else _lib.LM_HEAD_E4M3, stream_order=int(stream_order), ld=st["codes"].stride(0))
    if stream_order:
        if st["stream"] is None:
            st["stream"] = preshuffle_mxfp4(st["codes"], st["scales"], V) if mx else preshuffle(st["codes"], V)
        d.codes, d.scales = st["stream"].data_ptr(), None if mx else st["scales"].data_ptr()
    else:
        d.codes, d.scales = st["codes"].data_ptr(), st["scales"].data_ptr()
    if mx and rows > 64:
        if st["e4m3"] is None:        # W~ is e4m3-exact under one row scale (include/p2t_hip.h, "MXFP4 decoder weights"): the projections' rule
            st["e4m3"] = ops.quant_rows_fp8(ops.dequant_rows_mxfp4(st["codes"], st["scales"], H, round_up(H, 64)), H)
        d.codes_e4m3, d.scales_e4m3 = st["e4m3"][0].data_ptr(), st["e4m3"][1].data_ptr()
    return d, st


def lm_head_logits_q(x: torch.Tensor, norm_w: Optional[torch.Tensor], eps: float, head, vocab: int, ld_logits: Optional[int] = None,
                     return_act: bool = False, out: Optional[torch.Tensor] = None):
    """p2t_lm_head_logits_q: x f32 [M, hidden] (the residual stream; norm_w None: rows that are normalised already) -> logits bf16
    [M, ld_logits] on the quantised head `head` (_lib.LmHeadQC); return_act: also the e4m3 rows [M, Kq] and their E8M0 bytes [M] that
    the GEMM read.  `out`: write into this buffer (columns vocab .. are left as they are)."""
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise ValueError("lm_head_logits_q: x must be f32 [rows, hidden], row-major")
    M, H = x.shape
    ld = round_up(vocab, 64) if ld_logits is None else ld_logits
    if out is None:
        out = torch.zeros((M, ld), dtype=torch.bfloat16, device=x.device)
    aq = torch.empty((M, round_up(H, 128)), dtype=torch.uint8, device=x.device) if return_act else None
    asc = torch.empty((M,), dtype=torch.uint8, device=x.device) if return_act else None
    ws = None if return_act else torch.empty((call("p2t_lm_head_q_workspace_bytes", M, H),), dtype=torch.uint8, device=x.device)
    call("p2t_lm_head_logits_q", ptr(x), x.stride(0), ptr(norm_w), float(eps), C.byref(head), M, H, int(vocab), ptr(out), out.stride(0), ops.dt_of(out),
         ptr(aq), ptr(asc), ptr(ws), ws.numel() if ws is not None else 0, stream())
    return (out, aq, asc) if return_act else out


# A guard on buffer sizes, not a tuned value: one packed row of every prompt is the default, and beyond this many tokens the prompts go
# into rows of at most this many (the tower's workspace grows with rows x tokens either way; a row's attention tiles with its length).
PACK_TOKENS_MAX = 32768
# Tpk is a multiple of 64: the attention kernels walk a row's keys in 64-key tiles and p2t_kv_store_packed moves 64-key tiles, so a row
# that ends on a tile edge never has a partial tile behind its last prompt; the 128-query tile of the bf16 attention clamps by itself.
PACK_ROW_MULTIPLE = 64
PACK_PROMPTS_MAX = 256                                       # p2t_llama_prefill_packed: the placement travels in the launch arguments


def plan_prompt_rows(lens: Sequence[int], pack_tokens: Optional[int] = None):
    """Where the prompts of a packed prompt batch lie (include/p2t_hip.h, p2t_pack_rows): lens[b] valid tokens per prompt ->
    (R, Tpk, place) with place[b] = (row, start, len) in batch order.  First-fit decreasing, as data.pack_instruct_batch packs its
    samples: longest first, ties in batch order, each prompt into the first row with room, the prompts of a row back to back from token
    0.  `pack_tokens`: the rows' capacity; None = PACK_TOKENS_MAX, i.e. ONE row holding every prompt unless they exceed it.  Tpk = the
    fullest row rounded up to PACK_ROW_MULTIPLE.  A prompt longer than the capacity, or an empty one, raises ValueError."""
    lens = [int(n) for n in lens]
    cap = PACK_TOKENS_MAX if pack_tokens is None else int(pack_tokens)
    if not lens or cap < 1:
        raise ValueError("plan_prompt_rows: at least one prompt and pack_tokens >= 1")
    for b, n in enumerate(lens):
        if n < 1:
            raise ValueError("every prompt row needs at least one token under its attention mask")
        if n > cap:
            raise ValueError(f"prompt {b} has {n} tokens, more than pack_tokens = {cap}")
    used: list = []
    place: list = [None] * len(lens)
    for b in sorted(range(len(lens)), key=lambda i: -lens[i]):          # stable: ties keep the batch order
        r = next((r for r in range(len(used)) if cap - used[r] >= lens[b]), len(used))
        if r == len(used):
            used.append(0)
        place[b] = (r, used[r], lens[b])
        used[r] += lens[b]
    return len(used), round_up(max(used), PACK_ROW_MULTIPLE), place


class PackedPrompts:
    """What DecodeEngine.pack returns: embeds f32 [R, Tpk, H], mask i64 [R, Tpk], docs i32 [2, R, Tpk] (p2t_doc_prepare) and the placement."""

    def __init__(self, embeds, mask, position_ids, docs, place):
        self.embeds, self.mask, self.position_ids, self.docs, self.place = embeds, mask, position_ids, docs, place
        self.c_place = (C.c_int32 * (3 * len(place)))(*[v for p in place for v in p])


class DecodeEngine:
    """Cache + buffers of ONE generate() call: B0 prompts, `group` rows per prompt (beams), capacities Tp / G (multiples of 64).
    `step_rows` (None: B0 * group): the rows a decode step carries where that is more than the cache's -- several tokens per row
    (lookup.LookupEngine): the step's x / logits / workspace and the row limits of the weight forms are sized by it."""

    def __init__(self, decoder, B0: int, group: int, T: int, max_new_tokens: int, stream_copy: bool = True, fuse_rope: bool = True,
                 processors: Optional[dict] = None, eos_ids: Sequence[int] = (), prompt_kv_dtype: Optional[str] = None,
                 lm_head_dtype: Optional[str] = None, beam_cache: Optional[str] = None, step_rows: Optional[int] = None):
        m, s = decoder.model, decoder.spec
        rows = B0 * group if step_rows is None else int(step_rows)
        if beam_cache not in (None, "ancestry"):
            raise ValueError(f"beam_cache must be None or 'ancestry' (got {beam_cache!r})")
        if beam_cache is not None and not (2 <= group <= BEAMS_MAX and s.num_attention_heads // s.num_key_value_heads <= 16):
            raise ValueError(f"beam_cache='ancestry' serves 2 .. {BEAMS_MAX} rows per prompt and at most 16 query heads per kv head (got {group} rows, "
                             f"{s.num_attention_heads // s.num_key_value_heads} heads)")
        if prompt_kv_dtype not in (None, "fp8"):
            raise ValueError(f"prompt_kv_dtype must be None or 'fp8' (got {prompt_kv_dtype!r})")
        if prompt_kv_dtype == "fp8" and m.dtype != torch.bfloat16:
            raise ValueError("prompt_kv_dtype='fp8' (the e4m3 prompt segment of the KV cache) serves bf16 models only")
        if lm_head_dtype not in (None, "fp8", "mxfp4"):
            raise ValueError(f"lm_head_dtype must be None, 'fp8' or 'mxfp4' (got {lm_head_dtype!r})")
        if lm_head_dtype is not None and m.dtype != torch.bfloat16:
            raise ValueError(f"lm_head_dtype={lm_head_dtype!r} (the quantised LM head of the decode step) serves bf16 models only")
        if lm_head_dtype is not None and rows > 64 and s.vocab_size % 16:
            raise ValueError(f"lm_head_dtype={lm_head_dtype!r} with more than 64 rows (got {rows}) runs the general fp8 GEMM, which serves a "
                             f"vocabulary that is a multiple of 16 only (got {s.vocab_size})")
        self.flags = 0 if fuse_rope else 1          # P2T_DECODE_NO_ROPE_FUSION
        if s.hidden_size % 64:
            raise ValueError("the LM head path needs hidden_size % 64 == 0")
        self.decoder, self.spec, self.dtype = decoder, s, m.dtype
        self.dev = m.embed_tokens.weight.device
        self.e = m.ensure_engine(s.num_hidden_layers)
        self.B0, self.group, self.BB = B0, group, B0 * group
        self.Tp, self.G = round_up(max(T, 1), 64), round_up(max(max_new_tokens, 1), 64)
        L, nkv, dp = s.num_hidden_layers, s.num_key_value_heads, ops.head_dim_padded(s.head_dim)
        z = lambda *shape: torch.zeros(shape, dtype=self.dtype, device=self.dev)
        # the prompt segment: model dtype, or (prompt_kv_dtype="fp8") e4m3 codes in the same index order + one E8M0 byte per key for K and
        # for V (include/p2t_hip.h, p2t_kv_cache): the prefill quantises on its store, the step's attention reads half the bytes
        self.k_prompt_scale = self.v_prompt_scale = None
        if prompt_kv_dtype == "fp8":
            z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=self.dev)
            self.k_prompt, self.vt_prompt = z8(L, B0, nkv, self.Tp, dp), z8(L, B0, nkv, dp, self.Tp)
            self.k_prompt_scale, self.v_prompt_scale = z8(L, B0, nkv, self.Tp), z8(L, B0, nkv, self.Tp)
        else:
            self.k_prompt, self.vt_prompt = z(L, B0, nkv, self.Tp, dp), z(L, B0, nkv, dp, self.Tp)
        self.k_gen, self.vt_gen = z(L, self.BB, nkv, self.G, dp), z(L, self.BB, nkv, dp, self.G)
        self.k_alt = self.vt_alt = None                                  # second generated segment, beam search only
        # beam_cache="ancestry": the generated keys stay in the rows that wrote them, and this table says where a beam's history lies
        # (include/p2t_hip.h, p2t_kv_ancestry_update); reorder() is never called, k_alt / vt_alt are never allocated
        self.ancestry = torch.zeros((B0 * group, self.G), dtype=torch.uint8, device=self.dev) if beam_cache is not None else None
        self.lens = torch.zeros((B0,), dtype=torch.int32, device=self.dev)
        self.step = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.ld_logits = round_up(s.vocab_size, 64)
        self.logits = torch.zeros((rows, self.ld_logits), dtype=self.dtype, device=self.dev)
        self.x = torch.zeros((rows, s.hidden_size), dtype=torch.float32, device=self.dev)
        self.next_tokens = torch.zeros((self.BB,), dtype=torch.int64, device=self.dev)
        self.finished = torch.zeros((self.BB,), dtype=torch.int32, device=self.dev)
        self.sample_flags = torch.zeros((1,), dtype=torch.int32, device=self.dev)      # p2t_sample_select ORs into it (bit 0: table full)
        self.out_tokens = torch.zeros((self.BB, self.G), dtype=torch.int64, device=self.dev)
        self.ws = torch.empty((call("p2t_llama_decode_workspace_bytes", C.byref(self.e["cfg"]), rows, self.Tp, self.G),), dtype=torch.uint8,
                              device=self.dev)
        self.lm_head = decoder._lm_head_padded()
        # the stream-order copies are read by the skinny GEMMs only (<= 64 rows): beyond that every projection and the LM head
        # run on the row-major weights (the LM head had no row-major fallback and returned wrong logits)
        self.stream = stream_weights(decoder, lm_head=lm_head_dtype is None) if (stream_copy and self.dtype == torch.bfloat16 and rows <= 64) else None
        # "mxfp4" decoders: up to 64 rows step on the 4-bit weights (their stream copies, or row-major under stream_copy=False);
        # beyond that the e4m3 copies of the same values serve, as in "fp8" mode
        self.mx = None                                                    # (host array of p2t_llama_layer_mxfp4, what it points to)
        if m.gemm_mxfp4 and rows <= 64:
            self.mx = (self.stream["layers"], self.stream["keep"]) if self.stream else mxfp4_layers(self.e, False)
        # lm_head_dtype: the final RMSNorm + LM head of the prefill's first token AND of every step on ONE quantised head (p2t_lm_head_q);
        # its stream-order copy under the bf16 copies' condition (stream_copy, at most 64 rows), row-major e4m3 codes beyond 64 rows.
        # None: nothing built, nothing allocated, p2t_llama_decode_step[_mxfp4] as ever
        self.head_q = self.head_q_first = None
        if lm_head_dtype is not None:
            st = lm_head_q(decoder, lm_head_dtype)
            self.head_q = head_q_struct(decoder, st, stream_copy and rows <= 64, rows)
            self.head_q_first = head_q_struct(decoder, st, stream_copy and B0 <= 64, B0)      # the prefill's B0 rows
            self.ws = torch.empty((self.ws.numel() + call("p2t_lm_head_q_workspace_bytes", rows, s.hidden_size),), dtype=torch.uint8, device=self.dev)
        self._cache_struct()
        self.processors = processors                                      # _processor_args' settings, or None: nothing allocated, nothing launched
        if processors is not None:
            i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=self.dev)
            lens = [len(w) for w in processors["words"]]
            self.processed = torch.zeros((self.BB, self.ld_logits), dtype=torch.float32, device=self.dev)
            self.proc_eos = i64(list(eos_ids)) if processors["min_new"] > 0 else i64([])
            self.word_ids = i64([t for w in processors["words"] for t in w])
            self.word_offsets = torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32, device=self.dev)

    def _cache_struct(self):
        self.cache = _lib.KvCacheC(k_prompt=self.k_prompt.data_ptr(), vt_prompt=self.vt_prompt.data_ptr(), k_gen=self.k_gen.data_ptr(),
                                   vt_gen=self.vt_gen.data_ptr(), prompt_len=self.lens.data_ptr(), step=self.step.data_ptr(), B0=self.B0,
                                   group=self.group, Tp=self.Tp, G=self.G,
                                   k_prompt_scale=self.k_prompt_scale.data_ptr() if self.k_prompt_scale is not None else None,
                                   v_prompt_scale=self.v_prompt_scale.data_ptr() if self.v_prompt_scale is not None else None)

    # -- prompt -------------------------------------------------------------------------------------------------------------
    def compact(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, lens: Optional[torch.Tensor] = None):
        """Valid tokens first (positions = HF's cumsum(mask) - 1 on them); -> (embeds, prefix mask) trimmed to the longest row.
        `lens` (i32 [B], device): receives the rows' lengths in the cache's own prompt_len's place (a staging cache's)."""
        lens = self.lens if lens is None else lens
        B, T, H = inputs_embeds.shape
        x = inputs_embeds.to(device=self.dev, dtype=torch.float32).contiguous()
        mask = attention_mask.to(device=self.dev, dtype=torch.int64).contiguous()
        out, out_mask = torch.empty_like(x), torch.empty_like(mask)
        scratch = torch.empty((B * T,), dtype=torch.int32, device=self.dev)
        call("p2t_compact_rows", ptr(x), ptr(mask), B, T, H, ptr(out), ptr(out_mask), ptr(lens), ptr(scratch), stream())
        longest = int(lens.max().item())                            # the one host read of the prompt phase
        if longest < 1:
            raise ValueError("every prompt row needs at least one token under its attention mask")
        if longest < T:
            out, out_mask = out[:, :longest].contiguous(), out_mask[:, :longest].contiguous()
        return out, out_mask

    def prefill(self, embeds: torch.Tensor, mask: torch.Tensor, cache=None) -> torch.Tensor:
        """-> logits of the first new token, model dtype [B0, ld] (row b from prompt b's last valid token).  `cache`: another
        p2t_kv_cache of exactly the batch's rows than the engine's own (continuous batching's staging cache)."""
        B, T, H = embeds.shape
        cfg = self.e["cfg"]
        ws = torch.empty((call("p2t_llama_prefill_workspace_bytes", C.byref(cfg), B, T),), dtype=torch.uint8, device=self.dev)
        last = torch.empty((B, H), dtype=torch.float32, device=self.dev)
        call("p2t_llama_prefill", C.byref(cfg), C.byref(self.e["w"]), ptr(embeds), ptr(mask), B, T, C.byref(self.cache if cache is None else cache), ptr(last), ptr(ws),
             ws.numel(), stream())
        return self._first_logits(last)

    def _first_logits(self, last: torch.Tensor) -> torch.Tensor:
        """The first new token's logits from the prompts' last normalised hidden rows f32 [B0, H]."""
        if self.head_q_first is not None:        # token 0 is scored by the matrix that scores token 1: the normalised rows, quantised, on the same head
            return lm_head_logits_q(last, None, 0.0, self.head_q_first[0], self.spec.vocab_size, self.ld_logits)
        a = last if self.dtype == torch.float32 else ops.cast(last, self.dtype)
        return ops.gemm_nt(a, self.lm_head, None, n=self.spec.vocab_size, k=last.shape[1], out_dtype=self.dtype)

    def pack(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, pack_tokens: Optional[int] = None) -> PackedPrompts:
        """compact()'s counterpart for the padding-free prefill: the prompts back to back in a few long rows (plan_prompt_rows), each in
        compact()'s token order with positions restarting at 0, straight from the original rows (p2t_prompt_index + p2t_pack_rows), and
        the rows' documents (p2t_doc_prepare).  The cache's prompt_len receives the lengths."""
        B, T, H = inputs_embeds.shape
        if self.decoder.model.gemm_fp8:
            raise ValueError("prefill='packed' runs the model-dtype GEMMs: it does not serve set_gemm_dtype('fp8') / ('mxfp4') models")
        if B > PACK_PROMPTS_MAX:
            raise ValueError(f"prefill='packed' serves at most {PACK_PROMPTS_MAX} prompts per call (got {B})")
        x = inputs_embeds.to(device=self.dev, dtype=torch.float32).contiguous()
        mask = attention_mask.to(device=self.dev, dtype=torch.int64).contiguous()
        index = torch.empty((B * T,), dtype=torch.int32, device=self.dev)
        call("p2t_prompt_index", ptr(mask), B, T, ptr(index), ptr(self.lens), stream())
        R, Tpk, place = plan_prompt_rows(self.lens.tolist(), pack_tokens)      # the one host read of the prompt phase: the B lengths
        out = torch.empty((R, Tpk, H), dtype=torch.float32, device=self.dev)
        out_mask = torch.empty((R, Tpk), dtype=torch.int64, device=self.dev)
        pos = torch.empty((R, Tpk), dtype=torch.int32, device=self.dev)
        packed = PackedPrompts(out, out_mask, pos, torch.empty((2, R, Tpk), dtype=torch.int32, device=self.dev), place)
        call("p2t_pack_rows", ptr(x), ptr(index), ptr(self.lens), B, T, H, packed.c_place, R, Tpk, ptr(out), ptr(out_mask), ptr(pos), stream())
        flags = torch.empty((1,), dtype=torch.int32, device=self.dev)          # (zeroed by the call; the rows are well-formed by construction)
        call("p2t_doc_prepare", ptr(pos), 0, ptr(out_mask), R, Tpk, ptr(packed.docs), ptr(flags), stream())
        return packed

    def prefill_packed(self, packed: PackedPrompts) -> torch.Tensor:
        """prefill() on a packed prompt batch: the same layers over R x Tpk tokens instead of B0 x longest, every layer's keys and values
        scattered to each prompt's own row of the prompt segment (p2t_llama_prefill_packed) -> the first new token's logits, as prefill."""
        R, Tpk, H = packed.embeds.shape
        cfg = self.e["cfg"]
        ws = torch.empty((call("p2t_llama_prefill_packed_workspace_bytes", C.byref(cfg), R, Tpk),), dtype=torch.uint8, device=self.dev)
        last = torch.empty((self.B0, H), dtype=torch.float32, device=self.dev)
        call("p2t_llama_prefill_packed", C.byref(cfg), C.byref(self.e["w"]), ptr(packed.embeds), ptr(packed.mask), ptr(packed.docs), R, Tpk, len(packed.place),
             packed.c_place, C.byref(self.cache), ptr(last), ptr(ws), ws.numel(), stream())
        return self._first_logits(last)

    def prompt(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, prefill: Optional[str] = None, pack_tokens: Optional[int] = None):
        """The prompt phase of generate(): compact + prefill, or (prefill="packed") pack + prefill_packed -> the first token's logits."""
        if prefill == "packed":
            return self.prefill_packed(self.pack(inputs_embeds, attention_mask, pack_tokens))
        return self.prefill(*self.compact(inputs_embeds, attention_mask))

    # -- steps --------------------------------------------------------------------------------------------------------------
    def feed(self, tokens: torch.Tensor):
        """x <- embedding rows of the chosen tokens (i64 [BB], device)."""
        call("p2t_llama_embed_tokens", C.byref(self.e["cfg"]), C.byref(self.e["w"]), ptr(tokens), self.BB, ptr(self.x), stream())

    def step_weights(self):
        """-> (w_stream, mx_layers, lm_head, ld_head, lm_head_preshuffled, head_q) for every door of the step: stream-order copies or MXFP4 layers
        (never both) or neither; the model-dtype head (its stream copy where there is one) or the quantised head's descriptor in its place."""
        st = self.stream
        layers = C.cast(st["layers"], C.POINTER(_lib.LlamaLayerStreamC)) if (st and self.mx is None) else None
        mx = C.cast(self.mx[0], C.POINTER(_lib.LlamaLayerMxfp4C)) if self.mx is not None else None
        if self.head_q is not None:
            return layers, mx, None, self.lm_head.stride(0), 0, C.byref(self.head_q[0])
        return layers, mx, ptr(st["lm_head"] if st else self.lm_head), self.lm_head.stride(0), int(st is not None), None

    def decode_step(self):
        """One token per row from self.x -> self.logits; the device step counter advances."""
        layers, mx, head, ld_head, pre, hq = self.step_weights()
        rest = (C.byref(self.cache), ptr(self.x), ptr(self.logits), self.ld_logits, self.flags, ptr(self.ws), self.ws.numel(), stream())
        if self.ancestry is not None:
            call("p2t_llama_decode_step_beams", C.byref(self.e["cfg"]), C.byref(self.e["w"]), layers, mx, head, ld_head, pre, hq, *rest[:-1], ptr(self.ancestry),
                 stream())
        elif hq is not None:
            call("p2t_llama_decode_step_q", C.byref(self.e["cfg"]), C.byref(self.e["w"]), layers, mx, head, ld_head, pre, hq, *rest)
        elif mx is not None:
            call("p2t_llama_decode_step_mxfp4", C.byref(self.e["cfg"]), C.byref(self.e["w"]), mx, head, ld_head, pre, *rest)
        else:
            call("p2t_llama_decode_step", C.byref(self.e["cfg"]), C.byref(self.e["w"]), layers, head, ld_head, pre, *rest)

    def greedy_select(self, logits: torch.Tensor, eos: torch.Tensor, pad_id: int):
        call("p2t_greedy_select", ptr(logits), ops.dt_of(logits), logits.stride(0), self.spec.vocab_size, self.BB, ptr(eos) if eos.numel() else None,
             eos.numel(), int(pad_id), ptr(self.finished), ptr(self.next_tokens), ptr(self.out_tokens), self.G, ptr(self.step), self.G, stream())

    def sample_select(self, logits: torch.Tensor, eos: torch.Tensor, pad_id: int, temperature: float, top_k: int, top_p: float, seed: int,
                      scores: Optional[torch.Tensor] = None, row0: int = 0):
        """The sampled choice in the greedy one's place: row r draws as row0 + r at the device step counter (include/p2t_hip.h)."""
        call("p2t_sample_select", ptr(logits), ops.dt_of(logits), logits.stride(0), self.spec.vocab_size, self.BB, ptr(eos) if eos.numel() else None,
             eos.numel(), int(pad_id), ptr(self.finished), ptr(self.next_tokens), ptr(self.out_tokens), self.G, ptr(self.step), self.G,
             float(temperature), int(top_k), float(top_p), int(seed) & (2 ** 64 - 1), int(row0), ptr(scores) if scores is not None else None,
             scores.stride(0) if scores is not None else 0, ptr(self.sample_flags), stream())

    def process(self, logits: torch.Tensor, history: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The logits processors on the step's logits and the rows' own history out_tokens[:, : step[0]] (p2t_logits_process, inside the
        step graph like the selectors) -> the processed f32 buffer the selectors then read; `logits` stays as it is.  `history` (i64
        [BB, n], contiguous) and `step` (a device word): another token table and counter than the engine's own -- the torch beam path's
        running sequences, with the f32 log-probabilities as `logits`."""
        pr, opt = self.processors, lambda t: ptr(t) if t.numel() else None
        history, step = self.out_tokens if history is None else history, self.step if step is None else step
        call("p2t_logits_process", ptr(logits), ops.dt_of(logits), logits.stride(0), self.spec.vocab_size, self.BB, ptr(history),
             history.stride(0), ptr(step), history.shape[1], ptr(self.processed), self.processed.stride(0), pr["penalty"], pr["ngram"],
             pr["min_new"], opt(self.proc_eos), self.proc_eos.numel(), opt(self.word_ids), opt(self.word_offsets), len(pr["words"]),
             self.word_ids.numel(), stream())
        return self.processed

    def beam_process(self, logits: torch.Tensor, state: "BeamState", max_length: int, lp: torch.Tensor):
        """The logits processors under beam search (p2t_beam_logprobs_process, inside the step graph): log-softmax of the step's logits,
        processed with each beam's running sequence state.run_seq[step[0] & 1] as its history, into the f32 rows `lp`."""
        pr, opt = self.processors, lambda t: ptr(t) if t.numel() else None
        call("p2t_beam_logprobs_process", ptr(logits), ops.dt_of(logits), logits.stride(0), state.B, state.nb, self.spec.vocab_size, ptr(self.step),
             state.G, int(max_length), C.byref(state.c), pr["penalty"], pr["ngram"], pr["min_new"], opt(self.proc_eos), self.proc_eos.numel(),
             opt(self.word_ids), opt(self.word_offsets), len(pr["words"]), self.word_ids.numel(), ptr(lp), lp.stride(0), stream())

    def ancestry_update(self, src_rows: torch.Tensor):
        """beam_cache="ancestry": row r's history is row src_rows[r]'s, and its next key its own (in reorder's place; one launch, no copy)."""
        call("p2t_kv_ancestry_update", C.byref(self.cache), ptr(src_rows), ptr(self.ancestry), stream())

    def reorder(self, src_rows: torch.Tensor):
        """Generated segment row r <- row src_rows[r] (beam re-ordering; the prompt segment is shared by a prompt's beams)."""
        if self.k_alt is None:
            self.k_alt, self.vt_alt = torch.zeros_like(self.k_gen), torch.zeros_like(self.vt_gen)
        call("p2t_kv_reorder", C.byref(self.e["cfg"]), C.byref(self.cache), ptr(src_rows.to(torch.int64).contiguous()), ptr(self.k_alt),
             ptr(self.vt_alt), stream())
        self.k_gen, self.k_alt, self.vt_gen, self.vt_alt = self.k_alt, self.k_gen, self.vt_alt, self.vt_gen
        self._cache_struct()


def _trim(tokens: torch.Tensor, eos_ids: Sequence[int], n: int) -> torch.Tensor:
    """HF stops right after the step in which the last row finishes: cut the columns produced after that."""
    tokens = tokens[:, :n]
    if not eos_ids or n == 0:
        return tokens
    hit = torch.zeros_like(tokens, dtype=torch.bool)
    for e in eos_ids:
        hit |= tokens == e
    first = torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.full((tokens.shape[0],), n, device=tokens.device))
    return tokens[:, : int(first.max().item())]


@torch.no_grad()
def generate(decoder, inputs_embeds: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None, *,
             input_ids: Optional[torch.Tensor] = None, max_new_tokens: Optional[int] = None, max_length: Optional[int] = None,
             eos_token_id=None, pad_token_id: Optional[int] = None, do_sample: bool = False, temperature: Optional[float] = 1.0,
             top_k: Optional[int] = 50, top_p: Optional[float] = 1.0, num_beams: int = 1, length_penalty: float = 1.0,
             early_stopping=False, num_return_sequences: int = 1, return_dict_in_generate: bool = False, output_scores: bool = False,
             output_logits: bool = False, use_graph: bool = True, sync_every: int = 16, generator: Optional[torch.Generator] = None,
             stream_copy: bool = True, fuse_rope: bool = True, seed: Optional[int] = None, beam_select: Optional[str] = None,
             repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, min_new_tokens: Optional[int] = None,
             bad_words_ids: Optional[list] = None, suppress_tokens=None, prompt_kv_dtype: Optional[str] = None,
             lm_head_dtype: Optional[str] = None, beam_cache: Optional[str] = None, prefill: Optional[str] = None,
             pack_tokens: Optional[int] = None, prompt_lookup_num_tokens: Optional[int] = None,
             max_matching_ngram_size: Optional[int] = None, **unused):
    """`LlamaForCausalLM.generate` for prompts given as embeddings (or ids): greedy, sampling (temperature / top-k / top-p) and beam
    search with length penalty.  Returns the new token ids i64 [batch * num_return_sequences, n] (or a GenerateOutput).

    Sampling draws from torch's `generator` stream with torch ops on the logits (`seed=None`), or, with `seed=int`, on the device
    (p2t_sample_select) inside the replayed step graph: row b * num_return_sequences + r at step n draws
    synth.sample_uniform(seed, row, n), whatever else the batch holds.  The device path serves top_k 1 .. 1024 with top_p on or off, and
    both filters off; it also returns the processed scores (`output_scores=True`).  `seed` is ignored under greedy decoding.

    Beam sampling (`num_beams > 1, do_sample=True`: HF's beam-search multinomial sampling) is opt-in: `seed=int` with
    `beam_select="device"` runs p2t_beam_sample_select in the beam search's loop and graph (prompt b draws as prompt b at the device step
    counter: synth.beam_sample_uniform; top_k 0 or max(2, 1 + number of eos ids) * num_beams .. 1024, top_p only with top_k), and
    `generator=` with `beam_select="torch"` runs the torch restatement of HF's two lines (torch.multinomial without replacement).  Every
    other form of that call raises NotImplementedError.

    Beam search (`num_beams > 1`) selects on the device as well (p2t_beam_select, two launches per token) and, with `use_graph`, replays
    a captured graph of two steps; the host reads the search's `done` word every `sync_every` tokens.  `beam_select`: None (default) =
    the device path wherever it applies (num_beams <= 16, max(2, 1 + number of eos ids) * num_beams <= 64), the torch bookkeeping
    otherwise; "device" = required (ValueError outside that range); "torch" = the torch bookkeeping, one host read per token.  Ties
    rank by (score descending, candidate index ascending) on the device path; torch.topk leaves them unspecified.

    Logits processors (`num_beams == 1`): `repetition_penalty` (off: None, 1.0), `no_repeat_ngram_size` (off: None, 0), `min_new_tokens`
    (off: None, 0, or no eos id), `bad_words_ids` and `suppress_tokens`, with HF's semantics for prompts given as embeddings: the history
    is the generated tokens only.  One kernel (p2t_logits_process) in front of the greedy / sampled choice, inside the replayed step graph,
    and in front of the torch filters under `generator=`; `output_scores` then returns the processed scores, `output_logits` the raw rows.
    With none of them active nothing is launched or allocated.

    `prompt_kv_dtype="fp8"` (bf16 models; ValueError otherwise) keeps the PROMPT segment of the KV cache as e4m3 codes with one
    power-of-two scale per key and kv head for K and for V (p2t_kv_quant_store on the prefill's store, the attention of
    p2t_attention_decode_prompt_fp8 in the step): half the cache bytes a step reads; the generated segment stays bf16.  The prefill
    attends before the store, so the first token's logits do not change; every decoding mode runs unchanged around it.

    `lm_head_dtype="fp8" | "mxfp4"` (bf16 models; ValueError otherwise; independent of `set_gemm_dtype` and `prompt_kv_dtype`) scores every
    token -- the prefill's first one included -- with a quantised LM head: e4m3 codes + one power-of-two scale per vocabulary row, or
    MXFP4 codes + one per 32 columns (lm_head_q: p2t_quant_rows_fp8 / p2t_quant_rows_mxfp4 of the bf16 head, built once per model),
    against the final RMSNorm's row written as e4m3 (p2t_lm_head_logits_q inside p2t_llama_decode_step_q): half / 27 % of the bytes of
    the step's largest launch.  It changes arithmetic and only which logits the decoding modes read; the bf16 head stays for None (the
    parent's path, nothing built), for training and, with tied embeddings, for the embedding lookup.  More than 64 rows run the general
    fp8 GEMM on row-major e4m3 codes of the same values.

    Logits processors under beam search (`num_beams > 1`) are opt-in: HF runs them on the log-softmax inside the beam step, with the
    beam's running sequence as the history, and ranks the processed rows.  `beam_select="device"` does that with two entry points inside
    the two-step graph (p2t_beam_logprobs_process, then p2t_beam_select_logprobs on its rows; ValueError outside p2t_beam_select's
    range), `beam_select="torch"` with p2t_logits_process on the torch path's log-softmax; `output_scores` returns the processed rows,
    `output_logits` the raw ones.  `beam_select=None` raises NotImplementedError, and so does beam sampling with a processor (HF then
    runs the warpers after the processors, and the device beam sampler cuts by stored logit).

    `beam_cache="ancestry"` (opt-in; `num_beams > 1` on the device selection, i.e. `beam_select` None inside p2t_beam_select's range or
    "device"; ValueError otherwise, and with more than 16 query heads per kv head) runs the search without the per-step copy of the
    generated keys and values: they stay in the row that wrote them, p2t_kv_ancestry_update keeps one byte per row and token that says
    in which row of the prompt a beam's key lies, and the step's attention (p2t_llama_decode_step_beams) runs one block per (prompt, kv
    head) whose 16 head slots are (beam, head) pairs -- the prompt segment is streamed once for all beams.  No second generated segment
    is allocated.  It serves beam search, seeded beam sampling and the logits processors under beams alike.

    `prefill="packed"` (opt-in; None / "padded" = compact + p2t_llama_prefill over batch x longest tokens, unchanged) runs the decoder's
    prompt phase without padding: the prompts lie back to back in a few long rows (plan_prompt_rows; `pack_tokens` = the rows' capacity,
    default one row up to PACK_TOKENS_MAX tokens), attention and rotation are confined per prompt, and each layer's keys and values are
    scattered into each prompt's own row of the cache's prompt segment (p2t_llama_prefill_packed).  Only the writer of the prompt
    segment changes, so every decoding mode, `prompt_kv_dtype` and `lm_head_dtype` run unchanged behind it; the first token's logits
    differ from the padded path's by rounding (another summation order, and the rotation after the projection instead of inside it).
    ValueError for another value, for `pack_tokens` without it, for more than PACK_PROMPTS_MAX prompts and on set_gemm_dtype("fp8") /
    ("mxfp4") models: the packed prefill runs the model-dtype GEMMs.

    `prompt_lookup_num_tokens=k` (opt-in; HF's keyword, 1 .. 7; None: off, nothing changes) is HF's prompt-lookup decoding for greedy
    decoding: every step carries k + 1 tokens per row -- the token chosen last and a draft of up to k tokens that follow the EARLIEST
    earlier occurrence of the row's trailing n-gram in its own generated text (`max_matching_ngram_size=n`, 1 .. 4, None: HF's 2; longest
    n first) -- through ONE decode step (p2t_llama_decode_step_multi), keeps the longest prefix of the draft the model agrees with plus
    the model's own next token (p2t_lookup_verify_rows), and so returns greedy decoding's tokens in fewer steps (lookup.LookupEngine).
    `return_dict_in_generate` adds `lookup_stats`, i64 [batch, 3] = (verify steps, drafted tokens, accepted tokens) per row.
    NotImplementedError with sampling, beams, any logits processor or output_scores; ValueError for k or n outside its range, for
    batch * (k + 1) > 64 and for more than 16 query heads per kv head."""
    if max_matching_ngram_size is not None and prompt_lookup_num_tokens is None:
        raise ValueError("generate: max_matching_ngram_size is the n-gram length of prompt_lookup_num_tokens")
    if prefill not in (None, "padded", "packed"):
        raise ValueError(f"generate: prefill = {prefill!r}: None, 'padded' or 'packed'")
    if pack_tokens is not None and prefill != "packed":
        raise ValueError("generate: pack_tokens is the row capacity of prefill='packed'")
    if prefill == "packed" and decoder.model.gemm_fp8:
        raise ValueError("generate(prefill='packed') runs the model-dtype GEMMs: it does not serve set_gemm_dtype('fp8') / ('mxfp4') models")
    if beam_cache is not None:
        if beam_cache != "ancestry":
            raise ValueError(f"generate: beam_cache = {beam_cache!r}: 'ancestry' or None")
        if num_beams < 2:
            raise ValueError("generate(beam_cache='ancestry'): a beam cache needs num_beams > 1")
        if beam_select == "torch":
            raise ValueError("generate(beam_cache='ancestry') runs on the device selection: beam_select None or 'device', not 'torch'")
        if decoder.spec.num_attention_heads // decoder.spec.num_key_value_heads > 16:
            raise ValueError("generate(beam_cache='ancestry'): at most 16 query heads per kv head")
    if (inputs_embeds is None) == (input_ids is None):
        raise ValueError("pass exactly one of inputs_embeds / input_ids")
    if unused:
        bad = [k for k in unused if unused[k] is not None and k not in ("use_cache", "output_attentions", "output_hidden_states", "synced_gpus")]
        if bad:
            raise NotImplementedError(f"generate(): unsupported arguments {bad}")
    if input_ids is not None:
        inputs_embeds = decoder.model.embed(input_ids)
    if inputs_embeds.dim() != 3 or inputs_embeds.shape[2] != decoder.spec.hidden_size:
        raise ValueError(f"inputs_embeds must be [batch, seq_len, {decoder.spec.hidden_size}]")
    B, T, _ = inputs_embeds.shape
    if attention_mask is None:
        attention_mask = torch.ones((B, T), dtype=torch.int64, device=inputs_embeds.device)
    if tuple(attention_mask.shape) != (B, T):
        raise ValueError(f"attention_mask shape {tuple(attention_mask.shape)} != inputs {(B, T)}")
    if max_new_tokens is None:
        if max_length is None:
            raise ValueError("generate() needs max_new_tokens (or max_length)")
        max_new_tokens = max_length - T      # HF: `max_length` counts the (padded) prompt, for embeddings too (generate(): max_length -= inputs_embeds.shape[1])
    if max_new_tokens < 1:
        raise ValueError("max_new_tokens must be >= 1")
    eos_ids = _as_id_list(eos_token_id)
    if pad_token_id is None:
        if not eos_ids:
            pad_token_id = 0
        else:
            pad_token_id = eos_ids[0]                                        # HF's fallback (with a warning)
    V = decoder.spec.vocab_size
    proc = _processor_args(V, eos_ids, repetition_penalty, no_repeat_ngram_size, min_new_tokens, bad_words_ids, suppress_tokens)
    if num_beams < 1 or num_return_sequences < 1 or num_return_sequences > num_beams and num_beams > 1:
        raise ValueError("num_beams >= 1 and 1 <= num_return_sequences <= num_beams")
    if prompt_lookup_num_tokens is not None:
        from . import lookup
        lookup.refuse_unsupported(num_beams, do_sample, proc, output_scores, num_return_sequences)
        return lookup.generate_lookup(decoder, inputs_embeds, attention_mask, SimpleNamespace(
            k=prompt_lookup_num_tokens, n=max_matching_ngram_size, max_new_tokens=max_new_tokens, eos_ids=eos_ids, pad_id=int(pad_token_id),
            return_dict=return_dict_in_generate, output_logits=output_logits, use_graph=use_graph, sync_every=sync_every, stream_copy=stream_copy,
            fuse_rope=fuse_rope, prompt_kv_dtype=prompt_kv_dtype, lm_head_dtype=lm_head_dtype, prefill=prefill, pack_tokens=pack_tokens))
    if num_beams > 1 and proc is not None:
        if do_sample:
            raise NotImplementedError("generate(): repetition_penalty / no_repeat_ngram_size / min_new_tokens / bad_words_ids / suppress_tokens are not "
                                      "supported under beam sampling (num_beams > 1 with do_sample=True): HF runs the warpers after the processors, "
                                      "and p2t_beam_sample_select cuts by stored logit")
        if beam_select not in ("device", "torch"):
            raise NotImplementedError("generate(): repetition_penalty / no_repeat_ngram_size / min_new_tokens / bad_words_ids / suppress_tokens with "
                                      "num_beams > 1 are opt-in: HF applies the processors to the log-softmax inside the beam step, which "
                                      "p2t_beam_select computes itself from the logits; pass beam_select='device' (p2t_beam_logprobs_process + "
                                      "p2t_beam_select_logprobs) or beam_select='torch'")
    if num_beams > 1:
        sampling = None
        if do_sample:
            sampling = _beam_sampling_args(num_beams, len(eos_ids), temperature, top_k, top_p, seed, generator, beam_select)
        return _beam_search(decoder, inputs_embeds, attention_mask, SimpleNamespace(
            max_length=max_new_tokens, eos_ids=eos_ids, pad_id=int(pad_token_id), nb=num_beams, length_penalty=float(length_penalty),
            early_stopping=early_stopping, num_return_sequences=num_return_sequences, return_dict=return_dict_in_generate,
            output_scores=output_scores, output_logits=output_logits, stream_copy=stream_copy, beam_select=beam_select, use_graph=use_graph,
            sync_every=sync_every, sampling=sampling, processors=proc, prompt_kv_dtype=prompt_kv_dtype, lm_head_dtype=lm_head_dtype,
            beam_cache=beam_cache, prefill=prefill, pack_tokens=pack_tokens))
    R = int(num_return_sequences)
    if R != 1 and not do_sample:
        raise ValueError("greedy decoding returns one sequence per prompt: num_return_sequences > 1 needs do_sample=True or num_beams > 1")
    # R samples per prompt (HF repeats the prompt R times): R rows that SHARE the prompt segment of the cache, like the beams of a prompt
    eng = DecodeEngine(decoder, B, R, T, max_new_tokens, stream_copy, fuse_rope, processors=proc, eos_ids=eos_ids, prompt_kv_dtype=prompt_kv_dtype,
                       lm_head_dtype=lm_head_dtype)
    logits = eng.prompt(inputs_embeds, attention_mask, prefill, pack_tokens)
    if R > 1:
        logits = logits.repeat_interleave(R, dim=0)
    eos = torch.tensor(eos_ids, dtype=torch.int64, device=eng.dev)
    on_device = bool(do_sample) and seed is not None
    if on_device:
        temperature, k, p = _sampler_args(temperature, top_k, top_p, seed, generator)
    if do_sample and return_dict_in_generate and output_scores and not on_device:
        # HF returns the PROCESSED scores (after temperature / top-k / top-p) under sampling; nothing here is pinned on that
        # (the goldens cover greedy and beam search), so the combination is refused rather than answered with the raw logits
        raise NotImplementedError("generate: output_scores with do_sample is not supported (ask for output_logits: the raw LM-head rows)")
    keep_scores = [] if (on_device and return_dict_in_generate and output_scores) else None
    # greedy with processors: the step's scores are the processed rows (a clone of the engine's buffer), not the raw logits
    keep_processed = [] if (proc is not None and return_dict_in_generate and output_scores and not do_sample) else None
    keep_logits = [] if (return_dict_in_generate and (output_logits or (output_scores and not on_device and keep_processed is None))) else None
    scores_buf = torch.empty((eng.BB, V), dtype=torch.float32, device=eng.dev) if keep_scores is not None else None
    pad = int(pad_token_id)
    warned = set()

    def sample(lg: torch.Tensor):
        eng.sample_select(lg, eos, pad, temperature, k, p, seed, scores_buf)

    def choose(lg: torch.Tensor, col: int):
        if proc is not None:
            lg = eng.process(lg)                         # history: out_tokens[:, : step[0]], step[0] == col
        if on_device:
            sample(lg)                                   # writes column step[0] == col; step[0] is the draw's counter
        elif do_sample:
            scores = filter_logits(lg[:, :V].float(), temperature, top_k, top_p)
            nxt = torch.multinomial(scores.softmax(dim=-1), num_samples=1, generator=generator).squeeze(1)
            nxt = torch.where(eng.finished.bool(), torch.full_like(nxt, pad), nxt)
            eng.next_tokens.copy_(nxt)
            eng.out_tokens[:, col] = nxt
            if eos_ids:
                eng.finished |= torch.isin(nxt, eos).int()
        else:
            eng.greedy_select(lg, eos, pad)              # writes column step[0] == col

    def advance():                                        # chosen tokens -> embeddings -> all layers over the cache -> logits -> choice
        eng.feed(eng.next_tokens)
        eng.decode_step()
        if do_sample and not on_device:
            return                                        # the torch path chooses outside (choose)
        lg = eng.process(eng.logits) if proc is not None else eng.logits
        if on_device:
            sample(lg)
        else:
            eng.greedy_select(lg, eos, pad)

    choose(logits, 0)
    if keep_logits is not None:
        keep_logits.append(logits[:, :V].float().clone())
    if keep_scores is not None:
        keep_scores.append(scores_buf.clone())
    if keep_processed is not None:
        keep_processed.append(eng.processed[:, :V].clone())
    graph, n = None, 1
    while n < max_new_tokens:
        if eos_ids and (n == 1 or n % sync_every == 0):
            if on_device and not warned:                  # the sampler's flags word (bit 0 only), read where the finished flags are
                _warn_flags(eng.sample_flags, warned, 3)
            if bool(eng.finished.all().item()):
                break
        if use_graph and (on_device or not do_sample) and n >= 2:        # the first step ran eagerly (lazy one-time initialisation inside the library)
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    advance()
            graph.replay()
        else:
            advance()
        if do_sample and not on_device:
            choose(eng.logits, n)
        if keep_logits is not None:
            keep_logits.append(eng.logits[:, :V].float().clone())
        if keep_scores is not None:
            keep_scores.append(scores_buf.clone())
        if keep_processed is not None:
            keep_processed.append(eng.processed[:, :V].clone())
        n += 1
    if on_device and not warned:
        _warn_flags(eng.sample_flags, warned, 3)
    seqs = _trim(eng.out_tokens, eos_ids, n)
    if not return_dict_in_generate:
        return seqs
    keep = tuple(keep_logits[: seqs.shape[1]]) if keep_logits is not None else None
    if keep_processed is not None:
        keep_scores = keep_processed
    if keep_scores is not None:
        return GenerateOutput(seqs, scores=tuple(keep_scores[: seqs.shape[1]]), logits=keep if output_logits else None)
    return GenerateOutput(seqs, scores=keep if output_scores else None, logits=keep if output_logits else None)


# ---------------------------------------------------------------------------------------------------------------------------
# beam search: transformers/generation/utils.py `_beam_search` (5.x, vectorised form) with an empty id prompt (decoder_prompt_len 0)
# ---------------------------------------------------------------------------------------------------------------------------
def _gather_beams(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, dim=1)


def _beam_sampling_args(nb: int, n_eos: int, temperature, top_k, top_p, seed, generator, beam_select) -> dict:
    """The sampling side of `num_beams > 1, do_sample=True`: which path, and its filters checked up front."""
    device = seed is not None and beam_select == "device"
    opted_in = device or (generator is not None and beam_select == "torch")
    if not opted_in and (seed is None or generator is None):          # both given: _sampler_args refuses that first, as ever
        raise NotImplementedError("beam sampling (num_beams > 1 with do_sample=True) is opt-in: pass seed=int together with beam_select='device' "
                                  "(p2t_beam_sample_select), or generator= together with beam_select='torch'")
    temperature, k, p = _sampler_args(temperature, top_k, top_p, seed, generator, device)
    keep = beam_keep(nb, n_eos)
    if 0 < k < keep:
        raise ValueError(f"generate: beam sampling draws max(2, 1 + number of eos ids) * num_beams = {keep} continuations per prompt, and the first "
                         f"step has one live beam: top_k = {k} cannot supply them (needs top_k >= {keep}, or 0)")
    return dict(device=device, temperature=temperature, top_k=k, top_p=p, seed=seed, generator=generator)


BEAMS_MAX, KEEP_MAX = 16, 64                  # p2t_beam_select's supported range (include/p2t_hip.h)


def beam_keep(nb: int, n_eos: int) -> int:
    return max(2, 1 + n_eos) * nb


def beam_select_supported(B: int, nb: int, n_eos: int, V: int) -> bool:
    keep = beam_keep(nb, n_eos)
    return 1 <= nb <= BEAMS_MAX and keep <= KEEP_MAX and V >= keep and B * nb * V < 2 ** 31


def beam_state_init(B: int, nb: int, max_length: int, pad_id: int, dev) -> dict:
    """The state `_beam_search` starts from (HF: running_sequences, running_beam_scores, sequences, beam_scores, is_sent_finished,
    next_token_hits_stopping_criteria's open flag, running_beam_indices, beam_indices)."""
    running = torch.full((B, nb, max_length), pad_id, dtype=torch.int64, device=dev)
    running_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
    running_scores[:, 1:] = -1e9
    running_idx = torch.full((B, nb, max_length), -1, dtype=torch.int32, device=dev)
    return dict(running=running, sequences=running.clone(), running_scores=running_scores,
                beam_scores=torch.full((B, nb), -1e9, dtype=torch.float32, device=dev),
                is_finished=torch.zeros((B, nb), dtype=torch.bool, device=dev), heuristic_open=torch.ones((B, 1), dtype=torch.bool, device=dev),
                running_idx=running_idx, beam_idx_tab=running_idx.clone())


def beam_step_torch(st: dict, logits: torch.Tensor, cur: int, nb: int, eos: torch.Tensor, length_penalty: float, early_stopping,
                    max_length: int, do_sample: bool = False, generator: Optional[torch.Generator] = None, temperature: float = 1.0,
                    top_k: Optional[int] = None, top_p: Optional[float] = None, process=None):
    """One step of the torch path on f32 logits [B * nb, V] (any device): -> (new state, log_probs, src_rows i64 [B * nb], hits, go_on).
    do_sample: the warpers run on the log-probabilities (HF appends the processed rows as the step's scores) and the keep continuations
    are torch.multinomial draws without replacement, HF's two lines; the new state then also holds them as "drawn" [B, keep].
    process(log_probs [B * nb, V], running [B, nb, max_length], cur) -> the rows after the logits processors (HF runs them on the
    log-softmax, with the beams' running sequences as histories); the returned log_probs are then the processed rows."""
    dev, V = logits.device, logits.shape[1]
    B = logits.shape[0] // nb
    keep = beam_keep(nb, eos.numel())
    top_mask = torch.cat((torch.ones(nb, dtype=torch.bool), torch.zeros(keep - nb, dtype=torch.bool))).to(dev)
    running, running_scores, running_idx = st["running"], st["running_scores"], st["running_idx"]
    sequences, beam_scores, beam_idx_tab = st["sequences"], st["beam_scores"], st["beam_idx_tab"]
    is_finished, heuristic_open = st["is_finished"], st["heuristic_open"]
    log_probs = torch.log_softmax(logits, dim=-1)
    if process is not None:
        log_probs = process(log_probs, running, cur)
    if do_sample:
        log_probs = filter_logits(log_probs, temperature, top_k, top_p)
    acc = (log_probs.view(B, nb, V) + running_scores[:, :, None]).reshape(B, nb * V)
    if do_sample:
        topk_i = torch.multinomial(torch.softmax(acc, dim=-1), num_samples=keep, generator=generator)
        topk_lp = torch.gather(acc, 1, topk_i)
    else:
        topk_lp, topk_i = torch.topk(acc, k=keep)
    src_beam = topk_i // V
    topk_idx = _gather_beams(running_idx, src_beam)
    topk_seq = _gather_beams(running, src_beam)
    topk_seq[:, :, cur] = topk_i % V
    topk_idx[:, :, cur] = (src_beam + torch.arange(B, device=dev).view(-1, 1) * nb).to(torch.int32)
    # stopping criteria on the candidates: max length, eos
    hits = torch.full((B, keep), cur + 1 >= max_length, dtype=torch.bool, device=dev)
    if eos.numel():
        hits |= torch.isin(topk_seq[:, :, cur], eos)
    # beams that go on
    live_lp = topk_lp + hits.float() * -1.0e9
    nxt = torch.topk(live_lp, k=nb)[1]
    running = _gather_beams(topk_seq, nxt)
    running_scores = _gather_beams(live_lp, nxt)
    running_idx = _gather_beams(topk_idx, nxt)
    # finished hypotheses
    just_done = hits & top_mask[None, :]
    fin_lp = topk_lp / ((cur + 1) ** length_penalty)
    full = torch.all(is_finished, dim=-1, keepdim=True) & (early_stopping is True)
    fin_lp = fin_lp + full.float() * -1.0e9 + (~heuristic_open).float() * -1.0e9 + (~just_done).float() * -1.0e9
    m_seq, m_sc = torch.cat((sequences, topk_seq), 1), torch.cat((beam_scores, fin_lp), 1)
    m_idx, m_fin = torch.cat((beam_idx_tab, topk_idx), 1), torch.cat((is_finished, just_done), 1)
    sel = torch.topk(m_sc, k=nb)[1]
    sequences, beam_scores = _gather_beams(m_seq, sel), _gather_beams(m_sc, sel)
    beam_idx_tab, is_finished = _gather_beams(m_idx, sel), _gather_beams(m_fin, sel)
    # the rows the next step continues from
    src_rows = running_idx[:, :, cur].reshape(-1).to(torch.int64)
    cur += 1
    best_len = max_length if (early_stopping == "never" and length_penalty > 0.0) else cur
    best_running = running_scores[:, :1] / (best_len ** length_penalty)
    worst_done = torch.where(is_finished, torch.min(beam_scores, dim=1, keepdim=True)[0], torch.full_like(beam_scores, -1.0e9))
    heuristic_open = heuristic_open & torch.any(best_running > worst_done, dim=-1, keepdim=True)
    go_on = torch.any(heuristic_open) & ~(torch.all(is_finished) & (early_stopping is True)) & ~torch.all(hits)
    new = dict(running=running, sequences=sequences, running_scores=running_scores, beam_scores=beam_scores, is_finished=is_finished,
               heuristic_open=heuristic_open, running_idx=running_idx, beam_idx_tab=beam_idx_tab)
    if do_sample:
        new["drawn"] = topk_i
    return new, log_probs, src_rows, hits, go_on


def _beam_output(o, sequences, beam_scores, beam_idx_tab, B, all_scores, all_logits):
    R = o.num_return_sequences
    sequences, beam_scores, beam_idx_tab = sequences[:, :R].reshape(B * R, -1), beam_scores[:, :R].reshape(-1), beam_idx_tab[:, :R].reshape(B * R, -1)
    n = int(((beam_idx_tab + 1).bool()).sum(dim=1).max().item())
    sequences = sequences[:, :n]
    if not o.return_dict:
        return sequences
    return GenerateOutput(sequences, scores=tuple(all_scores) if o.output_scores else None, logits=tuple(all_logits) if o.output_logits else None,
                          sequences_scores=beam_scores if o.output_scores else None, beam_indices=beam_idx_tab[:, :n])


def _beam_search(decoder, inputs_embeds, attention_mask, o):
    """`o`: what generate() decided for the search, under the names of its one call site (max_length counts the new tokens)."""
    if o.beam_select not in (None, "device", "torch"):
        raise ValueError(f"generate: beam_select = {o.beam_select!r}: 'device', 'torch' or None")
    B, V, nb, max_length = inputs_embeds.shape[0], decoder.spec.vocab_size, o.nb, o.max_length
    if o.beam_select != "torch":
        if beam_select_supported(B, nb, len(o.eos_ids), V):
            return _beam_search_device(decoder, inputs_embeds, attention_mask, o)
        if o.beam_select == "device" or o.beam_cache is not None:
            raise ValueError(f"generate(beam_select='device'{'' if o.beam_cache is None else ', beam_cache=' + repr(o.beam_cache)}): p2t_beam_select serves 1 <= num_beams <= {BEAMS_MAX} with max(2, 1 + number of eos ids) * "
                             f"num_beams <= {KEEP_MAX} <= vocabulary (got num_beams = {nb}, {len(o.eos_ids)} eos ids); the torch path serves the rest")
    eng = DecodeEngine(decoder, B, nb, inputs_embeds.shape[1], max_length, o.stream_copy, processors=o.processors, eos_ids=o.eos_ids,
                       prompt_kv_dtype=o.prompt_kv_dtype, lm_head_dtype=o.lm_head_dtype)
    dev = eng.dev
    first_logits = eng.prompt(inputs_embeds, attention_mask, o.prefill, o.pack_tokens)      # [B, ld]: the beams of a prompt start from the same state
    eos = torch.tensor(o.eos_ids, dtype=torch.int64, device=dev)
    st = beam_state_init(B, nb, max_length, o.pad_id, dev)
    all_scores, all_logits = [], []
    draw = {} if o.sampling is None else dict(do_sample=True, **{k: o.sampling[k] for k in ("generator", "temperature", "top_k", "top_p")})
    if o.processors is not None:
        cur_word = torch.zeros((1,), dtype=torch.int32, device=dev)

        def process(log_probs, running, cur):               # p2t_logits_process on the f32 log-probabilities, history = the running sequences
            cur_word.fill_(cur)
            return eng.process(log_probs.contiguous(), running.reshape(B * nb, max_length).contiguous(), cur_word)[:, :V].clone()

        draw["process"] = process
    cur = 0
    while True:
        if cur == 0:
            logits = first_logits[:, :V].float().repeat_interleave(nb, dim=0)     # HF expands the prompt nb times before its prefill
        else:
            logits = eng.logits[:, :V].float()
        if o.return_dict and o.output_logits:
            all_logits.append(logits.clone())
        st, log_probs, src_rows, _, go_on = beam_step_torch(st, logits, cur, nb, eos, o.length_penalty, o.early_stopping, max_length, **draw)
        if o.return_dict and o.output_scores:
            all_scores.append(log_probs)
        cur += 1
        if not bool(go_on.item()) or cur >= max_length:
            break
        if cur > 1:
            eng.reorder(src_rows)                       # generated keys / values follow their beams (nothing is cached before step 1)
        eng.next_tokens.copy_(st["running"][:, :, cur - 1].reshape(-1))
        eng.feed(eng.next_tokens)
        eng.decode_step()
    return _beam_output(o, st["sequences"], st["beam_scores"], st["beam_idx_tab"], B, all_scores, all_logits)


class BeamState:
    """p2t_beam_state of one generate() call (include/p2t_hip.h): double-buffered tables, a fresh state in half 0."""

    def __init__(self, B: int, nb: int, G: int, pad_id: int, dev, sample: bool = False):
        self.B, self.nb, self.G = B, nb, G
        self.run_seq = torch.full((2, B, nb, G), pad_id, dtype=torch.int64, device=dev)
        self.fin_seq = self.run_seq.clone()
        self.run_idx = torch.full((2, B, nb, G), -1, dtype=torch.int32, device=dev)
        self.fin_idx = self.run_idx.clone()
        self.run_scores = torch.zeros((2, B, nb), dtype=torch.float32, device=dev)
        self.run_scores[:, :, 1:] = -1e9
        self.fin_scores = torch.full((2, B, nb), -1e9, dtype=torch.float32, device=dev)
        self.is_finished = torch.zeros((2, B, nb), dtype=torch.int32, device=dev)
        self.heuristic_open = torch.ones((B,), dtype=torch.int32, device=dev)
        self.done = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.sync = torch.zeros((1 + B,), dtype=torch.int32, device=dev)
        self.workspace = torch.zeros((call("p2t_beam_sample_workspace_bytes" if sample else "p2t_beam_workspace_bytes", B, nb) // 4,),
                                     dtype=torch.float32, device=dev)
        self.flags = torch.zeros((1,), dtype=torch.int32, device=dev)      # p2t_beam_sample_select ORs into it (bit 0: table full, bit 1: ran dry)
        self.c = _lib.BeamStateC(**{n: getattr(self, n).data_ptr() for n, _ in _lib.BeamStateC._fields_})


def _beam_call(name: str, logits, V, state, eos, pad_id, length_penalty, early_stopping, max_length, step, next_tokens, src_rows, scores, *more):
    """Entry point `name` on p2t_beam_select's argument list, then `more`, then the stream."""
    es = 1 if early_stopping is True else (2 if early_stopping == "never" else 0)
    call(name, ptr(logits), ops.dt_of(logits), logits.stride(0), state.B, state.nb, V, ptr(eos) if eos.numel() else None, eos.numel(),
         int(pad_id), float(length_penalty), es, int(max_length), state.G, ptr(step), C.byref(state.c), ptr(next_tokens), ptr(src_rows),
         ptr(scores) if scores is not None else None, scores.stride(0) if scores is not None else 0, *more, stream())


def beam_select(logits: torch.Tensor, V: int, state: BeamState, eos: torch.Tensor, pad_id: int, length_penalty: float, early_stopping,
                max_length: int, step: torch.Tensor, next_tokens: torch.Tensor, src_rows: torch.Tensor, scores: Optional[torch.Tensor] = None):
    """One p2t_beam_select call: logits `dtype` [B nb, ld >= V] -> next_tokens, src_rows i64 [B nb] and the state's other half."""
    _beam_call("p2t_beam_select", logits, V, state, eos, pad_id, length_penalty, early_stopping, max_length, step, next_tokens, src_rows, scores)


def beam_select_logprobs(lp: torch.Tensor, V: int, state: BeamState, eos: torch.Tensor, pad_id: int, length_penalty: float, early_stopping,
                         max_length: int, step: torch.Tensor, next_tokens: torch.Tensor, src_rows: torch.Tensor):
    """One p2t_beam_select_logprobs call: beam_select on f32 rows [B nb, ld >= V] that already hold (processed) log-probabilities."""
    es = 1 if early_stopping is True else (2 if early_stopping == "never" else 0)
    call("p2t_beam_select_logprobs", ptr(lp), lp.stride(0), state.B, state.nb, V, ptr(eos) if eos.numel() else None, eos.numel(), int(pad_id),
         float(length_penalty), es, int(max_length), state.G, ptr(step), C.byref(state.c), ptr(next_tokens), ptr(src_rows), stream())


def beam_sample_select(logits: torch.Tensor, V: int, state: BeamState, eos: torch.Tensor, pad_id: int, length_penalty: float, early_stopping,
                       max_length: int, step: torch.Tensor, next_tokens: torch.Tensor, src_rows: torch.Tensor, temperature: float, top_k: int,
                       top_p: float, seed: int, scores: Optional[torch.Tensor] = None, prompt0: int = 0):
    """One p2t_beam_sample_select call (`state` built with sample=True): beam_select's arguments plus the sampler's; prompt b draws as
    prompt0 + b at the device step counter.  The flags word is state.flags."""
    _beam_call("p2t_beam_sample_select", logits, V, state, eos, pad_id, length_penalty, early_stopping, max_length, step, next_tokens, src_rows,
               scores, float(temperature), int(top_k), float(top_p), int(seed) & (2 ** 64 - 1), int(prompt0), ptr(state.flags))


def _beam_search_device(decoder, inputs_embeds, attention_mask, o):
    """The same search with p2t_beam_select (`o.sampling`: p2t_beam_sample_select; `o.processors`: p2t_beam_logprobs_process +
    p2t_beam_select_logprobs) in the torch bookkeeping's place: the first token from
    the prefill logits, one eager step, then a replayed graph of TWO steps (reorder, feed, decode, select, twice: the engine's cache
    buffers are back where the capture found them), an odd remainder eagerly.  The host reads `done` every `sync_every` tokens and at
    the end; steps run past the stop leave the state as it is."""
    B, V, nb, max_length, sampling = inputs_embeds.shape[0], decoder.spec.vocab_size, o.nb, o.max_length, o.sampling
    eng = DecodeEngine(decoder, B, nb, inputs_embeds.shape[1], max_length, o.stream_copy, processors=o.processors, eos_ids=o.eos_ids,
                       prompt_kv_dtype=o.prompt_kv_dtype, lm_head_dtype=o.lm_head_dtype, beam_cache=o.beam_cache)
    dev = eng.dev
    first = eng.prompt(inputs_embeds, attention_mask, o.prefill, o.pack_tokens).repeat_interleave(nb, dim=0).contiguous()     # HF expands the prompt nb times before its prefill
    eos = torch.tensor(o.eos_ids, dtype=torch.int64, device=dev)
    st = BeamState(B, nb, eng.G, o.pad_id, dev, sample=sampling is not None)
    src_rows = torch.zeros((eng.BB,), dtype=torch.int64, device=dev)
    keep_scores, keep_logits = o.return_dict and o.output_scores, o.return_dict and o.output_logits
    # two step slots: a replayed pair leaves the logits / log-probabilities of both its steps to be cloned afterwards
    lslots = [eng.logits, torch.zeros_like(eng.logits)] if keep_logits else [eng.logits, eng.logits]
    sslots = [torch.empty((eng.BB, V), dtype=torch.float32, device=dev) for _ in range(2)] if keep_scores else [None, None]
    # the rows of processed log-probabilities (HF's scores of the step): the two score slots, or, when nobody asks for the scores, the
    # engine's one f32 buffer for both steps of the graph
    lp_slots = sslots if keep_scores else [eng.processed, eng.processed] if o.processors is not None else None
    all_scores, all_logits = [], []
    warned = set()

    def read_done() -> bool:                              # one host read: `done` and, under sampling, the flags word next to it
        if sampling is not None:
            _warn_flags(st.flags, warned, 6)              # this closure, this function, _beam_search, generate(), its caller
        return bool(st.done[0].item())

    def select(lg, slot):
        common = (lg, V, st, eos, o.pad_id, o.length_penalty, o.early_stopping, max_length, eng.step, eng.next_tokens, src_rows)
        if o.processors is not None:                    # the processed log-probabilities, then their ranking as they stand
            eng.beam_process(lg, st, max_length, lp_slots[slot])
            beam_select_logprobs(lp_slots[slot], *common[1:])
        elif sampling is None:
            beam_select(*common, sslots[slot])
        else:
            beam_sample_select(*common, sampling["temperature"], sampling["top_k"], sampling["top_p"], sampling["seed"], sslots[slot])

    def keep(lg, slot):
        if keep_logits:
            all_logits.append(lg[:, :V].float().clone())
        if keep_scores:
            all_scores.append(sslots[slot].clone())

    def advance(slot):
        eng.logits = lslots[slot]
        if eng.ancestry is not None:
            eng.ancestry_update(src_rows)               # the generated keys / values stay; the table follows the beams
        else:
            eng.reorder(src_rows)                       # generated keys / values follow their beams (a no-op while nothing is cached)
        eng.feed(eng.next_tokens)
        eng.decode_step()
        select(eng.logits, slot)

    select(first, 0)
    keep(first, 0)
    graph, n, read_at = None, 1, 0
    while n < max_length:
        if n == 1 or n - read_at >= o.sync_every:
            read_at = n
            if read_done():
                break
        if o.use_graph and n >= 2 and max_length - n >= 2:                # the first step ran eagerly (lazy one-time initialisation inside the library)
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    advance(0)
                    advance(1)
            graph.replay()
            keep(lslots[0], 0)
            keep(lslots[1], 1)
            n += 2
        else:
            advance(0)
            keep(lslots[0], 0)
            n += 1
    read_done()
    done, steps = (int(v) for v in st.done.tolist())
    if not done:
        raise RuntimeError("generate: the beam search ran its max_new_tokens steps and p2t_beam_select did not raise `done`")
    half = steps & 1
    return _beam_output(o, st.fin_seq[half], st.fin_scores[half], st.fin_idx[half], B, all_scores[:steps], all_logits[:steps])
