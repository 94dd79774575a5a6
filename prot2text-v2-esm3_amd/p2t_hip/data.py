"""Host-side batch pipeline of the contrastive step.

What the reference does before the hot path sees a batch, restated without its dataset classes:

* protein side -- `dataset/dataset.py:392-397`: HF `EsmTokenizer` (33-token vocabulary, `<cls> seq <eos>`), then
  `dataset/dataloader.py:113-123`: right padding with the tokenizer's pad id and a 0/1 attention mask;
* description side -- `dataset/dataloader_light.py:222-239`: `description + eos`, no BOS, truncation to
  `max_description_length`, right padding to the longest, attention mask;
* sequence cropping -- `dataset/dataloader_light.py:172-179`: a random window of `max_sequence_length` residues.

`EsmSequenceTokenizer` is pinned against the installed `transformers.EsmTokenizer` (tests/test_data_pipeline.py);
`ContrastiveCollater` against the reference's own `Prot2TextLightCollater` run on the same rows with the same tiny
tokenizer (tests/golden/collate.json, written by tests/golden/make_golden.py).  `DevicePrefetcher` stages batches
through pinned memory and a copy stream so the H2D transfer of batch i+1 overlaps the step of batch i.

Ragged lengths: real proteins are much shorter than the longest of a batch.  `sort_batch_by_length` (host side, before
the H2D copy) orders the pairs of a batch by protein length and records the lengths, so that
`ContrastiveTrainer(num_segments=k, trim_padding=True)` can run each segment at ITS longest length instead of the
batch's.  The in-batch InfoNCE loss does not depend on the order of the pairs, and the segmented loss of equal segments
equals the unsegmented one (`scripts/train_contrast.py:94-114,367-379`), so the step's result is unchanged.
"""
from __future__ import annotations

import random
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Sequence

import torch

# facebook/esm2_* vocabulary (public, 33 entries; ids = positions).  SURVEY.md section 8: cls 0, pad 1, eos 2, mask 32.
ESM_VOCAB = ["<cls>", "<pad>", "<eos>", "<unk>", "L", "A", "G", "V", "S", "E", "R", "T", "I", "D", "P", "K", "Q", "N", "F",
             "Y", "M", "H", "W", "C", "X", "B", "U", "Z", "O", ".", "-", "<null_1>", "<mask>"]


def pad_sequences(sequences: Sequence[torch.Tensor], padding_value: int, padding_side: str = "right") -> torch.Tensor:
    """Stack 1-D tensors of different lengths (dataset/dataloader.py:199-228)."""
    if padding_side not in ("left", "right"):
        raise ValueError(f"Invalid padding side: {padding_side}")
    n = max(int(s.shape[-1]) for s in sequences)
    out = torch.full((len(sequences), n), padding_value, dtype=sequences[0].dtype)
    for i, s in enumerate(sequences):
        k = int(s.shape[-1])
        if padding_side == "right":
            out[i, :k] = s
        else:
            out[i, n - k:] = s
    return out


class EsmSequenceTokenizer:
    """Amino-acid tokenizer with the behaviour of HF `EsmTokenizer` on sequence strings: every vocabulary entry is
    matched wherever it occurs (special-token strings included), white space separates, and a maximal run of other
    characters becomes ONE `<unk>`."""

    def __init__(self, vocab: Sequence[str] = ESM_VOCAB):
        self.vocab = list(vocab)
        self.token_to_id = {t: i for i, t in enumerate(self.vocab)}
        self.cls_token_id, self.pad_token_id = self.token_to_id["<cls>"], self.token_to_id["<pad>"]
        self.eos_token_id, self.unk_token_id = self.token_to_id["<eos>"], self.token_to_id["<unk>"]
        self.mask_token_id = self.token_to_id["<mask>"]
        self._multi = sorted((t for t in self.vocab if len(t) > 1), key=len, reverse=True)

    def encode(self, sequence: str, add_special_tokens: bool = True) -> List[int]:
        ids: List[int] = [self.cls_token_id] if add_special_tokens else []
        i, n, in_unk = 0, len(sequence), False
        while i < n:
            ch = sequence[i]
            if ch.isspace():
                in_unk = False
                i += 1
                continue
            hit = None
            if ch == "<":
                hit = next((t for t in self._multi if sequence.startswith(t, i)), None)
            if hit is None and ch in self.token_to_id:
                hit = ch
            if hit is not None:
                ids.append(self.token_to_id[hit])
                in_unk = False
                i += len(hit)
            else:
                if not in_unk:
                    ids.append(self.unk_token_id)
                in_unk = True
                i += 1
        if add_special_tokens:
            ids.append(self.eos_token_id)
        return ids

    def __call__(self, sequences: Sequence[str], add_special_tokens: bool = True) -> Dict[str, torch.Tensor]:
        """Right-padded `input_ids` / `attention_mask` (int64), the protein half of the batch contract."""
        toks = [torch.tensor(self.encode(s, add_special_tokens), dtype=torch.int64) for s in sequences]
        return {"input_ids": pad_sequences(toks, self.pad_token_id, "right"),
                "attention_mask": pad_sequences([torch.ones_like(t) for t in toks], 0, "right")}


class ContrastiveCollater:
    """Rows {"AlphaFoldDB", "sequence", "function", ...} -> the batch dict `teacher_forcing_forward_pass` consumes.

    `description_tokenizer` is any HF tokenizer (the reference passes the LLM's); it is called exactly as upstream does.
    The random crop draws from Python's `random` in the upstream order (two draws per row for the name / taxon
    dropout, which this path does not otherwise use, then one per over-long sequence), so a seeded run sees the same
    windows as the reference collater."""

    def __init__(self, description_tokenizer, sequence_tokenizer: Optional[EsmSequenceTokenizer] = None,
                 max_sequence_length: int = 1021, max_description_length: int = 512, name_dropout: float = 0.8,
                 taxonomy_dropout: float = 0.8):
        self.description_tokenizer = description_tokenizer
        self.sequence_tokenizer = sequence_tokenizer or EsmSequenceTokenizer()
        self.max_sequence_length, self.max_description_length = max_sequence_length, max_description_length
        self.name_dropout, self.taxonomy_dropout = name_dropout, taxonomy_dropout

    def __call__(self, batch: List[Dict[str, Any]]) -> Dict[str, Any]:
        for key in ("Full Name", "taxon"):                  # RNG parity with the upstream collater (:159-170)
            for item in batch:
                if isinstance(item.get(key), str):
                    random.random()
        sequences = []
        for item in batch:
            seq = item["sequence"]
            if len(seq) > self.max_sequence_length:
                start = random.randint(0, len(seq) - self.max_sequence_length)
                seq = seq[start:start + self.max_sequence_length]
            sequences.append(seq)
        prot = self.sequence_tokenizer(sequences)
        tok = self.description_tokenizer
        tok.padding_side = "right"
        desc = tok([item["function"] + tok.eos_token for item in batch], add_special_tokens=False, truncation=True,
                   padding="longest", max_length=self.max_description_length, return_tensors="pt")
        d_ids, d_mask = desc["input_ids"], desc["attention_mask"]
        if d_ids.size(1) > self.max_description_length:
            d_ids, d_mask = d_ids[:, :self.max_description_length], d_mask[:, :self.max_description_length]
        return {"name": [item["AlphaFoldDB"] for item in batch], "protein_sequences": sequences,
                "protein_input_ids": prot["input_ids"], "protein_attention_mask": prot["attention_mask"],
                "description_input_ids": d_ids, "description_attention_mask": d_mask}


def sort_batch_by_length(batch: Dict[str, Any], descending: bool = True) -> Dict[str, Any]:
    """Reorder the pairs of a collated (host) batch by protein length and add `protein_lengths` (list of ints, host),
    `description_lengths` (host ints) and `description_order` (int64 tensor: rows by falling description length).
    Every per-pair entry (tensors with leading dimension B, lists of length B) is permuted the same way.
    The lengths feed ContrastiveTrainer(trim_padding=True), which cuts `ids[:, :T_s]`: that is only valid for RIGHT-padded
    rows (the contract of the contrastive batch, dataset/dataloader.py:113-123,139-149), so both masks are checked to be
    prefixes here, on the host; a left-padded batch (dataset/dataloader_derived.py:142-147 can build one) is refused."""
    mask = batch["protein_attention_mask"]
    if mask.is_cuda:
        raise ValueError("sort_batch_by_length works on the host batch (before the H2D copy)")
    for key in ("protein_attention_mask", "description_attention_mask"):
        m = batch.get(key)
        if m is not None and m.dim() == 2 and m.shape[1] > 1 and not bool((m[:, :-1] >= m[:, 1:]).all()):
            raise ValueError(f"{key} is not right-padded (a row has a 1 after a 0): trimming by length would cut valid tokens")
    lengths = mask.sum(dim=1)
    order = torch.argsort(lengths, descending=descending, stable=True)
    B = int(mask.shape[0])
    idx = order.tolist()
    out: Dict[str, Any] = {}
    for k, v in batch.items():
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B:
            out[k] = v[order]
        elif isinstance(v, (list, tuple)) and len(v) == B:
            out[k] = [v[i] for i in idx]
        else:
            out[k] = v
    out["protein_lengths"] = [int(lengths[i]) for i in idx]
    if "description_attention_mask" in out:
        # the text tower may run in its own length order (rows are independent there): lengths in the new batch order
        # (host) and the rows by falling length (a tensor, so it travels to the device with the batch)
        dlen = out["description_attention_mask"].sum(dim=1)
        out["description_lengths"] = [int(v) for v in dlen]
        out["description_order"] = torch.argsort(dlen, descending=True, stable=True)
    return out


def pack_instruct_batch(batch: Dict[str, Any], max_tokens: int, loss_weighting: str = "token", pad_token_id: Optional[int] = None) -> Dict[str, Any]:
    """Stage-2 batch in the reference collater's layout (dataset/dataloader.py:112-143: each row [left pad + bos + prompt with the
    protein placeholders + description + eot + right pad]) -> the same samples packed into padding-free rows of at most
    `max_tokens` tokens (transformers' DataCollatorWithFlattening convention, include/p2t_hip.h "packed rows"):

    * both pads are stripped from every sample; samples go into rows first-fit decreasing (longest first, ties in batch order);
    * rows are right-padded to the longest row; `position_ids` run 0, 1, 2, ... inside every sample (0 on padding);
    * `labels` are the samples' labels with -100 at every document start and on padding;
    * `protein_input_ids` / `protein_attention_mask` are permuted to the order in which the samples now appear (row-major), so
      that the row-major order of the placeholders still matches the order of the encoder rows (reference :138);
    * loss_weighting "token": no weights -- the loss is the token mean over all supervised tokens, as the padded batch's;
      "sample": `loss_weights` f32 [rows, T] = 1 / (n_docs * n_supervised(doc)) on every supervised target -- the mean of the
      per-sample losses, i.e. the reference's batch_size_per_device = 1 micro-batches, averaged (documents without a supervised
      token are not counted);
    * `pack_layout`: one (sample index, row, start, length) per sample in placement order (enough to unpack the rows);
    * `num_targets`: the number of positions t >= 1 of the packed labels that are not -100, a host upper bound on the targets the
      LM loss counts (`forward(num_targets=...)`: under `fused_lm_loss()` it sizes the head's buffers without a device read).
    A sample longer than max_tokens raises ValueError.  Works on the host batch; other per-sample entries are dropped."""
    if loss_weighting not in ("token", "sample"):
        raise ValueError(f"loss_weighting must be 'token' or 'sample', got {loss_weighting!r}")
    ids, mask, labels = batch["input_ids"].cpu(), batch["attention_mask"].cpu(), batch["labels"].cpu()
    B = int(ids.shape[0])
    if tuple(mask.shape) != tuple(ids.shape) or tuple(labels.shape) != tuple(ids.shape):
        raise ValueError("input_ids, attention_mask and labels must have the same [B, T] shape")
    if pad_token_id is None:
        pads = ids[mask == 0]
        pad_token_id = int(pads[0]) if pads.numel() else 0
    samples = []
    for i in range(B):
        keep = mask[i] != 0
        n = int(keep.sum())
        if n > max_tokens:
            raise ValueError(f"sample {i} has {n} tokens, more than max_tokens = {max_tokens}")
        idx = torch.nonzero(keep).flatten()
        if n and int(idx[-1] - idx[0]) + 1 != n:
            raise ValueError(f"sample {i}: the attention mask is not one contiguous run (left pad + tokens + right pad)")
        samples.append((ids[i, keep], labels[i, keep]))
    order = sorted(range(B), key=lambda i: -samples[i][0].numel())          # stable: ties keep the batch order
    rows: List[List[int]] = []
    room: List[int] = []
    for i in order:
        n = samples[i][0].numel()
        for r in range(len(rows)):
            if room[r] >= n:
                rows[r].append(i)
                room[r] -= n
                break
        else:
            rows.append([i])
            room.append(max_tokens - n)
    R = len(rows)
    T = max(max_tokens - rm for rm in room) if R else 0
    out_ids = torch.full((R, T), pad_token_id, dtype=ids.dtype)
    out_mask = torch.zeros((R, T), dtype=mask.dtype)
    out_pos = torch.zeros((R, T), dtype=torch.int64)
    out_lab = torch.full((R, T), -100, dtype=labels.dtype)
    out_w = torch.zeros((R, T), dtype=torch.float32) if loss_weighting == "sample" else None
    layout = []
    n_docs = sum(1 for i in range(B) if int((samples[i][1][1:] != -100).sum()) > 0)
    for r, members in enumerate(rows):
        t0 = 0
        for i in members:
            x, y = samples[i]
            n = x.numel()
            out_ids[r, t0:t0 + n] = x
            out_mask[r, t0:t0 + n] = 1
            out_pos[r, t0:t0 + n] = torch.arange(n)
            out_lab[r, t0:t0 + n] = y
            out_lab[r, t0] = -100                                               # a document start is never a target
            if out_w is not None:
                sup = out_lab[r, t0:t0 + n] != -100
                k = int(sup.sum())
                if k:
                    out_w[r, t0:t0 + n][sup] = 1.0 / (n_docs * k)
            layout.append((i, r, t0, n))
            t0 += n
    placed = [i for _, members in enumerate(rows) for i in members]
    out: Dict[str, Any] = {"input_ids": out_ids, "attention_mask": out_mask, "position_ids": out_pos, "labels": out_lab, "pack_layout": layout}
    perm = torch.tensor(placed, dtype=torch.int64)
    for key in ("protein_input_ids", "protein_attention_mask"):
        if key in batch:
            out[key] = batch[key].cpu()[perm]
    if out_w is not None:
        out["loss_weights"] = out_w
    out["num_targets"] = int((out_lab[:, 1:] != -100).sum()) if T > 1 else 0
    return out


class DevicePrefetcher:
    """Iterate device-resident batches one step ahead of the consumer: tensors go through pinned host memory and are
    copied on a dedicated stream; the consumer's stream only waits on the copy event of the batch it is handed.
    On a CPU-only host it degrades to a plain iterator (tests)."""

    def __init__(self, batches: Iterable[Dict[str, Any]], device: torch.device | str,
                 transform: Optional[Callable[[Dict[str, Any]], Dict[str, Any]]] = None):
        self.batches, self.device, self.transform = batches, torch.device(device), transform
        self.cuda = self.device.type == "cuda" and torch.cuda.is_available()
        self.copy_stream = torch.cuda.Stream(device=self.device) if self.cuda else None

    def _stage(self, batch: Dict[str, Any]):
        if self.transform is not None:
            batch = self.transform(batch)
        if not self.cuda:
            return {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in batch.items()}, None
        out = {}
        with torch.cuda.stream(self.copy_stream):
            for k, v in batch.items():
                out[k] = v.pin_memory().to(self.device, non_blocking=True) if torch.is_tensor(v) else v
            ready = self.copy_stream.record_event()
        return out, ready

    def __iter__(self) -> Iterator[Dict[str, Any]]:
        it = iter(self.batches)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur, ready = nxt
            try:
                nxt = self._stage(next(it))                 # enqueue the next copy before handing out this batch
            except StopIteration:
                nxt = None
            if ready is not None:
                torch.cuda.current_stream(self.device).wait_event(ready)
                for v in cur.values():
                    if torch.is_tensor(v):
                        v.record_stream(torch.cuda.current_stream(self.device))
            yield cur
