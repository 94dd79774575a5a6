#!/usr/bin/env python3
"""Generate tests/golden/generate_processors_tiny.npz: `generate` of the REFERENCE model with HF's logits processors switched on, on the
tiny models and inputs of generate_tiny.npz (make_golden.py run_generate: the same weight seeds, prompts and pad id), in fp32 on the CPU.

Argument sets (greedy decoding, max_new_tokens of the parent fixture):
    rp_ng2      repetition_penalty 1.3, no_repeat_ngram_size 2
    ng3_min6    no_repeat_ngram_size 3, min_new_tokens 6 with the eos id of the parent fixture (a token plain greedy emits early)
    bad_sup     bad_words_ids (an adjacent pair of row 0's plain greedy output, a three-token word of row 1's, a one-token word) and
                suppress_tokens (the tokens plain greedy emits first in rows 1 and 2)
Only the sequences are kept (and the argument sets, in meta_json).  As make_golden.py does for `greedy_logits`, the smallest top-1 / top-2
gap of the PROCESSED scores over every step a row is still running is asserted to be far above fp32 noise, so the ids are a stable target.

Everything of the reference comes through make_golden.py's loader; this file holds none of it.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_generate_processors.py"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from make_golden import HERE, build_reference_model, load_reference
from p2t_hip import specs

MIN_GAP = 5e-3                 # make_golden.py run_generate's bound on the top-2 gap


def argument_sets(g, case):
    """Per set, its variants in the order they are tried (as run_generate tries weight seeds): the first one whose every choice is
    clear-cut is the fixture (none on a model: that model is left out for the set; three of the
    four must remain).  The settings the sets are named for stay; what varies is the penalty, the eos id, the banned words."""
    seq0, eos = g[f"{case}.greedy"], int(g["meta"]["cases"][case]["eos"])
    w = lambda r, i, n: [int(t) for t in seq0[r, i:i + n]]
    return {
        "rp_ng2": [dict(repetition_penalty=p, no_repeat_ngram_size=2) for p in (1.3, 1.2, 1.5, 1.1)],
        "ng3_min6": [dict(repetition_penalty=1.0, no_repeat_ngram_size=3, min_new_tokens=6, eos_token_id=e)
                     for e in [eos] + [int(seq0[r, i]) for i in (1, 2, 3, 4, 5) for r in (0, 1, 2)]],
        "bad_sup": [dict(bad_words_ids=[w(0, i, 2), w(1, i - 1, 3), w(2, i + 3, 1)], suppress_tokens=[int(seq0[1, j]), int(seq0[2, j])])
                    for j in (0, 1, 2, 3) for i in (2, 3, 4, 5, 6, 7, 8)],
    }


def run_set(model, kw, args, plain):
    """-> (sequences, the smallest top-1 / top-2 gap of the processed scores over every step a row is still running)."""
    with torch.no_grad():
        o = model.generate(**{"eos_token_id": None, **kw, **args})
    seq = o.sequences.numpy()
    sc = torch.stack(o.scores, 0).numpy()                                          # [n, B, V], processed
    eos = args.get("eos_token_id")
    gap = np.inf
    for r in range(seq.shape[0]):
        for n in range(seq.shape[1]):
            if eos is not None and n > 0 and (seq[r, :n] == eos).any():
                break                                                              # a finished row emits pad whatever its scores are
            top2 = np.sort(sc[n, r])[-2:]
            assert np.isfinite(top2).all() and int(np.argmax(sc[n, r])) == seq[r, n], (args, r, n)
            gap = min(gap, float(top2[1] - top2[0]))
    if np.array_equal(seq, plain[:, : seq.shape[1]]):                              # the processors changed nothing: no fixture
        gap = 0.0
    return seq, gap


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = load_reference()
    z = np.load(os.path.join(HERE, "generate_tiny.npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = meta = json.loads(bytes(g.pop("meta_json")).decode())
    t = lambda a: torch.from_numpy(a)
    out, sets = {}, {}
    for case, m in meta["cases"].items():
        model = build_reference_model(ref, specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"]), m["weight_seed"])
        model.config.placeholder_id = meta["placeholder_id"]
        kw = dict(inputs=t(g["input_ids"]), attention_mask=t(g["attention_mask"]), protein_input_ids=t(g["protein_input_ids"]),
                  protein_attention_mask=t(g["protein_attention_mask"]), pad_token_id=meta["pad_id"], return_dict_in_generate=True,
                  max_new_tokens=meta["max_new_tokens"], do_sample=False, num_beams=1, output_scores=True)
        plain = g[f"{case}.greedy"]
        with torch.no_grad():
            assert np.array_equal(model.generate(**kw, eos_token_id=None).sequences.numpy(), plain), case     # the parent fixture's model and inputs
        sets[case] = {}
        for name, variants in argument_sets(g, case).items():
            for args in variants:
                seq, gap = run_set(model, kw, args, plain)
                if gap > MIN_GAP:
                    break
            if not gap > MIN_GAP:                  # no variant is clear-cut on this model: the set is pinned on the other model sizes
                print(f"{case}.{name}: no variant with every top-2 gap above {MIN_GAP}: left out")
                continue
            sets[case][name] = args
            out[f"{case}.{name}"] = seq
            print(f"{case}.{name}: {args}: {seq.shape}, min top-2 gap of the processed scores {gap:.3e}, row 0 {seq[0, :8]}...")
    for name in ("rp_ng2", "ng3_min6", "bad_sup"):
        assert sum(name in v for v in sets.values()) >= 3, (name, "needs three of the four model sizes")
    path = os.path.join(HERE, "generate_processors_tiny.npz")
    np.savez_compressed(path, meta_json=np.frombuffer(json.dumps(dict(sets=sets, min_top2_gap=MIN_GAP)).encode(), dtype=np.uint8), **out)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
