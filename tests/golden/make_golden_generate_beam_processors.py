#!/usr/bin/env python3
"""Generate tests/golden/generate_beam_processors_tiny.npz: `generate` of the REFERENCE model under BEAM SEARCH with HF's logits processors
switched on, on the tiny models and inputs of generate_tiny.npz (make_golden.py run_generate: the same weight seeds, prompts and pad id),
in fp32 on the CPU, num_beams = 3, num_return_sequences = 3, length_penalty 1.0 and 0.8.

Argument sets (max_new_tokens of the parent fixture):
    rp_ng2      repetition_penalty 1.3, no_repeat_ngram_size 2
    ng3_min6    no_repeat_ngram_size 3, min_new_tokens 6 with the eos id of the parent fixture
    bad_sup     bad_words_ids (a pair, a three-token word and a one-token word of the plain beam search's best hypotheses) and
                suppress_tokens (tokens the plain beam search emits in prompts 1 and 2)
`sequences` and `sequences_scores` are kept (and the argument sets, in meta_json).  A variant is the fixture only if
  1. its sequences differ from the plain beam search's with the same length penalty and eos id (the processors changed something),
  2. the same call with the reference model in float64 returns the same sequences, and
  3. neighbouring sequences_scores of a prompt lie further apart than make_golden.py's MIN_GAP.
Variants are tried in order, as make_golden_generate_processors.py does; a (set, length penalty) that no variant satisfies on a model is
left out there, and every set must remain (with one length penalty at least) on three of the four model sizes.

Everything of the reference comes through make_golden.py's loader; this file holds none of it.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_generate_beam_processors.py"""
from __future__ import annotations

import copy
import json
import os

import numpy as np
import torch

from make_golden import HERE, build_reference_model, load_reference
from p2t_hip import specs

MIN_GAP = 5e-3                 # make_golden.py run_generate's bound
NB = 3
LENGTH_PENALTIES = (1.0, 0.8)


def argument_sets(plain, eos):
    """plain: the plain beam search's sequences [3 prompts * 3, n] (no eos id).  Per set, its variants in the order they are tried: the
    settings the sets are named for stay; what varies is the penalty, the eos id (the parent fixture's first, then none, then tokens the
    plain search emits: hypotheses of different lengths score further apart) and the banned words."""
    w = lambda r, i, n: [int(t) for t in plain[r * NB, i:i + n]]
    emitted = []
    for i in range(1, 9):
        for r in (0, 1, 2):
            if int(plain[r * NB, i]) not in emitted + [eos]:
                emitted.append(int(plain[r * NB, i]))
    return {
        "rp_ng2": [dict(repetition_penalty=p, no_repeat_ngram_size=2, eos_token_id=e) for e in [eos, None] + emitted for p in (1.3, 1.2, 1.5, 1.1)],
        "ng3_min6": [dict(repetition_penalty=1.0, no_repeat_ngram_size=3, min_new_tokens=6, eos_token_id=e) for e in [eos] + emitted],
        "bad_sup": [dict(bad_words_ids=[w(0, i, 2), w(1, i - 1, 3), w(2, i + 3, 1)], suppress_tokens=[int(plain[NB, j]), int(plain[2 * NB, j])],
                         eos_token_id=e) for e in [None, eos] + emitted[:4] for j in (0, 1, 2, 3) for i in (2, 3, 4, 5, 6, 7, 8)],
    }


def beam(model, kw, lp, **args):
    with torch.no_grad():
        o = model.generate(**{"eos_token_id": None, **kw, **args}, length_penalty=lp)
    return o.sequences.numpy(), o.sequences_scores.double().numpy()


def score_gap(scores):
    s = np.sort(scores.reshape(-1, NB), axis=1)
    return float(np.min(s[:, 1:] - s[:, :-1]))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref = load_reference()
    z = np.load(os.path.join(HERE, "generate_tiny.npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = meta = json.loads(bytes(g.pop("meta_json")).decode())
    t = lambda a: torch.from_numpy(a)
    out, sets, float64 = {}, {}, True
    for case, m in meta["cases"].items():
        model = build_reference_model(ref, specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"]), m["weight_seed"])
        model.config.placeholder_id = meta["placeholder_id"]
        kw = dict(inputs=t(g["input_ids"]), attention_mask=t(g["attention_mask"]), protein_input_ids=t(g["protein_input_ids"]),
                  protein_attention_mask=t(g["protein_attention_mask"]), pad_token_id=meta["pad_id"], return_dict_in_generate=True,
                  max_new_tokens=meta["max_new_tokens"], do_sample=False, num_beams=NB, num_return_sequences=NB, output_scores=True)
        seq, _ = beam(model, dict(kw, num_return_sequences=1), 1.0, eos_token_id=m["eos"])
        assert np.array_equal(seq, g[f"{case}.beam3_lp1.0"]), case                          # the parent fixture's model and inputs
        # float64: the decoder's eager attention adds finfo(float64).min to the scores of a left-padded row and returns NaN there, so the
        # float64 copy runs transformers' sdpa attention (a setting of the HF decoder; the arithmetic is the same)
        model64 = copy.deepcopy(model).double()
        model64.llama_decoder.config._attn_implementation = "sdpa"
        seq64, sc64 = beam(model64, kw, 1.0)
        if not np.isfinite(sc64).all():                                                     # the reference class cannot run in float64
            print(f"{case}: the float64 run returns non-finite scores; condition 2 is not checked")
            model64, float64 = None, False
        plain0, _ = beam(model, kw, 1.0)
        sets[case] = {}
        for name, variants in argument_sets(plain0, int(m["eos"])).items():
            for lp in LENGTH_PENALTIES:
                chosen = None
                for args in variants:
                    seq, sc = beam(model, kw, lp, **args)
                    gap = score_gap(sc)
                    if not gap > MIN_GAP:
                        continue
                    plain, _ = beam(model, kw, lp, eos_token_id=args.get("eos_token_id"))
                    if seq.shape == plain.shape and np.array_equal(seq, plain):
                        continue
                    if model64 is not None:
                        seq64 = beam(model64, kw, lp, **args)[0]
                        if seq64.shape != seq.shape or not np.array_equal(seq64, seq):
                            continue
                    chosen = (args, seq, sc, gap)
                    break
                if chosen is None:
                    print(f"{case}.{name}.lp{lp}: no variant meets the three conditions: left out")
                    continue
                args, seq, sc, gap = chosen
                sets[case][f"{name}.lp{lp}"] = dict(args, length_penalty=lp)
                out[f"{case}.{name}.lp{lp}"] = seq
                out[f"{case}.{name}.lp{lp}_scores"] = sc.astype(np.float32)
                print(f"{case}.{name}.lp{lp}: {args}: {seq.shape}, min gap of a prompt's sequences_scores {gap:.3e}, row 0 {seq[0, :8]}...")
    for name in ("rp_ng2", "ng3_min6", "bad_sup"):
        assert sum(any(f"{name}.lp{lp}" in v for lp in LENGTH_PENALTIES) for v in sets.values()) >= 3, (name, "needs three of the four model sizes")
    path = os.path.join(HERE, "generate_beam_processors_tiny.npz")
    meta_out = dict(sets=sets, min_score_gap=MIN_GAP, num_beams=NB, float64_checked=float64)
    np.savez_compressed(path, meta_json=np.frombuffer(json.dumps(meta_out).encode(), dtype=np.uint8), **out)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
