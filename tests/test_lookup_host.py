"""CPU: prompt-lookup decoding's rules (tests/lookup_reference.py) -- the draft against HF's PromptLookupCandidateGenerator.get_candidates,
the verify rule on hand cases, the simulator on the golden greedy tokens -- and generate()'s refusals, which all stand in front of the
first GPU call."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lookup_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_draft_rule_is_hfs_get_candidates(k, n):
    """Batch 1, no eos, a max_length far away: a small vocabulary makes n-grams repeat, so every branch (several matches, a match whose
    continuation is cut by the end, the fall to a shorter n-gram, no match) occurs many times."""
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=k, max_matching_ngram_size=n, max_length=10 ** 6)
    rs = np.random.RandomState(100 * k + n)
    lens, empty = [], 0
    for _ in range(300):
        h = rs.randint(0, rs.randint(4, 7), size=rs.randint(1, 40)).tolist()
        ids = torch.tensor([h], dtype=torch.int64)
        want = gen.get_candidates(ids)[0][0, len(h):].tolist()
        got = R.draft(h, k, n)
        assert got == want, (h, got, want)
        toks, c = R.step_tokens(h, k, n, 99)
        assert toks == [h[-1]] + got + [99] * (k - len(got)) and c == len(got) <= k
        lens.append(len(got))
        empty += not got
    assert empty > 0 and max(lens) == k and (k == 1 or 0 < min(l for l in lens if l) < k)


def test_draft_prefers_the_longest_ngram_then_the_earliest_match():
    #    0  1  2  3  4  5  6  7  8
    h = [5, 1, 2, 7, 1, 2, 8, 1, 2]
    assert R.draft(h, 3, 2) == [7, 1, 2]              # (1, 2) first at 1: what followed it there
    assert R.draft(h, 3, 1) == [7, 1, 2]              # (2) first at 2
    assert R.draft([3, 4, 9, 3, 9], 2, 2) == [3, 9]   # no earlier (3, 9): falls to (9) at 2
    assert R.draft([9, 9], 3, 2) == [9]               # the continuation is cut by the end of the text
    assert R.draft([1, 2, 3], 3, 2) == [] and R.draft([4], 3, 2) == []


def test_verify_rule_hand_cases():
    eos = (50,)
    # full accept: the model agrees with all three draft tokens and adds its own
    assert R.verify([11, 12, 13, 14], [10, 11, 12, 13], 3, 4, 100, eos) == ([11, 12, 13, 14], 0, 3)
    # reject at 0: only the model's own token
    assert R.verify([21, 12, 13, 14], [10, 11, 12, 13], 3, 4, 100, eos) == ([21], 0, 0)
    # reject in the middle; what lies behind the first disagreement is never looked at
    assert R.verify([11, 22, 13, 14], [10, 11, 12, 13], 3, 4, 100, eos) == ([11, 22], 0, 1)
    # a short draft (c = 1): the pad behind it is never compared, even where the model happens to emit it
    assert R.verify([11, 0, 0, 0], [10, 11, 0, 0], 1, 4, 100, eos) == ([11, 0], 0, 1)
    # eos inside the accepted run: cut behind it, the agreement count is the uncut one
    assert R.verify([11, 50, 13, 14], [10, 11, 50, 13], 3, 4, 100, eos) == ([11, 50], R.EOS_BIT, 3)
    # the limit inside the run: tokens 5, 6 are the last two of a row limited to 7
    assert R.verify([11, 12, 13, 14], [10, 11, 12, 13], 3, 4, 7, eos) == ([11, 12], R.LIMIT_BIT, 2)
    # eos exactly at the limit: both bits
    assert R.verify([11, 50, 13, 14], [10, 11, 50, 13], 3, 4, 7, eos) == ([11, 50], R.EOS_BIT | R.LIMIT_BIT, 2)
    # a finished row
    assert R.verify([11, 12, 13, 14], [10, 11, 12, 13], 3, 4, 100, eos, finished=R.LIMIT_BIT) == ([], R.LIMIT_BIT, 0)
    # ties: the lowest index among equal maxima
    lg = np.full((2, 16), -1.0, np.float32)
    lg[0, [9, 3, 12]] = 2.0
    lg[1, 11] = 5.0
    lg[1, 13] = 7.0                                   # a column behind V
    assert R.argmax_rows(lg, 12).tolist() == [3, 11]


def test_simulator_on_the_golden_greedy_tokens():
    """The (verify steps, accepted tokens) per row of the four golden cases at k = 3, n = 2: every case accepts, rejects and leaves its
    rows out of step.  steps + tokens kept + 1 = the sequence's length."""
    z = np.load(os.path.join(HERE, "golden", "generate_tiny.npz"))
    want = {"d16": [(11, 2), (9, 4), (13, 0)], "d64": [(9, 5), (13, 0), (11, 2)], "d128": [(12, 2), (12, 1), (13, 0)],
            "qwen3": [(12, 2), (13, 0), (12, 1)]}
    for case, rows in want.items():
        got = [R.simulate(r, 3, 2) for r in z[f"{case}.greedy"]]
        assert [(s, a) for s, _, a in got] == rows, case
        assert all(d >= a for _, d, a in got)
    meta = json.loads(bytes(z["meta_json"]).decode())
    eos = meta["cases"]["d16"]["eos"]
    assert R.simulate(z["d16.greedy"][1], 3, 2, (eos,))[0] == 4              # the row that stops at its 5th token


def _decoder(heads=4, kv=2):
    spec = SimpleNamespace(hidden_size=8, vocab_size=32, num_attention_heads=heads, num_key_value_heads=kv)
    return SimpleNamespace(spec=spec, model=SimpleNamespace(gemm_fp8=False))


def test_generate_refusals():
    from p2t_hip import generation
    x = torch.zeros((2, 4, 8))
    gen = lambda dec=None, B=2, **kw: generation.generate(dec or _decoder(), torch.zeros((B, 4, 8)), max_new_tokens=4, **kw)
    for kw in (dict(do_sample=True), dict(num_beams=2), dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[3]]),
               dict(suppress_tokens=[1]), dict(min_new_tokens=2, eos_token_id=5), dict(output_scores=True, return_dict_in_generate=True)):
        with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
            gen(prompt_lookup_num_tokens=3, **kw)
    for k in (0, 8, -1, 2.0, True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens must be an integer in 1 .. 7"):
            gen(prompt_lookup_num_tokens=k)
    for n in (0, 5, 1.5):
        with pytest.raises(ValueError, match="max_matching_ngram_size must be an integer in 1 .. 4"):
            gen(prompt_lookup_num_tokens=3, max_matching_ngram_size=n)
    with pytest.raises(ValueError, match="17 prompts x 4 tokens per step exceed the 64 rows"):
        gen(B=17, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="9 prompts x 8 tokens"):
        gen(B=9, prompt_lookup_num_tokens=7)
    with pytest.raises(ValueError, match="at most 16 query heads per kv head"):
        gen(dec=_decoder(34, 2), prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="max_matching_ngram_size is the n-gram length of prompt_lookup_num_tokens"):
        gen(max_matching_ngram_size=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        gen(prompt_lookup_num_tokens=3, num_return_sequences=2)
    assert x.shape == (2, 4, 8)


def test_continuous_batching_refuses_the_switch():
    from p2t_hip.continuous import ContinuousDecoder
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        ContinuousDecoder(_decoder(), 2, 8, 8, prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        ContinuousDecoder(_decoder(), 2, 8, 8, choice="device", prompt_lookup_num_tokens=3)
