"""CPU: what `choice="device"` opens on ContinuousDecoder / continuous_generator before any device state exists (p2t_hip/continuous.py)
-- each newly served keyword constructs, the helpers of `generate` check their ranges, beams stay refused --, the draw keys of
submit(sample_keys=) through a stub engine, and the numpy restatement's own properties (tests/continuous_choice_reference.py)."""
import numpy as np
import pytest
import torch

import continuous_choice_reference as ccr
from test_continuous_host import EOS, PAD, StubEngine, _decoder


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2), dict(bad_words_ids=[[3], [4, 5]]),
                                dict(suppress_tokens=[3]), dict(output_scores=True), dict(do_sample=True, seed=7),
                                dict(do_sample=True, seed=-3, temperature=0.7, top_k=5, top_p=0.9), dict(do_sample=True, seed=2 ** 63, top_k=0, top_p=1.0),
                                dict(do_sample=True, seed=1, top_k=None, top_p=None), dict()],
                         ids=lambda k: ",".join(k) or "plain")
def test_choice_device_serves_what_choice_none_refuses(kw):
    model, make = _decoder()
    if kw:
        with pytest.raises(NotImplementedError, match="continuous batching"):
            make(**kw)
    dec = make(choice="device", **kw)
    assert dec.choice is not None and dec.scheduler.keyed and getattr(dec, "_engine", None) is None
    assert (dec.choice["sampling"] is not None) == bool(kw.get("do_sample")) and dec.choice["output_scores"] == bool(kw.get("output_scores"))
    gen = model.continuous_generator(slots=2, max_prompt_tokens=6, max_new_tokens=8, eos_token_id=EOS, pad_token_id=PAD, choice="device", **kw)
    assert gen.decoder.choice == dec.choice


def test_choice_device_settings_are_generates():
    """The dict the engine gets: _processor_args' settings (min_new_tokens needs an eos id, [eos] is no bad word, suppressed ids are words
    of one token) and _sampler_args' (top_k None / 0 = off, top_p >= 1 = off)."""
    _, make = _decoder()
    c = make(choice="device", eos_token_id=7, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3, bad_words_ids=[[7], [4, 5]], suppress_tokens=[9]).choice
    assert c["processors"] == dict(penalty=1.3, ngram=2, min_new=3, words=[[4, 5], [9]]) and c["sampling"] is None
    assert make(choice="device", min_new_tokens=3, eos_token_id=None).choice["processors"] is None
    assert make(choice="device", repetition_penalty=1.0, no_repeat_ngram_size=0).choice["processors"] is None
    c = make(choice="device", do_sample=True, seed=11, temperature=0.8, top_k=5, top_p=0.9).choice
    assert c["sampling"] == dict(temperature=0.8, top_k=5, top_p=0.9, seed=11) and c["processors"] is None
    assert make(choice="device", do_sample=True, seed=11).choice["sampling"] == dict(temperature=1.0, top_k=50, top_p=1.0, seed=11)
    assert make(choice="device", do_sample=True, seed=11, top_k=0, top_p=2.0).choice["sampling"]["top_k"] == 0
    assert make(choice="device", do_sample=False, seed=11, temperature=0.5).choice["sampling"] is None           # greedy ignores the sampler's keywords


@pytest.mark.parametrize("kw,exc,match", [
    (dict(do_sample=True), ValueError, "seed"),
    (dict(do_sample=True, seed=None, top_k=5), ValueError, "seed"),
    (dict(do_sample=True, seed=1.5), ValueError, "seed"),
    (dict(do_sample=True, generator=torch.Generator()), NotImplementedError, "continuous batching.*generator"),
    (dict(do_sample=True, seed=3, generator=torch.Generator()), NotImplementedError, "continuous batching.*generator"),
    (dict(do_sample=True, seed=3, temperature=0.0), ValueError, "temperature"),
    (dict(do_sample=True, seed=3, top_p=0.0), ValueError, "top_p"),
    (dict(do_sample=True, seed=3, top_k=2000), ValueError, "top_k 1 .. 1024"),
    (dict(do_sample=True, seed=3, top_k=0, top_p=0.9), ValueError, "both filters off"),
    (dict(repetition_penalty=0.0), ValueError, "`penalty` has to be a strictly positive float"),
    (dict(no_repeat_ngram_size=-1), ValueError, "`ngram_size`"),
    (dict(min_new_tokens=-2), ValueError, "`min_new_tokens`"),
    (dict(bad_words_ids=[]), ValueError, "non-empty list"),
    (dict(bad_words_ids=[[64]]), ValueError, "vocabulary size is 64"),
    (dict(num_beams=2), NotImplementedError, "continuous batching.*num_beams"),
    (dict(num_beams=3, do_sample=True, seed=1), NotImplementedError, "continuous batching.*num_beams"),
    (dict(num_return_sequences=2, do_sample=True, seed=1), NotImplementedError, "continuous batching.*num_return_sequences"),
    (dict(assistant_model=object()), NotImplementedError, "continuous batching.*assistant_model"),
], ids=lambda v: ",".join(v) if isinstance(v, dict) else None)
def test_choice_device_refusals(kw, exc, match):
    model, make = _decoder()
    with pytest.raises(exc, match=match):
        make(choice="device", **kw)
    with pytest.raises(exc, match=match):
        model.continuous_generator(slots=2, max_prompt_tokens=6, max_new_tokens=8, choice="device", **kw)


def test_choice_takes_none_or_device():
    _, make = _decoder()
    for bad in ("torch", "host", True, 1):
        with pytest.raises(ValueError, match="choice must be None or 'device'"):
            make(choice=bad)
    assert make().choice is None and not make().scheduler.keyed


def test_sample_keys_are_checked_by_submit():
    _, make = _decoder()
    x, mask = torch.zeros((2, 4, 64)), torch.ones((2, 4), dtype=torch.int64)
    dec = make(choice="device", do_sample=True, seed=5)
    for bad in ([1], [1, 2, 3], [1, 2.0], [1, "2"], [True, 2], [1, 2 ** 63], [-2 ** 63 - 1, 0], [None, 1]):
        with pytest.raises(ValueError, match="sample_keys"):
            dec.submit(x, mask, sample_keys=bad)
    assert len(dec.scheduler.queue) == 0
    assert dec.submit(x, mask, sample_keys=[2 ** 63 - 1, -2 ** 63]) == [0, 1]
    assert dec.submit(x, mask, sample_keys=torch.tensor([5, 6])) == [2, 3] and dec.submit(x, mask, sample_keys=np.array([8, 9])) == [4, 5]
    assert [q[3] for q in dec.scheduler.queue] == [2 ** 63 - 1, -2 ** 63, 5, 6, 8, 9]
    with pytest.raises(ValueError, match="sample_keys.*choice='device'"):            # a greedy decoder draws nothing
        make().submit(x, mask, sample_keys=[1, 2])


class KeyedStub(StubEngine):
    """StubEngine whose load() takes the draw keys, as ContinuousEngine's does, and records them per slot."""

    def __init__(self, slots):
        super().__init__(slots)
        self.keys = []

    def load(self, slots, payloads, limits, keys):
        assert len(keys) == len(slots)
        self.keys.append(dict(zip(slots, keys)))
        super().load(slots, payloads, limits)


def test_default_keys_are_the_request_ids_and_explicit_keys_travel_with_their_request():
    from p2t_hip.continuous import ContinuousScheduler
    eng = KeyedStub(2)
    sch = ContinuousScheduler(eng, 2, 2, keyed=True)
    scripts = [[10 + i, 20 + i, 30 + i, 40 + i] for i in range(5)]
    limits = [4, 1, 2, 3, 1]
    ids = [sch.submit(s, l) for s, l in zip(scripts, limits)]
    got = dict(sch.run())
    assert ids == list(range(5)) and all(got[i] == scripts[i][: limits[i]] for i in ids)
    loaded = [k for load in eng.keys for k in load.values()]
    assert sorted(loaded) == ids                                # every request's key is its id, whichever slot it got
    assert eng.keys[0] == {0: 0, 1: 1}
    # explicit keys, a second wave on the same scheduler: ids go on, the keys are the caller's
    more = [sch.submit([7, 8], 2, key=k) for k in (2 ** 40 + 1, -5)]
    n_before = len(eng.keys)
    assert sorted(dict(sch.run())) == more == [5, 6]
    assert sorted(k for load in eng.keys[n_before:] for k in load.values()) == [-5, 2 ** 40 + 1]
    # an unkeyed scheduler calls load() with three arguments, as before
    plain = StubEngine(1)
    sch = ContinuousScheduler(plain, 1, 1)
    sch.submit([1, 2], 2, key=99)
    assert list(sch.run()) == [(0, [1, 2])]


def test_the_decoder_hands_its_keys_to_the_engine():
    """ContinuousDecoder over a stub engine: the default key of a row is its request id; sample_keys replace it."""
    _, make = _decoder()
    dec = make(choice="device", do_sample=True, seed=5)
    eng = KeyedStub(2)
    dec._engine = eng
    x, mask = torch.zeros((3, 4, 64)), torch.ones((3, 4), dtype=torch.int64)
    # the stub emits a script: hand it one in the payload's place
    dec.submit(x, mask, max_new_tokens=1)
    dec.submit(x[:2], mask[:2], max_new_tokens=1, sample_keys=[70, -70])
    dec.scheduler.queue = type(dec.scheduler.queue)((rid, [rid + 1], limit, key) for rid, _, limit, key in dec.scheduler.queue)
    got = dict(dec.run())
    assert got == {i: [i + 1] for i in range(5)}
    assert sorted(k for load in eng.keys for k in load.values()) == [-70, 0, 1, 2, 70]


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------
def _state(BB, G, rng, V):
    return dict(finished=np.zeros(BB, np.int32), next_tokens=np.full(BB, -1, np.int64), out_tokens=rng.integers(0, V, (BB, G)).astype(np.int64),
                row_step=rng.integers(0, G, BB).astype(np.int32), row_limit=np.full(BB, G, np.int32))


def test_reference_a_finished_row_changes_nothing():
    rng = np.random.default_rng(0)
    V, BB, G = 40, 4, 8
    st = _state(BB, G, rng, V)
    st["finished"][2] = 2
    logits = rng.standard_normal((BB, V)).astype(np.float32)
    logits[2] = np.nan                                          # never read
    keys = np.array([3, 4, 5, 6], np.int64)
    before = {k: v.copy() for k, v in st.items()}
    scores = np.full((BB, V), 7.0, np.float32)
    res = ccr.sample_select_rows(logits, V, st["finished"], st["next_tokens"], st["out_tokens"], st["row_step"], st["row_limit"], keys, [EOS], PAD, 0.9, 5, 0.9, 1,
                                 scores=scores)
    assert sorted(res) == [0, 1, 3]
    assert st["next_tokens"][2] == PAD and st["finished"][2] == 2 and np.array_equal(st["out_tokens"][2], before["out_tokens"][2])
    assert np.all(scores[2] == 7.0) and np.all(np.isfinite(scores[[0, 1, 3]]).sum(1) >= 1)
    out = np.full((BB, V), 7.0, np.float32)
    ccr.logits_process_rows(logits, V, st["out_tokens"], st["row_step"], out, finished=st["finished"], penalty=1.5, ngram=2)
    assert np.all(out[2] == 7.0) and not np.any(out[[0, 1, 3]] == 7.0)
    # a row the engine does not have touches nothing either
    st2 = {k: v.copy() for k, v in before.items()}
    res = ccr.sample_select_rows(logits[:2], V, st2["finished"], st2["next_tokens"], st2["out_tokens"], st2["row_step"], st2["row_limit"], keys, [EOS], PAD, 1.0, 5,
                                 1.0, 1, row_map=[BB, -1])
    assert res == {} and all(np.array_equal(st2[k], before[k]) for k in before)


def test_reference_the_draw_depends_on_key_and_row_step_only():
    """The same logits row under the same (key, row_step) at another i, r and BB: the same token and scores; another key or another step
    moves the draw (over 64 trials the uniform numbers differ every time)."""
    from p2t_hip.synth import sample_uniform
    rng = np.random.default_rng(1)
    V, G = 50, 8
    row = rng.standard_normal(V).astype(np.float32)

    def run(BB, i, r, key, step, n):
        st = _state(BB, G, rng, V)
        st["row_step"][r] = step
        logits = rng.standard_normal((n, V)).astype(np.float32)
        logits[i] = row
        others = [int(v) for v in rng.permutation(BB) if v != r][: n - 1]
        rmap = np.array(others[:i] + [r] + others[i:])
        keys = rng.integers(-2 ** 62, 2 ** 62, BB)
        keys[r] = key
        scores = np.zeros((n, V), np.float32)
        res = ccr.sample_select_rows(logits, V, st["finished"], st["next_tokens"], st["out_tokens"], st["row_step"], st["row_limit"], keys, [], PAD, 0.8, 8, 0.95,
                                     123, row_map=rmap, scores=scores)
        assert st["out_tokens"][r, step] == res[i]["token"] == st["next_tokens"][r]
        return res[i]["token"], scores[i].copy()

    a = run(4, 0, 3, 2 ** 41 + 7, 5, 4)
    b = run(7, 2, 1, 2 ** 41 + 7, 5, 3)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    us = {sample_uniform(123, 2 ** 41 + 7, 5)}
    for t in range(64):
        us.add(sample_uniform(123, 2 ** 41 + 8 + t, 5))
        us.add(sample_uniform(123, 2 ** 41 + 7, 6 + t))
    assert len(us) == 129
    assert sample_uniform(123, -1, 0) == sample_uniform(123, 2 ** 64 - 1, 0) != sample_uniform(123, 2 ** 32 - 1, 0)      # the key is all 64 bits


def test_reference_bits_and_history_are_per_row():
    """The limit bit at the row's own limit, the eos bit on an eos draw (top_k = 1 makes the draw the argmax), and a history that is the
    row's own prefix."""
    V, BB, G = 12, 3, 8
    st = dict(finished=np.zeros(BB, np.int32), next_tokens=np.zeros(BB, np.int64), out_tokens=np.zeros((BB, G), np.int64),
              row_step=np.array([0, 3, 7], np.int32), row_limit=np.array([5, 4, 8], np.int32))
    logits = np.zeros((BB, V), np.float32)
    logits[0, 4], logits[1, 9], logits[2, 2] = 5, 5, 5
    ccr.sample_select_rows(logits, V, st["finished"], st["next_tokens"], st["out_tokens"], st["row_step"], st["row_limit"], np.arange(BB), [9], PAD, 1.0, 1, 1.0, 0)
    assert st["finished"].tolist() == [0, 3, 2] and st["next_tokens"].tolist() == [4, 9, 2]
    assert st["out_tokens"][0, 0] == 4 and st["out_tokens"][1, 3] == 9 and st["out_tokens"][2, 7] == 2
    hist = np.array([[1, 1, 1, 1, 0, 0, 0, 0], [2, 3, 2, 9, 9, 9, 9, 9], [5] * 8], np.int64)
    out = np.zeros((BB, V), np.float32)
    x = np.ones((BB, V), np.float32)
    ccr.logits_process_rows(x, V, hist, np.array([0, 3, 99], np.int32), out, ngram=2, min_new=2, eos_ids=[7])
    assert np.isinf(out[0]).nonzero()[0].tolist() == [7]            # row_step 0: no history, min_new active
    assert np.isinf(out[1]).nonzero()[0].tolist() == [3]            # history 2 3 2: the bi-gram (2, 3) bans 3; min_new over
    assert np.isinf(out[2]).nonzero()[0].tolist() == [5]            # cur clamps to G
