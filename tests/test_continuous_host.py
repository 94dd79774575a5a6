"""CPU: the scheduler of continuous batching (p2t_hip/continuous.py) over a stub engine -- a Python object with the engine's four
methods that emits scripted tokens per request -- and what ContinuousDecoder refuses before it builds any device state."""
import pytest
import torch

EOS, PAD = 99, 0


class StubEngine:
    """Slots with their own counters, as the device keeps them: a request's payload is the script of tokens it would emit; it ends at
    EOS (bit 1) or at its limit (bit 2).  A finished slot keeps its counter through further steps; a load resets it."""

    def __init__(self, slots):
        self.script = [None] * slots
        self.tokens = [[] for _ in range(slots)]
        self.finished, self.row_step, self.limit = [2] * slots, [0] * slots, [1] * slots
        self.loads, self.steps_run, self.polls = [], 0, 0

    def _emit(self, s):
        t = self.script[s][self.row_step[s]]
        self.tokens[s].append(t)
        self.finished[s] |= (1 if t == EOS else 0) | (2 if self.row_step[s] + 1 >= self.limit[s] else 0)

    def load(self, slots, payloads, limits):
        assert len(set(slots)) == len(slots) == len(payloads) == len(limits)
        self.loads.append(list(slots))
        for s, p, l in zip(slots, payloads, limits):
            assert self.finished[s], "a live slot was overwritten"
            self.script[s], self.tokens[s], self.finished[s], self.row_step[s], self.limit[s] = p, [], 0, 0, l
            self._emit(s)

    def steps(self, n):
        for _ in range(n):
            self.steps_run += 1
            for s in range(len(self.script)):
                if not self.finished[s]:
                    self.row_step[s] += 1
                    self._emit(s)

    def poll(self):
        self.polls += 1
        return list(self.finished), list(self.row_step)

    def harvest(self, slot, n):
        return (list(self.tokens[slot][:n]),)


def _requests(n):
    """Request i emits 100 i + 0, 100 i + 1, ...; every third one carries an EOS at a position of its own."""
    scripts, limits = [], []
    for i in range(n):
        s = [100 * (i + 1) + j for j in range(12)]
        if i % 3 == 1:
            s[(2 * i) % 7] = EOS
        scripts.append(s)
        limits.append([1, 12, 5, 3, 1, 9][i % 6])
    return scripts, limits


def _expected(script, limit):
    out = script[:limit]
    return out[: out.index(EOS) + 1] if EOS in out else out


@pytest.mark.parametrize("sync_every", [1, 4])
@pytest.mark.parametrize("n_requests", [1, 3, 11])
@pytest.mark.parametrize("slots", [1, 2, 5])
def test_every_request_returns_once_with_its_own_tokens(slots, n_requests, sync_every):
    """More requests than slots and fewer, limits of 1 among them: every id comes back exactly once, with the tokens of ITS script up to
    its eos or its limit -- never a neighbour's, never a token of the slot's previous occupant."""
    from p2t_hip.continuous import ContinuousScheduler
    eng = StubEngine(slots)
    sch = ContinuousScheduler(eng, slots, sync_every)
    scripts, limits = _requests(n_requests)
    ids = [sch.submit(s, l) for s, l in zip(scripts, limits)]
    assert ids == list(range(n_requests))
    got = list(sch.run())
    assert sorted(r for r, _ in got) == ids
    for rid, toks in got:
        assert toks == _expected(scripts[rid], limits[rid]), rid
    assert not sch.pending() and all(eng.finished)
    assert all(len(l) <= slots for l in eng.loads) and sum(len(l) for l in eng.loads) == n_requests
    assert eng.steps_run % sync_every == 0


def test_a_second_wave_can_be_submitted_after_the_first_drained():
    from p2t_hip.continuous import ContinuousScheduler
    eng = StubEngine(2)
    sch = ContinuousScheduler(eng, 2, 4)
    a = sch.submit([1, 2, 3], 3)
    assert list(sch.run()) == [(a, [1, 2, 3])]
    b, c, d = (sch.submit([10 * k, EOS, 7], 3) for k in (1, 2, 3))
    assert sorted(sch.run()) == [(b, [10, EOS]), (c, [20, EOS]), (d, [30, EOS])]


def test_limit_one_requests_need_no_step():
    from p2t_hip.continuous import ContinuousScheduler
    eng = StubEngine(2)
    sch = ContinuousScheduler(eng, 2, 8)
    ids = [sch.submit([7 + k, 8, 9], 1) for k in range(5)]
    assert sorted(sch.run()) == [(i, [7 + k]) for k, i in enumerate(ids)]
    assert eng.steps_run == 0 and eng.polls == 3


def test_bad_scheduler_arguments():
    from p2t_hip.continuous import ContinuousScheduler
    for slots, sync in ((0, 1), (2, 0)):
        with pytest.raises(ValueError):
            ContinuousScheduler(StubEngine(1), slots, sync)


def _decoder(**kw):
    import p2t_hip as P
    from p2t_hip import specs
    from p2t_hip.continuous import ContinuousDecoder
    esm = specs.EsmSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2)
    llama = specs.LlamaSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=2, vocab_size=64)
    model = P.Esm2LlamaInstructForCausalLM.from_specs(esm, llama, specs.AdapterSpec(64, 64, 64, 0.0), dtype=torch.float32, device="cpu", seed=None)
    return model, lambda **k2: ContinuousDecoder(model.llama_decoder, **{**dict(slots=2, max_prompt_tokens=6, max_new_tokens=8, eos_token_id=EOS, pad_token_id=PAD), **kw, **k2})


@pytest.mark.parametrize("kw,word", [(dict(num_beams=2), "num_beams"), (dict(do_sample=True), "do_sample"), (dict(output_scores=True), "output_scores"),
                                     (dict(repetition_penalty=1.2), "logits processors"), (dict(no_repeat_ngram_size=2), "logits processors"),
                                     (dict(min_new_tokens=2), "logits processors"), (dict(bad_words_ids=[[3]]), "logits processors"),
                                     (dict(suppress_tokens=[3]), "logits processors"), (dict(num_return_sequences=2), "num_return_sequences"),
                                     (dict(assistant_model=object()), "assistant_model")], ids=lambda v: v if isinstance(v, str) else None)
def test_out_of_scope_modes_are_refused_by_name(kw, word):
    model, make = _decoder()
    with pytest.raises(NotImplementedError, match="continuous batching.*" + word):
        make(**kw)
    with pytest.raises(NotImplementedError, match="continuous batching.*" + word):
        model.continuous_generator(slots=2, max_prompt_tokens=6, max_new_tokens=8, **kw)


def test_neutral_generate_keywords_pass_and_submit_checks_its_arguments():
    """What greedy `generate` ignores is accepted; an over-long prompt, an empty one, a malformed batch and a limit outside
    1 .. max_new_tokens raise ValueError before any device state exists."""
    _, make = _decoder()
    dec = make(num_beams=1, do_sample=False, temperature=1.0, top_k=50, top_p=1.0, length_penalty=1.0, return_dict_in_generate=False)
    x = torch.zeros((2, 8, 64))
    mask = torch.tensor([[1, 1, 1, 0, 0, 0, 0, 0], [0, 0, 1, 1, 1, 1, 1, 1]])
    assert dec.submit(x, mask, max_new_tokens=[1, 8]) == [0, 1] and dec.submit(x[:1], mask[:1]) == [2]
    with pytest.raises(ValueError, match="7 tokens exceeds max_prompt_tokens = 6"):
        dec.submit(x, torch.tensor([[1] * 3 + [0] * 5, [0] + [1] * 7]))
    with pytest.raises(ValueError, match="at least one token"):
        dec.submit(x, torch.zeros((2, 8), dtype=torch.int64))
    with pytest.raises(ValueError, match="inputs_embeds must be"):
        dec.submit(torch.zeros((2, 8, 32)), mask)
    with pytest.raises(ValueError, match="attention_mask shape"):
        dec.submit(x, mask[:, :4])
    for bad in (0, 9, [1], [1, 0]):
        with pytest.raises(ValueError, match="max_new_tokens"):
            dec.submit(x, mask, max_new_tokens=bad)
    assert len(dec.scheduler.queue) == 3 and getattr(dec, "_engine", None) is None
    for bad in (dict(slots=0), dict(max_prompt_tokens=0), dict(max_new_tokens=0), dict(sync_every=0)):
        with pytest.raises(ValueError):
            make(**bad)
