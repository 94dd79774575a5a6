"""CPU: the f32 restatement of p2t_beam_select_logprobs (tests/beam_logprobs_reference.py) against two independent statements of the beam
step, and the ABI of the two entry points of the logits processors under beam search.
(a) against the fp64 restatement of p2t_beam_select (tests/beam_reference.py) on the unprocessed f32 log-softmax rows of the chains of
    beam_reference.CASES: every prompt the fp64 restatement calls decidable agrees in tokens, src_rows and tables, and the share left out
    stays under the cap tests/test_beam_reference_host.py allows for the same cases.
(b) against p2t_hip.generation.beam_step_torch on the CPU with process= the numpy logits_process_reference.process, over multi-step
    chains with the processors on, on logits whose fp64 gaps between neighbouring candidates are asserted (torch.topk leaves ties open).
(c) p2t_beam_logprobs_process and p2t_beam_select_logprobs are declared, exported and bound, and refuse every argument outside their
    contracts before any GPU call."""
import os
import re

import numpy as np
import pytest
import torch

import beam_logprobs_reference as BL
import beam_reference as BR
import logits_process_reference as LR
from test_beam_reference_host import _np_state, run_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
FAKE = 4096          # a non-null "pointer": never dereferenced, the checks come first


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
def test_restatement_agrees_with_the_fp64_step_wherever_that_is_decidable():
    count = {"f32": [0, 0], "bf16": [0, 0]}
    for case in BR.CASES:
        name, V, ld, B0, nb, n_eos, dtype, steps, L, lp_pen, es = case
        eos_ids = BR.case_eos(V, n_eos)

        def on_step(cur, logits, st, ref):
            if st["done"]:
                return
            got = BL.step(BL.log_softmax_f32(logits), st, cur, nb, eos_ids, lp_pen, es, L, 0)
            g, r = got["state"], ref["state"]
            count[dtype][0] += int((~ref["decidable"]).sum())
            count[dtype][1] += len(ref["decidable"])
            for b in np.nonzero(ref["decidable"])[0]:
                rows = slice(b * nb, (b + 1) * nb)
                assert np.array_equal(g["sequences"][b], r["sequences"][b]) and np.array_equal(g["beam_idx"][b], r["beam_idx"][b]), (name, cur, b)
                assert np.array_equal(g["is_finished"][b], r["is_finished"][b]), (name, cur, b)
                assert np.allclose(g["beam_scores"][b], r["beam_scores"][b], rtol=1e-6, atol=1e-5)
                if ref["running_decidable"][b]:
                    assert np.array_equal(got["next_tokens"][rows], ref["next_tokens"][rows]), (name, cur, b)
                    assert np.array_equal(got["src_rows"][rows], ref["src_rows"][rows]), (name, cur, b)
                    assert np.array_equal(g["running"][b], r["running"][b]) and np.array_equal(g["running_idx"][b], r["running_idx"][b]), (name, cur, b)
                    assert g["heuristic_open"][b] == r["heuristic_open"][b], (name, cur, b)
            if ref["decidable"].all() and ref["running_decidable"].all():
                assert g["done"] == r["done"] and g["steps"] == r["steps"], (name, cur)

        run_case(case, on_step)
    assert count["f32"][1] > 20 and count["bf16"][1] > 20
    assert count["f32"][0] <= 0.02 * count["f32"][1], count          # the caps of test_undecidable_share_of_the_gpu_cases
    assert count["bf16"][0] <= 0.05 * count["bf16"][1], count


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
MIN_GAP = 1e-4        # fp64 gap asserted between neighbouring candidates; f32 rounding of values around 30 is 2e-6


def _gaps(vals, n):
    """Smallest gap among the n + 1 largest finite values."""
    v = np.sort(np.asarray(vals, dtype=np.float64)[np.isfinite(vals)])[::-1][: n + 1]
    return np.inf if len(v) < 2 else float(np.min(v[:-1] - v[1:]))


SETTINGS = {
    "rp_ng2": dict(penalty=1.3, ngram=2),
    "all": dict(penalty=1.2, ngram=3, min_new=3, words=[[5, 9], [17], [3, 4, 5], [40]]),
}


@pytest.mark.parametrize("which", list(SETTINGS))
@pytest.mark.parametrize("length_penalty,early_stopping,n_eos", [(1.0, False, 1), (0.8, True, 2), (2.0, "never", 0)])
def test_restatement_equals_the_torch_step_with_processors(which, length_penalty, early_stopping, n_eos):
    from p2t_hip import generation as G
    B, nb, V, L, pad = 2, 3, 61, 8, 0
    eos_ids = BR.case_eos(V, n_eos)
    s = dict(SETTINGS[which])
    if s.get("min_new") and not eos_ids:
        s.pop("min_new")
    if "min_new" in s:
        s["eos_ids"] = eos_ids
    eos = torch.tensor(eos_ids, dtype=torch.int64)
    keep = G.beam_keep(nb, n_eos)
    st = G.beam_state_init(B, nb, L, pad, "cpu")
    changed, cur = 0, 0

    def process(log_probs, running, cur):
        hist = running.reshape(B * nb, L).numpy()
        return torch.from_numpy(LR.process(log_probs.numpy(), [hist[r, :cur] for r in range(B * nb)], **s))

    for cur in range(L):
        # a narrow alphabet of likely tokens, so that histories repeat and the processors bite
        logits = BR.case_logits(31 + n_eos, cur, B * nb, V, "f32", eos_ids)
        logits[:, 1:7] += np.float32(6.0)
        before = _np_state(st)
        new, lp, src_rows, hits, go_on = G.beam_step_torch(st, torch.from_numpy(logits), cur, nb, eos, length_penalty, early_stopping, L, process=process)
        lp = lp.numpy()
        plain = torch.log_softmax(torch.from_numpy(logits), dim=-1).numpy()
        changed += int((lp.view(np.uint32) != plain.view(np.uint32)).sum())
        hist = before["running"].reshape(B * nb, L)
        assert np.array_equal(lp.view(np.uint32), LR.process(plain, [hist[r, :cur] for r in range(B * nb)], **s).view(np.uint32))
        # no cross-beam near-ties: candidates, and the finished merge
        for b in range(B):
            acc = (lp[b * nb:(b + 1) * nb].astype(np.float64) + before["running_scores"][b].astype(np.float64)[:, None]).reshape(-1)
            assert _gaps(acc, keep) > MIN_GAP, (cur, b)
        ref = BL.step(lp, before, cur, nb, eos_ids, length_penalty, early_stopping, L, pad)
        r = ref["state"]
        fin = r["is_finished"]
        for b in range(B):
            merged = np.concatenate([r["beam_scores"][b][fin[b]], before["beam_scores"][b][before["is_finished"][b]]]).astype(np.float64)
            assert _gaps(np.unique(merged), len(merged)) > MIN_GAP / 100 or len(np.unique(merged)) < 2, (cur, b)
        assert np.array_equal(new["is_finished"].numpy(), fin), cur
        assert np.array_equal(new["sequences"].numpy()[fin], r["sequences"][fin]) and np.array_equal(new["beam_idx_tab"].numpy()[fin], r["beam_idx"][fin])
        assert np.array_equal(new["beam_scores"].numpy()[fin].view(np.uint32), r["beam_scores"][fin].view(np.uint32)), cur
        assert (new["beam_scores"].numpy()[~fin] <= -1e9).all() and (r["beam_scores"][~fin] <= -1e9).all()
        went_on = bool(go_on) and cur + 1 < L
        assert r["done"] == (not went_on), cur
        if cur + 1 < L:                                                  # in the last step every live score is -1e9 +- an ulp: order open, nothing reads it
            assert np.array_equal(new["running"].numpy(), r["running"]) and np.array_equal(new["running_idx"].numpy(), r["running_idx"]), cur
            assert np.array_equal(new["running_scores"].numpy().view(np.uint32), r["running_scores"].view(np.uint32)), cur
            assert np.array_equal(src_rows.numpy(), ref["src_rows"]) and np.array_equal(new["heuristic_open"].numpy()[:, 0], r["heuristic_open"])
        st = new
        for k, v in (("sequences", r["sequences"]), ("beam_idx_tab", r["beam_idx"]), ("beam_scores", r["beam_scores"])):      # the open -1e9 ties
            st[k] = torch.where(torch.from_numpy(fin).reshape(fin.shape + (1,) * (st[k].dim() - 2)), st[k], torch.from_numpy(v))
        if not went_on:
            break
    assert changed > 0 and cur >= 3                                       # the processors did something, over several steps


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
PROCESS, SELECT = "p2t_beam_logprobs_process", "p2t_beam_select_logprobs"


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, n_args in ((PROCESS, 22), (SELECT, 17)):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, f"{name} is not declared in include/p2t_hip.h"
        assert len(m.group(1).split(",")) == n_args
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.version() == 103


def _state(**null):
    from p2t_hip import _lib
    return _lib.BeamStateC(**{n: (None if n in null else FAKE) for n, _ in _lib.BeamStateC._fields_})


def _process(logits=FAKE, dtype=1, ld=320, B0=2, nb=3, V=300, step=FAKE, G=64, max_length=20, state="ok", penalty=1.3, ngram=2, min_new=0, eos=None,
             n_eos=0, words=None, offsets=None, n_words=0, n_word_ids=0, lp=FAKE, ld_lp=320):
    import ctypes as C

    from p2t_hip import _lib
    st = None if state is None else C.byref(_state(**({} if state == "ok" else {state: 1})))
    return _lib.call(PROCESS, logits, dtype, ld, B0, nb, V, step, G, max_length, st, penalty, ngram, min_new, eos, n_eos, words, offsets, n_words,
                     n_word_ids, lp, ld_lp, None)


def _select(lp=FAKE, ld=320, B0=2, nb=3, V=300, eos=None, n_eos=0, pad=0, length_penalty=1.0, es=0, max_length=20, G=64, step=FAKE, state="ok",
            nxt=FAKE, src=FAKE):
    import ctypes as C

    from p2t_hip import _lib
    st = None if state is None else C.byref(_state(**({} if state == "ok" else {state: 1})))
    return _lib.call(SELECT, lp, ld, B0, nb, V, eos, n_eos, pad, length_penalty, es, max_length, G, step, st, nxt, src, None)


_ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(logits=None), dict(step=None), dict(state=None), dict(lp=None), dict(state="run_seq"), dict(state="done"),
                                 dict(dtype=2), dict(dtype=-1), dict(ld=299), dict(ld_lp=299), dict(ld_lp=0), dict(B0=0), dict(nb=0), dict(nb=-2),
                                 dict(V=0), dict(G=0), dict(G=96), dict(max_length=0), dict(max_length=65), dict(penalty=0.0), dict(penalty=-1.5),
                                 dict(penalty=float("inf")), dict(penalty=float("nan")), dict(ngram=-1), dict(min_new=-1), dict(n_eos=1, eos=None),
                                 dict(n_eos=-1), dict(n_words=1, n_word_ids=1, words=None, offsets=FAKE),
                                 dict(n_words=1, n_word_ids=1, words=FAKE, offsets=None), dict(n_words=1, n_word_ids=0, words=FAKE, offsets=FAKE),
                                 dict(n_words=-1)], ids=_ids)
def test_process_argument_errors(bad):
    with pytest.raises(ValueError, match=PROCESS):
        _process(**bad)


@pytest.mark.parametrize("bad", [dict(lp=None), dict(step=None), dict(state=None), dict(nxt=None), dict(src=None), dict(state="run_seq"),
                                 dict(state="workspace"), dict(state="sync"), dict(ld=299), dict(B0=0), dict(nb=0), dict(V=0), dict(n_eos=1, eos=None),
                                 dict(n_eos=-1), dict(G=0), dict(G=96), dict(max_length=0), dict(max_length=65), dict(length_penalty=float("nan")),
                                 dict(es=3), dict(es=-1)], ids=_ids)
def test_select_argument_errors(bad):
    with pytest.raises(ValueError, match=SELECT):
        _select(**bad)


@pytest.mark.parametrize("fn,bad", [(_process, dict(nb=17)), (_process, dict(B0=4096, nb=8, V=128256, ld=128256, ld_lp=128256)), (_select, dict(nb=17)),
                                    (_select, dict(nb=16, n_eos=4, eos=FAKE)), (_select, dict(V=5, ld=8)),
                                    (_select, dict(B0=4096, nb=8, V=128256, ld=128256))], ids=lambda v: _ids(v) if isinstance(v, dict) else v.__name__)
def test_outside_the_supported_range(fn, bad):
    from p2t_hip._lib import P2TError
    with pytest.raises(P2TError, match="supported"):
        fn(**bad)
