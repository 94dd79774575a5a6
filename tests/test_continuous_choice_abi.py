"""CPU: the per-row choice entry points of continuous batching (include/p2t_hip.h: p2t_sample_select_rows, p2t_logits_process_rows) are
declared, exported and bound, and every call outside the contract is refused before any GPU call -- P2T_ERR_ARG as ValueError, the
sampler's unsupported combination as P2T_ERR_UNSUPPORTED (-3).  The fake-pointer pattern of tests/test_continuous_abi.py: a non-null
"pointer" is never dereferenced, the checks come first."""
import re

import pytest

from test_continuous_abi import FAKE, HEADER

NAMES = {"p2t_sample_select_rows": 26, "p2t_logits_process_rows": 24}


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    # the sampler: p2t_sample_select's arguments without step and row0, with row_step, row_limit, row_map, row_key, BB in step's place
    lock, rows = _lib.SIGNATURES["p2t_sample_select"][1], _lib.SIGNATURES["p2t_sample_select_rows"][1]
    assert rows[:12] == lock[:12] and rows[17:22] == lock[13:18] and rows[22:] == lock[19:] and len(rows) == len(lock) + 3
    # the processors: p2t_logits_process's, with row_step, row_map, finished, BB in step's place
    lock, rows = _lib.SIGNATURES["p2t_logits_process"][1], _lib.SIGNATURES["p2t_logits_process_rows"][1]
    assert rows[:7] == lock[:7] and rows[11:] == lock[8:] and len(rows) == len(lock) + 3


def _sample(logits=FAKE, dtype=1, ld=512, V=500, n=4, eos=None, n_eos=0, fin=FAKE, nxt=FAKE, out=FAKE, ld_tok=64, row_step=FAKE, row_limit=FAKE, row_map=None,
            row_key=FAKE, BB=4, G=64, temperature=1.0, top_k=50, top_p=1.0, scores=None, ld_scores=0, flags=FAKE):
    from p2t_hip import _lib
    return _lib.call("p2t_sample_select_rows", logits, dtype, ld, V, n, eos, n_eos, 0, fin, nxt, out, ld_tok, row_step, row_limit, row_map, row_key, BB, G,
                     temperature, top_k, top_p, 7, scores, ld_scores, flags, None)


@pytest.mark.parametrize("bad", [dict(logits=None), dict(fin=None), dict(nxt=None), dict(out=None), dict(row_step=None), dict(row_limit=None), dict(row_key=None),
                                 dict(flags=None), dict(dtype=2), dict(n=0), dict(BB=0), dict(n=5), dict(n=2), dict(V=0), dict(ld=499), dict(ld_tok=63),
                                 dict(G=0), dict(n_eos=1), dict(n_eos=-1), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
                                 dict(temperature=float("nan")), dict(top_k=-1), dict(top_k=1025), dict(top_p=0.0), dict(top_p=-0.5),
                                 dict(scores=FAKE, ld_scores=499)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_sample_select_rows_argument_errors(bad):
    """Null buffers (the key array among them), logits that are neither f32 nor bf16, more logits rows than engine rows, a subset without
    its row_map, a token table narrower than G, eos ids announced but not given, sampler settings out of range, a scores pitch below V."""
    with pytest.raises(ValueError, match="p2t_sample_select_rows"):
        _sample(**bad)


def test_sample_select_rows_top_p_without_top_k_is_unsupported():
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_sample_select_rows failed \(-3\).*top_p = 0.9 without top_k") as e:
        _sample(top_k=0, top_p=0.9)
    assert not isinstance(e.value, ValueError)


def _process(logits=FAKE, dtype=1, ld=512, V=500, n=4, out_tokens=FAKE, ld_tok=64, row_step=FAKE, row_map=None, fin=None, BB=4, G=64, out=FAKE, ld_out=512,
             penalty=1.2, ngram=2, min_new=0, eos=None, n_eos=0, words=None, offsets=None, n_words=0, n_word_ids=0):
    from p2t_hip import _lib
    return _lib.call("p2t_logits_process_rows", logits, dtype, ld, V, n, out_tokens, ld_tok, row_step, row_map, fin, BB, G, out, ld_out, penalty, ngram, min_new,
                     eos, n_eos, words, offsets, n_words, n_word_ids, None)


@pytest.mark.parametrize("bad", [dict(logits=None), dict(out_tokens=None), dict(row_step=None), dict(out=None), dict(dtype=2), dict(n=0), dict(BB=0), dict(n=5),
                                 dict(n=2), dict(V=0), dict(ld=499), dict(ld_out=499), dict(ld_tok=63), dict(G=0), dict(penalty=0.0), dict(penalty=float("inf")),
                                 dict(ngram=-1), dict(min_new=-1), dict(n_eos=1), dict(n_eos=-1), dict(n_words=1), dict(n_words=1, words=FAKE, offsets=FAKE),
                                 dict(n_words=-1)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_logits_process_rows_argument_errors(bad):
    """Null buffers (finished may be NULL: it is not among them), a bad dtype, the row-count rules, pitches below V or G, and
    processor_args_check's refusals under this entry point's name."""
    with pytest.raises(ValueError, match="p2t_logits_process_rows"):
        _process(**bad)


def test_the_lock_step_twins_keep_their_messages():
    """The shared checks name the entry point that was called."""
    from p2t_hip import _lib
    with pytest.raises(ValueError, match=r"p2t_sample_select: top_k = 2000: 0 \(off\) or 1 \.\. 1024"):
        _lib.call("p2t_sample_select", FAKE, 1, 512, 500, 4, None, 0, 0, FAKE, FAKE, FAKE, 64, FAKE, 64, 1.0, 2000, 1.0, 7, 0, None, 0, FAKE, None)
    with pytest.raises(_lib.P2TError, match=r"p2t_sample_select failed \(-3\)"):
        _lib.call("p2t_sample_select", FAKE, 1, 512, 500, 4, None, 0, 0, FAKE, FAKE, FAKE, 64, FAKE, 64, 1.0, 0, 0.5, 7, 0, None, 0, FAKE, None)
    with pytest.raises(ValueError, match="p2t_logits_process: repetition_penalty 0 is not"):
        _lib.call("p2t_logits_process", FAKE, 1, 512, 500, 4, FAKE, 64, FAKE, 64, FAKE, 512, 0.0, 0, 0, None, 0, None, None, 0, 0, None)
