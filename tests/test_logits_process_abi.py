"""CPU: p2t_logits_process (csrc/logits_process.hip, the logits processors in front of the token selectors) is declared, exported and
bound, and every argument outside its contract is refused with a message naming it before any GPU call (as
tests/test_sample_select_abi.py checks for the sampler): P2T_ERR_ARG as ValueError."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAME = "p2t_logits_process"
FAKE = 4096          # a non-null "pointer": never dereferenced, the checks come first


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, src), f"{NAME} is not declared in include/p2t_hip.h"
    assert hasattr(_lib.lib, NAME), f"{NAME} is not exported"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 21
    assert _lib.version() == 103


def _call(logits=FAKE, dtype=1, ld=320, V=300, BB=2, out_tokens=FAKE, ld_tokens=64, step=FAKE, G=64, out=FAKE, ld_out=320, penalty=1.3, ngram=2,
          min_new=0, eos=None, n_eos=0, words=None, offsets=None, n_words=0, n_word_ids=0):
    from p2t_hip import _lib
    return _lib.call(NAME, logits, dtype, ld, V, BB, out_tokens, ld_tokens, step, G, out, ld_out, penalty, ngram, min_new, eos, n_eos, words, offsets,
                     n_words, n_word_ids, None)


_ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(logits=None), dict(out_tokens=None), dict(step=None), dict(out=None), dict(dtype=2), dict(dtype=-1),
                                 dict(ld=299), dict(ld=0), dict(ld_out=299), dict(ld_out=0), dict(BB=0), dict(BB=-3), dict(V=0), dict(V=-1),
                                 dict(G=0), dict(G=-2), dict(ld_tokens=63), dict(penalty=0.0), dict(penalty=-1.5), dict(penalty=float("inf")),
                                 dict(penalty=float("nan")), dict(ngram=-1), dict(min_new=-1), dict(n_eos=1, eos=None), dict(n_eos=-1),
                                 dict(n_words=1, n_word_ids=1, words=None, offsets=FAKE), dict(n_words=1, n_word_ids=1, words=FAKE, offsets=None),
                                 dict(n_words=1, n_word_ids=0, words=FAKE, offsets=FAKE), dict(n_words=-1)], ids=_ids)
def test_argument_errors(bad):
    with pytest.raises(ValueError, match=NAME):
        _call(**bad)
