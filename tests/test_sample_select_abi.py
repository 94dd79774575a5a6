"""CPU: p2t_sample_select (csrc/sample_select.hip, the sampled token choice) is declared, exported and bound, and every argument outside
its contract is refused with a message naming it before any GPU call (as tests/test_lm_loss_abi.py checks for the LM-loss entry points):
P2T_ERR_ARG as ValueError, top-p without top-k as P2T_ERR_UNSUPPORTED."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAME = "p2t_sample_select"
FAKE = 4096          # a non-null "pointer": never dereferenced, the checks come first


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, src), f"{NAME} is not declared in include/p2t_hip.h"
    assert hasattr(_lib.lib, NAME), f"{NAME} is not exported"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 23
    assert _lib.version() == 103


def _call(logits=FAKE, dtype=1, ld=320, V=300, BB=2, eos=None, n_eos=0, pad=0, finished=FAKE, nxt=FAKE, out=FAKE, ld_tokens=64, step=FAKE, G=64,
          temperature=1.0, top_k=50, top_p=1.0, seed=0, row0=0, scores=None, ld_scores=0, flags=FAKE):
    from p2t_hip import _lib
    return _lib.call(NAME, logits, dtype, ld, V, BB, eos, n_eos, pad, finished, nxt, out, ld_tokens, step, G, temperature, top_k, top_p, seed, row0,
                     scores, ld_scores, flags, None)


_ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(logits=None), dict(finished=None), dict(nxt=None), dict(out=None), dict(step=None), dict(flags=None),
                                 dict(BB=0), dict(BB=-3), dict(V=0), dict(V=-1), dict(ld=299), dict(ld=0), dict(temperature=0.0),
                                 dict(temperature=-0.5), dict(temperature=float("nan")), dict(top_k=-1), dict(top_k=1025), dict(top_p=0.0),
                                 dict(top_p=-0.1), dict(top_p=float("nan")), dict(dtype=2), dict(dtype=-1), dict(scores=FAKE, ld_scores=299),
                                 dict(scores=FAKE, ld_scores=0), dict(n_eos=1, eos=None), dict(n_eos=-1), dict(G=0), dict(ld_tokens=63)], ids=_ids)
def test_argument_errors(bad):
    with pytest.raises(ValueError, match=NAME):
        _call(**bad)


@pytest.mark.parametrize("bad", [dict(top_k=0, top_p=0.9), dict(top_k=0, top_p=0.5, scores=FAKE, ld_scores=300)], ids=_ids)
def test_top_p_without_top_k_is_unsupported(bad):
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_sample_select failed \(-3\).*top_k") as e:
        _call(**bad)
    assert not isinstance(e.value, ValueError)


def test_an_argument_error_comes_before_the_unsupported_combination():
    with pytest.raises(ValueError, match=NAME):
        _call(top_k=0, top_p=0.9, temperature=0.0)
