"""CPU: p2t_beam_select (csrc/beam_select.hip, the beam-search step) is declared, exported and bound, and every argument outside its
contract is refused with a message naming it before any GPU call (as tests/test_sample_select_abi.py checks for the sampler):
P2T_ERR_ARG as ValueError, a well-formed call outside the supported range as P2T_ERR_UNSUPPORTED."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAME = "p2t_beam_select"
FAKE = 4096          # a non-null "pointer": never dereferenced, the checks come first
FIELDS = ("run_seq", "run_idx", "run_scores", "fin_seq", "fin_idx", "fin_scores", "is_finished", "heuristic_open", "done", "sync", "workspace")


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, src), f"{NAME} is not declared in include/p2t_hip.h"
    assert re.search(r"\}\s*p2t_beam_state\s*;", src) and re.search(r"\bp2t_beam_workspace_bytes\s*\(", src)
    assert hasattr(_lib.lib, NAME), f"{NAME} is not exported"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 20
    assert tuple(n for n, _ in _lib.BeamStateC._fields_) == FIELDS
    assert _lib.lib.p2t_struct_size(14) == ctypes.sizeof(_lib.BeamStateC) == 8 * len(FIELDS)
    assert _lib.call("p2t_beam_workspace_bytes", 3, 5) == 3 * 5 * (2 * 64 + 2) * 4 and _lib.call("p2t_beam_workspace_bytes", 0, 5) == 0
    assert _lib.version() == 103


def _call(logits=FAKE, dtype=1, ld=320, B0=2, nb=3, V=300, eos=None, n_eos=0, pad=0, lp=1.0, es=0, max_length=20, G=64, step=FAKE, state=True,
          nxt=FAKE, src=FAKE, scores=None, ld_scores=0, **fields):
    from p2t_hip import _lib
    st = _lib.BeamStateC(**{**{n: FAKE for n in FIELDS}, **fields}) if state else None
    return _lib.call(NAME, logits, dtype, ld, B0, nb, V, eos, n_eos, pad, lp, es, max_length, G, step, ctypes.byref(st) if st is not None else None,
                     nxt, src, scores, ld_scores, None)


_ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(logits=None), dict(step=None), dict(state=False), dict(nxt=None), dict(src=None)]
                         + [{n: None} for n in FIELDS]
                         + [dict(B0=0), dict(B0=-1), dict(nb=0), dict(nb=-2), dict(V=0), dict(V=-5), dict(ld=299), dict(ld=0), dict(dtype=2), dict(dtype=-1),
                            dict(n_eos=-1), dict(n_eos=1, eos=None), dict(G=0), dict(G=96), dict(G=-64), dict(max_length=0), dict(max_length=65),
                            dict(max_length=129, G=128), dict(lp=float("nan")), dict(es=3), dict(es=-1), dict(scores=FAKE, ld_scores=299),
                            dict(scores=FAKE, ld_scores=0)], ids=_ids)
def test_argument_errors(bad):
    with pytest.raises(ValueError, match=NAME):
        _call(**bad)


@pytest.mark.parametrize("bad", [dict(nb=17), dict(nb=22, n_eos=2, eos=FAKE), dict(nb=13, n_eos=4, eos=FAKE), dict(nb=16, V=20, ld=64)], ids=_ids)
def test_outside_the_supported_range_is_unsupported(bad):
    """nb = 17; keep = 3 * 22 = 66 and 5 * 13 = 65 > 64; a vocabulary smaller than keep."""
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_beam_select failed \(-3\).*num_beams") as e:
        _call(**bad)
    assert not isinstance(e.value, ValueError)


def test_an_argument_error_comes_before_the_unsupported_combination():
    with pytest.raises(ValueError, match=NAME):
        _call(nb=17, ld=10)
    with pytest.raises(ValueError, match=NAME):
        _call(nb=13, n_eos=4, eos=FAKE, G=100)


def test_generate_refuses_a_bad_keyword_and_knows_the_range():
    from p2t_hip import generation as G
    assert G.beam_select_supported(8, 4, 1, 128256) and G.beam_select_supported(1, 16, 1, 1000) and G.beam_select_supported(3, 16, 3, 1000)
    assert not G.beam_select_supported(1, 17, 0, 1000) and not G.beam_select_supported(1, 13, 4, 1000) and not G.beam_select_supported(1, 16, 1, 20)
    assert G.beam_keep(3, 0) == 6 and G.beam_keep(3, 1) == 6 and G.beam_keep(3, 2) == 9
