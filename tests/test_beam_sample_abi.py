"""CPU: p2t_beam_sample_select (csrc/beam_sample_select.hip, the beam-sampling step) is declared, exported and bound, and every argument
outside its contract is refused with a message naming it before any GPU call (as tests/test_beam_select_abi.py checks for beam search):
P2T_ERR_ARG as ValueError, a well-formed call outside the supported range as P2T_ERR_UNSUPPORTED."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAME = "p2t_beam_sample_select"
FAKE = 4096          # a non-null "pointer": never dereferenced, the checks come first
FIELDS = ("run_seq", "run_idx", "run_scores", "fin_seq", "fin_idx", "fin_scores", "is_finished", "heuristic_open", "done", "sync", "workspace")


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, src), f"{NAME} is not declared in include/p2t_hip.h"
    assert re.search(r"\bp2t_beam_sample_workspace_bytes\s*\(", src)
    assert hasattr(_lib.lib, NAME) and hasattr(_lib.lib, "p2t_beam_sample_workspace_bytes"), f"{NAME} is not exported"
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 26
    assert _lib.SIGNATURES[NAME][1][:19] == _lib.SIGNATURES["p2t_beam_select"][1][:19]          # p2t_beam_select's arguments first
    assert _lib.call("p2t_beam_sample_workspace_bytes", 3, 5) == 3 * 5 * (3 * 64 + 1) * 4
    assert _lib.call("p2t_beam_sample_workspace_bytes", 0, 5) == 0 and _lib.call("p2t_beam_sample_workspace_bytes", 2, -1) == 0
    # the neighbours keep their signatures
    assert len(_lib.SIGNATURES["p2t_beam_select"][1]) == 20 and len(_lib.SIGNATURES["p2t_sample_select"][1]) == 23
    assert _lib.call("p2t_beam_workspace_bytes", 3, 5) == 3 * 5 * (2 * 64 + 2) * 4


def _call(logits=FAKE, dtype=1, ld=320, B0=2, nb=3, V=300, eos=None, n_eos=0, pad=0, lp=1.0, es=0, max_length=20, G=64, step=FAKE, state=True,
          nxt=FAKE, src=FAKE, scores=None, ld_scores=0, temperature=0.7, top_k=50, top_p=0.9, seed=1, prompt0=0, flags=FAKE, **fields):
    from p2t_hip import _lib
    st = _lib.BeamStateC(**{**{n: FAKE for n in FIELDS}, **fields}) if state else None
    return _lib.call(NAME, logits, dtype, ld, B0, nb, V, eos, n_eos, pad, lp, es, max_length, G, step, ctypes.byref(st) if st is not None else None,
                     nxt, src, scores, ld_scores, temperature, top_k, top_p, seed, prompt0, flags, None)


_ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(logits=None), dict(step=None), dict(state=False), dict(nxt=None), dict(src=None), dict(flags=None)]
                         + [{n: None} for n in FIELDS]
                         + [dict(B0=0), dict(B0=-1), dict(nb=0), dict(nb=-2), dict(V=0), dict(V=-5), dict(ld=299), dict(ld=0), dict(dtype=2), dict(dtype=-1),
                            dict(n_eos=-1), dict(n_eos=1, eos=None), dict(G=0), dict(G=96), dict(G=-64), dict(max_length=0), dict(max_length=65),
                            dict(max_length=129, G=128), dict(lp=float("nan")), dict(es=3), dict(es=-1), dict(scores=FAKE, ld_scores=299),
                            dict(scores=FAKE, ld_scores=0),
                            dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                            dict(top_k=-1), dict(top_k=1025), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=float("nan"))], ids=_ids)
def test_argument_errors(bad):
    with pytest.raises(ValueError, match=NAME):
        _call(**bad)


@pytest.mark.parametrize("bad", [dict(nb=17), dict(nb=22, n_eos=2, eos=FAKE), dict(nb=13, n_eos=4, eos=FAKE), dict(nb=16, V=20, ld=64)], ids=_ids)
def test_outside_the_beam_range_is_unsupported(bad):
    """nb = 17; keep = 3 * 22 = 66 and 5 * 13 = 65 > 64; a vocabulary smaller than keep."""
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_beam_sample_select failed \(-3\).*num_beams") as e:
        _call(**bad)
    assert not isinstance(e.value, ValueError)


@pytest.mark.parametrize("bad", [dict(top_k=0, top_p=0.9), dict(top_k=0, top_p=0.01)], ids=_ids)
def test_top_p_without_top_k_is_unsupported(bad):
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_beam_sample_select failed \(-3\).*top_p") as e:
        _call(**bad)
    assert not isinstance(e.value, ValueError)


def test_an_argument_error_comes_before_the_unsupported_combination():
    with pytest.raises(ValueError, match=NAME):
        _call(nb=17, ld=10)
    with pytest.raises(ValueError, match=NAME):
        _call(top_k=0, top_p=0.9, temperature=0.0)
    with pytest.raises(ValueError, match=NAME):
        _call(nb=13, n_eos=4, eos=FAKE, top_k=2000)


def test_generate_checks_the_sampling_arguments_up_front():
    from p2t_hip import generation as G
    ok = G._beam_sampling_args(3, 1, 0.7, 50, 0.9, 3, None, "device")
    assert ok["device"] and ok["top_k"] == 50 and abs(ok["top_p"] - 0.9) < 1e-12 and ok["seed"] == 3
    assert G._beam_sampling_args(3, 1, None, None, None, 3, None, "device")["top_k"] == 0
    for kw in (dict(seed=None, generator=None, beam_select=None), dict(seed=None, generator=None, beam_select="device"),
               dict(seed=1, generator=None, beam_select=None), dict(seed=1, generator=None, beam_select="torch"),
               dict(seed=None, generator=object(), beam_select="device"), dict(seed=None, generator=object(), beam_select=None)):
        with pytest.raises(NotImplementedError, match=r"seed=.*beam_select='device'"):
            G._beam_sampling_args(2, 0, 1.0, 50, 1.0, **kw)
    with pytest.raises(ValueError, match="not both"):
        G._beam_sampling_args(2, 0, 1.0, 50, 1.0, 1, object(), "device")
    for kw, msg in ((dict(top_k=1025), "1 .. 1024"), (dict(top_k=0, top_p=0.9), "1 .. 1024"), (dict(temperature=0.0), "temperature"),
                    (dict(temperature=float("inf")), "temperature"), (dict(top_p=0.0), "top_p"), (dict(top_k=5), "top_k = 5 cannot supply"),
                    (dict(top_k=1), "cannot supply")):
        args = {**dict(temperature=1.0, top_k=50, top_p=1.0), **kw}
        with pytest.raises(ValueError, match=msg):
            G._beam_sampling_args(3, 1, args["temperature"], args["top_k"], args["top_p"], 7, None, "device")
    assert G._beam_sampling_args(3, 1, 1.0, 6, 1.0, 7, None, "device")["top_k"] == 6          # top_k == keep is enough
