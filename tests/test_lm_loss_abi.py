"""CPU: the three entry points of the target-rows form in csrc/lm_loss.hip (the LM loss over the target rows only) are declared, exported and bound, and every
argument outside their contracts is P2T_ERR_ARG with a message before any GPU call (as tests/test_abi.py checks for the others)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = ("p2t_lm_target_rows", "p2t_lm_loss_grad_rows", "p2t_lm_loss_reduce")
FAKE = 4096          # a non-null, 16-byte aligned "pointer": never dereferenced, the checks come first


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES
    assert _lib.version() == 103


def _select(labels=FAKE, B=2, T=8, V=100, ignore=-100, cap=16, rows=FAKE, targets=FAKE, count=FAKE):
    from p2t_hip import _lib
    return _lib.call("p2t_lm_target_rows", labels, B, T, V, ignore, cap, rows, targets, count, None)


def _rows(logits=FAKE, ld=320, dtype=1, R=4, V=300, rows=FAKE, targets=FAKE, count=FAKE, first=0, cap=128, weights=None, n_weights=0,
          row_loss=FAKE, with_grad=1):
    from p2t_hip import _lib
    return _lib.call("p2t_lm_loss_grad_rows", logits, ld, dtype, R, V, rows, targets, count, first, cap, weights, n_weights, row_loss, with_grad, None)


def _reduce(row_loss=FAKE, rows=FAKE, count=FAKE, cap=128, weights=None, n_weights=0, loss=FAKE):
    from p2t_hip import _lib
    return _lib.call("p2t_lm_loss_reduce", row_loss, rows, count, cap, weights, n_weights, loss, None)


_ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(labels=None), dict(rows=None), dict(targets=None), dict(count=None), dict(B=0), dict(T=0), dict(V=0),
                                 dict(cap=0), dict(cap=-1), dict(B=1 << 16, T=1 << 15)], ids=_ids)
def test_target_rows_argument_errors(bad):
    with pytest.raises(ValueError, match="p2t_lm_target_rows"):
        _select(**bad)


@pytest.mark.parametrize("bad", [dict(logits=None), dict(rows=None), dict(targets=None), dict(count=None), dict(row_loss=None), dict(R=0),
                                 dict(V=0), dict(first=-1), dict(cap=0), dict(first=126), dict(R=129), dict(ld=256), dict(ld=300),
                                 dict(ld=0), dict(logits=FAKE + 8), dict(dtype=2), dict(dtype=-1), dict(weights=FAKE, n_weights=0)], ids=_ids)
def test_loss_grad_rows_argument_errors(bad):
    with pytest.raises(ValueError, match="p2t_lm_loss_grad_rows"):
        _rows(**bad)


@pytest.mark.parametrize("bad", [dict(row_loss=None), dict(rows=None), dict(count=None), dict(loss=None), dict(cap=0),
                                 dict(weights=FAKE, n_weights=0)], ids=_ids)
def test_reduce_argument_errors(bad):
    with pytest.raises(ValueError, match="p2t_lm_loss_reduce"):
        _reduce(**bad)


def test_the_message_names_the_offending_stride():
    with pytest.raises(ValueError, match=r"ld = 256 .* V = 300"):
        _rows(ld=256)
