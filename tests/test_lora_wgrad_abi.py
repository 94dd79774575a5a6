"""CPU: p2t_lora_wgrad (csrc/lora_wgrad.hip) is declared, exported and bound, its workspace sizing runs without a device, and every
argument outside its contract is P2T_ERR_ARG before any GPU call (as tests/test_abi.py checks for the other entry points)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = ("p2t_lora_wgrad", "p2t_lora_wgrad_workspace_bytes")
FAKE = 4096          # a non-null "pointer": never dereferenced, the checks come first


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES
    assert _lib.version() == 103


def _call(X=FAKE, ld_x=32, U=FAKE, ld_u=64, dtype=1, G=FAKE, ld_g=16, transposed=0, M=8, C=24, R=16, p=0.0, ws=FAKE, ws_bytes=1 << 30):
    from p2t_hip import _lib
    return _lib.call("p2t_lora_wgrad", X, ld_x, U, ld_u, dtype, G, ld_g, transposed, M, C, R, p, 0, ws, ws_bytes, None)


@pytest.mark.parametrize("bad", [dict(X=None), dict(U=None), dict(G=None), dict(ws=None), dict(R=0), dict(R=65, ld_u=128, ld_g=128),
                                 dict(C=20), dict(ld_x=36), dict(M=0), dict(C=0), dict(dtype=2), dict(p=1.0), dict(ld_x=16), dict(ld_u=8),
                                 dict(ld_g=8), dict(transposed=1, ld_g=16), dict(ws_bytes=16)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_argument_errors_without_gpu(bad):
    with pytest.raises(ValueError, match="p2t_lora_wgrad"):
        _call(**bad)


def test_f32_takes_any_column_count_as_far_as_the_checks_go():
    """fp32 has no multiple-of-8 rule: C = 20 passes the dtype check and fails only on the workspace it is then given."""
    with pytest.raises(ValueError, match="workspace"):
        _call(dtype=0, C=20, ws_bytes=0)


def test_workspace_sizing():
    from p2t_hip import _lib
    size = lambda C, R, M: _lib.call("p2t_lora_wgrad_workspace_bytes", C, R, M)
    for C, R, M in ((8, 4, 1), (136, 16, 200), (4096, 64, 4864), (14336, 16, 4864)):
        b = size(C, R, M)
        assert b >= C * R * 4 and b % (C * R * 4) == 0            # f32 [splits, C, R]
        assert b // (C * R * 4) <= -(-M // 64)                    # never more splits than 64-token tiles
    assert size(8, 4, 1) == 8 * 4 * 4                             # one tile: one split
    assert size(8, 4, 200) > 8 * 4 * 4                            # few columns, several tiles: the token axis is split
    assert size(0, 4, 8) == 0 and size(8, 0, 8) == 0 and size(8, 65, 8) == 0 and size(8, 4, 0) == 0
