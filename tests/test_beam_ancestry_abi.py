"""CPU: the entry points of beam search without the cache copy (include/p2t_hip.h: p2t_kv_ancestry_update, p2t_attention_decode_beams,
p2t_llama_decode_step_beams) are declared, exported and bound, p2t_kv_cache keeps its size (the table travels beside it), and every
call outside the contract is refused before any GPU call -- P2T_ERR_ARG as ValueError, what the kernels do not serve as
P2T_ERR_UNSUPPORTED (-3)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = {"p2t_kv_ancestry_update": 4, "p2t_attention_decode_beams": 24, "p2t_llama_decode_step_beams": 17}
FAKE = 4096          # a non-null, 16-byte aligned "pointer": never dereferenced, the checks come first


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    # the step: p2t_llama_decode_step_q's arguments, then the table in front of the stream
    q, beams = _lib.SIGNATURES["p2t_llama_decode_step_q"][1], _lib.SIGNATURES["p2t_llama_decode_step_beams"][1]
    assert beams[:15] == q[:15] and beams[-1] == q[-1] and len(beams) == len(q) + 1
    # the attention: p2t_attention_decode_prompt_fp8's arguments, then the table in front of the stream
    f8, ab = _lib.SIGNATURES["p2t_attention_decode_prompt_fp8"][1], _lib.SIGNATURES["p2t_attention_decode_beams"][1]
    assert ab[:22] == f8[:22] and ab[-1] == f8[-1] and len(ab) == len(f8) + 1
    # p2t_kv_cache keeps its layout: no new struct either
    assert _lib.lib.p2t_struct_size(10) == C.sizeof(_lib.KvCacheC) == 6 * 8 + 4 * 4 + 2 * 8
    assert _lib.lib.p2t_struct_size(len(_lib._STRUCTS)) == 0


def _cfg(dtype=1, **kw):
    from p2t_hip import _lib
    base = dict(n_layers=2, hidden=128, ffn=256, heads=4, kv_heads=2, head_dim=64, vocab=512, dtype=dtype, rms_norm_eps=1e-5, rope_theta=1e4)
    base.update(kw)
    return _lib.LlamaConfigC(**base)


def _cache(**kw):
    from p2t_hip import _lib
    base = dict(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=FAKE, B0=2, group=3, Tp=64, G=64)
    base.update(kw)
    return _lib.KvCacheC(**base)


def _update(cache=None, src=FAKE, anc=FAKE):
    from p2t_hip import _lib
    return _lib.call("p2t_kv_ancestry_update", C.byref(cache) if cache is not False else None, src, anc, None)


@pytest.mark.parametrize("bad,match", [
    (dict(cache=False), "null argument"), (dict(src=None), "null argument"), (dict(anc=None), "null ancestry table"),
    (dict(anc=FAKE + 8), "16-byte aligned"), (dict(cache=dict(step=None)), "null argument"), (dict(cache=dict(group=1)), "group >= 2"),
    (dict(cache=dict(group=0)), "group >= 2"), (dict(cache=dict(G=100)), "multiple of 64"), (dict(cache=dict(B0=0)), "prompts"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_update_argument_errors(bad, match):
    if isinstance(bad.get("cache"), dict):
        bad = dict(bad, cache=_cache(**bad["cache"]))
    elif "cache" not in bad:
        bad = dict(bad, cache=_cache())
    with pytest.raises(ValueError, match="p2t_kv_ancestry_update.*" + match):
        _update(**bad)


def test_update_more_than_16_rows_per_prompt_is_unsupported():
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_kv_ancestry_update failed \(-3\).*at most 16 rows") as e:
        _update(cache=_cache(group=17))
    assert not isinstance(e.value, ValueError)


def _attn(q=FAKE, kp=FAKE, lens=FAKE, step=FAKE, B0=2, group=3, nh=4, nkv=2, d=64, Tp=128, G=64, dtype=1, use_mfma=1, out=FAKE, ld_out=256, ks=None, vs=None,
          anc=FAKE):
    from p2t_hip import _lib
    return _lib.call("p2t_attention_decode_beams", q, kp, FAKE, FAKE, FAKE, lens, step, B0, group, nh, nkv, d, Tp, G, 0.125, 1, dtype, use_mfma, out, ld_out, ks,
                     vs, anc, None)


def test_attention_beams_argument_errors():
    from p2t_hip import _lib
    for bad in (dict(anc=None), dict(group=1), dict(ks=FAKE), dict(vs=FAKE), dict(q=None), dict(kp=None), dict(lens=None), dict(step=None), dict(Tp=100),
                dict(G=32), dict(nh=5), dict(nkv=0), dict(ld_out=255), dict(dtype=0, use_mfma=1)):
        with pytest.raises(ValueError, match="p2t_attention_decode"):
            _attn(**bad)
    for bad in (dict(group=17), dict(nh=34, ld_out=34 * 64), dict(ks=FAKE, vs=FAKE, use_mfma=0), dict(ks=FAKE, vs=FAKE, dtype=0, use_mfma=0)):
        with pytest.raises(_lib.P2TError, match=r"p2t_attention_decode_beams failed \(-3\)") as e:
            _attn(**bad)
        assert not isinstance(e.value, ValueError)


def _step(cache=None, anc=FAKE, ws_bytes=1 << 30, layers_ok=True, cfg=None):
    from p2t_hip import _lib
    cfg = cfg or _cfg()
    layers = (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=layers if layers_ok else None, final_norm_w=FAKE)
    return _lib.call("p2t_llama_decode_step_beams", C.byref(cfg), C.byref(w), None, None, FAKE, 128, 0, None, C.byref(cache or _cache()), FAKE, FAKE, 512, 0, FAKE,
                     ws_bytes, anc, None)


def test_step_beams_argument_errors():
    from p2t_hip import _lib
    with pytest.raises(ValueError, match="p2t_llama_decode_step_beams: null ancestry table"):
        _step(anc=None)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_beams.*group >= 2"):
        _step(cache=_cache(group=1))
    for bad in (dict(cache=_cache(group=17)), dict(cfg=_cfg(heads=34))):
        with pytest.raises(_lib.P2TError, match=r"p2t_llama_decode_step_beams failed \(-3\)") as e:
            _step(**bad)
        assert not isinstance(e.value, ValueError)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_beams: null argument"):
        _step(layers_ok=False)
    with pytest.raises(ValueError, match="capacities"):
        _step(cache=_cache(G=100))
    with pytest.raises(ValueError, match="null cache field"):
        _step(cache=_cache(step=None))
    with pytest.raises(ValueError, match="p2t_llama_decode_step_beams: workspace too small"):      # the last check: every one before it passed
        _step(ws_bytes=16)


def test_the_existing_doors_take_no_table():
    """p2t_llama_decode_step_q and p2t_attention_decode on a beam group, with the arguments they always took: each still stops at the
    check that was always its last."""
    from p2t_hip import _lib
    cfg, layers = _cfg(), (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=layers, final_norm_w=FAKE)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: workspace too small"):
        _lib.call("p2t_llama_decode_step_q", C.byref(cfg), C.byref(w), None, None, FAKE, 128, 0, None, C.byref(_cache()), FAKE, FAKE, 512, 0, FAKE, 16, None)
    with pytest.raises(ValueError, match="p2t_attention_decode: bad arguments"):
        _lib.call("p2t_attention_decode", FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 3, 4, 2, 64, 128, 64, 0.125, 1, 1, 1, FAKE, 255, None)
