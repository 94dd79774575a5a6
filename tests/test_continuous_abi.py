"""CPU: the entry points of continuous batching (include/p2t_hip.h: p2t_llama_decode_step_rows, p2t_greedy_select_rows,
p2t_kv_slot_load, p2t_attention_decode_rows) are declared, exported and bound, and every call outside the contract is refused before any
GPU call -- P2T_ERR_ARG as ValueError, what the kernels do not serve as P2T_ERR_UNSUPPORTED (-3).  The lock-step entry points still
pass their own checks with the arguments they always took."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = {"p2t_llama_decode_step_rows": 18, "p2t_greedy_select_rows": 18, "p2t_kv_slot_load": 10, "p2t_attention_decode_rows": 22}
FAKE = 4096          # a non-null, 16-byte aligned "pointer": never dereferenced, the checks come first


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    # the step: p2t_llama_decode_step_q's arguments, then row_step and frozen in front of the stream
    q, rows = _lib.SIGNATURES["p2t_llama_decode_step_q"][1], _lib.SIGNATURES["p2t_llama_decode_step_rows"][1]
    assert rows[:15] == q[:15] and rows[-1] == q[-1] and len(rows) == len(q) + 2
    # p2t_kv_cache keeps its layout: the counters travel beside it, no new struct
    assert _lib.lib.p2t_struct_size(10) == C.sizeof(_lib.KvCacheC) == 6 * 8 + 4 * 4 + 2 * 8
    assert _lib.lib.p2t_struct_size(len(_lib._STRUCTS)) == 0


def _cfg(dtype=1, **kw):
    from p2t_hip import _lib
    base = dict(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=dtype, rms_norm_eps=1e-5, rope_theta=1e4)
    base.update(kw)
    return _lib.LlamaConfigC(**base)


def _cache(**kw):
    from p2t_hip import _lib
    base = dict(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=None, B0=4, group=1, Tp=64, G=64)
    base.update(kw)
    return _lib.KvCacheC(**base)


def _step(cache=None, row_step=FAKE, frozen=None, ws_bytes=1 << 30, layers_ok=True, stream_layers=None, mx=None, cfg=None):
    from p2t_hip import _lib
    cfg = cfg or _cfg()
    layers = (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=layers if layers_ok else None, final_norm_w=FAKE)
    return _lib.call("p2t_llama_decode_step_rows", C.byref(cfg), C.byref(w), stream_layers, mx, FAKE, 128, 0, None, C.byref(cache or _cache()), FAKE, FAKE, 512, 0, FAKE,
                     ws_bytes, row_step, frozen, None)


def test_step_rows_argument_errors():
    from p2t_hip import _lib
    with pytest.raises(ValueError, match="p2t_llama_decode_step_rows: null row_step"):
        _step(row_step=None)
    with pytest.raises(_lib.P2TError, match=r"p2t_llama_decode_step_rows failed \(-3\).*group == 1") as e:
        _step(cache=_cache(B0=2, group=2))
    assert not isinstance(e.value, ValueError)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_rows: null argument"):
        _step(layers_ok=False)
    with pytest.raises(ValueError, match="capacities"):
        _step(cache=_cache(G=100))
    with pytest.raises(ValueError, match="go together"):
        _step(cache=_cache(k_prompt_scale=FAKE))
    with pytest.raises(ValueError, match="p2t_llama_decode_step_rows: workspace too small"):        # the last check: cache->step == NULL passed every one before
        _step(ws_bytes=16)
    with pytest.raises(ValueError, match="w_stream and mx_layers"):
        _step(stream_layers=(_lib.LlamaLayerStreamC * 2)(), mx=(_lib.LlamaLayerMxfp4C * 2)())
    with pytest.raises(ValueError, match="mx_layers need a gemm_fp8"):
        _step(mx=(_lib.LlamaLayerMxfp4C * 2)())


def _select(logits=FAKE, dtype=1, ld=512, V=500, n=4, eos=None, n_eos=0, fin=FAKE, nxt=FAKE, out=FAKE, ld_tok=64, row_step=FAKE, row_limit=FAKE, row_map=None,
            BB=4, G=64):
    from p2t_hip import _lib
    return _lib.call("p2t_greedy_select_rows", logits, dtype, ld, V, n, eos, n_eos, 0, fin, nxt, out, ld_tok, row_step, row_limit, row_map, BB, G, None)


@pytest.mark.parametrize("bad", [dict(logits=None), dict(fin=None), dict(nxt=None), dict(out=None), dict(row_step=None), dict(row_limit=None), dict(dtype=2),
                                 dict(n=0), dict(n=5), dict(n=2), dict(V=0), dict(ld=499), dict(ld_tok=63), dict(G=0), dict(n_eos=1), dict(n_eos=-1)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_select_rows_argument_errors(bad):
    """Null buffers, logits that are neither f32 nor bf16, more logits rows than engine rows, a subset without its row_map, a token table
    narrower than G, eos ids announced but not given."""
    with pytest.raises(ValueError, match="p2t_greedy_select_rows"):
        _select(**bad)


def _load(staging=None, cache=None, slots=(1, 3), limits=(5, 64), k=None, row_step=FAKE, fin=FAKE, row_limit=FAKE, cfg=None):
    from p2t_hip import _lib
    k = len(slots) if k is None else k
    staging = staging or _cache(B0=k)
    arr = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    return _lib.call("p2t_kv_slot_load", C.byref(cfg or _cfg()), C.byref(staging), C.byref(cache or _cache()), arr(slots), arr(limits), k, row_step, fin,
                     row_limit, None)


@pytest.mark.parametrize("bad,match", [
    (dict(slots=(1, 4)), r"slot 4 \(entry 1\) outside \[0, 4\)"),
    (dict(slots=(-1, 2)), "outside"),
    (dict(slots=(2, 2)), "slot 2 is named twice"),
    (dict(limits=(0, 5)), r"row limit 0 \(entry 0\) outside 1 \.\. 64"),
    (dict(limits=(5, 65)), "row limit 65"),
    (dict(staging=_cache(B0=2, Tp=128)), "staging cache holds 128 prompt tokens"),
    (dict(staging=_cache(B0=3)), "2 slots from a staging cache of 3 rows"),
    (dict(staging=_cache(B0=2, k_prompt_scale=FAKE, v_prompt_scale=FAKE)), "scale arrays on one of them only"),
    (dict(cache=_cache(k_prompt_scale=FAKE, v_prompt_scale=FAKE)), "scale arrays on one of them only"),
    (dict(staging=_cache(B0=2, k_prompt_scale=FAKE)), "go together"),
    (dict(cache=_cache(B0=2, group=2)), "group == 1"),
    (dict(staging=_cache(B0=2, k_prompt=FAKE + 8)), "16-byte aligned"),
    (dict(cache=_cache(vt_prompt=None)), "null cache field"),
    (dict(row_step=None), "null argument"), (dict(fin=None), "null argument"), (dict(row_limit=None), "null argument"),
    (dict(slots=(0, 1, 2, 3, 0), limits=(1,) * 5, staging=_cache(B0=5)), "5 slots from a staging cache of 5 rows into 4 slots"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_slot_load_argument_errors(bad, match):
    """Slots outside the engine or named twice, limits outside 1 .. G (host arrays: checked before the launch), a staging cache of another
    shape or format than the engine's."""
    with pytest.raises(ValueError, match="p2t_kv_slot_load.*" + match):
        _load(**bad)


def test_slot_load_fp8_on_an_f32_model_and_too_many_slots_are_unsupported():
    from p2t_hip import _lib
    sc = dict(k_prompt_scale=FAKE, v_prompt_scale=FAKE)
    with pytest.raises(_lib.P2TError, match=r"p2t_kv_slot_load failed \(-3\)"):
        _load(cfg=_cfg(dtype=0), staging=_cache(B0=2, **sc), cache=_cache(**sc))
    n = 300
    with pytest.raises(_lib.P2TError, match=r"p2t_kv_slot_load failed \(-3\).*at most 256 slots"):
        _load(slots=tuple(range(n)), limits=(1,) * n, staging=_cache(B0=n), cache=_cache(B0=n))


def _attn(q=FAKE, kp=FAKE, lens=FAKE, row_step=FAKE, B0=3, nh=4, nkv=2, d=64, Tp=128, G=64, dtype=1, use_mfma=1, out=FAKE, ld_out=256, ks=None, vs=None):
    from p2t_hip import _lib
    return _lib.call("p2t_attention_decode_rows", q, kp, FAKE, FAKE, FAKE, lens, row_step, B0, nh, nkv, d, Tp, G, 0.125, 1, dtype, use_mfma, out, ld_out, ks, vs, None)


def test_attention_rows_argument_errors():
    from p2t_hip import _lib
    for bad in (dict(row_step=None), dict(ks=FAKE), dict(vs=FAKE), dict(q=None), dict(kp=None), dict(lens=None), dict(Tp=100), dict(G=32), dict(nh=5),
                dict(ld_out=255), dict(dtype=0, use_mfma=1)):
        with pytest.raises(ValueError, match="p2t_attention_decode"):
            _attn(**bad)
    for bad in (dict(ks=FAKE, vs=FAKE, use_mfma=0), dict(ks=FAKE, vs=FAKE, dtype=0, use_mfma=0)):
        with pytest.raises(_lib.P2TError, match=r"p2t_attention_decode_rows failed \(-3\)"):
            _attn(**bad)


def test_the_lock_step_entry_points_accept_what_they_accepted():
    """The same fake arguments as above through p2t_llama_decode_step_q / p2t_greedy_select / p2t_attention_decode: each passes every
    argument check and stops at the one that was always its last (the workspace size), or needs its cache's own counter as before."""
    from p2t_hip import _lib
    cfg, layers = _cfg(), (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=layers, final_norm_w=FAKE)
    step = lambda cache, ws: _lib.call("p2t_llama_decode_step_q", C.byref(cfg), C.byref(w), None, None, FAKE, 128, 0, None, C.byref(cache), FAKE, FAKE, 512, 0, FAKE,
                                       ws, None)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: workspace too small"):
        step(_cache(step=FAKE), 16)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: workspace too small"):           # group > 1 is the lock-step entry points' own
        step(_cache(step=FAKE, B0=2, group=2), 16)
    with pytest.raises(ValueError, match="null cache field"):                                       # its counter is still required there
        step(_cache(step=None), 1 << 30)
    with pytest.raises(ValueError, match="p2t_greedy_select: bad arguments"):
        _lib.call("p2t_greedy_select", FAKE, 1, 512, 500, 4, None, 0, 0, FAKE, FAKE, FAKE, 63, FAKE, 64, None)
    with pytest.raises(ValueError, match="p2t_attention_decode: bad arguments"):
        _lib.call("p2t_attention_decode", FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 1, 4, 2, 64, 128, 64, 0.125, 1, 1, 1, FAKE, 255, None)
