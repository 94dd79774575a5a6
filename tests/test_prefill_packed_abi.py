"""CPU: the entry points of the padding-free prefill (include/p2t_hip.h: p2t_prompt_index, p2t_pack_rows, p2t_kv_store_packed,
p2t_llama_prefill_packed + its workspace size) are declared, exported and bound; p2t_kv_cache keeps its layout; and every call outside
the contract is refused before any GPU call -- P2T_ERR_ARG as ValueError, what the kernels do not serve as P2T_ERR_UNSUPPORTED (-3)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = {"p2t_prompt_index": 6, "p2t_pack_rows": 13, "p2t_kv_store_packed": 10, "p2t_llama_prefill_packed": 14,
         "p2t_llama_prefill_packed_workspace_bytes": 3}
FAKE = 4096          # a non-null, 16-byte aligned "pointer": never dereferenced, the checks come first


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    i32, vp, sz = C.c_int32, C.c_void_p, C.c_size_t
    cfg, w, kc, host = C.POINTER(_lib.LlamaConfigC), C.POINTER(_lib.LlamaWeightsC), C.POINTER(_lib.KvCacheC), C.POINTER(C.c_int32)
    assert _lib.SIGNATURES["p2t_prompt_index"] == (i32, [vp, i32, i32, vp, vp, vp])
    assert _lib.SIGNATURES["p2t_pack_rows"] == (i32, [vp, vp, vp, i32, i32, i32, host, i32, i32, vp, vp, vp, vp])
    assert _lib.SIGNATURES["p2t_kv_store_packed"] == (i32, [cfg, kc, i32, vp, vp, i32, i32, host, i32, vp])
    assert _lib.SIGNATURES["p2t_llama_prefill_packed"] == (i32, [cfg, w, vp, vp, vp, i32, i32, i32, host, kc, vp, vp, sz, vp])
    assert _lib.SIGNATURES["p2t_llama_prefill_packed_workspace_bytes"] == (sz, [cfg, i32, i32])
    # the padded door keeps its arguments, p2t_kv_cache its layout, and no struct was added
    assert _lib.SIGNATURES["p2t_llama_prefill"] == (i32, [cfg, w, vp, vp, i32, i32, kc, vp, vp, sz, vp])
    assert _lib.lib.p2t_struct_size(10) == C.sizeof(_lib.KvCacheC) == 6 * 8 + 4 * 4 + 2 * 8
    assert _lib.lib.p2t_struct_size(len(_lib._STRUCTS)) == 0


def _cfg(dtype=1, **kw):
    from p2t_hip import _lib
    base = dict(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=dtype, rms_norm_eps=1e-5, rope_theta=1e4)
    base.update(kw)
    return _lib.LlamaConfigC(**base)


def _cache(**kw):
    from p2t_hip import _lib
    base = dict(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=FAKE, B0=3, group=1, Tp=128, G=64)
    base.update(kw)
    return _lib.KvCacheC(**base)


PLACE = ((0, 0, 100), (0, 100, 28), (1, 0, 7))           # 3 prompts in 2 rows of 128 tokens


def _arr(place):
    flat = [v for p in place for v in p]
    return (C.c_int32 * max(len(flat), 1))(*flat)


def _prefill(place=PLACE, n=None, R=2, Tpk=128, cache=None, cfg=None, embeds=FAKE, docs=FAKE, ws_bytes=1 << 30):
    from p2t_hip import _lib
    layers = (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=layers, final_norm_w=FAKE)
    n = len(place) if n is None else n
    return _lib.call("p2t_llama_prefill_packed", C.byref(cfg or _cfg()), C.byref(w), embeds, FAKE, docs, R, Tpk, n, _arr(place), C.byref(cache or _cache(B0=n)),
                     FAKE, FAKE, ws_bytes, None)


def _store(place=PLACE, n=None, R=2, Tpk=128, cache=None, cfg=None, layer=1, k=FAKE, v=FAKE):
    from p2t_hip import _lib
    n = len(place) if n is None else n
    return _lib.call("p2t_kv_store_packed", C.byref(cfg or _cfg()), C.byref(cache or _cache(B0=n)), layer, k, v, R, Tpk, _arr(place), n, None)


def _pack(place=PLACE, B=None, T=130, H=64, R=2, Tpk=128, x=FAKE, out=2 * FAKE):
    from p2t_hip import _lib
    B = len(place) if B is None else B
    return _lib.call("p2t_pack_rows", x, FAKE, FAKE, B, T, H, _arr(place), R, Tpk, out, FAKE, FAKE, None)


BAD_PLACE = [
    (dict(place=((0, 0, 100), (0, 99, 28), (1, 0, 7))), r"prompts 0 and 1 overlap in packed row 0"),
    (dict(place=((0, 20, 50), (0, 0, 21), (1, 0, 7))), r"prompts 0 and 1 overlap in packed row 0"),
    (dict(place=((0, 0, 100), (0, 100, 29), (1, 0, 7))), r"prompt 1 \(start 100, 29 tokens\) does not fit a packed row of 128 tokens"),
    (dict(place=((0, 0, 100), (2, 0, 28), (1, 0, 7))), r"prompt 1 lies in packed row 2, outside \[0, 2\)"),
    (dict(place=((0, 0, 100), (-1, 0, 28), (1, 0, 7))), r"outside \[0, 2\)"),
    (dict(place=((0, 0, 100), (0, 100, 0), (1, 0, 7))), r"prompt 1 has 0 tokens"),
    (dict(place=((0, 0, 100), (1, -1, 8), (1, 7, 7))), r"does not fit"),
]


@pytest.mark.parametrize("bad,match", BAD_PLACE, ids=lambda v: v if isinstance(v, str) else None)
def test_a_bad_placement_is_refused_by_every_entry_point(bad, match):
    """Overlapping prompts, start + len > Tpk, rows outside the batch, empty prompts: the HOST array is checked before the launch."""
    for fn, name in ((_prefill, "p2t_llama_prefill_packed"), (_store, "p2t_kv_store_packed"), (_pack, "p2t_pack_rows")):
        with pytest.raises(ValueError, match=name + ".*" + match):
            fn(**bad)


def test_prefill_packed_argument_errors():
    from p2t_hip import _lib
    with pytest.raises(ValueError, match=r"p2t_llama_prefill_packed: prompt 0 has 100 tokens, the cache's prompt segment holds 64"):
        _prefill(cache=_cache(Tp=64))
    with pytest.raises(ValueError, match=r"p2t_llama_prefill_packed: cache holds 4 rows, the packed batch 3 prompts"):
        _prefill(cache=_cache(B0=4))
    with pytest.raises(ValueError, match="p2t_llama_prefill_packed: null/empty argument"):
        _prefill(docs=None)
    with pytest.raises(ValueError, match="p2t_llama_prefill_packed: null/empty argument"):
        _prefill(embeds=None)
    with pytest.raises(ValueError, match="p2t_llama_prefill_packed: null cache field"):
        _prefill(cache=_cache(k_prompt=None))
    with pytest.raises(ValueError, match="capacities"):
        _prefill(cache=_cache(Tp=100))
    with pytest.raises(ValueError, match="p2t_llama_prefill_packed: workspace too small"):       # the last check: everything else passed
        _prefill(ws_bytes=16)
    n = 257
    place = tuple((0, i, 1) for i in range(n))
    with pytest.raises(_lib.P2TError, match=r"p2t_llama_prefill_packed failed \(-3\).*at most 256 prompts") as e:
        _prefill(place=place, R=1, Tpk=320, cache=_cache(B0=n))
    assert not isinstance(e.value, ValueError)
    with pytest.raises(ValueError, match="workspace too small"):                                # 256 prompts are served
        _prefill(place=place[:256], R=1, Tpk=256, cache=_cache(B0=256), ws_bytes=16)
    with pytest.raises(_lib.P2TError, match=r"p2t_llama_prefill_packed failed \(-3\).*model-dtype GEMMs.*gemm_fp8"):
        _prefill(cfg=_cfg(gemm_fp8=1))
    with pytest.raises(_lib.P2TError, match=r"p2t_llama_prefill_packed failed \(-3\).*fp8 prompt segment serves bf16"):
        _prefill(cfg=_cfg(dtype=0), cache=_cache(k_prompt_scale=FAKE, v_prompt_scale=FAKE))
    assert _lib.call("p2t_llama_prefill_packed_workspace_bytes", C.byref(_cfg()), 2, 128) == _lib.call("p2t_llama_prefill_workspace_bytes", C.byref(_cfg()), 2, 128) > 0
    assert _lib.call("p2t_llama_prefill_packed_workspace_bytes", C.byref(_cfg()), 0, 128) == 0


def test_store_and_pack_argument_errors():
    from p2t_hip import _lib
    with pytest.raises(ValueError, match=r"p2t_kv_store_packed: prompt 0 has 100 tokens, the cache's prompt segment holds 64"):
        _store(cache=_cache(Tp=64))
    with pytest.raises(ValueError, match=r"p2t_kv_store_packed: cache holds 2 rows, the packed batch 3 prompts"):
        _store(cache=_cache(B0=2))
    with pytest.raises(ValueError, match=r"p2t_kv_store_packed: layer 2 outside \[0, 2\)"):
        _store(layer=2)
    with pytest.raises(ValueError, match="p2t_kv_store_packed: null argument"):
        _store(k=None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _store(v=FAKE + 8)
    with pytest.raises(ValueError, match="go together"):
        _store(cache=_cache(k_prompt_scale=FAKE))
    with pytest.raises(_lib.P2TError, match=r"p2t_kv_store_packed failed \(-3\).*at most 256 prompts"):
        _store(place=tuple((0, i, 1) for i in range(300)), R=1, Tpk=320, cache=_cache(B0=300))
    with pytest.raises(ValueError, match=r"p2t_pack_rows: bad arguments \(H must be a multiple of 4"):
        _pack(H=66)
    with pytest.raises(ValueError, match="p2t_pack_rows: bad arguments"):
        _pack(out=FAKE)                                                                          # in place
    with pytest.raises(ValueError, match=r"p2t_pack_rows: prompt 1 starts at token 101 of packed row 0 behind a gap"):
        _pack(place=((0, 0, 100), (0, 101, 27), (1, 0, 7)))
    with pytest.raises(_lib.P2TError, match=r"p2t_pack_rows failed \(-3\).*at most 256 prompts"):
        _pack(place=tuple((0, i, 1) for i in range(300)), R=1, Tpk=320)
    with pytest.raises(ValueError, match="p2t_prompt_index: null/empty argument"):
        _lib.call("p2t_prompt_index", FAKE, 2, 0, FAKE, FAKE, None)
    with pytest.raises(ValueError, match="p2t_prompt_index: null/empty argument"):
        _lib.call("p2t_prompt_index", FAKE, 2, 8, None, FAKE, None)


def test_the_padded_prefill_accepts_what_it_accepted():
    """The same fake arguments through p2t_llama_prefill: every argument check passes and it stops at its last one (the workspace size)."""
    from p2t_hip import _lib
    layers = (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=layers, final_norm_w=FAKE)
    with pytest.raises(ValueError, match="p2t_llama_prefill: workspace too small"):
        _lib.call("p2t_llama_prefill", C.byref(_cfg()), C.byref(w), FAKE, FAKE, 3, 100, C.byref(_cache()), FAKE, FAKE, 16, None)
