"""CPU: the entry points of prompt-lookup decoding (include/p2t_hip.h: p2t_lookup_draft_rows, p2t_attention_decode_multi,
p2t_llama_decode_step_multi, p2t_lookup_verify_rows) are declared, exported and bound; the doors beside them keep their arguments; and
every call outside the contract is refused before any GPU call -- P2T_ERR_ARG as ValueError, what the kernels do not serve as
P2T_ERR_UNSUPPORTED (-3)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = {"p2t_lookup_draft_rows": 12, "p2t_attention_decode_multi": 23, "p2t_llama_decode_step_multi": 18, "p2t_lookup_verify_rows": 21}
FAKE = 4096          # a non-null, 16-byte aligned "pointer": never dereferenced, the checks come first


def _args(name):
    """the declaration's arguments in the header, as a list of strings"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
    assert m, f"{name} is not declared in include/p2t_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    for name, nargs in NAMES.items():
        assert len(_args(name)) == nargs, name
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    i32, i64, f32, vp, sz = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t
    cfg, w, kc = C.POINTER(_lib.LlamaConfigC), C.POINTER(_lib.LlamaWeightsC), C.POINTER(_lib.KvCacheC)
    ws, mx, hq = C.POINTER(_lib.LlamaLayerStreamC), C.POINTER(_lib.LlamaLayerMxfp4C), C.POINTER(_lib.LmHeadQC)
    S = _lib.SIGNATURES
    assert S["p2t_lookup_draft_rows"] == (i32, [vp, i64, vp, vp, i32, i32, i32, i32, i64, vp, vp, vp])
    assert S["p2t_lookup_verify_rows"] == (i32, [vp, i32, i64, i32, i32, i32, vp, vp, vp, i32, i64, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp])
    # the multi doors: the per-row doors' arguments with q_tokens in front of the stream (the step: without `frozen`)
    rows = S["p2t_attention_decode_rows"][1]
    assert S["p2t_attention_decode_multi"] == (i32, rows[:-1] + [i32, vp])
    step = S["p2t_llama_decode_step_rows"][1]
    assert step == [cfg, w, ws, mx, vp, i64, i32, hq, kc, vp, vp, i64, i32, vp, sz, vp, vp, vp]
    assert S["p2t_llama_decode_step_multi"] == (i32, step[:-2] + [i32, vp])
    assert [a.split()[-1].lstrip("*") for a in _args("p2t_attention_decode_multi")][-2:] == ["q_tokens", "stream"]
    assert [a.split()[-1].lstrip("*") for a in _args("p2t_llama_decode_step_multi")][-3:] == ["row_step", "q_tokens", "stream"]
    assert "const int32_t* row_step" in _args("p2t_llama_decode_step_multi")          # read only: the verify kernel advances it
    # no struct was added and the library keeps its version
    assert _lib.lib.p2t_struct_size(len(_lib._STRUCTS)) == 0 and _lib.version() == 103


def _cfg(dtype=1, **kw):
    from p2t_hip import _lib
    base = dict(n_layers=2, hidden=128, ffn=256, heads=4, kv_heads=2, head_dim=64, vocab=512, dtype=dtype, rms_norm_eps=1e-5, rope_theta=1e4)
    base.update(kw)
    return _lib.LlamaConfigC(**base)


def _cache(**kw):
    from p2t_hip import _lib
    base = dict(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=None, B0=3, group=1, Tp=128, G=64)
    base.update(kw)
    return _lib.KvCacheC(**base)


def _step(q_tokens=4, cache=None, cfg=None, row_step=FAKE, x=FAKE, ws_bytes=16, mx=None):
    from p2t_hip import _lib
    layers = (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=layers, final_norm_w=FAKE)
    return _lib.call("p2t_llama_decode_step_multi", C.byref(cfg or _cfg()), C.byref(w), None, mx, FAKE, 128, 0, None, C.byref(cache or _cache()), x, FAKE,
                     512, 0, FAKE, ws_bytes, row_step, q_tokens, None)


def test_step_multi_refusals_come_before_any_launch():
    from p2t_hip import _lib
    with pytest.raises(ValueError, match="p2t_llama_decode_step_multi: null row_step"):
        _step(row_step=None)
    for q in (0, -3):
        with pytest.raises(ValueError, match=r"p2t_llama_decode_step_multi: q_tokens -?\d+ outside 1 .. 64"):
            _step(q_tokens=q)
    with pytest.raises(ValueError, match="q_tokens 65 outside 1 .. 64"):
        _step(q_tokens=65)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_multi: null argument"):
        _step(x=None)
    with pytest.raises(_lib.P2TError, match=r"p2t_llama_decode_step_multi failed \(-3\).*3 rows x 22 tokens exceed the 64 rows") as e:
        _step(q_tokens=22)
    assert not isinstance(e.value, ValueError)
    with pytest.raises(_lib.P2TError, match=r"failed \(-3\).*per-row counters serve group == 1 only"):
        _step(cache=_cache(B0=1, group=3))
    with pytest.raises(_lib.P2TError, match=r"failed \(-3\).*at most 16 query heads per kv head \(got 17\)"):
        _step(cfg=_cfg(heads=34, kv_heads=2))
    # 3 rows x 21 tokens = 63 rows are served: every check passes and the call stops at its last one, the workspace's size
    with pytest.raises(ValueError, match="p2t_llama_decode_step_multi: workspace too small"):
        _step(q_tokens=21)
    # ... which is that of B0 * q_tokens rows
    need = _lib.call("p2t_llama_decode_workspace_bytes", C.byref(_cfg()), 12, 128, 64)
    assert need > _lib.call("p2t_llama_decode_workspace_bytes", C.byref(_cfg()), 3, 128, 64)
    with pytest.raises(ValueError, match="workspace too small"):
        _step(q_tokens=4, ws_bytes=need - 1)
    # the per-row door is what it was: the same fake call stops at the same last check
    layers = (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=layers, final_norm_w=FAKE)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_rows: workspace too small"):
        _lib.call("p2t_llama_decode_step_rows", C.byref(_cfg()), C.byref(w), None, None, FAKE, 128, 0, None, C.byref(_cache()), FAKE, FAKE, 512, 0, FAKE, 16,
                  FAKE, None, None)


def _attn(q_tokens=4, nh=4, nkv=2, row_step=FAKE, dtype=1, use_mfma=1, ks=None, vs=None, q=FAKE, Tp=128):
    from p2t_hip import _lib
    return _lib.call("p2t_attention_decode_multi", q, FAKE, FAKE, FAKE, FAKE, FAKE, row_step, 3, nh, nkv, 64, Tp, 64, 0.125, 0, dtype, use_mfma, FAKE, 256,
                     ks, vs, q_tokens, None)


def test_attention_multi_refusals():
    from p2t_hip import _lib
    with pytest.raises(ValueError, match="p2t_attention_decode_multi: null row_step"):
        _attn(row_step=None)
    with pytest.raises(ValueError, match="p2t_attention_decode_multi: q_tokens 0 outside 1 .. 64"):
        _attn(q_tokens=0)
    with pytest.raises(_lib.P2TError, match=r"p2t_attention_decode_multi failed \(-3\).*at most 16 query heads per kv head \(got 17\)"):
        _attn(nh=34)
    with pytest.raises(ValueError, match="go together"):
        _attn(ks=FAKE)
    with pytest.raises(ValueError, match="bad arguments"):
        _attn(q=None)
    with pytest.raises(ValueError, match="capacities"):
        _attn(Tp=100)
    with pytest.raises(_lib.P2TError, match=r"failed \(-3\).*matrix-pipe kernel only"):
        _attn(ks=FAKE, vs=FAKE, use_mfma=0)
    with pytest.raises(ValueError, match="matrix-pipe kernel is bf16 only"):
        _attn(dtype=0, use_mfma=1)


def test_draft_and_verify_refusals():
    from p2t_hip import _lib
    draft = lambda out=FAKE, BB=3, G=64, ld=64, k=3, n=2: _lib.call("p2t_lookup_draft_rows", out, ld, FAKE, FAKE, BB, G, k, n, 0, FAKE, FAKE, None)
    with pytest.raises(ValueError, match="p2t_lookup_draft_rows: null argument"):
        draft(out=None)
    with pytest.raises(ValueError, match="p2t_lookup_draft_rows: bad shape arguments"):
        draft(ld=63)
    for k in (0, 8):
        with pytest.raises(ValueError, match=r"p2t_lookup_draft_rows: num_tokens \d outside 1 .. 7"):
            draft(k=k)
    for n in (0, 5):
        with pytest.raises(ValueError, match=r"p2t_lookup_draft_rows: max_ngram \d outside 1 .. 4"):
            draft(n=n)

    def verify(logits=FAKE, dtype=0, ld=512, V=512, Q=4, n_eos=0, eos=None, choice=FAKE, ld_tok=64):
        return _lib.call("p2t_lookup_verify_rows", logits, dtype, ld, V, 3, Q, FAKE, FAKE, eos, n_eos, 0, FAKE, FAKE, FAKE, ld_tok, FAKE, FAKE, 64, FAKE, choice,
                         None)
    with pytest.raises(ValueError, match="p2t_lookup_verify_rows: null argument"):
        verify(choice=None)
    with pytest.raises(ValueError, match="logits are f32 or bf16"):
        verify(dtype=2)
    for q in (1, 9):
        with pytest.raises(ValueError, match=r"p2t_lookup_verify_rows: q_tokens \d outside 2 .. 8"):
            verify(Q=q)
    for bad in (dict(ld=500), dict(ld_tok=32), dict(n_eos=1)):
        with pytest.raises(ValueError, match="p2t_lookup_verify_rows: bad shape arguments"):
            verify(**bad)
