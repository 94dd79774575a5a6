"""CPU: the quantised LM head's ABI (include/p2t_hip.h: p2t_lm_head_q, p2t_lm_head_logits_q, p2t_lm_head_q_workspace_bytes,
p2t_llama_decode_step_q) is declared, exported and bound, the descriptor has the size of its mirror, and calls outside the contract are
refused by name before any GPU call -- P2T_ERR_ARG as ValueError, the unsupported combinations as P2T_ERR_UNSUPPORTED (-3)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = {"p2t_lm_head_logits_q": 16, "p2t_lm_head_q_workspace_bytes": 2, "p2t_llama_decode_step_q": 16}
FAKE = 4096          # a non-null, 16-byte aligned "pointer": never dereferenced, the checks come first
FIELDS = ("format", "stream_order", "codes", "scales", "ld", "codes_e4m3", "scales_e4m3")


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert re.search(r"\}\s*p2t_lm_head_q\s*;", src)
    assert tuple(n for n, _ in _lib.LmHeadQC._fields_) == FIELDS
    assert _lib.lib.p2t_struct_size(16) == ctypes.sizeof(_lib.LmHeadQC) == 2 * 4 + 5 * 8
    assert (_lib.LM_HEAD_E4M3, _lib.LM_HEAD_MXFP4) == (1, 2) and re.search(r"P2T_LM_HEAD_E4M3\s*=\s*1\s*,\s*P2T_LM_HEAD_MXFP4\s*=\s*2", src)
    # the step's new door takes what the two existing ones take between them, plus the descriptor
    old, mx, new = (_lib.SIGNATURES[n][1] for n in ("p2t_llama_decode_step", "p2t_llama_decode_step_mxfp4", "p2t_llama_decode_step_q"))
    assert new[:3] == old[:3] and new[3] == mx[2] and new[4:7] == old[3:6] and new[8:] == old[6:]
    assert _lib.call("p2t_lm_head_q_workspace_bytes", 8, 4096) >= 8 * 4096 + 8 and _lib.call("p2t_lm_head_q_workspace_bytes", 0, 64) == 0


def _head(fmt=1, so=0, codes=FAKE, scales=FAKE, ld=256, c8=None, s8=None):
    from p2t_hip import _lib
    return _lib.LmHeadQC(format=fmt, stream_order=so, codes=codes, scales=scales, ld=ld, codes_e4m3=c8, scales_e4m3=s8)


def _logits(x=FAKE, ld_x=192, nw=FAKE, head="default", M=8, H=192, V=300, out=FAKE, ld=320, odt=1, aq=None, asc=None, ws=FAKE, ws_bytes=1 << 20):
    from p2t_hip import _lib
    head = _head() if head == "default" else head
    return _lib.call("p2t_lm_head_logits_q", x, ld_x, nw, 1e-5, ctypes.byref(head) if head is not None else None, M, H, V, out, ld, odt, aq, asc, ws,
                     ws_bytes, None)


_ids = lambda b: ",".join(f"{k}={v if not hasattr(v, '_fields_') else 'head'}" for k, v in b.items())


@pytest.mark.parametrize("bad", [
    dict(x=None), dict(out=None), dict(head=None), dict(M=0), dict(H=0), dict(H=188, ld_x=188), dict(V=0), dict(ld=296), dict(ld=322), dict(ld_x=128),
    dict(ld_x=196), dict(x=FAKE + 4), dict(aq=FAKE), dict(asc=FAKE), dict(aq=FAKE + 8, asc=FAKE), dict(ws=None), dict(ws_bytes=64),
], ids=_ids)
def test_logits_argument_errors(bad):
    with pytest.raises(ValueError, match="p2t_lm_head_logits_q"):
        _logits(**bad)


@pytest.mark.parametrize("kw", [
    dict(fmt=0), dict(fmt=3), dict(codes=None), dict(codes=FAKE + 8), dict(scales=None), dict(fmt=1, so=1, scales=None), dict(fmt=2, scales=None),
    dict(ld=248), dict(ld=128), dict(fmt=2, ld=120), dict(fmt=2, ld=64), dict(fmt=2, ld=128, c8=FAKE), dict(fmt=2, ld=128, s8=FAKE),
    dict(fmt=1, c8=FAKE, s8=FAKE),
], ids=_ids)
def test_descriptor_errors(kw):
    with pytest.raises(ValueError, match="p2t_lm_head_logits_q"):
        _logits(head=_head(**kw))


@pytest.mark.parametrize("kw", [
    dict(odt=0),                                                    # an f32 model
    dict(M=65, head=_head(so=1)), dict(M=65, head=_head(fmt=2, so=1, scales=None)),       # a stream copy beyond 64 rows
    dict(M=65, head=_head(fmt=2, ld=128)),                          # MXFP4 beyond 64 rows without its e4m3 copy
    dict(M=65, head=_head(ld=272), V=304),                          # the general GEMM reads the e4m3 head at ld = Kq
    dict(M=65),                                                     # ... and takes a vocabulary that is a multiple of 16 (V = 300)
], ids=["f32", "stream_e4m3", "stream_mxfp4", "mxfp4_no_copy", "ld", "vocab"])
def test_unsupported_combinations(kw):
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_lm_head_logits_q failed \(-3\)") as e:
        _logits(**kw)
    assert not isinstance(e.value, ValueError) and "p2t_lm_head_logits_q" in str(e.value).split("(-3)")[1]


def test_decode_step_q_refuses_what_it_cannot_run():
    from p2t_hip import _lib
    C = ctypes
    mk = lambda **kw: _lib.LlamaConfigC(**{**dict(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=1, gemm_fp8=0), **kw})
    layers = (_lib.LlamaLayerC * 2)()
    w = _lib.LlamaWeightsC(embed=FAKE, layers=C.cast(layers, C.POINTER(_lib.LlamaLayerC)), final_norm_w=FAKE)
    mxl, stl = (_lib.LlamaLayerMxfp4C * 2)(), (_lib.LlamaLayerStreamC * 2)()
    cache = lambda B0=4, group=2: _lib.KvCacheC(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=FAKE, B0=B0, group=group, Tp=64,
                                                G=64)

    def step(cfg=None, st=None, mx=None, lm=None, head=None, kc=None, ld_logits=512, ws_bytes=1 << 30):
        cfg, kc = cfg or mk(), kc or cache()
        return _lib.call("p2t_llama_decode_step_q", C.byref(cfg), C.byref(w), C.cast(st, C.POINTER(_lib.LlamaLayerStreamC)) if st is not None else None,
                         C.cast(mx, C.POINTER(_lib.LlamaLayerMxfp4C)) if mx is not None else None, lm, 128, 0, C.byref(head) if head is not None else None,
                         C.byref(kc), FAKE, FAKE, ld_logits, 0, FAKE, ws_bytes, None)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: w_stream and mx_layers"):
        step(st=stl, mx=mxl, head=_head())
    with pytest.raises(ValueError, match="gemm_fp8"):
        step(mx=mxl, head=_head())                                   # mx_layers on a configuration that is not gemm_fp8
    with pytest.raises(ValueError, match="at most 64 rows"):
        step(cfg=mk(gemm_fp8=1), mx=mxl, head=_head(), kc=cache(13, 5))
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: null argument"):
        step()                                                       # neither a bf16 head nor a descriptor
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: head format"):
        step(head=_head(fmt=7))
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: null head scales"):
        step(head=_head(scales=None))
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: workspace too small"):
        step(head=_head(ld=128), ws_bytes=_lib.call("p2t_llama_decode_workspace_bytes", C.byref(mk()), 8, 64, 64))
    with pytest.raises(_lib.P2TError, match=r"\(-3\).*bf16 models only"):
        step(cfg=mk(dtype=0), head=_head(ld=128))
    with pytest.raises(_lib.P2TError, match=r"\(-3\).*at most 64 rows"):
        step(head=_head(so=1), kc=cache(13, 5))


def test_decode_step_q_refuses_before_its_first_enqueue():
    """The refusals that used to sit behind launches -- the pre-shuffled head beyond 64 rows (after all layers), a layer's row scales, its
    q_norm / k_norm pairing and its MXFP4 codes (inside the layer loop, after the layers before it) -- come from the checking pass in front
    of the first copy: fake pointers, no device, a ValueError by name."""
    from p2t_hip import _lib
    C = ctypes
    mk = lambda **kw: _lib.LlamaConfigC(**{**dict(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=1, gemm_fp8=0), **kw})
    scales = dict(qkv_ws=FAKE, o_ws=FAKE, gu_ws=FAKE, down_ws=FAKE)
    mxw = dict(qkv_w=FAKE, o_w=FAKE, gu_w=FAKE, down_w=FAKE, qkv_bs=FAKE, o_bs=FAKE, gu_bs=FAKE, down_bs=FAKE)

    def step(cfg, layers, mx=None, pre=0, B0=4):
        arr = (_lib.LlamaLayerC * 2)(*[_lib.LlamaLayerC(**kw) for kw in layers])
        w = _lib.LlamaWeightsC(embed=FAKE, layers=C.cast(arr, C.POINTER(_lib.LlamaLayerC)), final_norm_w=FAKE)
        mxa = (_lib.LlamaLayerMxfp4C * 2)(*[_lib.LlamaLayerMxfp4C(**kw) for kw in mx]) if mx is not None else None
        kc = _lib.KvCacheC(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=FAKE, B0=B0, group=1, Tp=64, G=64)
        return _lib.call("p2t_llama_decode_step_q", C.byref(cfg), C.byref(w), None, C.cast(mxa, C.POINTER(_lib.LlamaLayerMxfp4C)) if mx is not None else None,
                         FAKE, 128, pre, None, C.byref(kc), FAKE, FAKE, 512, 0, FAKE, 1 << 30, None)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: .*at most 64 rows"):
        step(mk(), [{}, {}], pre=1, B0=65)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: .*row scales of layer 1"):
        step(mk(gemm_fp8=1), [scales, {**scales, "down_ws": None}])
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: .*go together"):
        step(mk(), [{}, dict(q_norm_w=FAKE)])
    with pytest.raises(ValueError, match="p2t_llama_decode_step_q: .*null codes"):
        step(mk(gemm_fp8=1), [scales, scales], mx=[mxw, {**mxw, "o_w": None}])


def test_generate_refuses_an_unknown_dtype_and_an_fp32_model():
    import torch
    from p2t_hip import generation
    from types import SimpleNamespace
    dec = SimpleNamespace(model=SimpleNamespace(dtype=torch.float32), spec=None)
    with pytest.raises(ValueError, match="lm_head_dtype must be None, 'fp8' or 'mxfp4'"):
        generation.DecodeEngine(dec, 1, 1, 4, 4, lm_head_dtype="int4")
    for fmt in ("fp8", "mxfp4"):
        with pytest.raises(ValueError, match="serves bf16 models only"):
            generation.DecodeEngine(dec, 1, 1, 4, 4, lm_head_dtype=fmt)
