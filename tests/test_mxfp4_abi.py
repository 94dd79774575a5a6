"""CPU: the MXFP4 entry points (include/p2t_hip.h "MXFP4 decoder weights": quantiser, de-quantiser, stream copy, the decode GEMM and the
decode step that streams them) are declared, exported and bound, p2t_llama_layer_mxfp4 has the size of its mirror, and calls outside
the contract are refused before any GPU call -- P2T_ERR_ARG as ValueError, an unsupported shape as P2T_ERR_UNSUPPORTED (-3)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = {"p2t_quant_rows_mxfp4": 9, "p2t_dequant_rows_mxfp4": 8, "p2t_preshuffle_w_mxfp4": 7, "p2t_gemm_nt_skinny_mxfp4": 15,
         "p2t_llama_decode_step_mxfp4": 14}
FAKE = 4096          # a non-null "pointer": never dereferenced, the checks come first
FIELDS = ("qkv_w", "o_w", "gu_w", "down_w", "qkv_bs", "o_bs", "gu_bs", "down_bs", "stream_order", "reserved")


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert re.search(r"\}\s*p2t_llama_layer_mxfp4\s*;", src)
    assert tuple(n for n, _ in _lib.LlamaLayerMxfp4C._fields_) == FIELDS
    assert _lib.lib.p2t_struct_size(15) == ctypes.sizeof(_lib.LlamaLayerMxfp4C) == 8 * 8 + 2 * 4
    assert _lib.SIGNATURES["p2t_gemm_nt_skinny_mxfp4"][1] == _lib.SIGNATURES["p2t_gemm_nt_skinny_fp8"][1]     # the fp8 entry point's argument shape
    assert _lib.version() == 103


def _gemm(A=FAKE, lda=256, a_scale=FAKE, W=FAKE, ldw=128, bs=FAKE, pre=0, out=FAKE, ldc=64, M=8, N=64, K=256, out_dtype=0, epi=0):
    from p2t_hip import _lib
    return _lib.call("p2t_gemm_nt_skinny_mxfp4", A, lda, a_scale, W, ldw, bs, pre, out, ldc, M, N, K, out_dtype, epi, None)


_ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(A=None), dict(a_scale=None), dict(W=None), dict(bs=None), dict(out=None)], ids=_ids)
def test_gemm_null_arguments(bad):
    with pytest.raises(ValueError, match="p2t_gemm_nt_skinny_mxfp4"):
        _gemm(**bad)


@pytest.mark.parametrize("bad", [dict(K=64, lda=64, ldw=32), dict(K=0), dict(K=192), dict(M=65), dict(M=0), dict(N=0), dict(lda=264), dict(lda=128),
                                 dict(ldw=136), dict(ldw=112), dict(ldc=66), dict(epi=1), dict(epi=3, N=96, out_dtype=1), dict(epi=3, out_dtype=0)], ids=_ids)
def test_gemm_outside_the_supported_range_is_unsupported(bad):
    """K < 128 or no multiple of 128, more than 64 rows, leading dimensions that are misaligned or too short, an epilogue the stream
    kernel does not have (GELU), SwiGLU over a row count that is no multiple of 64 or into an f32 output."""
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_gemm_nt_skinny_mxfp4 failed \(-3\)") as e:
        _gemm(**bad)
    assert not isinstance(e.value, ValueError)


def test_quantiser_dequantiser_and_stream_copy_argument_errors():
    from p2t_hip import _lib
    q = lambda x=FAKE, dt=1, ld_x=256, rows=4, cols=200, codes=FAKE, ld_codes=128, sc=FAKE: _lib.call("p2t_quant_rows_mxfp4", x, dt, ld_x, rows, cols, codes,
                                                                                                  ld_codes, sc, None)
    for bad in (dict(x=None), dict(codes=None), dict(sc=None), dict(dt=2), dict(cols=0), dict(rows=-1), dict(ld_x=100), dict(ld_x=252), dict(ld_codes=120),
                dict(ld_codes=64), dict(ld_codes=100)):
        with pytest.raises(ValueError, match="p2t_quant_rows_mxfp4"):
            q(**bad)
    assert q(rows=0) == 0
    d = lambda codes=FAKE, ld_codes=128, sc=FAKE, rows=4, cols=200, out=FAKE, ld_out=200: _lib.call("p2t_dequant_rows_mxfp4", codes, ld_codes, sc, rows, cols, out,
                                                                                                ld_out, None)
    for bad in (dict(codes=None), dict(sc=None), dict(out=None), dict(cols=0), dict(ld_codes=64), dict(ld_codes=120), dict(ld_out=199)):
        with pytest.raises(ValueError, match="p2t_dequant_rows_mxfp4"):
            d(**bad)
    p = lambda codes=FAKE, ld=128, sc=FAKE, N=48, K=256, out=FAKE: _lib.call("p2t_preshuffle_w_mxfp4", codes, ld, sc, N, K, out, None)
    for bad in (dict(codes=None), dict(sc=None), dict(out=None), dict(N=0), dict(K=64), dict(K=192), dict(ld=120), dict(ld=64)):
        with pytest.raises(ValueError, match="p2t_preshuffle_w_mxfp4"):
            p(**bad)


def test_decode_step_refuses_what_it_cannot_run():
    from p2t_hip import _lib
    C = ctypes
    cfg = _lib.LlamaConfigC(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=1, gemm_fp8=1)
    w = _lib.LlamaWeightsC()
    layers = (_lib.LlamaLayerMxfp4C * 2)()
    cache = _lib.KvCacheC(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=FAKE, B0=4, group=2, Tp=64, G=64)

    def step(cfg=cfg, layers=layers, cache=cache):
        lp = C.cast(layers, C.POINTER(_lib.LlamaLayerMxfp4C)) if layers is not None else None
        return _lib.call("p2t_llama_decode_step_mxfp4", C.byref(cfg), C.byref(w), lp, FAKE, 128, 0, C.byref(cache) if cache is not None else None, FAKE, FAKE, 512,
                         0, FAKE, 1 << 30, None)
    with pytest.raises(ValueError, match="p2t_llama_decode_step_mxfp4: null"):
        step(layers=None)
    with pytest.raises(ValueError, match="gemm_fp8"):
        step(cfg=_lib.LlamaConfigC(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=1, gemm_fp8=0))
    with pytest.raises(ValueError, match="gemm_fp8"):
        step(cfg=_lib.LlamaConfigC(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=0, gemm_fp8=1))
    with pytest.raises(ValueError, match="at most 64 rows"):
        step(cache=_lib.KvCacheC(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=FAKE, B0=13, group=5, Tp=64, G=64))
    layers[1].stream_order = 1
    with pytest.raises(ValueError, match="stream_order"):
        step()
    layers[1].stream_order = 0
    with pytest.raises(ValueError, match="null argument"):              # the weight set is empty: refused by the shared step before any launch
        step()


def test_the_model_switch_knows_the_third_value():
    import torch
    import p2t_hip as P
    from p2t_hip import specs
    esm = specs.EsmSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2)
    llama = specs.LlamaSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=2, vocab_size=64)
    model = P.Esm2LlamaInstructForCausalLM.from_specs(esm, llama, specs.AdapterSpec(64, 64, 64, 0.0), dtype=torch.bfloat16, device="cpu", seed=None)
    dec = model.llama_decoder.model
    model.set_gemm_dtype("mxfp4")
    assert model.esm_encoder.gemm_fp8 and dec.gemm_fp8 and dec.gemm_mxfp4 and not getattr(model.esm_encoder, "gemm_mxfp4", False)
    model.set_gemm_dtype("fp8")
    assert model.esm_encoder.gemm_fp8 and dec.gemm_fp8 and not dec.gemm_mxfp4
    model.set_gemm_dtype("model")
    assert not model.esm_encoder.gemm_fp8 and not dec.gemm_fp8 and not dec.gemm_mxfp4
    with pytest.raises(ValueError, match="mxfp4"):
        model.set_gemm_dtype("int4")
    f32 = P.Esm2LlamaInstructForCausalLM.from_specs(esm, llama, specs.AdapterSpec(64, 64, 64, 0.0), dtype=torch.float32, device="cpu", seed=None)
    with pytest.raises(ValueError):
        f32.set_gemm_dtype("mxfp4")
