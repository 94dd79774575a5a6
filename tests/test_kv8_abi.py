"""CPU: the fp8 prompt segment's entry points (include/p2t_hip.h: p2t_kv_cache's scale arrays, p2t_kv_quant_store,
p2t_attention_decode_prompt_fp8) are declared, exported and bound, p2t_kv_cache has the size of its mirror, and calls outside the
contract are refused before any GPU call -- P2T_ERR_ARG as ValueError, what the kernels do not serve as P2T_ERR_UNSUPPORTED (-3)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p2t_hip.h")
NAMES = {"p2t_kv_quant_store": 12, "p2t_attention_decode_prompt_fp8": 23}
FAKE = 4096          # a non-null, 16-byte aligned "pointer": never dereferenced, the checks come first
FIELDS = ("k_prompt", "vt_prompt", "k_gen", "vt_gen", "prompt_len", "step", "B0", "group", "Tp", "G", "k_prompt_scale", "v_prompt_scale")


def test_header_declares_and_library_exports():
    from p2t_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/p2t_hip.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert re.search(r"uint8_t\s*\*\s*k_prompt_scale\s*;\s*uint8_t\s*\*\s*v_prompt_scale\s*;\s*\}\s*p2t_kv_cache\s*;", src)      # appended at the end
    assert tuple(n for n, _ in _lib.KvCacheC._fields_) == FIELDS
    assert _lib.lib.p2t_struct_size(10) == ctypes.sizeof(_lib.KvCacheC) == 6 * 8 + 4 * 4 + 2 * 8
    # the bf16 entry point's arguments, the two scale arrays in front of the stream
    assert _lib.SIGNATURES["p2t_attention_decode_prompt_fp8"][1][:20] == _lib.SIGNATURES["p2t_attention_decode"][1][:20]
    c = _lib.KvCacheC(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=FAKE, B0=1, group=1, Tp=64, G=64)
    assert c.k_prompt_scale is None and c.v_prompt_scale is None          # callers that build the struct by keyword get today's cache


def _attn(q=FAKE, kp=FAKE, vtp=FAKE, kg=FAKE, vtg=FAKE, lens=FAKE, step=FAKE, B0=2, group=1, nh=4, nkv=2, d=64, Tp=128, G=64, dtype=1, use_mfma=1, out=FAKE,
          ld_out=256, ks=FAKE, vs=FAKE):
    from p2t_hip import _lib
    return _lib.call("p2t_attention_decode_prompt_fp8", q, kp, vtp, kg, vtg, lens, step, B0, group, nh, nkv, d, Tp, G, 0.125, 1, dtype, use_mfma, out, ld_out,
                     ks, vs, None)


_ids = lambda b: ",".join(f"{k}={v}" for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(ks=None), dict(vs=None), dict(ks=None, vs=None), dict(q=None), dict(out=None), dict(kp=None), dict(vtg=None),
                                 dict(lens=None), dict(Tp=100), dict(G=32), dict(Tp=0), dict(nh=5), dict(d=130), dict(ld_out=255), dict(ks=FAKE + 8),
                                 dict(kp=FAKE + 4)], ids=_ids)
def test_attention_argument_errors(bad):
    """One scale array without the other (or none: that is p2t_attention_decode's cache), null buffers, capacities that are no multiples
    of 64, head shapes the cache does not have, buffers the 16-byte loads cannot read: P2T_ERR_ARG."""
    with pytest.raises(ValueError, match="p2t_attention_decode"):
        _attn(**bad)


@pytest.mark.parametrize("bad", [dict(dtype=0), dict(use_mfma=0), dict(dtype=0, use_mfma=0)], ids=_ids)
def test_attention_outside_the_supported_range_is_unsupported(bad):
    """An f32 cache with scales, and the lane-per-key kernel (use_mfma = 0), which reads no fp8 segment."""
    from p2t_hip import _lib
    with pytest.raises(_lib.P2TError, match=r"p2t_attention_decode_prompt_fp8 failed \(-3\)") as e:
        _attn(**bad)
    assert not isinstance(e.value, ValueError)


def test_quant_store_argument_errors():
    from p2t_hip import _lib
    st = lambda k=FAKE, v=FAKE, B=2, nkv=2, T=70, d=64, Tp=128, kq=FAKE, vq=FAKE, ks=FAKE, vs=FAKE: _lib.call("p2t_kv_quant_store", k, v, B, nkv, T, d, Tp, kq,
                                                                                                          vq, ks, vs, None)
    for bad in (dict(k=None), dict(v=None), dict(kq=None), dict(vq=None), dict(ks=None), dict(vs=None), dict(B=0), dict(nkv=0), dict(T=0), dict(d=0),
                dict(d=63), dict(d=130), dict(Tp=100), dict(T=129), dict(k=FAKE + 2), dict(vq=FAKE + 8)):
        with pytest.raises(ValueError, match="p2t_kv_quant_store"):
            st(**bad)


def test_the_cache_checks_reach_the_prefill_the_step_and_the_reorder():
    """check_cache serves every entry point that takes a p2t_kv_cache: one scale array alone is an argument error, scales on an f32
    model are unsupported -- in front of everything else the calls check."""
    from p2t_hip import _lib
    C = ctypes
    base = dict(k_prompt=FAKE, vt_prompt=FAKE, k_gen=FAKE, vt_gen=FAKE, prompt_len=FAKE, step=FAKE, B0=2, group=1, Tp=64, G=64)
    w = _lib.LlamaWeightsC()

    def calls(cfg, cache):
        yield "p2t_llama_prefill", lambda: _lib.call("p2t_llama_prefill", C.byref(cfg), C.byref(w), FAKE, FAKE, 2, 8, C.byref(cache), FAKE, FAKE, 1 << 30, None)
        yield "p2t_kv_reorder", lambda: _lib.call("p2t_kv_reorder", C.byref(cfg), C.byref(cache), FAKE, FAKE, FAKE, None)

    bf = _lib.LlamaConfigC(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=1)
    f32 = _lib.LlamaConfigC(n_layers=2, hidden=128, ffn=256, heads=2, kv_heads=2, head_dim=64, vocab=512, dtype=0)
    for name, f in calls(bf, _lib.KvCacheC(**base, k_prompt_scale=FAKE)):
        with pytest.raises(ValueError, match="go together"):
            f()
    for name, f in calls(bf, _lib.KvCacheC(**base, v_prompt_scale=FAKE)):
        with pytest.raises(ValueError, match="go together"):
            f()
    for name, f in calls(f32, _lib.KvCacheC(**base, k_prompt_scale=FAKE, v_prompt_scale=FAKE)):
        with pytest.raises(_lib.P2TError, match=r"%s failed \(-3\)" % name) as e:
            f()
        assert not isinstance(e.value, ValueError)


def test_the_engine_refuses_without_a_gpu():
    """generate(prompt_kv_dtype=): a float32 model and an unknown value raise ValueError before anything is allocated."""
    import torch
    import p2t_hip as P
    from p2t_hip import generation, specs
    esm = specs.EsmSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2)
    llama = specs.LlamaSpec(num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=2, num_key_value_heads=2, vocab_size=64)
    for dt, value in ((torch.float32, "fp8"), (torch.bfloat16, "int8")):
        model = P.Esm2LlamaInstructForCausalLM.from_specs(esm, llama, specs.AdapterSpec(64, 64, 64, 0.0), dtype=dt, device="cpu", seed=None)
        with pytest.raises(ValueError, match="prompt_kv_dtype"):
            generation.DecodeEngine(model.llama_decoder, 2, 1, 8, 8, prompt_kv_dtype=value)
