"""`generate(prompt_kv_dtype="fp8")`: the prompt segment of the KV cache as e4m3 codes with one power-of-two scale per key and kv head
(p2t_kv_quant_store on the prefill's store, p2t_attention_decode_prompt_fp8's kernel in the step), on the generate_tiny.npz models in
bf16.  The reference is the cache-less bf16 oracle whose generated rows see the quantise-dequantised prompt keys and values
(tests/kv8_reference.py patched_oracle): the reference changed with the feature, so the bf16 cache's bounds did not."""
import json
import os

import numpy as np
import pytest
import torch

import kv8_reference as K
from oracle import p2t_oracle as O
from gpu_util import build_model, dev, observe, rel, to_dev, to_np
from helpers import model_weights
from p2t_hip import specs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["d16", "d64", "d128", "qwen3"]


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(HERE, "golden", "generate_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


def _model(g, case, dtype=torch.bfloat16):
    m = g["meta"]["cases"][case]
    model = build_model(specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"]), dtype, m["weight_seed"])
    model.config.placeholder_id = g["meta"]["placeholder_id"]
    model.eval()
    return model


def _inputs(g):
    return dict(inputs=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                protein_attention_mask=to_dev(g["protein_attention_mask"]))


def _decoder_inputs(model, g):
    return model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                 protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)


def _greedy(model, g, n, **kw):
    return model.generate(**_inputs(g), max_new_tokens=n, eos_token_id=None, pad_token_id=g["meta"]["pad_id"], do_sample=False, return_dict_in_generate=True,
                          output_logits=True, **kw)


def _oracle_steps(g, case, model, toks, prec):
    """Per-step logits of the patched cache-less oracle, teacher-forced with `toks`."""
    m = g["meta"]["cases"][case]
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    W = model_weights(esm, llama, ad, m["weight_seed"], lm_head=True)
    emb, mask = _decoder_inputs(model, g)
    mask = to_np(mask)
    with K.patched_oracle((mask != 0).sum(1), llama.num_hidden_layers):
        _, ref = O.generate_greedy(llama, W, to_np(emb), mask, toks.shape[1], (), g["meta"]["pad_id"], prec=prec, forced=toks)
    return ref


@pytest.mark.parametrize("case", CASES)
def test_bf16_steps_vs_patched_bf16_oracle(g, case):
    """6 greedy steps.  The first token's logits are bit-equal to the bf16 cache's (the prefill attends before the store); every step's
    logits against the patched bf16 oracle fed the same tokens, under test_bf16_steps_vs_bf16_oracle_and_own_forward's bound for the
    bf16 cache (4e-2); the replayed graph equals the eager steps bit for bit."""
    model = _model(g, case)
    n = 6
    base = _greedy(model, g, n)
    out = _greedy(model, g, n, prompt_kv_dtype="fp8")
    assert torch.equal(out.logits[0], base.logits[0]) and torch.equal(out.sequences[:, 0], base.sequences[:, 0])
    assert not torch.equal(torch.stack(out.logits[1:], 0), torch.stack(base.logits[1:], 0))            # the switch does something
    eager = _greedy(model, g, n, prompt_kv_dtype="fp8", use_graph=False)
    assert torch.equal(out.sequences, eager.sequences) and torch.equal(torch.stack(out.logits, 0), torch.stack(eager.logits, 0))
    # the same steps from the row-major weights and with the rotation + append as its own launch: the attention is the only thing that changed
    for kw in (dict(stream_copy=False), dict(fuse_rope=False)):
        o2 = _greedy(model, g, n, prompt_kv_dtype="fp8", **kw)
        assert torch.equal(out.sequences, o2.sequences) and torch.equal(torch.stack(out.logits, 0), torch.stack(o2.logits, 0)), kw
    toks, lg = to_np(out.sequences), to_np(torch.stack(out.logits, 0))
    ref = _oracle_steps(g, case, model, toks, O.BF16)
    observe(f"generate[{case}].kv8_bf16_vs_patched_bf16oracle.logits", rel(lg, ref), 4e-2)
    # (step 1 only: from step 2 on the two runs may have chosen different tokens)
    print(f"kv8[{case}]: logits of step 1 vs the bf16 cache's on the same first token, relative: {rel(lg[1], to_np(base.logits[1])):.3e}")


def test_beam_search_graph_equals_eager_and_the_rebuilt_cache_keeps_its_scales(g):
    """3 beams share a prompt's fp8 segment; p2t_beam_select on the device, two steps per replayed graph.  Graph == eager bit for bit,
    the torch bookkeeping (which re-orders through DecodeEngine.reorder and rebuilds the cache struct) finds the same best scores, and
    the struct rebuilt after a segment swap still carries both scale arrays."""
    from p2t_hip import generation
    model = _model(g, "d64")
    m = g["meta"]["cases"]["d64"]
    kw = dict(max_new_tokens=9, eos_token_id=m["eos"], pad_token_id=g["meta"]["pad_id"], do_sample=False, num_beams=3, length_penalty=1.0,
              return_dict_in_generate=True, output_scores=True, prompt_kv_dtype="fp8")
    a = model.generate(**_inputs(g), **kw, beam_select="device")
    b = model.generate(**_inputs(g), **kw, beam_select="device", use_graph=False)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores, b.sequences_scores)
    t = model.generate(**_inputs(g), **kw, beam_select="torch")
    # the two paths rank the same bf16 logits with two f32 log-softmax codes (differences ~1e-6 per step): near-tied beams may swap, the
    # best scores may not move by more than that
    assert t.sequences.shape == a.sequences.shape and np.abs(to_np(a.sequences_scores) - to_np(t.sequences_scores)).max() < 1e-3
    eng = generation.DecodeEngine(model.llama_decoder, 3, 3, 40, 8, prompt_kv_dtype="fp8")
    eng.reorder(torch.tensor([1, 0, 2, 3, 5, 4, 8, 7, 6], device=dev()))
    assert eng.cache.k_prompt_scale == eng.k_prompt_scale.data_ptr() and eng.cache.v_prompt_scale == eng.v_prompt_scale.data_ptr()
    assert eng.cache.k_gen == eng.k_gen.data_ptr()


def test_70_tokens_cross_the_tile_edge_of_the_generated_segment(g):
    """70 new tokens: the bf16 generated segment grows past its first 64-key tile behind the fp8 prompt tiles.  Every step's logits
    against the patched bf16 oracle fed the same tokens, under the bf16 cache's bound."""
    case = "d64"
    model = _model(g, case)
    out = _greedy(model, g, 70, prompt_kv_dtype="fp8", sync_every=32)
    toks, lg = to_np(out.sequences), to_np(torch.stack(out.logits, 0))
    assert toks.shape == (3, 70) and np.isfinite(lg).all()
    ref = _oracle_steps(g, case, model, toks, O.BF16)
    observe(f"generate[{case}].kv8_bf16_70_tokens_vs_patched_bf16oracle.logits", rel(lg, ref), 4e-2)
    observe(f"generate[{case}].kv8_bf16_70_tokens_vs_patched_bf16oracle.logits_last6", rel(lg[64:], ref[64:]), 4e-2)


@pytest.mark.parametrize("mode", ["fp8", "mxfp4"])
def test_fp8_and_mxfp4_weight_models_run_on_the_fp8_prompt_segment(g, mode):
    """Both decode entry points reach the same attention launcher: `set_gemm_dtype("fp8")` / `("mxfp4")` models with the fp8 prompt
    segment; graph == eager and stream copies == row-major weights bit for bit, the first token's logits those of the bf16 cache, and
    (fp8 weights) the step logits against the patched fp8 oracle under that mode's bound for the bf16 cache (1e-1)."""
    case = "d64"
    model = _model(g, case)
    model.set_gemm_dtype(mode)
    n = 6
    base = _greedy(model, g, n)
    out = _greedy(model, g, n, prompt_kv_dtype="fp8")
    eager = _greedy(model, g, n, prompt_kv_dtype="fp8", use_graph=False, stream_copy=False)
    assert torch.equal(out.sequences, eager.sequences) and torch.equal(torch.stack(out.logits, 0), torch.stack(eager.logits, 0))
    assert torch.equal(out.logits[0], base.logits[0])
    lg = to_np(torch.stack(out.logits, 0))
    assert np.isfinite(lg).all() and not np.array_equal(lg[1:], to_np(torch.stack(base.logits, 0))[1:])
    if mode == "fp8":
        toks = to_np(out.sequences)
        ref = _oracle_steps(g, case, model, toks, O.FP8)
        observe(f"generate[{case}].kv8_fp8_vs_patched_fp8oracle.logits", rel(lg, ref), 1e-1)


@pytest.mark.parametrize("case", ["d16", "d128"])
def test_a_nan_poisoned_tail_of_the_prompt_buffers_changes_nothing(g, case):
    """After the prefill, everything behind each row's prompt length in the four prompt buffers becomes e4m3 NaN codes (0x7F) and 0xFF
    scale bytes: two steps give the bits of two steps over the clean buffers."""
    from p2t_hip.generation import DecodeEngine
    model = _model(g, case)
    emb, mask = _decoder_inputs(model, g)
    eos, pad, V = torch.zeros((0,), dtype=torch.int64, device=dev()), g["meta"]["pad_id"], model.llama_decoder.spec.vocab_size
    outs = []
    for poison in (False, True):
        eng = DecodeEngine(model.llama_decoder, emb.shape[0], 1, emb.shape[1], 8, prompt_kv_dtype="fp8")
        assert eng.k_prompt.dtype == torch.uint8 and eng.k_prompt_scale.shape == eng.k_prompt.shape[:-1]
        eng.greedy_select(eng.prefill(*eng.compact(emb, mask)), eos, pad)
        if poison:
            for b, n0 in enumerate(eng.lens.tolist()):
                assert 0 < n0 < eng.Tp
                eng.k_prompt[:, b, :, n0:] = 0x7F; eng.vt_prompt[:, b, :, :, n0:] = 0x7F
                eng.k_prompt_scale[:, b, :, n0:] = 0xFF; eng.v_prompt_scale[:, b, :, n0:] = 0xFF
        for _ in range(2):
            eng.feed(eng.next_tokens)
            eng.decode_step()
            eng.greedy_select(eng.logits, eos, pad)
        outs.append((eng.logits[:, :V].clone(), eng.out_tokens[:, :3].clone()))
    assert torch.isfinite(outs[1][0].float()).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_refusals_and_the_switch_off(g):
    from p2t_hip.generation import DecodeEngine
    f32 = _model(g, "d16", torch.float32)
    with pytest.raises(ValueError, match="bf16"):
        f32.generate(**_inputs(g), max_new_tokens=2, prompt_kv_dtype="fp8")
    model = _model(g, "d16")
    with pytest.raises(ValueError, match="prompt_kv_dtype"):
        model.generate(**_inputs(g), max_new_tokens=2, prompt_kv_dtype="fp4")
    eng = DecodeEngine(model.llama_decoder, 3, 1, 40, 8)                              # prompt_kv_dtype=None: today's cache, no scale tensors
    assert eng.k_prompt_scale is None and eng.v_prompt_scale is None and eng.k_prompt.dtype == torch.bfloat16
    assert eng.cache.k_prompt_scale is None and eng.cache.v_prompt_scale is None
    on = DecodeEngine(model.llama_decoder, 3, 1, 40, 8, prompt_kv_dtype="fp8")
    assert on.k_prompt.numel() == eng.k_prompt.numel() and on.k_prompt.element_size() == 1          # half the bytes, plus one byte per key
    assert on.k_prompt_scale.shape == (on.spec.num_hidden_layers, 3, on.spec.num_key_value_heads, on.Tp)
