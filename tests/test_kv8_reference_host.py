"""CPU: tests/kv8_reference.py, the numpy reference of the fp8 prompt segment of the KV cache, pinned on torch.float8_e4m3fn and on
itself: codes and scales of the per-key quantiser, its idempotence, the all-zero key, both sides of the scale rule's 0.75-mantissa
threshold, the patched oracle as a no-op under the identity, and -- on record, not asserted -- how far the prompt quantisation alone
moves the step logits of the fp32 oracle on the generate_tiny.npz models."""
import json
import os

import numpy as np
import pytest
import torch

import kv8_reference as K
from helpers import model_weights
from oracle import p2t_oracle as O
from p2t_hip import specs, synth

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def _keys(seed, shape, spread=3.0):
    rs = np.random.RandomState(seed)
    x = rs.randn(*shape) * np.exp(rs.randn(*shape[:-1], 1) * spread)
    return synth.bf16_round(x.astype(F32))


def test_codes_equal_torch_float8_of_x_over_scale():
    x = _keys(0, (7, 3, 50, 48))
    codes, E, deq = K.quant_keys(x)
    assert codes.dtype == np.uint8 and E.dtype == np.uint8 and codes.shape == x.shape and E.shape == x.shape[:-1]
    s = np.ldexp(F32(1.0), E.astype(np.int32) - 127)[..., None]
    want = torch.from_numpy((x / s).astype(F32)).to(torch.float8_e4m3fn)
    assert np.array_equal(codes, want.view(torch.uint8).numpy())
    assert np.array_equal(deq, want.float().numpy() * s)
    assert np.array_equal(K.dequant(codes, E), deq)
    # the scale is the smallest power of two that keeps the key inside e4m3: amax / 2^e <= 448 < amax / 2^(e - 1)
    amax = np.abs(x).max(-1)
    assert (amax / s[..., 0] <= 448).all() and (amax / s[..., 0] * 2 > 448).all()
    # the byte table against torch, all 256 codes
    allb = np.arange(256, dtype=np.uint8)
    tv = torch.from_numpy(allb).view(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(np.nan_to_num(K.e4m3_values(allb), nan=7e7), np.nan_to_num(tv, nan=7e7))
    fin = np.isfinite(tv)
    assert np.array_equal(K.e4m3_bytes(tv[fin]) & 0x7F, allb[fin] & 0x7F) and np.isnan(tv[0x7F]) and np.isnan(tv[0xFF])


def test_requantising_dequantised_keys_returns_them_bit_for_bit():
    x = _keys(1, (4, 2, 33, 64))
    codes, E, deq = K.quant_keys(x)
    assert np.array_equal(deq, synth.bf16_round(deq))                     # e4m3 times a power of two is a bf16 value
    # the VALUES come back; the pair (scale, codes) may not: a maximum that rounded down onto 1.75 2^a (225 -> 224) now fits the scale below
    codes2, E2, deq2 = K.quant_keys(deq)
    assert np.array_equal(deq2, deq) and np.array_equal(K.dequant(codes2, E2), deq)
    assert (E2 <= E).all() and (E2 >= E - 1).all() and (E2 == E).mean() > 0.5


def test_all_zero_keys_and_the_mantissa_threshold_of_the_scale_rule():
    x = _keys(2, (5, 32), spread=0.5)
    x[1] = 0.0
    x[3, 5:] = 0.0                                                        # a key with a few elements only
    codes, E, deq = K.quant_keys(x)
    assert E[1] == 127 and not codes[1].any() and not deq[1].any()
    # amax = (1 + f) 2^a: f <= 0.75 -> 448 2^(a - 8) holds it (e = a - 8); above -> e = a - 7.  1.75 2^a sits ON the threshold: code 448.
    for a in (-20, -3, 0, 9, 20):
        for f, de, top in ((0.75, 0, 448.0), (0.7578125, 1, 224.0), (0.0, 0, 256.0), (0.9921875, 1, 256.0)):     # (225 -> 224, 255 -> 256)
            row = np.zeros((1, 32), dtype=F32)
            row[0, 7] = -(1 + f) * 2.0 ** a
            row[0, 9] = 2.0 ** (a - 3)
            c, e, dq = K.quant_keys(row)
            assert int(e[0]) == 127 + a - 8 + de, (a, f)
            assert K.e4m3_values(c)[0, 7] == -top and dq[0, 9] == row[0, 9], (a, f)
            assert np.array_equal(dq, row) == (f in (0.75, 0.0)), (a, f)                 # a value with <= 4 significant bits survives
    # ties of the e4m3 grid go to the even code: with amax 448 (scale 1) 17 and 19 sit between 16, 18, 20 -> 16 and 20; 0.5 / 512 -> 0
    row = np.array([[448.0, 17.0, 19.0, -17.0, 2.0 ** -10, 3 * 2.0 ** -10] + [0.0] * 26], dtype=F32)
    c, e, dq = K.quant_keys(row)
    assert e[0] == 127 and dq[0, :6].tolist() == [448.0, 16.0, 20.0, -16.0, 0.0, 2 * 2.0 ** -9]


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(HERE, "golden", "generate_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


def _decoder_case(g, case, n_prompt=(9, 5), seed=11):
    """The case's decoder on synthetic prompt embeddings (the oracle's decoder functions take embeddings; no encoder needed)."""
    m = g["meta"]["cases"][case]
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    W = model_weights(esm, llama, ad, m["weight_seed"], lm_head=True)
    rs = np.random.RandomState(seed)
    T = max(n_prompt)
    emb = (rs.randn(len(n_prompt), T, llama.hidden_size) * 0.5).astype(F32)
    mask = np.array([[0] * (T - n) + [1] * n for n in n_prompt], dtype=np.int64)      # left padded
    return llama, W, emb, mask


@pytest.mark.parametrize("case", ["d16", "d64", "d128", "qwen3"])
def test_patched_oracle_identity_is_a_no_op_and_the_effect_is_on_record(g, case):
    llama, W, emb, mask = _decoder_case(g, case)
    lens, L, n = mask.sum(1), llama.num_hidden_layers, 4
    toks, ref = O.generate_greedy(llama, W, emb, mask, n, (), 0)
    for prec in (O.FP32, O.BF16):
        _, plain = O.generate_greedy(llama, W, emb, mask, n, (), 0, prec=prec, forced=toks)
        with K.patched_oracle(lens, L, quantiser=lambda x: x):
            _, same = O.generate_greedy(llama, W, emb, mask, n, (), 0, prec=prec, forced=toks)
        assert np.array_equal(plain, same)
    assert O.attention_heads.__name__ == "attention_heads"                # the patch is gone
    with K.patched_oracle(lens, L):
        _, q8 = O.generate_greedy(llama, W, emb, mask, n, (), 0, forced=toks)
    assert np.array_equal(q8[0], ref[0])                                  # the first token comes from the prefill: plain keys and values
    change = [float(np.linalg.norm(q8[s] - ref[s]) / np.linalg.norm(ref[s])) for s in range(1, n)]
    print(f"kv8 effect[{case}]: relative change of the fp32 step logits from the prompt quantisation alone, steps 1..{n - 1}: "
          + " ".join(f"{c:.3e}" for c in change))
    assert all(np.isfinite(change)) and max(change) > 0.0                 # on record, not held to a number
