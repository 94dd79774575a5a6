"""numpy reference of the fp8 prompt segment of the KV cache (include/p2t_hip.h, p2t_kv_cache with the scale arrays set):

* `quant_keys`: one power-of-two scale per key over its dp features (oracle.e8m0_of_amax) and e4m3 codes of x / 2^e
  (oracle.e4m3_round) -> code bytes, scale bytes, dequantised values;
* `decode_attention`: the decode step's attention of one query token per row over the two cache segments, in the operands' precision
  (fp64 operands: the fp64 reference; test_gpu_generate._attn_ref's formula);
* `patched_oracle`: oracle.attention_heads replaced so that query rows at GENERATED positions see the quantise-dequantised keys and
  values of the PROMPT positions, and prompt rows the plain ones (the prefill attends before its store): under it
  oracle.llama_next_token_logits / generate_greedy are the cache-less reference of generate(prompt_kv_dtype="fp8")."""
import contextlib

import numpy as np

from oracle import p2t_oracle as O

F32 = np.float32
_E4M3_VALUES = None


def e4m3_bytes(q: np.ndarray) -> np.ndarray:
    """e4m3fn byte of every value of q (already on the e4m3 grid, |q| <= 448): sign, 4 exponent bits (bias 7), 3 mantissa bits."""
    q = np.ascontiguousarray(q, dtype=F32)
    a = np.abs(q)
    m, e = np.frexp(a)                                           # a = m 2^e, m in [0.5, 1)
    normal = a >= F32(2.0 ** -6)
    exp = np.where(normal, e - 1 + 7, 0).astype(np.int32)
    man = np.where(normal, np.rint((m * 2 - 1) * 8), np.rint(a * 512)).astype(np.int32)
    code = (exp << 3) | man
    assert ((man >= 0) & (man <= 7) & (exp >= 0) & (code <= 0x7E)).all(), "value off the e4m3 grid"
    return (code | np.where(np.signbit(q), 0x80, 0)).astype(np.uint8)


def e4m3_values(codes: np.ndarray) -> np.ndarray:
    """The f32 value of every e4m3fn byte (0x7F / 0xFF: NaN)."""
    global _E4M3_VALUES
    if _E4M3_VALUES is None:
        b = np.arange(256)
        e, m = (b >> 3) & 15, b & 7
        v = np.where(e == 0, m / 512.0, (1 + m / 8.0) * np.exp2(e - 7.0))
        v = np.where((b & 0x7F) == 0x7F, np.nan, v)
        _E4M3_VALUES = np.where(b & 0x80, -v, v).astype(F32)
    return _E4M3_VALUES[np.asarray(codes, dtype=np.uint8)]


def scale_values(E: np.ndarray) -> np.ndarray:
    return np.ldexp(F32(1.0), np.asarray(E).astype(np.int32) - 127).astype(F32)


def quant_keys(x: np.ndarray):
    """x [..., dp] (bf16-rounded values for bit-equality with the kernel) -> (codes uint8 [..., dp], scale bytes uint8 [...],
    dequantised f32 [..., dp]): one scale per key = the smallest 2^e with amax / 2^e <= 448 (byte 127 for an all-zero key), codes =
    e4m3_round(x / 2^e), ties to even.  x / 2^e is exact, so the e4m3 rounding is the only one."""
    x = np.ascontiguousarray(x, dtype=F32)
    E = O.e8m0_of_amax(np.abs(x).max(axis=-1))
    s = scale_values(E)[..., None]
    q = O.e4m3_round(x / s)
    return e4m3_bytes(q), E, (q * s).astype(F32)


def dequant(codes: np.ndarray, E: np.ndarray) -> np.ndarray:
    return (e4m3_values(codes) * scale_values(E)[..., None]).astype(F32)


def decode_attention(q, kp, vp, kg, vg, lens, step, group, scale):
    """q [BB, nh, d]; prompt keys / values [B0, nkv, Tp, d], generated [BB, nkv, G, d] -> (o [BB, nh, d], A = P |v|: the term of
    gpu_util.attn_o_bound), in the operands' precision."""
    BB, nh, d = q.shape
    nkv = kp.shape[1]
    G = nh // nkv
    out, A = np.zeros((BB, nh, d), dtype=q.dtype), np.zeros((BB, nh, d), dtype=q.dtype)
    for bb in range(BB):
        b0 = bb // group
        for h in range(nh):
            kv = h // G
            k = np.concatenate([kp[b0, kv, :lens[b0]], kg[bb, kv, :step + 1]], 0)
            v = np.concatenate([vp[b0, kv, :lens[b0]], vg[bb, kv, :step + 1]], 0)
            s = (k @ q[bb, h]) * scale
            p = np.exp(s - s.max())
            out[bb, h], A[bb, h] = (p / p.sum()) @ v, (p / p.sum()) @ np.abs(v)
    return out, A


@contextlib.contextmanager
def patched_oracle(prompt_lens, n_layers, quantiser=None):
    """Inside: oracle.attention_heads as the fp8 prompt segment sees it.  oracle.llama_next_token_logits runs its rows one at a time
    (batch 1) through n_layers layers, so call number c serves row (c // n_layers) % len(prompt_lens), whose first prompt_lens[row]
    positions are the prompt.  Query rows < that length attend to the plain k / v (the prefill); the others to k / v whose prompt
    positions went through `quantiser` (default: quant_keys' dequantised values; the identity makes the patch a no-op, bit for bit)."""
    quantiser = quantiser or (lambda x: quant_keys(x)[2])
    plain, calls = O.attention_heads, [0]

    def patched(q, k, v, bias, scale, prec):
        row = (calls[0] // n_layers) % len(prompt_lens)
        calls[0] += 1
        n0, T = int(prompt_lens[row]), q.shape[2]
        assert q.shape[0] == 1 and T >= n0, "patched_oracle serves llama_next_token_logits' one-row calls"
        out = plain(q, k, v, bias, scale, prec)
        if T > n0:
            k8, v8 = np.array(k, dtype=F32, copy=True), np.array(v, dtype=F32, copy=True)
            k8[:, :, :n0], v8[:, :, :n0] = quantiser(k8[:, :, :n0]), quantiser(v8[:, :, :n0])
            out[:, n0:] = plain(q, k8, v8, bias, scale, prec)[:, n0:]      # (the same call shape: the same bits under the identity)
        return out

    O.attention_heads = patched
    try:
        yield
    finally:
        O.attention_heads = plain
