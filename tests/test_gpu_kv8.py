"""The fp8 prompt segment of the KV cache, kernel by kernel (csrc/kv_cache.hip, csrc/attn_decode.hip; format in include/p2t_hip.h, p2t_kv_cache):

* p2t_kv_quant_store (the prefill's store: codes + one E8M0 byte per key for K and for V, V transposed) bit for bit against
  tests/kv8_reference.py, with sentinels behind the written positions;
* p2t_attention_decode_prompt_fp8 (the step's attention: e4m3 prompt tiles, bf16 generated tiles) row by row against fp64 on the
  dequantised stored operands, under the bf16 kernel's own bound (gpu_util.attn_o_bound, unchanged), NaN codes and 0xFF scale bytes
  behind every valid prefix;
* witnesses that catch a scale read from the wrong key, row, kv head or layer offset, and an ignored K scale."""
import numpy as np
import pytest
import torch

import kv8_reference as K
from gpu_util import attn_o_bound, check_rows, dev, to_dev, to_np
from p2t_hip import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = [(16, 4, 2, 1, 100, 3), (64, 4, 2, 2, 700, 70), (128, 8, 2, 1, 1500, 130), (48, 5, 1, 3, 64, 0), (128, 2, 2, 1, 5, 63), (64, 16, 1, 1, 200, 9)]
NAN8, NOSCALE = 0x7F, 0xFF                      # what sits behind every valid prefix: e4m3 NaN codes, the E8M0 NaN byte


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev())


@pytest.mark.parametrize("T", [1, 63, 65, 200])
@pytest.mark.parametrize("d", [16, 48, 64, 128])
def test_quant_store_vs_numpy(d, T):
    """Codes and both scale arrays bit for bit the reference's, V transposed, every byte at positions >= T still the 0xAA it held.  Among
    the keys: an all-zero one (scale byte 127), one whose maximum is -448 2^e exactly, the e4m3 ties (17, 19 -> 16, 20), and what the
    padded columns d .. dp of the input hold (3e4) in no maximum and no code."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    B, nkv = 3, 2
    dp, Tp = ops.head_dim_padded(d), ops.round_up(T, 64) + 64
    rs = np.random.RandomState(1000 * d + T)

    def keys():
        x = rs.randn(B, nkv, T, d) * np.exp2(rs.randint(-12, 13, size=(B, nkv, T, 1)))
        x[0, 0, 0] = 0.0
        x[1, 1, T // 2] = np.clip(x[1, 1, T // 2], -1, 1) * 2.0 ** -5
        x[1, 1, T // 2, 3] = -448.0 * 2.0 ** -9
        x[2, 0, T - 1, :6] = np.array([448.0, 17.0, 19.0, -17.0, 2.0 ** -10, 3 * 2.0 ** -10]) * 4.0
        x[2, 0, T - 1, 6:] = 0.0
        return synth.bf16_round(x.astype(F32))

    k, v = keys(), keys()
    pad = lambda a: np.concatenate([a, np.full(a.shape[:-1] + (dp - d,), 3e4, F32)], -1)
    kd, vd = to_dev(pad(k), torch.bfloat16), to_dev(pad(v), torch.bfloat16)
    kq, vq = torch.full((B, nkv, Tp, dp), 0xAA, dtype=torch.uint8, device=dev()), torch.full((B, nkv, dp, Tp), 0xAA, dtype=torch.uint8, device=dev())
    ks, vs = torch.full((B, nkv, Tp), 0xAA, dtype=torch.uint8, device=dev()), torch.full((B, nkv, Tp), 0xAA, dtype=torch.uint8, device=dev())
    _lib.call("p2t_kv_quant_store", ptr(kd), ptr(vd), B, nkv, T, d, Tp, ptr(kq), ptr(vq), ptr(ks), ptr(vs), stream())
    kq, vq, ks, vs = (to_np(t) for t in (kq, vq, ks, vs))
    zpad = lambda c: np.concatenate([c, np.zeros(c.shape[:-1] + (dp - d,), np.uint8)], -1)
    for name, x, codes, sc, transposed in (("k", k, kq, ks, False), ("v", v, vq, vs, True)):
        want_c, want_s, _ = K.quant_keys(x)
        if transposed:
            codes = codes.transpose(0, 1, 3, 2)
        assert np.array_equal(sc[:, :, :T], want_s), name
        assert np.array_equal(codes[:, :, :T], zpad(want_c)), name
        assert (codes[:, :, T:] == 0xAA).all() and (sc[:, :, T:] == 0xAA).all(), name
    assert ks[0, 0, 0] == 127 and not kq[0, 0, 0].any()
    assert K.e4m3_values(kq[1, 1, T // 2, 3]) == -448.0 and ks[1, 1, T // 2] == 127 - 9
    assert K.dequant(kq[2, 0, T - 1, :6], ks[2, 0, T - 1]).tolist() == [1792.0, 64.0, 80.0, -64.0, 0.0, 2 ** -6]


def _case(shape, seed):
    """The operands of one shape: q and the generated segment in bf16, the prompt segment as codes + scale bytes with their dequantised
    values; lens = the longest prompt, a third of it, a single key."""
    from p2t_hip import ops
    d, nh, nkv, group, n0max, step = shape
    B0 = 3
    BB, dp = B0 * group, ops.head_dim_padded(d)
    Tp, G = ops.round_up(n0max, 64), ops.round_up(step + 1, 64)
    lens = np.array([n0max, max(1, n0max // 3), 1], dtype=np.int32)
    rs = np.random.RandomState(seed)
    f = lambda *s: synth.bf16_round((rs.randn(*s) * 0.7).astype(F32))
    q, kg, vg = f(BB, nh, d), f(BB, nkv, G, d), f(BB, nkv, G, d)
    kp = synth.bf16_round(f(B0, nkv, Tp, d) * np.exp2(rs.randint(-2, 2, size=(B0, nkv, Tp, 1))).astype(F32))
    vp = synth.bf16_round(f(B0, nkv, Tp, d) * np.exp2(rs.randint(-4, 5, size=(B0, nkv, Tp, 1))).astype(F32))
    return dict(d=d, nh=nh, nkv=nkv, group=group, step=step, B0=B0, BB=BB, dp=dp, Tp=Tp, G=G, lens=lens, q=q, kg=kg, vg=vg, kp=K.quant_keys(kp), vp=K.quant_keys(vp))


def _run(c, q, kc, ks, vc, vs, kg, vg, use_mfma=1):
    """One p2t_attention_decode_prompt_fp8 call: prompt codes [B0, nkv, Tp, d] + scale bytes [B0, nkv, Tp], generated keys / values f32
    [BB, nkv, G, d]; everything behind the valid prefixes is poisoned here.  -> o f32 [BB, nh, d]."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    d, dp, nh, nkv, B0, BB, Tp, G, lens, step = (c[k] for k in ("d", "dp", "nh", "nkv", "B0", "BB", "Tp", "G", "lens", "step"))
    kc, ks, vc, vs, kg, vg = (np.array(a, copy=True) for a in (kc, ks, vc, vs, kg, vg))
    for b in range(B0):
        kc[b, :, lens[b]:] = NAN8; vc[b, :, lens[b]:] = NAN8
        ks[b, :, lens[b]:] = NOSCALE; vs[b, :, lens[b]:] = NOSCALE
    kg[:, :, step + 1:] = np.nan; vg[:, :, step + 1:] = np.nan
    padf = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (dp - d,), F32)], -1)
    pad8 = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (dp - d,), np.uint8)], -1)
    qd, kgd = to_dev(padf(q), torch.bfloat16), to_dev(padf(kg), torch.bfloat16)
    vtg = to_dev(np.ascontiguousarray(padf(vg).transpose(0, 1, 3, 2)), torch.bfloat16)
    kcd, vtc = _u8(pad8(kc)), _u8(pad8(vc).transpose(0, 1, 3, 2))
    ksd, vsd = _u8(ks), _u8(vs)
    QO = ops.round_up(nh * d, 64)
    out = torch.zeros((BB, QO), dtype=torch.bfloat16, device=dev())
    lens_d, step_d = to_dev(lens), torch.tensor([step], dtype=torch.int32, device=dev())
    _lib.call("p2t_attention_decode_prompt_fp8", ptr(qd), ptr(kcd), ptr(vtc), ptr(kgd), ptr(vtg), ptr(lens_d), ptr(step_d), B0, c["group"], nh, nkv, d, Tp, G,
              float(d ** -0.5), 1, ops.dt_of(torch.bfloat16), use_mfma, ptr(out), QO, ptr(ksd), ptr(vsd), stream())
    got = to_np(out).astype(F32)[:, : nh * d].reshape(BB, nh, d)
    assert np.isfinite(got).all()
    return got


def _ref64(c, q, kp, vp, kg, vg):
    o, A = K.decode_attention(*(a.astype(np.float64) for a in (q, kp, vp, kg, vg)), c["lens"], c["step"], c["group"], np.log(2.0))
    return dict(o=o[:, :, None], A=A[:, :, None])


@pytest.mark.parametrize("shape", SHAPES)
def test_attention_prompt_fp8_rows_vs_fp64(shape):
    """Every element of every row against fp64 on the dequantised stored operands, under the bf16 kernel's bound (one bf16 step +
    (2^-7 + 2^-20) P |v|): the powers of two fold exactly, so nothing rounds where the bf16 kernel does not.  q holds scale * log2(e)
    (log2_scores), as the decode step stores it.  Behind every valid prefix: 0x7F codes, 0xFF scale bytes, NaN in the generated segment."""
    c = _case(shape, 7 + shape[0] + shape[1])
    (kc, ks, kdq), (vc, vs, vdq) = c["kp"], c["vp"]
    got = _run(c, c["q"], kc, ks, vc, vs, c["kg"], c["vg"])
    r64 = _ref64(c, c["q"], kdq, vdq, c["kg"], c["vg"])
    check_rows(f"attn_rows[decode_kv8,d{shape[0]},nh{shape[1]},g{shape[3]},n{shape[4]},s{shape[5]}]", [("o", got[:, :, None], r64["o"], attn_o_bound(r64, True, True))])


@pytest.mark.parametrize("shape", SHAPES)
def test_witnesses(shape):
    """(a) q = 0: every visible p is exactly 1 / n.  Key j of the prompt segment of batch row b holds the CODE of 1 + kv + nkv b at column
    j mod c under the V scale byte 127 + (j mod 5) - 2; key j of the generated segment of beam bb holds 1 + kv + nkv (B0 + bb) at column
    (7 j + 3) mod c: small integers times powers of two, so the quotient is exact to one bf16 step -- a scale read from another key, row
    or kv head moves it by a factor of two or more.
    (b) every K code is 1.0 and the K scale byte of key j is 127 + (j mod 5) - 2; q is the unit vector, so key j scores 2^((j mod 5) - 2)
    in base 2, the generated keys (zero) score 0; V is one-hot per key as in (a) with value 1.  The probabilities are known in closed
    form, and the bf16 kernel's bound holds against them: an ignored or mis-indexed K scale does not survive."""
    c = _case(shape, 3)
    d, nh, nkv, B0, BB, Tp, G, lens, step, group = (c[k] for k in ("d", "nh", "nkv", "B0", "BB", "Tp", "G", "lens", "step", "group"))
    cc = min(d, 64)
    jp, jg = np.arange(Tp), np.arange(G)
    sc5 = (127 + (jp % 5) - 2).astype(np.uint8)
    one_byte = K.e4m3_bytes(np.array([1.0], F32))[0]
    # (a)
    wp, wg = np.zeros((B0, nkv, Tp, d), F32), np.zeros((BB, nkv, G, d), F32)
    for kv in range(nkv):
        for b in range(B0):
            wp[b, kv, jp, jp % cc] = 1 + kv + nkv * b
        for bb in range(BB):
            wg[bb, kv, jg, (7 * jg + 3) % cc] = 1 + kv + nkv * (B0 + bb)
    vcodes, vscale = K.e4m3_bytes(wp), np.broadcast_to(sc5, (B0, nkv, Tp))
    kc, ks, _ = c["kp"]
    q0 = np.zeros_like(c["q"])
    got = _run(c, q0, kc, ks, vcodes, vscale, c["kg"], wg)
    r64 = _ref64(c, q0, np.zeros_like(wp), K.dequant(vcodes, vscale), np.zeros_like(wg), wg)
    check_rows(f"attn_rows[decode_kv8,witness_v,d{d},nh{nh},g{group}]", [("o", got[:, :, None], r64["o"], attn_o_bound(r64, True, True, witness=True))])
    # (b)
    kcodes = np.full((B0, nkv, Tp, d), one_byte, np.uint8)
    hot_p, hot_g = (wp != 0).astype(F32), (wg != 0).astype(F32)
    qe = np.zeros_like(c["q"]); qe[:, :, 0] = 1.0
    got = _run(c, qe, kcodes, np.broadcast_to(sc5, (B0, nkv, Tp)), K.e4m3_bytes(hot_p), np.full((B0, nkv, Tp), 127, np.uint8), np.zeros_like(wg), hot_g)
    want = np.zeros((BB, nh, d))
    for bb in range(BB):
        n0 = int(lens[bb // group])
        w = np.concatenate([np.exp2(np.exp2((jp[:n0] % 5) - 2.0)), np.ones(step + 1)])           # 2^score of every visible key
        cols = np.concatenate([jp[:n0] % cc, (7 * jg[:step + 1] + 3) % cc])
        np.add.at(want[bb, 0], cols, w / w.sum())
        want[bb, 1:] = want[bb, 0]
    r64 = dict(o=want[:, :, None], A=want[:, :, None])
    check_rows(f"attn_rows[decode_kv8,witness_k,d{d},nh{nh},g{group}]", [("o", got[:, :, None], r64["o"], attn_o_bound(r64, True, True))])


def test_the_lane_per_key_kernel_is_refused_on_the_device_too():
    from p2t_hip import _lib
    c = _case(SHAPES[0], 1)
    (kc, ks, _), (vc, vs, _) = c["kp"], c["vp"]
    with pytest.raises(_lib.P2TError, match=r"failed \(-3\)"):
        _run(c, c["q"], kc, ks, vc, vs, c["kg"], c["vg"], use_mfma=0)
