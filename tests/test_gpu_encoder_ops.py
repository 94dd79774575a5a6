"""The entry points of the encoder LoRA step (p2t_hip/encoder_train.py) one by one against fp64, at ESM2 shapes and at the edges of
their loops: p2t_layernorm_backward, p2t_gelu_rows (all eight dtype forms), p2t_esm2_embed with p2t_mask_prepare (bit-exact against
HF's fp32 arithmetic), and the bidirectional attention forward / backward at ESM2 head geometry.

Conventions as tests/test_gpu_stage2_ops.py (helpers in tests/gpu_util.py): fp32 outputs within 1e-6 |ref| plus a stated absolute term,
a bf16 output within one bf16 rounding step of the fp64 value computed from the operands as stored, every output buffer one row longer
and 64 columns wider than the contract writes with a sentinel that must survive, columns the contract zeroes exactly zero."""
import numpy as np
import pytest
import torch

import encoder_ops_reference as E
from gpu_util import _assert_sentinel, _check, _q, _sentinel, dev, observe, rel, to_np
from p2t_hip import _lib, ops
from p2t_hip._lib import call
from p2t_hip.ops import ptr, round_up, stream

pytestmark = pytest.mark.gpu
DTS = (torch.float32, torch.bfloat16)
U32 = 2.0 ** -23                                        # fp32 machine epsilon
REFUSED = (ValueError, _lib.P2TError)


# ---------------------------------------------------------------------------------------------
def _ln_inputs(rows, cols, seed):
    """x [rows, cols] fp32 in three regimes by row: r % 3 == 0 randn * 2 + 0.5; r % 3 == 1 mean 100, unit spread (the mean pass cancels);
    row 2 (when there is one) constant 0.7 (var = 0, r = rsqrt(eps)).  -> x, w, dy (numpy fp32), regime [rows] in {0, 1, 2}."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, cols)) * 2 + 0.5).astype(np.float32)
    regime = np.zeros(rows, dtype=np.int64)
    regime[1::3] = 1
    n = rng.standard_normal((int((regime == 1).sum()), cols))
    n = (n - n.mean(1, keepdims=True)) / n.std(1, keepdims=True)      # unit spread in every row (r = 1), also where cols = 4: the bound's premise
    x[regime == 1] = (n + 100).astype(np.float32)
    if rows > 2:
        regime[2] = 2
        x[2] = np.float32(0.7)
    w = (1 + 0.3 * rng.standard_normal(cols)).astype(np.float32)
    dy = rng.standard_normal((rows, cols)).astype(np.float32)
    return x, w, dy, regime


def _ln_atol(x, w, dy, eps, regime, ref):
    """The absolute term of the fp32 bound on g = r (gw - m1 - xhat c2), gw = w dy, m1 = mean gw, c2 = mean gw xhat, from fp32's precision:
    * every product / difference is rounded at the scale of its summands: 4 U32 r (|gw| + |m1| + |xhat c2|);
    * a mean over `cols` fp32 terms accumulated `depth` deep (4 ceil(cols / 256) sequential adds in a lane + 6 butterfly levels) is off
      by at most depth U32 mean|term|: depth U32 r (mean|gw| + |xhat| mean|gw xhat|);
    * the mean mu itself is off by delta <= depth U32 mean|x|, which moves xhat by e = r delta:
        g' - g = r e (c2 + xhat m1) + O(e^2)   (s2' = sum gw (xc - delta) = s2 - delta s1; var' = var + delta^2, so r'/r - 1 = -e^2 / 2)
      -> r e (|c2| + |xhat| |m1|) + r e^2 (|m1| + mean|gw|) + e^2 |g| / 2.  The second-order part matters only on the constant row,
      where r = eps^-1/2 = 316 multiplies delta.
    * rows with mean 100 and unit spread (r = 1): a single rounding of mu is already delta = U32 * 100, and with r = 1 and
      |c2 + xhat m1| <= 2 max|xhat| mean|gw| <= sum|gw| the first-order term r e (...) is at most U32 * 100 * r * sum_j |w_j dy_j| over the
      row.  That expression is a ceiling on those rows (it is first order in r only because r = 1: the sensitivity is r^2 delta, so the
      inputs keep the spread at 1); it grows with cols, so the per-element form of the same term above is what binds wherever it is the
      smaller of the two -- the bound is never wider than U32 * 100 * r * sum|gw| and at cols = 5120 about a thousand times tighter."""
    t = E.layernorm_bwd_terms(x, w, dy, eps)
    cols = x.shape[1]
    depth = 4 * -(-cols // 256) + 6
    r, xh = t["r"], np.abs(t["xhat"])
    atol = U32 * r * (4 * (np.abs(t["gw"]) + np.abs(t["m1"]) + xh * np.abs(t["c2"])) + depth * (t["a1"] + xh * t["a2"]))
    e = r * depth * U32 * t["ax"]
    mu_term = r * e * (np.abs(t["c2"]) + xh * np.abs(t["m1"])) + r * e * e * (np.abs(t["m1"]) + t["a1"]) + 0.5 * e * e * np.abs(ref)
    mean100 = U32 * 100.0 * r * np.abs(t["gw"]).sum(1, keepdims=True) * np.ones_like(xh)
    return atol + np.where((regime == 1)[:, None], np.minimum(mean100, mu_term), mu_term)


def _ln_case(rows, cols, dyt, acc, seed):
    eps = 1e-5
    x, w, dy, regime = _ln_inputs(rows, cols, seed)
    ld_x, ld_dy, ld_dx = cols + 4, cols + 8, cols + 64
    xd = torch.zeros((rows, ld_x), device=dev())
    xd[:, :cols] = torch.from_numpy(x).to(dev())
    dyd = torch.zeros((rows, ld_dy), dtype=dyt, device=dev())
    dyd[:, :cols] = torch.from_numpy(dy).to(dev(), dyt)
    wd = torch.from_numpy(w).to(dev())
    dy64 = _q(dy, dyt)
    out = _sentinel((rows + 1, ld_dx), torch.float32)    # accumulate = 0: the sentinel must be overwritten, not added to
    base = None
    if acc:
        base = torch.randn((rows, cols), generator=torch.Generator().manual_seed(seed + 1))
        out[:rows, :cols] = base.to(dev())
    call("p2t_layernorm_backward", ptr(xd), ld_x, ptr(wd), eps, ptr(dyd), ld_dy, ops.dt_of(dyt), ptr(out), ld_dx, rows, cols, acc, stream())
    ref = E.layernorm_bwd64(x, w, dy64, eps)
    atol = _ln_atol(x, w, dy64, eps, regime, ref)
    got = to_np(out)[:rows, :cols].astype(np.float64)
    if acc:
        b64 = base.double().numpy()
        got, atol = got - b64, atol + 1e-6 * np.abs(b64)
    for reg in (0, 1, 2):
        sel = regime == reg
        if sel.any():
            _check(got[sel], ref[sel], torch.float32, atol=atol[sel], what=f"dx (regime {reg})")
    _assert_sentinel(out, cols=cols, rows=rows)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dyt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 5, 2049])
@pytest.mark.parametrize("cols", [4, 64, 200, 320, 480, 640, 1280, 2560, 5120])
def test_layernorm_backward(cols, rows, dyt, acc):
    _ln_case(rows, cols, dyt, acc, cols * 3 + rows)


@pytest.mark.parametrize("dyt,acc", [(torch.bfloat16, 0), (torch.float32, 1)], ids=["bf16_set", "f32_acc"])
def test_layernorm_backward_at_the_cfg3_batch(dyt, acc):
    _ln_case(16384, 2560, dyt, acc, 5)


def test_layernorm_backward_refusals_write_nothing():
    rows, cols = 5, 64
    x, w = torch.randn((rows, cols), device=dev()), torch.ones(cols, device=dev())
    dy = torch.randn((rows, cols), device=dev())
    out = _sentinel((rows + 1, cols + 64), torch.float32)
    bad = [dict(cols=62), dict(ld_x=cols - 4), dict(ld_dy=cols - 4), dict(ld_dx=cols - 4), dict(dt=2), dict(dt=_lib.F32 - 1)]
    for kw in bad:
        a = dict(cols=cols, ld_x=cols, ld_dy=cols, ld_dx=cols + 64, dt=_lib.F32)
        a.update(kw)
        with pytest.raises(REFUSED):
            call("p2t_layernorm_backward", ptr(x), a["ld_x"], ptr(w), 1e-5, ptr(dy), a["ld_dy"], a["dt"], ptr(out), a["ld_dx"], rows, a["cols"], 0, stream())
        _assert_sentinel(out, rows=0)


# ---------------------------------------------------------------------------------------------
# erff is accurate to 4 ulp (the HIP math API's stated bound): |erff - erf| <= 4 * 2^-23 since |erf| <= 1; forming 1 + erf and the two
# products round once each.  Where z < 0, 1 + erf cancels and none of that is relative to the result any more, hence an absolute term
# |z| / 2 * 2^-23 * C_FWD with C_FWD = 4 (erff) + 2 (the sum and the argument's rounding).  Backward: Phi = (1 + erff) / 2 carries half of
# that (2.5), z phi(z) with expf at 1 ulp and the argument -z^2 / 2 rounded (|z|^3 phi(z) / 2 <= 0.25) another 0.5, the final sum 1.
C_FWD, C_BWD = 6.0, 4.0
GELU_SHAPES = [(1, 8), (19, 100), (37, 1280), (257, 8200), (2048, 10240)]      # (257, 8200): 2 121 792 outputs > 8192 * 256, a partial second stride


@pytest.mark.parametrize("M,N", GELU_SHAPES)
@pytest.mark.parametrize("ot", DTS, ids=["out_f32", "out_bf16"])
@pytest.mark.parametrize("dt_", DTS, ids=["dy_f32", "dy_bf16"])
@pytest.mark.parametrize("zt", DTS, ids=["z_f32", "z_bf16"])
def test_gelu_rows_forward_and_backward(zt, dt_, ot, M, N):
    zg = E.gelu_grid(M * N, M + N).reshape(M, N)
    dyg = np.random.default_rng(N).standard_normal((M, N)).astype(np.float32)
    z64, dy64 = _q(zg, zt), _q(dyg, dt_)
    ld_z, ld_dy = N + 3, N + 5
    z = torch.zeros((M, ld_z), dtype=zt, device=dev())
    z[:, :N] = torch.from_numpy(zg).to(dev(), zt)
    dy = torch.zeros((M, ld_dy), dtype=dt_, device=dev())
    dy[:, :N] = torch.from_numpy(dyg).to(dev(), dt_)
    Np = round_up(N, 64)
    # the bf16-output forward runs the Abramowitz-Stegun erf: E from the fp32 restatement against fp64 on THIS grid (as stored), doubled
    # for the hardware rcp / exp (1 ulp each) that numpy's IEEE division and exp do not model.  Never from the kernel.
    e_as = 2.0 * E.erf_as_error(z64.astype(np.float32))
    assert e_as < 2e-6
    lds = [Np + 64] + ([N] if N % 64 else [])            # ld_out == N < round_up(N, 64): the zero fill is clamped to the row
    for ld_out in lds:
        n_zero = min(Np, ld_out)
        for bwd in (False, True):
            out = _sentinel((M + 1, ld_out), ot)
            call("p2t_gelu_rows", ptr(z), ops.dt_of(zt), ld_z, ptr(dy) if bwd else None, ops.dt_of(dt_), ld_dy, ptr(out), ops.dt_of(ot), ld_out, M, N,
                 stream())
            got = to_np(out)
            if bwd:
                ref = dy64 * E.gelu_grad64(z64)
                atol = np.abs(dy64) * U32 * C_BWD         # gelu_erf_grad keeps erff whatever the output type
            else:
                ref = E.gelu64(z64)
                atol = np.abs(z64) / 2 * (U32 * C_FWD if ot == torch.float32 else e_as)
            _check(got[:M, :N], ref, ot, atol=atol + 1e-37, what=f"{'backward' if bwd else 'forward'} ld_out {ld_out}")
            assert np.all(got[:M, N:n_zero] == 0), "columns N .. round_up(N, 64) are zeroed"
            _assert_sentinel(out, cols=n_zero, rows=M)    # with ld_out == N a write past the row's end lands in the next row: the last one is the sentinel's


def test_gelu_rows_refusals_write_nothing():
    M, N = 4, 100
    z, dy = torch.randn((M, N), device=dev()), torch.randn((M, N), device=dev())
    out = _sentinel((M + 1, 192), torch.float32)
    F = _lib.F32
    for a in (dict(zt=2), dict(ot=3), dict(dt=5), dict(ld_z=N - 1), dict(ld_out=N - 1), dict(ld_dy=N - 1)):
        k = dict(zt=F, ot=F, dt=F, ld_z=N, ld_out=192, ld_dy=N)
        k.update(a)
        with pytest.raises(REFUSED):
            call("p2t_gelu_rows", ptr(z), k["zt"], k["ld_z"], ptr(dy), k["dt"], k["ld_dy"], ptr(out), k["ot"], k["ld_out"], M, N, stream())
        _assert_sentinel(out, rows=0)


# ---------------------------------------------------------------------------------------------
VOCAB, MASK_ID = 33, 32


def _embed_batch(B, T, seed):
    """Right-padded proteins of B different lengths.  Row b carries b <mask> tokens under the mask (row 0 none, row 1 one, then many) and,
    on odd rows, one more in the padding (HF counts it in the ratio; so does mask_prepare_kernel): a different observed ratio on every
    row.  Where T >= 37, two ids of row 0 (which carries no <mask>) are -1 and `vocab`: the kernel's contract maps them to a zero row (HF
    would fault on them).
    No fully padded row: with token dropout its ratio is 0 / 0 = NaN in HF as well -- callers must not pass one; that is the contract,
    not a case."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(4, 24, size=(B, T)).astype(np.int64)
    mask = np.zeros((B, T), dtype=np.int64)
    lens = [T - (b * T) // (B + 1) for b in range(B)]
    for b, n in enumerate(lens):
        mask[b, :n] = 1
        ids[b, rng.choice(n, size=min(b, n - 1), replace=False)] = MASK_ID
        if b % 2 == 1 and n + 1 < T:
            ids[b, n + 1] = MASK_ID                      # in the padding
    if T >= 37:
        free = np.flatnonzero(ids[0] != MASK_ID)
        ids[0, free[5]], ids[0, free[6]] = -1, VOCAB
    return ids, mask, lens


@pytest.mark.parametrize("td", [1, 0], ids=["token_dropout", "plain"])
@pytest.mark.parametrize("tt", DTS, ids=["table_f32", "table_bf16"])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 37), (16, 1024)])
@pytest.mark.parametrize("H", [64, 320, 2560])
def test_esm2_embed_and_mask_prepare_bit_exact(H, B, T, tt, td):
    ids, mask, lens = _embed_batch(B, T, H + T)
    table = torch.randn((VOCAB, H), generator=torch.Generator().manual_seed(H)).to(tt)
    idd, md, tab = torch.from_numpy(ids).to(dev()), torch.from_numpy(mask).to(dev()), table.to(dev())
    key_mask, kv_info, emb_scale = ops.mask_prepare(md, idd, MASK_ID, bool(td))
    x = _sentinel((B * T + 1, H), torch.float32)
    call("p2t_esm2_embed", ptr(idd), ptr(md), ptr(tab), ops.dt_of(tt), ptr(emb_scale), B, T, H, VOCAB, MASK_ID, td, ptr(x), stream())
    # mask_prepare against numpy: fp32 arithmetic as HF's (count.float() / length, 1 - ratio)
    n_mask = (ids == MASK_ID).sum(1).astype(np.float32)
    ratio = n_mask / mask.sum(1).astype(np.float32)
    want_scale = np.stack([np.full(B, 0.88, np.float32), (np.float32(1) - ratio).astype(np.float32)], 1) if td else np.ones((B, 2), np.float32)
    assert np.array_equal(to_np(emb_scale).reshape(B, 2), want_scale)
    if td and T > 1:
        assert len(set(want_scale[:, 1].tolist())) == B, "every row has its own ratio: a wrong emb_scale row index cannot pass"
    assert np.array_equal(to_np(key_mask), mask.astype(np.uint8))
    assert np.array_equal(to_np(kv_info), np.concatenate([np.array(lens), np.ones(B)]).astype(np.int32))
    # the embedding rows: HF in torch fp32, bit for bit (out-of-range ids: a zero row)
    safe = torch.from_numpy(np.where((ids < 0) | (ids >= VOCAB), 0, ids))
    want = E.esm_embed_f32(safe, torch.from_numpy(mask), table, MASK_ID, bool(td)).reshape(B * T, H).clone()
    oob = torch.from_numpy(((ids < 0) | (ids >= VOCAB)).reshape(-1))
    want[oob] = 0.0
    got = x[:B * T].cpu()
    same = got.view(torch.int32) == want.view(torch.int32)
    assert bool(same.all()), f"{int((~same).sum())} elements differ in their bits from HF's fp32 arithmetic, first at {np.argwhere(~same.numpy())[:1].tolist()}"
    _assert_sentinel(x, rows=B * T)


def test_mask_prepare_flags_a_mask_that_is_not_a_prefix():
    mask = torch.tensor([[1, 1, 0, 1, 0], [0, 1, 1, 1, 1], [1, 1, 1, 0, 0]], dtype=torch.int64, device=dev())
    key_mask, kv_info, _ = ops.mask_prepare(mask)
    assert to_np(kv_info).tolist() == [4, 5, 3, 0, 0, 1]
    assert np.array_equal(to_np(key_mask), to_np(mask).astype(np.uint8))


# ---------------------------------------------------------------------------------------------
ATTN = [(24, 20, 130, [130, 77, 1]), (32, 20, 300, [300, 1]), (64, 20, 1024, [1024, 611, 1]), (64, 40, 512, [512, 383]), (128, 40, 256, [256, 100])]


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("d,nh,T,lens", ATTN, ids=[f"d{c[0]}_h{c[1]}_T{c[2]}" for c in ATTN])
def test_bidirectional_attention_at_esm2_geometry(d, nh, T, lens, dt):
    """p2t_attention (lse) and p2t_attention_backward as the encoder step calls them (nh == nkv, causal = 0, right-padded keys, the
    query scale folded into q; bf16: log2_scores and the forward's default kernel choice) against the fp64 textbook attention on the
    stored operands.  d_o is non-zero on padded query rows too: they still see the valid keys, so their lse, output and dq are defined
    and compared like any other row -- nothing is excluded."""
    B = len(lens)
    l2s = dt == torch.bfloat16
    name = f"esm_d{d}_h{nh}_T{T}_{'bf16' if l2s else 'f32'}"
    mask = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    fold = d ** -0.5 * (1.4426950408889634 if l2s else 1.0)
    g = torch.Generator().manual_seed(d + nh + T)
    qkv = (torch.randn((B * T, round_up(3 * nh * d, 64)), generator=g) * 1.5).to(dev(), dt)
    inv = (1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))).to(dev())
    key_mask, kv_info, _ = ops.mask_prepare(torch.from_numpy(mask).to(dev()))
    q, k, v = ops.qkv_post(qkv, inv, B, T, nh, nh, d, fold)
    dp = ops.head_dim_padded(d)
    assert q.shape[-1] == dp and all(not to_np(t)[..., d:].any() for t in (q, k, v))
    lse = torch.empty((B, nh, T), dtype=torch.float32, device=dev())
    o = ops.attention(q, k, v, key_mask, kv_info, d, 1.0, False, log2_scores=l2s, lse=lse)
    d_o = torch.randn(tuple(o.shape), generator=g).to(dev(), dt)
    d_o[:, nh * d:] = 0
    forms = {"exact": ops.attention_backward(q, k, v, o, d_o, lse, key_mask, kv_info, d, 0.6931471805599453 if l2s else 1.0, False, log2_scores=l2s,
                                             use_mfma=0)}
    if l2s and d in (64, 128):
        forms["mfma"] = ops.attention_backward(q, k, v, o, d_o, lse, key_mask, kv_info, d, 0.6931471805599453, False, log2_scores=True, use_mfma=1)
    cut = lambda t: to_np(t).astype(np.float64).reshape(B, T, -1)[..., :nh * d].reshape(B, T, nh, d).transpose(0, 2, 1, 3)
    qn, kn, vn = (to_np(t).astype(np.float64)[..., :d] for t in (q, k, v))
    got_o = cut(o)
    ref = E.attention_fwd_bwd64(qn, kn, vn, cut(d_o), mask, False, np.log(2.0) if l2s else 1.0, o_stored=got_o)
    assert ref["rows"].all(), "every query row, padded ones included, sees a key"
    got_lse = to_np(lse).astype(np.float64)
    assert np.isfinite(got_lse).all()
    assert np.abs(got_lse - ref["lse"]).max() < (2e-5 if not l2s else 2e-2)
    assert rel(got_o, ref["o"]) < (2e-5 if not l2s else 1e-2)
    assert not to_np(o)[:, nh * d:].any(), "the o-proj K padding is zeroed"
    pad = mask == 0                                       # [B, T]
    tol = 3e-5 if not l2s else 2e-2
    for form, (dq, dk, dv) in forms.items():
        for nm, got, want in (("dq", dq, ref["dq"]), ("dk", dk, ref["dk"]), ("dv", dv, ref["dv"])):
            gn = to_np(got).astype(np.float64)
            assert np.isfinite(gn).all() and not gn[..., d:].any(), (form, nm, "padded head-dim columns [d, dp) are zero")
            observe(f"attn_bwd[{name},{form}].{nm}", rel(gn[..., :d], want), tol)
        for nm, got in (("dk", dk), ("dv", dv)):
            gp = to_np(got).transpose(0, 2, 1, 3)[pad]
            assert not gp.any(), (form, nm, "exactly zero at padded keys")
        # padded query rows on their own, so that the valid rows cannot hide them
        gq_all = to_np(dq).astype(np.float64)[..., :d].transpose(0, 2, 1, 3)              # [B, T, nh, d]
        wq_all = ref["dq"].transpose(0, 2, 1, 3)
        many = pad & (np.asarray(lens) > 1)[:, None]
        if many.any():
            observe(f"attn_bwd[{name},{form}].dq_padded_rows", rel(gq_all[many], wq_all[many]), tol)
        for b in np.flatnonzero(np.asarray(lens) == 1):
            # a one-residue protein: every row sees one key, P = 1 and dS = dO.v0 - D with D = dO.O and O = v0, so dq = 0 up to the
            # rounding of two length-d fp32 dot products: |dq| <= c_s |k0| (2 d + 2) 2^-23 sum_j |dO_j v0_j| (+ the reference's own ~1e-16)
            dO_b, v0, k0 = cut(d_o)[b], vn[b, :, 0, :], kn[b, :, 0, :]                  # [nh, T, d], [nh, d], [nh, d]
            s_abs = np.abs(dO_b * v0[:, None, :]).sum(-1)                                # [nh, T]
            bound = (np.log(2.0) if l2s else 1.0) * (2 * d + 2) * U32 * s_abs[..., None] * np.abs(k0)[:, None, :] + 1e-12
            err = np.abs(gq_all[b] - wq_all[b]).transpose(1, 0, 2)                       # [nh, T, d]
            assert np.all(err <= bound), (form, "dq of a one-residue protein", float((err / bound).max()))
