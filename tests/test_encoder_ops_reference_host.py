"""tests/encoder_ops_reference.py on its own (no GPU): the fp32 restatement of the Abramowitz-Stegun erf against math.erf (the E of the
bf16-output GELU bound in tests/test_gpu_encoder_ops.py), and every reference helper against torch autograd / the fp64 encoder
restatement at a small shape."""
import math

import numpy as np
import torch

import encoder_ops_reference as E
import esm_lora_reference as R


def test_abramowitz_stegun_erf_in_fp32_stays_below_1e_6():
    """csrc/common.h erf_as: 1.5e-7 is formula 7.1.26's bound in exact arithmetic; evaluated in fp32 (IEEE division and exp) it is up to
    ~5e-7 from math.erf over linspace(-40, 40) -- the bf16-output bound of p2t_gelu_rows takes its E from this restatement."""
    z = np.linspace(-40, 40, 801, dtype=np.float32)
    a = (z * np.float32(E.SQRT1_2)).astype(np.float32)
    got = E.erf_as_f32(a).astype(np.float64)
    want = np.array([math.erf(float(v) / math.sqrt(2.0)) for v in z.astype(np.float64)])
    err = float(np.abs(got - want).max())
    print(f"erf_as in fp32 vs math.erf over linspace(-40, 40, 801): max abs error {err:.3e}")
    assert 1.5e-7 < err < 1e-6                           # not the exact-arithmetic bound; within the 1e-6 the GELU bound assumes
    assert abs(E.erf_as_error(z) - err) < 1e-15          # erf64 (torch.erf in fp64) is math.erf on this grid
    for n in (8, 1900, 100000):
        grid = E.gelu_grid(n, n)
        assert E.erf_as_error(grid) < 1e-6
        assert grid.min() == -40 and grid.max() == 40 and np.any(np.signbit(grid) & (grid == 0)) and np.any(~np.signbit(grid) & (grid == 0))


def test_gelu_reference_vs_torch_autograd():
    z = torch.from_numpy(E.gelu_grid(1900, 3).astype(np.float64)).requires_grad_(True)
    y = torch.nn.functional.gelu(z)
    dy = torch.randn(z.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    dz = torch.autograd.grad(y, z, dy)[0]
    zn = z.detach().numpy()
    assert np.abs(E.gelu64(zn) - y.detach().numpy()).max() < 1e-14
    assert np.abs(dy.numpy() * E.gelu_grad64(zn) - dz.numpy()).max() < 1e-14


def test_layernorm_backward_reference_vs_closed_form():
    rng = np.random.default_rng(0)
    x, w, dy = rng.standard_normal((7, 40)) * 2 + 0.5, rng.standard_normal(40), rng.standard_normal((7, 40))
    x[3] = 1.25                                          # a constant row: var = 0, r = rsqrt(eps)
    t = E.layernorm_bwd_terms(x, w, dy, 1e-5)
    closed = t["r"] * (t["gw"] - t["m1"] - t["xhat"] * t["c2"])
    ref = E.layernorm_bwd64(x, w, dy, 1e-5)
    assert np.abs(ref - closed).max() < 1e-10 * np.abs(closed).max()
    assert abs(float(t["r"][3, 0]) - 1e-5 ** -0.5) < 1e-9


def test_esm_embed_reference_vs_fp64_encoder_embedding():
    g = torch.Generator().manual_seed(1)
    vocab, H, B, T, mask_id = 33, 16, 3, 9, 32
    table = torch.randn((vocab, H), generator=g)
    ids = torch.randint(4, 24, (B, T), generator=g)
    mask = torch.zeros((B, T), dtype=torch.int64)
    for b, n in enumerate((9, 5, 1)):
        mask[b, :n] = 1
    ids[0, 2], ids[0, 7], ids[1, 1], ids[1, 8] = mask_id, mask_id, mask_id, mask_id      # [1, 8]: a <mask> in the padding counts in the ratio
    for td in (True, False):
        got = E.esm_embed_f32(ids, mask, table, mask_id, td)
        e = table.double()[ids]
        if td:
            is_mask = ids == mask_id
            e = e.masked_fill(is_mask[..., None], 0.0)
            e = e * (1.0 - 0.15 * 0.8) / (1.0 - is_mask.sum(-1).double() / mask.sum(-1).double())[:, None, None]
        want = e * mask[..., None].double()
        assert got.dtype == torch.float32
        assert float((got.double() - want).abs().max()) < 1e-6 * float(want.abs().max())
    # the same embedding as tests/esm_lora_reference.encoder starts from: layer count 0 leaves LayerNorm(embedding)
    W = {"embeddings.word_embeddings.weight": table.double(), "encoder.emb_layer_norm_after.weight": torch.ones(H, dtype=torch.float64),
         "encoder.emb_layer_norm_after.bias": torch.zeros(H, dtype=torch.float64)}
    cfg = dict(n_layers=0, heads=2, head_dim=8, eps=1e-5, mask_id=mask_id, token_dropout=True, inv_freq=torch.ones(4))
    out = R.encoder(W, cfg, ids, mask)
    ln = torch.nn.functional.layer_norm(E.esm_embed_f32(ids, mask, table, mask_id, True).double(), (H,), None, None, 1e-5)
    assert float((out - ln).abs().max()) < 1e-5


def test_attention_reference_vs_torch_autograd():
    g = torch.Generator().manual_seed(2)
    B, nh, nkv, T, d = 2, 4, 2, 11, 6
    q, k, v = (torch.randn((B, h, T, d), dtype=torch.float64, generator=g).requires_grad_(True) for h in (nh, nkv, nkv))
    d_o = torch.randn((B, nh, T, d), dtype=torch.float64, generator=g)          # non-zero on padded query rows too
    mask = np.zeros((B, T), dtype=np.int64)
    mask[0, :], mask[1, :1] = 1, 1                       # a full row and a one-residue protein
    c_s = 0.37
    for causal in (False, True):
        kr, vr = k.repeat_interleave(nh // nkv, 1), v.repeat_interleave(nh // nkv, 1)
        s = (q @ kr.transpose(-1, -2)) * c_s
        ok = torch.from_numpy(mask != 0)[:, None, None, :]
        if causal:
            ok = ok & torch.tril(torch.ones((T, T), dtype=torch.bool))
        s = s.masked_fill(~ok, float("-inf"))
        rows = ok.any(-1).expand(B, nh, T)
        p = torch.softmax(s, -1).nan_to_num(0.0)
        o = p @ vr
        dq, dk, dv = torch.autograd.grad(o, (q, k, v), d_o * rows[..., None])
        r = E.attention_fwd_bwd64(q.detach().numpy(), k.detach().numpy(), v.detach().numpy(), d_o.numpy(), mask, causal, c_s)
        assert np.array_equal(r["rows"], rows.numpy())
        lse = torch.logsumexp(s, -1).detach().numpy()
        assert np.abs(r["lse"][r["rows"]] - lse[r["rows"]]).max() < 1e-12 and np.all(np.isposinf(r["lse"][~r["rows"]]))
        for nm, want in (("o", o.detach()), ("dq", dq), ("dk", dk), ("dv", dv)):
            assert np.abs(r[nm] - want.numpy()).max() < 1e-12, (causal, nm)
        if not causal:                                   # right-padded, bidirectional: padded keys get nothing, padded queries still see keys
            assert not r["dk"][1, :, 1:].any() and not r["dv"][1, :, 1:].any() and r["dq"][1, :, 1:].any()
