"""tests/attention_reference.py on its own, without a GPU: the fp64 reference with documents and bound terms against torch autograd and
against per-document references; the conditions every input set is built to meet; the numpy restatement of the MFMA kernels' forward
inside the caps of gpu_util.check_rows on every input set the GPU file uses (so a cap that fails on the GPU is not the arithmetic the
kernels are documented to run), the measured R32; and the sensitivity of the row check to six defects a kernel could have, next to
what the whole-tensor norm rel() makes of each."""
import numpy as np
import pytest
import torch

import attention_reference as R
from encoder_ops_reference import attention_fwd_bwd64
from gpu_util import R32, attn_lse_bound, attn_o_bound, check_rows, rel

HAND_SHAPES = ("g64", "g40", "h64")                      # head_dim padded to 64: where the hand-placed kernel runs


def test_reference_with_bound_terms_vs_torch_autograd():
    """GQA, causal and not, a mask with a hole and a hidden first key: values against fp64 autograd, the bound terms against their definitions."""
    g = torch.Generator().manual_seed(5)
    B, nh, nkv, T, d = 2, 4, 2, 13, 6
    rep = nh // nkv
    q, k, v = (torch.randn((B, h, T, d), dtype=torch.float64, generator=g).requires_grad_(True) for h in (nh, nkv, nkv))
    d_o = torch.randn((B, nh, T, d), dtype=torch.float64, generator=g)
    mask = np.ones((B, T), dtype=np.int64)
    mask[0, 4:7], mask[1, 0], mask[1, 10:] = 0, 0, 0
    c_s = 0.41
    for causal in (False, True):
        kr, vr = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
        ok = torch.from_numpy(mask != 0)[:, None, None, :].expand(B, nh, T, T)
        if causal:
            ok = ok & torch.tril(torch.ones((T, T), dtype=torch.bool))
        s = ((q @ kr.transpose(-1, -2)) * c_s).masked_fill(~ok, float("-inf"))
        rows = ok.any(-1)
        p = torch.softmax(s, -1).nan_to_num(0.0)
        o = p @ vr
        dq, dk, dv = torch.autograd.grad(o, (q, k, v), d_o * rows[..., None])
        r = attention_fwd_bwd64(q.detach().numpy(), k.detach().numpy(), v.detach().numpy(), d_o.numpy(), mask, causal, c_s, bounds=True)
        assert np.array_equal(r["rows"], rows.numpy()) and np.array_equal(r["n_visible"], ok.sum(-1).numpy())
        assert causal == (not r["rows"][1, :, 0].any()), "causal: row 0 of the batch row whose key 0 is hidden sees nothing"
        for nm, want in (("o", o.detach()), ("dq", dq), ("dk", dk), ("dv", dv)):
            assert np.abs(r[nm] - want.numpy()).max() < 1e-12, (causal, nm)
        pd, dOd = p.detach(), d_o * rows[..., None]
        dS = pd * (dOd @ vr.detach().transpose(-1, -2) - (dOd * o.detach()).sum(-1, keepdim=True))
        F = pd * (dOd.abs() @ vr.detach().abs().transpose(-1, -2) + (dOd.abs() * o.detach().abs()).sum(-1, keepdim=True))
        fold = lambda t: t.reshape(B, nkv, rep, T, d).sum(2)
        want = dict(A=pd @ vr.detach().abs(), dq_abs=c_s * dS.abs() @ kr.detach().abs(), dq_F=c_s * F @ kr.detach().abs(),
                    dk_abs=fold(c_s * dS.abs().transpose(-1, -2) @ q.detach().abs()), dk_F=fold(c_s * F.transpose(-1, -2) @ q.detach().abs()),
                    dv_abs=fold(pd.transpose(-1, -2) @ dOd.abs()), p_diag=torch.diagonal(pd, dim1=-2, dim2=-1))
        for nm, w in want.items():
            assert np.abs(r[nm] - w.numpy()).max() < 1e-12, (causal, nm)


def test_reference_with_documents_equals_the_documents_on_their_own():
    rng = np.random.default_rng(3)
    B, nh, nkv, T, d = 2, 4, 2, 40, 8
    rows = ([1, 9, 1, 17], [30, 10])                      # row 0 ends in 12 padding tokens
    q, k, v, d_o = (rng.standard_normal((B, h, T, d)) for h in (nh, nkv, nkv, nh))
    mask, start = np.zeros((B, T), dtype=np.int64), np.tile(np.arange(T), (B, 1))
    for b, lens in enumerate(rows):
        t = 0
        for n in lens:
            mask[b, t:t + n], start[b, t:t + n] = 1, t
            t += n
    r = attention_fwd_bwd64(q, k, v, d_o, mask, True, 0.3, docs=start, bounds=True)
    assert not r["rows"][0, :, 28:].any() and np.all(np.isposinf(r["lse"][0, :, 28:])) and not r["dq"][0, :, 28:].any()
    for b, lens in enumerate(rows):
        t = 0
        for n in lens:
            sl = lambda a: a[b:b + 1, :, t:t + n]
            one = attention_fwd_bwd64(sl(q), sl(k), sl(v), sl(d_o), np.ones((1, n), dtype=np.int64), True, 0.3, bounds=True)
            for nm in ("o", "lse", "dq", "dk", "dv", "A", "dq_abs", "dk_abs", "dv_abs", "dq_F", "dk_F", "n_visible"):
                assert np.abs(sl(r[nm]) - one[nm]).max() < 1e-12, (b, t, n, nm)
            t += n


def _ratio(got, ref, bound):
    err = np.abs(got - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(err <= bound, np.where(bound > 0, err / bound, 0.0), np.inf).max())


@pytest.fixture(scope="module")
def sets():
    """(case, inputs, fp64 reference) of every forward input set, built once."""
    out = []
    for c in R.forward_cases():
        x = R.inputs(c)
        out.append((c, x, R.reference(c, x, False)))
    return out


def test_every_input_set_meets_its_conditions(sets):
    """Dominant keys hold >= 0.25 of their partner row; the rescale cases jump by >= 12 (resp. >= 40) log2 units for half a 32-query group
    and by (1, 7) for the other half; witness rows have lse = ln n_visible.  Also: the masks hide what they are meant to hide."""
    for c, x, ref in sets:
        R.assert_conditions(c, x, ref)
        assert np.all(x["d_o"] != 0)
        if c.layout == "masks":
            n = ref["n_visible"][:, 0]
            kinds = dict(zip(R.MASK_KINDS, n))
            assert (kinds["single"][:c.T - 1] == (0 if c.causal else 1)).all() and kinds["single"][c.T - 1] == 1
            assert (kinds["first"][:70] == (0 if c.causal else c.T - 70)).all() and kinds["first"][70] > 0
            assert kinds["tile"][300] == (301 - 64 if c.causal else c.T - 64) and kinds["key0"][0] == (0 if c.causal else c.T - 1)
        if c.layout == "docs":
            n = ref["n_visible"][:, 0]
            assert (n[2] == 1).all() and np.array_equal(n[3], np.arange(1, c.T + 1)) and (n[0, 562:] == 0).all() and n[1, 512] == 1


def test_restated_kernels_stay_inside_the_caps_on_every_input_set(sets):
    """The arithmetic the MFMA kernels are documented to run, in numpy, against the caps check_rows applies on the GPU: worst err / bound below 1
    on every input set, for the general kernel's form and (head_dim padded to 64) the hand-placed kernel's; witnesses within one bf16 step and
    1e-6 of ln n.  The fp32 form gives R32: gpu_util.R32 must be 4 to 8 times the worst err / A measured here."""
    worst, worst32 = {}, 0.0
    for c, x, ref in sets:
        start, _ = c.docs()
        fin = np.isfinite(ref["lse"])
        forms = [("general", False)] + ([("hand", True)] if c.shape in HAND_SHAPES and start is None else [])
        for form, sum_rounded in forms:
            got = R.restate_forward(x["q"], x["k"], x["v"], c.mask(), c.causal, R.LN2, docs=start, sum_rounded=sum_rounded)
            assert np.array_equal(np.isposinf(got["lse"]), ~fin) and np.isfinite(got["o"]).all()
            ro = _ratio(got["o"], ref["o"], attn_o_bound(ref, True, True, c.witness))
            lim = 1e-6 if c.witness else attn_lse_bound(ref, sum_rounded)[fin]
            rl = float((np.abs(got["lse"][fin] - ref["lse"][fin]) / lim).max())
            assert ro < 1.0 and rl < 1.0, (c.name, form, ro, rl)
            key = (form, "witness" if c.witness else "peaked")
            worst[key] = max(worst.get(key, (0.0, 0.0)), (ro, rl))
        got = R.restate_forward(x["q"], x["k"], x["v"], c.mask(), c.causal, R.LN2, docs=start, p_bf16=False, out_bf16=False)
        err, A = np.abs(got["o"] - ref["o"]), ref["A"]
        assert not err[A == 0].any()
        worst32 = max(worst32, float((err[A > 0] / A[A > 0]).max()))
        assert np.abs(got["lse"][fin] - ref["lse"][fin]).max() < 1e-5
    print({k: (round(a, 3), round(b, 3)) for k, (a, b) in worst.items()}, f"worst fp32 err / A {worst32:.3e}, R32 {R32:.3e}")
    assert 4.0 * worst32 <= R32 <= 8.0 * worst32


SENSITIVITY = [  # corruption, the input sets it is tried on
    ("drop_diag", [("g64", "lens", True, "diag"), ("g64", "lens", True, "boundary"), ("g64", "lens", True, "v_pos")]),
    ("drop_last", [("g64", "lens", False, "boundary"), ("g64", "lens", False, "v_pos"), ("g64", "masks", False, "diag")]),
    ("leak_end", [("g64", "lens", False, "v_pos"), ("g64", "lens", True, "v_tile"), ("g64", "lens", False, "diag")]),
    ("key_plus_64", [("g64", "lens", False, "v_tile"), ("g64", "lens", False, "v_pos"), ("g64", "lens", True, "boundary")]),
    ("kv_head", [("g128", "lens", False, "v_pos"), ("h64", "lens", True, "v_tile"), ("g128", "lens", True, "diag")]),
    ("rescale_l", [("g64", "lens", True, "rescale12"), ("g64", "lens", False, "rescale12"), ("g64", "lens", True, "rescale40")]),
]


@pytest.mark.parametrize("corruption,where", SENSITIVITY, ids=[s[0] for s in SENSITIVITY])
def test_row_check_flags_each_corruption(corruption, where):
    """Each defect, planted in the restatement, must fail check_rows on at least one input set; printed beside it: what rel() (one Frobenius
    ratio over all of o, the measure of the older tests, cap 1e-2) makes of the same output."""
    flagged = 0
    for args in where:
        c = R.Case(*args)
        x = R.inputs(c)
        ref = R.reference(c, x, False)
        start, _ = c.docs()
        kw = dict(mask=c.mask(), causal=c.causal, c_s=R.LN2, docs=start)
        clean = R.restate_forward(x["q"], x["k"], x["v"], **kw)
        bad = R.restate_forward(x["q"], x["k"], x["v"], corrupt=(corruption,), **kw)
        parts = lambda g: [("o", g["o"], ref["o"], attn_o_bound(ref, True, True, c.witness)),
                           ("lse", g["lse"], ref["lse"], attn_lse_bound(ref, False, c.witness))]
        check_rows(c.name, parts(clean), record=False)
        off = int((np.abs(bad["o"] - ref["o"]) > attn_o_bound(ref, True, True, c.witness)).sum())
        try:
            check_rows(c.name, parts(bad), record=False)
            verdict = "passes"
        except AssertionError:
            verdict = "FLAGGED"
            flagged += 1
        fin = np.isfinite(ref["lse"])
        print(f"{corruption:12s} {c.name:28s} rows: {verdict}, {off} elements of o off, lse off by {np.abs(bad['lse'] - ref['lse'])[fin].max():.2e}; "
              f"rel(o) {rel(clean['o'], ref['o']):.2e} -> {rel(bad['o'], ref['o']):.2e}")
    assert flagged, corruption
