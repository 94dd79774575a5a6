"""The four-wave forms of the bf16 GEMM (csrc/gemm_w4.hip: GEMM_W4_TILE, GEMM_W4_PERSIST with and without in-stream split-K pairs,
GEMM_W4_PAIRS), every epilogue each is built for, element by element against fp64 -- and the same cases on the eight-wave forms
(policy 9: GEMM_PERSIST, GEMM_TILE256 / 128, GEMM_SPLITK), so a failure says which family is wrong.

The cases (tests/gemm_forms_cases.py) are the smallest shapes that plan to each form; tests/test_gemm_plan.py asserts those plans
without a GPU.  A host product of the whole output is too slow, so the fp64 check runs on sampled rows and every column
(gpu_util.sample_rows: per 256-row tile the first / last row, both sides of each wave's share and of the 128-row half, plus 7 seeded
rows; the same sample under both policies), on the bf16 operands as the device holds them; the rows in between are covered by
comparing the two policies' whole outputs on the device -- bit for bit wherever both plans split K the same way, which is every case of
the table today (gemm_forms_cases.k_split_tiles).

Bound per element (gpu_util._check): fp32 outputs rtol 1e-6 * |ref| + atol, bf16 outputs one bf16 step at |ref| + atol.  atol covers
the fp32 accumulation of K products (and, for GELU / SwiGLU / rotary, the fp32 evaluation of the activation near zero, where a bf16
step is smaller than that): 4 x the worst error in excess of the rounding term that the eight-wave kernels (policy 9) and the FMA kernel
showed against fp64, per epilogue and K -- OBSERVED below and tests/tolerance_changes.md (the four-wave forms observed the same excess,
and both policies' whole outputs were bit-identical in every case, split K included).  The kernels are deterministic, so where no
element exceeded its rounding term the bound is the rounding term alone.

The second half passes what no other GPU test passes to p2t_gemm_nt / p2t_gemm_qkv_rope: strided operands with NaN behind column K,
outputs wider and longer than the contract writes (sentinel-filled), accumulate with EPI_STORE_F32 / EPI_STORE, EPI_RESID without a
bias -- at a whole-round shape, a three-quarter-round shape and a shape with edge tiles."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import p2t_oracle as O
from gemm_forms_cases import BF16, CASES, EPILOGUES, case_id, k_split_tiles
from gpu_util import SENT, _assert_sentinel, _check, _sentinel, _ulp_bf16, dev, observe, rel, sample_rows, to_np
from helpers import EPI_STORE_F32, gemm_epilogue_ref, pack_d128, qkv_rope_ref
from test_gpu_kernels import _no_timeout, gemm_policy, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

RTOL = 1e-6            # fp32 outputs: a handful of fp32 roundings of the result

# OBSERVED[epilogue][K]: the worst |got - ref64| in excess of the rounding term under policy 9 (eight-wave forms) and, for EPI_STORE_F32,
# the FMA kernel, over every test of this file that runs the pair; 0 = no element exceeded its rounding term.  atol = 4 x that.
OBSERVED = {
    "store_bf16": {256: 1.5e-8, 320: 0.0, 384: 3.9e-8, 512: 2.2e-7, 6144: 1.0e-6, 8192: 4.2e-7},
    "store_f32": {256: 9.1e-7, 320: 3.4e-7, 384: 8.7e-7, 512: 7.0e-7, 8192: 3.8e-6},
    "resid": {256: 5.6e-7, 320: 5.0e-7, 384: 7.9e-7, 512: 8.8e-7, 6144: 7.0e-6, 8192: 4.0e-6},
    "gelu": {256: 7.6e-8, 320: 6.5e-8, 384: 8.1e-8, 512: 8.1e-8, 6144: 5.0e-7},
    "swiglu": {256: 9.2e-9, 320: 0.0, 384: 4.2e-8, 512: 5.0e-8},
    "qkv_d64": {256: 4.8e-9, 320: 0.0, 384: 3.0e-7, 512: 2.2e-7},
    "qkv_d128": {256: 1.1e-7, 320: 0.0, 384: 1.9e-7, 512: 2.2e-7},
}


def _atol(epi, K):
    epi = {"gelu_z": "gelu", "f32": "store_f32"}.get(epi, epi.split("_s")[0])
    return 4 * OBSERVED[epi][K]


def _figure(what, **figures):
    """One line per measurement, printed before anything asserts: what OBSERVED and tests/tolerance_changes.md are written from."""
    print(f"gemm_forms figure: {what} " + " ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


@pytest.fixture(scope="module")
def fix():
    """One zeroed split-K fix-up workspace for the module and a launch counter for its epochs."""
    from p2t_hip import ops as P
    return SimpleNamespace(ws=P.gemm_fix_workspace(dev()), epoch=0)


@functools.lru_cache(maxsize=2)
def _operands(M, N, K):
    """Seeded operands of one shape, generated on the device; the sampled rows of A, all of W and the fp64 product of the two on
    the host (shared by every case of the shape and left unchanged).  Weights scaled so that the product is O(1) at every K."""
    from p2t_hip import ops as P
    a = torch.empty((M, K), dtype=torch.bfloat16, device=dev())
    w = torch.empty((N, K), dtype=torch.bfloat16, device=dev())
    bias = torch.empty((N,), dtype=torch.float32, device=dev())
    resid = torch.empty((M, N), dtype=torch.float32, device=dev())
    P.fill_hash_(a, 7, f"gf.a{M}x{K}", 1.0)
    P.fill_hash_(w, 7, f"gf.w{N}x{K}", 4.5 / math.sqrt(K))
    P.fill_hash_(bias, 7, f"gf.b{N}", 0.3)
    P.fill_hash_(resid, 7, f"gf.r{M}x{N}", 1.0)
    rows = sample_rows(M)
    rows_d = torch.from_numpy(rows).to(dev())
    acc = a[rows_d].double().cpu().numpy() @ w.double().cpu().numpy().T
    return SimpleNamespace(M=M, N=N, K=K, a=a, w=w, bias=bias, resid=resid, rows=rows, rows_d=rows_d, acc=acc,
                           bias64=bias.double().cpu().numpy(), resid64=resid[rows_d].double().cpu().numpy())


def _inv_freq(d):
    return O.default_inv_freq(10000.0, d) if d == 64 else O.llama3_inv_freq(500000.0, d, 8.0, 1.0, 4.0, 64)


def _q_scale(d):
    return 64 ** -0.5 if d == 64 else 1.0


def _natural(cols, d, nh, nkv):
    """Columns of a head_dim-128 product in the packed weight-row order of include/p2t_hip.h -> natural channel order (pack_d128 is its
    own inverse); head_dim 64 is stored in natural order."""
    if d == 64:
        return cols
    cut = (0, nh * d, (nh + nkv) * d, (nh + 2 * nkv) * d)
    return np.concatenate([pack_d128(np.ascontiguousarray(cols[..., s:e].T), h).T for s, e, h in zip(cut, cut[1:], (nh, nkv, nkv))], axis=-1)


def _reference(o, epi, qkv=None, bias=True):
    """fp64 reference on the sampled rows -> {output name: array}."""
    b = o.bias64 if bias else None
    if qkv is not None:
        d, nh, nkv, seq = qkv
        acc = _natural(o.acc + b, d, nh, nkv)
        q, k, v = qkv_rope_ref(acc, o.rows % seq, nh, nkv, d, _q_scale(d), _inv_freq(d))
        return {"q": q, "k": k, "v": v}
    ref = {"out": gemm_epilogue_ref(o.acc, None if epi == "swiglu" else b, EPILOGUES[epi][0], o.resid64)}
    if epi == "gelu_z":
        ref["z"] = o.acc + b
    return ref


def _launch(P, fix, o, epi, qkv=None, *, a=None, w=None, bias=True, out=None, z=None, accumulate=False, qkv_out=(None, None, None)):
    """One GEMM on the MFMA kernels with the fix-up workspace -> {output name: device tensor}."""
    a, w = o.a if a is None else a, o.w if w is None else w
    fix.epoch += 1
    if qkv is not None:
        d, nh, nkv, seq = qkv
        q, k, v = P.gemm_qkv_rope(a, w, o.bias, torch.from_numpy(_inv_freq(d)).to(dev()), seq, nh, nkv, d, _q_scale(d), k=o.K, use_mfma=1,
                                  fix_ws=fix.ws, fix_epoch=fix.epoch, q=qkv_out[0], kk=qkv_out[1], v=qkv_out[2])
        return {"q": q, "k": k, "v": v}
    if epi == "resid" and out is None:
        out = o.resid.clone()
    got = P.gemm_nt(a, w, o.bias if bias and epi != "swiglu" else None, k=o.K, epilogue=EPILOGUES[epi][0], out=out, z=z, accumulate=accumulate,
                    out_dtype=torch.float32 if epi == "store_f32" else torch.bfloat16, use_mfma=1, fix_ws=fix.ws, fix_epoch=fix.epoch)
    return {"out": got} if z is None else {"out": got, "z": z}


def _sampled(o, got, qkv=None):
    """The sampled rows of the outputs, as numpy, in the layout of _reference."""
    if qkv is None:
        return {k: to_np(t[o.rows_d]) for k, t in got.items()}
    seq = qkv[3]
    b, t = o.rows_d // seq, o.rows_d % seq
    return {k: to_np(x[b, :, t, :]) for k, x in got.items()}


def _excess(got, ref, dtype):
    """The worst error beyond the rounding term of _check: what atol has to cover."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float(np.max(err - (_ulp_bf16(ref) if dtype == torch.bfloat16 else RTOL * np.abs(ref))))


def _check_sampled(o, got, ref, atol, what, qkv=None, scale=1.0, fails=None):
    """Every sampled element inside its bound (the figures are printed before anything asserts) -> relative L2 of the whole sample."""
    s = _sampled(o, got, qkv)
    l2 = rel(np.concatenate([s[k][..., :ref[k].shape[-1]].ravel() for k in ref]), np.concatenate([ref[k].ravel() * scale for k in ref]))
    _figure(f"{what} {o.M}x{o.N}x{o.K}", excess=max(_excess(s[k][..., :r.shape[-1]], r * scale, got[k].dtype) for k, r in ref.items()),
            atol=atol, rel_l2=l2)
    for k, r in ref.items():
        r = r * scale
        n = r.shape[-1]
        g = s[k][..., :n]
        try:
            _check(g, r, got[k].dtype, rtol=RTOL, atol=atol, what=f"{what}.{k}")
        except AssertionError as e:
            if fails is None:
                raise
            fails.append(str(e))
    return l2


def _device_step_bf16(a, b):
    """One bf16 step at max(|a|, |b|), on the device."""
    m = torch.maximum(a.abs(), b.abs()).float().clamp_min(1e-38)
    return torch.exp2(torch.floor(torch.log2(m)) - 7)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_gemm_form_vs_fp64(ops, gemm_policy, fix, c):
    o = _operands(c.M, c.N, c.K)
    ref = _reference(o, c.epi, c.qkv)
    atol = _atol(c.epi, c.K)
    fails, outs = [], {}
    for pol, plan in ((9, c.p9), (0, c.p0)):
        gemm_policy(pol)
        outs[pol] = _launch(ops, fix, o, c.epi, c.qkv)
        l2 = _check_sampled(o, outs[pol], ref, atol, f"{c.epi} policy {pol} ({plan[0]})", c.qkv, fails=fails)
        try:
            observe(f"gemm_forms[{plan[0]},{c.epi},{c.M}x{c.N}x{c.K}]", l2, 2.5e-3 if c.out == BF16 else 3e-6)
        except AssertionError as e:
            fails.append(str(e))
    # the rows in between: the two policies against each other, whole outputs, per element.  Every case of the table today splits K the
    # same way under both plans, so the bounded branch is unused
    same_split = k_split_tiles(c.p0) == k_split_tiles(c.p9)
    for k in outs[0]:
        x, y = outs[0][k], outs[9][k]
        if same_split:
            ok = torch.equal(x, y)
        else:
            bound = _device_step_bf16(x, y) if x.dtype == torch.bfloat16 else 2 * atol
            ok = bool(((x.float() - y.float()).abs() <= bound).all())
        _figure(f"{case_id(c)} {k} policy 0 vs 9", check="equal" if same_split else "bounded", ok=ok, differing=int((x != y).sum()),
                max=float((x.float() - y.float()).abs().max()))
        if not ok:
            fails.append(f"{k}: the default policy ({c.p0[0]}) and policy 9 ({c.p9[0]}) differ " +
                         ("though they split K the same way" if same_split else "by more than one bf16 step / 2 atol"))
    assert _no_timeout()
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------
# Arguments no other GPU test passes.  Whole round (w4_persist / persist), three quarters of a round (w4_tile / tile256 where the
# epilogue has the form), and edge tiles in M and N (eight-wave per-tile kernel under both policies).
ARG_SHAPES = [(4096, 4096, 384), (2048, 6144, 256), (300, 320, 320)]
ARG_QKV = {(4096, 64): (32, 16, 512), (4096, 128): (16, 8, 512), (2048, 64): (32, 32, 512), (2048, 128): (32, 8, 512),
           (300, 64): (3, 1, 150), (300, 128): (1, 1, 150)}           # M, head_dim -> nh, nkv, seq


def _arg_case(shape, epi):
    """-> operands, qkv config: head_dim 128 needs N % 128 == 0, so at the edge shape it runs 300 x 384 x 320."""
    M, N, K = shape
    if not epi.startswith("qkv"):
        return _operands(M, N, K), None
    d = int(epi[5:])
    nh, nkv, seq = ARG_QKV[(M, d)]
    return _operands(M, (nh + 2 * nkv) * d, K), (d, nh, nkv, seq)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else v


@pytest.mark.parametrize("epi", ["store_bf16", "resid", "gelu", "swiglu", "qkv_d64", "qkv_d128"])
@pytest.mark.parametrize("shape", ARG_SHAPES, ids=_ids)
def test_strided_operands(ops, gemm_policy, fix, shape, epi):
    """lda = K + 64, ldw = K + 128 with NaN behind column K of both: a loader that reads past K poisons the output.  Against fp64 on the
    sampled rows, and bit for bit against the packed operands everywhere."""
    o, qkv = _arg_case(shape, epi)
    ab = torch.full((o.M, o.K + 64), float("nan"), dtype=torch.bfloat16, device=dev())
    wb = torch.full((o.N, o.K + 128), float("nan"), dtype=torch.bfloat16, device=dev())
    ab[:, :o.K] = o.a
    wb[:, :o.K] = o.w
    av, wv = ab[:, :o.K], wb[:, :o.K]
    assert av.stride(0) == o.K + 64 and wv.stride(0) == o.K + 128
    ref = _reference(o, epi, qkv)
    for pol in (9, 0):
        gemm_policy(pol)
        got = _launch(ops, fix, o, epi, qkv, a=av, w=wv)
        _check_sampled(o, got, ref, _atol(epi, o.K), f"strided {epi} policy {pol}", qkv)
        packed = _launch(ops, fix, o, epi, qkv)
        for k in got:
            assert torch.equal(got[k], packed[k]), f"{k}: strided and packed operands differ under policy {pol}"
    assert _no_timeout()


@pytest.mark.parametrize("epi", ["store_bf16", "store_f32", "resid", "gelu", "gelu_z", "swiglu", "qkv_d64", "qkv_d128"])
@pytest.mark.parametrize("shape", ARG_SHAPES, ids=_ids)
def test_wide_output_and_stray_writes(ops, gemm_policy, fix, shape, epi):
    """out (and z) two rows longer and 64 columns wider than the zero padding, q / k / v one head longer, all sentinel-filled: columns below
    n_out match fp64, n_out .. round_up(n_out, 64) are zero, everything else still holds the sentinel.  gelu_z (the pre-activation copy)
    routes to EpiGelu<..., true>, which has no four-wave form: its result is asserted, not its form.  N of the two large shapes is a
    multiple of 64, so there the zero padding is empty and the sentinel starts at column n_out; only SwiGLU at the edge shape (n_out 160
    -> 192) has padding to check, on the eight-wave per-tile kernel."""
    o, qkv = _arg_case(shape, epi)
    ref = _reference(o, epi, qkv)
    for pol in (9, 0):
        gemm_policy(pol)
        what = f"wide {epi} policy {pol}"
        if qkv is not None:
            d, nh, nkv, seq = qkv
            B = o.M // seq
            bufs = [_sentinel((B * h * seq * d + seq * d,), torch.bfloat16) for h in (nh, nkv, nkv)]
            views = [b[:B * h * seq * d].view(B, h, seq, d) for b, h in zip(bufs, (nh, nkv, nkv))]
            got = _launch(ops, fix, o, epi, qkv, qkv_out=views)
            _check_sampled(o, got, ref, _atol(epi, o.K), what, qkv)
            for b, h in zip(bufs, (nh, nkv, nkv)):
                _assert_sentinel(b[None, :], cols=B * h * seq * d)
            packed = _launch(ops, fix, o, epi, qkv)
        else:
            n_out = o.N // 2 if epi == "swiglu" else o.N
            n_zero = ops.round_up(n_out, 64)
            dt = torch.float32 if epi in ("store_f32", "resid") else torch.bfloat16
            out = _sentinel((o.M + 2, n_zero + 64), dt)
            if epi == "resid":
                out[:o.M, :o.N] = o.resid
            z = _sentinel((o.M + 2, n_zero + 64), dt) if epi == "gelu_z" else None
            got = _launch(ops, fix, o, epi, out=out, z=z)
            _check_sampled(o, got, ref, _atol(epi, o.K), what)
            for k, t in got.items():
                if epi != "resid":                                  # the residual stream has no zero padding
                    assert not t[:o.M, n_out:n_zero].any(), f"{what}.{k}: the zero padding is not zero"
                _assert_sentinel(t, cols=n_out if epi == "resid" else n_zero, rows=o.M)
            packed = _launch(ops, fix, o, epi, z=torch.empty((o.M, n_zero), dtype=dt, device=dev()) if epi == "gelu_z" else None)
            got = {k: t[:o.M, :n_out] for k, t in got.items()}
            packed = {k: t[:, :n_out] for k, t in packed.items()}
        for k in got:
            assert torch.equal(got[k], packed[k]), f"{what}.{k}: a wider ldc changes values"
    assert _no_timeout()


@pytest.mark.parametrize("shape", ARG_SHAPES, ids=_ids)
def test_accumulate_and_null_bias(ops, gemm_policy, fix, shape):
    """EPI_STORE_F32 twice into one buffer (accumulate = 0, then 1) = 2 x the product, with bf16 operands (MFMA kernels) and the same values
    as fp32 operands (FMA kernel); EPI_RESID without a bias onto a non-trivial stream; EPI_STORE ignores accumulate."""
    o = _operands(*shape)
    atol = _atol("f32", o.K)
    ref = {"out": o.acc}
    a32, w32 = o.a.float(), o.w.float()
    for pol in (9, 0):
        gemm_policy(pol)
        for what, kw in ((f"bf16 operands, policy {pol}", {}), ("fp32 operands", dict(a=a32, w=w32))):
            if kw and pol == 0:
                continue                                            # the FMA kernel has no launch policy
            out = _sentinel((o.M, o.N), torch.float32)
            for acc, scale in ((False, 1.0), (True, 2.0)):
                fix.epoch += 1
                got = ops.gemm_nt(kw.get("a", o.a), kw.get("w", o.w), None, epilogue=EPI_STORE_F32, out=out, accumulate=acc,
                                  use_mfma=0 if kw else 1, fix_ws=fix.ws, fix_epoch=fix.epoch)
                _check_sampled(o, {"out": got}, ref, scale * atol, f"STORE_F32 x {scale:g}, {what}", scale=scale)
        got = _launch(ops, fix, o, "resid", bias=False)
        _check_sampled(o, got, _reference(o, "resid", bias=False), _atol("resid", o.K), f"RESID without bias, policy {pol}")
        for epi in ("store_bf16", "store_f32"):
            plain, accd = _launch(ops, fix, o, epi), _launch(ops, fix, o, epi, accumulate=True, out=_sentinel(
                (o.M, o.N), torch.float32 if epi == "store_f32" else torch.bfloat16))
            assert torch.equal(plain["out"], accd["out"]), f"EPI_STORE ({epi}) changed under accumulate = 1, policy {pol}"
    assert _no_timeout()
