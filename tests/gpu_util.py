"""Helpers for the -m gpu tests: numpy <-> device tensors, bf16 rounding, model construction."""
import numpy as np
import torch

from p2t_hip import specs, synth


def dev():
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t.to(dtype) if dtype is not None else t


def to_np(t):
    return t.detach().float().cpu().numpy() if t.dtype in (torch.bfloat16, torch.float16) else t.detach().cpu().numpy()


def bf16r(a):
    return synth.bf16_round(np.asarray(a, dtype=np.float32))


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


# ---- elementwise checks of one entry point against fp64 (tests/test_gpu_stage2_ops.py, tests/test_gpu_encoder_ops.py): fp32 outputs
# within rtol * |ref| + atol, a bf16 output within one bf16 rounding step (+ atol); output buffers are larger than the contract writes
# and the rest holds a sentinel that must survive
SENT = -12352.0                                          # exact in bf16 and fp32


def _sentinel(shape, dtype):
    return torch.full(shape, SENT, dtype=dtype, device=dev())


def _kept(t, cols=None, rows=None):
    """The sentinel region: columns >= cols of every row and every row >= rows."""
    a = to_np(t)
    out = []
    if cols is not None:
        out.append(a[:, cols:].ravel())
    if rows is not None:
        out.append(a[rows:].ravel())
    return np.concatenate(out) if out else np.zeros(0)


def _assert_sentinel(t, cols=None, rows=None):
    k = _kept(t, cols, rows)
    assert np.all(k == SENT), f"{int(np.sum(k != SENT))} stray writes"


def _ulp_bf16(ref):
    """One bf16 rounding step at |ref| (8 significant bits)."""
    a = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 1e-38)))
    return np.exp2(e - 7)


def _check(got, ref, dtype, rtol=1e-6, atol=1e-30, what=""):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    err = np.abs(got - ref)
    bound = (_ulp_bf16(ref) + atol) if dtype == torch.bfloat16 else (rtol * np.abs(ref) + atol)
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off, worst {float(err.max()):.3e} at ref {float(ref.ravel()[np.argmax(err)]):.3e}"


def sample_rows(M, tile=256, offsets=(0, 15, 16, 63, 64, 127, 128, 200, 255), extra=7, seed=2024):
    """Rows of an [M, N] GEMM output to check element by element when a host product of the whole is too slow: from every `tile`-row
    tile its first and last row, both sides of each wave's 64-row share (the eight-wave kernels: 128-row) and of the 128-row half, and
    `extra` rows drawn by a seeded generator -> sorted unique int64 array."""
    rows = {t + o for t in range(0, M, tile) for o in offsets if t + o < M}
    rows |= set(np.random.default_rng(seed).integers(0, M, extra).tolist())
    return np.array(sorted(rows), dtype=np.int64)


def _q(a, dtype):
    """The values a tensor of `dtype` holds for a (bf16: rounded), as fp64."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)
    return t.double().numpy()


# ---- attention, row by row (tests/test_gpu_attention_rows.py, tests/test_gpu_generate.py; the terms come from
# encoder_ops_reference.attention_fwd_bwd64(bounds=True), the derivation is in tests/tolerance_changes.md)
U_P = 2.0 ** -7 + 2.0 ** -20                             # each probability rounded to bf16 once (unit roundoff 2^-8) in the numerator and, where the row
                                                         # sums run over the rounded P, once in the denominator; 2^-20: fp32 accumulation over <= 1100 keys
R32 = 2.81e-5                                            # the fp32-softmax kernels: 4 x the worst err / A of attention_reference.restate_forward in fp32
                                                         # against fp64 over the cases (tests/test_attention_reference_host.py re-measures it)


def attn_o_bound(ref, p_bf16, out_bf16, witness=False):
    """|o - ref| per element: one bf16 step at |ref| for a bf16 output, plus U_P * A (P rounded to bf16) or R32 * A (fp32 softmax), A = P |v|.
    witness (q = 0: every visible p is exactly 1): the rounding of the quotient alone -- one bf16 step, fp32: 4e-7 relative."""
    step = _ulp_bf16(ref["o"]) if out_bf16 else 0.0
    if witness:
        return step if out_bf16 else 4e-7 * np.abs(ref["o"])
    return step + (U_P if p_bf16 else R32) * ref["A"]


def attn_lse_bound(ref, sum_rounded, witness=False):
    """|lse - ref| in natural-log units where the row sees a key (+inf, exactly, where it sees none: check_rows)."""
    lse = np.where(np.isfinite(ref["lse"]), ref["lse"], 0.0)
    if witness:
        return np.full(lse.shape, 2e-6)
    return np.full(lse.shape, 2.0 ** -7 + 1e-5) if sum_rounded else 1e-5 + 2e-6 * np.abs(lse)


def attn_grad_bounds(ref, mfma, d):
    """dq, dk, dv (fp32 outputs): the bf16 MFMA kernels round P and dS to bf16, 2^-7 * (the abs-sum term); the exact kernels R32 * (that term);
    both evaluate dO v^T - D in fp32 over 2 d + 2 terms: (2 d + 2) 2^-23 * (the F term; dv does not pass through dS)."""
    c, f = (2.0 ** -7 if mfma else R32), (2 * d + 2) * 2.0 ** -23
    return dict(dq=c * ref["dq_abs"] + f * ref["dq_F"], dk=c * ref["dk_abs"] + f * ref["dk_F"], dv=c * ref["dv_abs"])


def check_rows(name, parts, record=True):
    """Every element of every query row (padded rows included) of each (label, got, ref, bound) against its own bound: |got - ref| <= bound,
    +inf exactly where ref is +inf, finite everywhere else.  The failure names the worst (b, h, row[, column]), the count off and the
    ratio; the worst err / bound over the parts is recorded as `name` (observe, cap 1).  -> that ratio."""
    worst, msgs = 0.0, []
    for label, got, ref, bound in parts:
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
        assert got.shape == ref.shape, (label, got.shape, ref.shape)
        inf = np.isposinf(ref)
        bad = np.where(inf, got != ref, ~np.isfinite(got))
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(inf | bad, 0.0, np.abs(got - ref))
            ratio = np.where(err <= bound, np.where(bound > 0, err / bound, 0.0), np.where(bound > 0, err / bound, np.inf))
        ratio = np.where(bad, np.inf, ratio)
        off = ratio > 1.0
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        worst = max(worst, float(ratio[at]))
        if off.any():
            msgs.append(f"{label}: {int(off.sum())} of {off.size} elements off, worst err / bound {float(ratio[at]):.3g} at (b, h, row[, col]) = "
                        f"{tuple(int(i) for i in at)}: got {got[at]!r}, ref {ref[at]!r}, bound {float(bound[at]):.3e}; "
                        f"{int(off.reshape(off.shape[0], off.shape[1], off.shape[2], -1).any(-1).sum())} rows touched")
    assert not msgs, f"{name}: " + " | ".join(msgs)
    if record:
        observe(name, worst, 1.0, what="ratio")
    return worst


_OBS_PATH = None
_TOL_TABLE = None


def observe(name, value, tol, what="rel"):
    """Assert `value < tolerance` AND append the observed error to gpurun_out/observed_errors.jsonl (merged back from the GPU
    box), so every bf16 / fp8 tolerance in the suite can be audited against what was actually measured.
    The tolerance enforced is the one in tests/tolerances.json when `name` is listed there (tools/update_tolerances.py writes
    it from a previous full run: 2 x the largest observed value, never above the inline `tol`), else the inline `tol`."""
    import json
    import os
    global _OBS_PATH, _TOL_TABLE
    if _TOL_TABLE is None:
        tp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tolerances.json")
        # P2T_TOL_TABLE=0: inline tolerances only -- the run that re-measures after a numerics change, before
        # tools/update_tolerances.py rewrites the table from it
        _TOL_TABLE = json.load(open(tp)) if os.path.exists(tp) and os.environ.get("P2T_TOL_TABLE", "1") != "0" else {}
    inline_tol = float(tol)
    if name in _TOL_TABLE:
        tol = min(inline_tol, float(_TOL_TABLE[name]["tol"]))
    if _OBS_PATH is None:
        root = os.environ.get("GRAFT_REPO_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        d = os.path.join(root, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        _OBS_PATH = os.path.join(d, "observed_errors.jsonl")
    value = float(value)
    with open(_OBS_PATH, "a") as f:
        f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "name": name, "kind": what,
                            "observed": value, "tol": float(tol), "inline_tol": inline_tol}) + "\n")
    assert value < tol, f"{name}: observed {what} error {value:.3e} >= tolerance {tol:.3e}"
    return value


def rnd(seed, name, shape, scale=1.0, offset=0.0):
    return synth.uniform_f32(seed, name, shape, scale, offset)


def adapter_forward_case(X, I, O, M, s1=0.1, s2=0.1, p=0.3, dtype=torch.float32, extra_rows=0):
    """One p2t_adapter_forward with dropout p on seeded inputs, its activations kept for a backward entry point, and the kernel's own
    keep-masks read back from the non-zero entries of h1 / g2 (tests/test_gpu_encoder_lora.py, tests/test_gpu_stage1_tail.py).
    s1 / s2: the weights' scale (the real shape: fan_in^-1/2 as nn.Linear initialises, so that pre-activations stay O(1) and the masks
    can be read back).  y has `extra_rows` rows more than the contract writes; they hold the sentinel.
    -> namespace: cfg / wts / saved (the C structs), p, X / I / O / M, CPU tensors x, w1, b1, w2, b2, dy (the operands as stored: bf16 ones
    widened), m1, m2, device tensors xg, dyg, y, z1, h1, z2, g2, inv."""
    import ctypes as C
    from types import SimpleNamespace
    from p2t_hip import _lib
    from p2t_hip.ops import dt_of, ptr, round_up, stream
    g = torch.Generator().manual_seed(3)
    w1, b1 = torch.randn((I, X), generator=g) * s1, torch.randn(I, generator=g) * 0.1
    w2, b2 = torch.randn((O, I), generator=g) * s2, torch.randn(O, generator=g) * 0.1
    x = torch.randn((M, X), generator=g)
    dy = torch.randn((M, O), generator=g)
    D = lambda t: t.to(dev()).contiguous()
    cfg = _lib.AdapterConfigC(input_dim=X, intermediate_dim=I, output_dim=O, dropout_p=p, dropout_seed=12345, dtype=dt_of(dtype))
    w1p = torch.zeros((I, round_up(X, 64))); w1p[:, :X] = w1
    w2p = torch.zeros((O, round_up(I, 64))); w2p[:, :I] = w2
    w1p, w2p, xg = D(w1p).to(dtype), D(w2p).to(dtype), D(x).to(dtype)
    b1g, b2g, dyg = D(b1), D(b2), D(dy)
    wts = _lib.AdapterWeightsC(fc1_w=w1p.data_ptr(), fc1_b=b1g.data_ptr(), fc2_w=w2p.data_ptr(), fc2_b=b2g.data_ptr())
    ld1, ld2 = round_up(I, 64), round_up(O, 64)
    z1, h1 = torch.empty((M, ld1), dtype=dtype, device=dev()), torch.empty((M, ld1), dtype=dtype, device=dev())
    z2, g2 = torch.empty((M, ld2), dtype=dtype, device=dev()), torch.empty((M, ld2), dtype=dtype, device=dev())
    inv, y = torch.empty((M,), device=dev()), _sentinel((M + extra_rows, ld2), dtype)
    saved = _lib.AdapterSavedC(z1=z1.data_ptr(), h1=h1.data_ptr(), z2=z2.data_ptr(), g2=g2.data_ptr(), inv_norm=inv.data_ptr())
    _lib.call("p2t_adapter_forward", C.byref(cfg), C.byref(wts), ptr(xg), xg.stride(0), M, ptr(y), C.byref(saved), stream())
    m1, m2 = (h1[:, :I] != 0).cpu(), (g2[:, :O] != 0).cpu()                    # the kernel's own keep-masks, read back
    assert 0.5 < float(m1.float().mean()) < 0.9 and 0.5 < float(m2.float().mean()) < 0.9
    return SimpleNamespace(cfg=cfg, wts=wts, saved=saved, p=p, X=X, I=I, O=O, M=M, x=xg.float().cpu(), w1=w1p[:, :X].float().cpu(), b1=b1,
                           w2=w2p[:, :I].float().cpu(), b2=b2, dy=dy, m1=m1, m2=m2, xg=xg, dyg=dyg, y=y, z1=z1, h1=h1, z2=z2, g2=g2, inv=inv,
                           _keep=(w1p, w2p, b1g, b2g))


def build_model(esm, llama, ad, dtype, seed=0, adapter_dtype=None):
    from p2t_hip import Esm2LlamaInstructForCausalLM
    return Esm2LlamaInstructForCausalLM.from_specs(esm, llama, ad, dtype=dtype, device=dev(), seed=seed,
                                                   adapter_dtype=adapter_dtype)
