"""The three kernels of the target-rows form in csrc/lm_loss.hip (the LM loss over the target rows only), one by one against fp64 numpy computed here on the
stored (rounded) inputs: the selection exactly, the row kernel's loss to 1e-5 relative and its in-place gradient to 2^-22 max|ref|
(f32 storage) / half a bf16 step of the reference + 2^-22 max|ref| (bf16 storage), the reduction, and bit-identical repeats."""
import numpy as np
import pytest
import torch

from gpu_util import dev, to_dev, to_np
from p2t_hip import _lib, ops
from p2t_hip.ops import ptr, stream

pytestmark = pytest.mark.gpu
SENT = -7


# ---------------------------------------------------------------------------------------------
# selection
def _labels(B, T, V, seed, frac_ignored=0.4):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, V, size=(B, T)).astype(np.int64)
    lab[rng.random((B, T)) < frac_ignored] = -100
    lab[0, 1], lab[0, 2], lab[B - 1, 3] = V, -5, V + 7            # out of range: not counted
    lab[:, 0] = 3                                                 # a counted value at t = 0 is never a target
    lab[:, T - 1] = V - 1                                         # ... at t = T - 1 it is the target of row T - 2
    return lab


def _want_rows(lab, V):
    B, T = lab.shape
    tgt = np.full((B, T), -1, dtype=np.int64)
    nxt = lab[:, 1:]
    tgt[:, :-1] = np.where((nxt != -100) & (nxt >= 0) & (nxt < V), nxt, -1)
    flat = tgt.reshape(-1)
    rows = np.flatnonzero(flat >= 0)
    return rows.astype(np.int32), flat[rows].astype(np.int32)


def _select_raw(lab, V, cap, size):
    """The entry point on buffers with a guard band of `SENT` on both sides of every output."""
    G = 8
    mk = lambda n: torch.full((n + 2 * G,), SENT, dtype=torch.int32, device=dev())
    rows, targets, count = mk(size), mk(size), mk(2)
    ld = to_dev(lab)
    B, T = lab.shape
    off = lambda t: ops.C.c_void_p(t.data_ptr() + 4 * G)
    _lib.call("p2t_lm_target_rows", ptr(ld), B, T, V, -100, cap, off(rows), off(targets), off(count), stream())
    outs = []
    for t, n in ((rows, size), (targets, size), (count, 2)):
        a = to_np(t)
        assert np.all(a[:G] == SENT) and np.all(a[G + n:] == SENT), "write outside the output"
        outs.append(a[G:G + n])
    return outs


@pytest.mark.parametrize("B,T", [(3, 7), (2, 130)])
def test_target_rows_exact(B, T):
    V = 50
    lab = _labels(B, T, V, seed=B * 100 + T)
    want_rows, want_tgt = _want_rows(lab, V)
    n = len(want_rows)
    assert n > 4 and (T - 2) in want_rows % T and not np.any(want_rows % T == T - 1)
    # capacity above the count: all listed, tail -1
    cap = n + 5
    rows, targets, count = _select_raw(lab, V, cap, cap)
    assert count.tolist() == [n, 0]
    assert np.array_equal(rows[:n], want_rows) and np.array_equal(targets[:n], want_tgt)
    assert np.all(rows[n:] == -1) and np.all(targets[n:] == -1)
    # capacity exactly the count
    rows, targets, count = _select_raw(lab, V, n, n)
    assert count.tolist() == [n, 0] and np.array_equal(rows, want_rows) and np.array_equal(targets, want_tgt)
    # capacity below the count: the flag, the first cap rows, nothing beyond cap touched
    cap = n - 3
    rows, targets, count = _select_raw(lab, V, cap, n)
    assert count.tolist() == [n, 1]
    assert np.array_equal(rows[:cap], want_rows[:cap]) and np.array_equal(targets[:cap], want_tgt[:cap])
    assert np.all(rows[cap:] == SENT) and np.all(targets[cap:] == SENT)
    # nothing counted
    none = np.full((B, T), -100, dtype=np.int64)
    rows, targets, count = _select_raw(none, V, 6, 6)
    assert count.tolist() == [0, 0] and np.all(rows == -1) and np.all(targets == -1)
    # the binding: buffers longer than the capacity come back with a -1 tail
    r2, t2, c2 = ops.lm_target_rows(to_dev(lab), V, n - 3, size=n + 100)
    assert r2.numel() == t2.numel() == n + 100
    assert to_np(c2).tolist() == [n, 1] and np.array_equal(to_np(r2)[:n - 3], want_rows[:n - 3]) and np.all(to_np(r2)[n - 3:] == -1)
    assert np.all(to_np(t2)[n - 3:] == -1)


# ---------------------------------------------------------------------------------------------
# row kernel
def _ulp_bf16(ref):
    a = np.abs(ref)
    return np.exp2(np.floor(np.log2(np.maximum(a, 1e-300))) - 7)


def _row_case(R, V, dtype, weighted, seed):
    """R logits rows; the list holds R + 2 entries of which n = R - 1 are counted: entry 1 has target -1 (a hole in the list) and the
    last chunk row lies beyond the count."""
    rng = np.random.default_rng(seed)
    ld = ops.round_up(V, 64)
    x = (rng.standard_normal((R, ld)) * 3.0).astype(np.float32)
    x[0, :V] = rng.uniform(-60.0, 60.0, V).astype(np.float32)      # a spread of +-60: exp() overflows without the max subtraction
    x[:, V:] = np.nan                                              # pad columns: whatever they hold, they come out 0
    cap = R + 2
    n = R - 1
    M = 64                                                         # flat rows of the imaginary [B, T] batch the weights belong to
    rows = np.full(cap, -1, dtype=np.int32)
    rows[:n] = np.sort(rng.choice(M - 1, n, replace=False)).astype(np.int32)
    targets = np.full(cap, -1, dtype=np.int32)
    targets[:n] = rng.integers(0, V, n)
    if n > 2:
        targets[2] = V - 1                                         # the last real column
    targets[1] = -1
    w = rng.uniform(0.01, 0.2, M).astype(np.float32) if weighted else None
    xt = to_dev(x, dtype)
    xs = xt.double().cpu().numpy()[:, :V]                          # the stored values
    m = xs.max(1, keepdims=True)
    lse = np.log(np.exp(xs - m).sum(1)) + m[:, 0]
    p = np.exp(xs - lse[:, None])
    want_g = np.zeros((R, ld))
    want_l = np.zeros(cap)
    for r in range(R):
        if r < n and targets[r] >= 0:
            s = float(w[rows[r] + 1]) if weighted else 1.0 / n
            g = p[r].copy()
            g[targets[r]] -= 1.0
            want_g[r, :V] = g * s
            want_l[r] = lse[r] - xs[r, targets[r]]
    count = np.array([n, 0], dtype=np.int32)
    return xt, rows, targets, count, w, want_g, want_l, n, cap


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,V", [(5, 300), (5, 1000), (3, 128256)])
def test_loss_grad_rows_vs_fp64(R, V, dtype, weighted):
    xt, rows, targets, count, w, want_g, want_l, n, cap = _row_case(R, V, dtype, weighted, seed=V + R)
    rd, td, cd = to_dev(rows), to_dev(targets), to_dev(count)
    wd = to_dev(w) if weighted else None
    x0 = xt.clone()
    # loss only: the logits stay as they are
    rl0 = torch.full((cap,), 5.0, dtype=torch.float32, device=dev())
    ops.lm_loss_grad_rows(xt, V, rd, td, cd, rl0, weights=wd, with_grad=False)
    assert torch.equal(xt.view(torch.int32 if dtype == torch.float32 else torch.int16), x0.view(torch.int32 if dtype == torch.float32 else torch.int16))
    outs = []
    for _ in range(2):
        buf = x0.clone()
        rl = torch.full((cap,), 5.0, dtype=torch.float32, device=dev())
        ops.lm_loss_grad_rows(buf, V, rd, td, cd, rl, weights=wd)
        outs.append((buf, rl))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "repeats differ"
    assert torch.equal(outs[0][1], rl0), "the loss depends on with_grad"
    got_g, got_l = outs[0][0].double().cpu().numpy(), to_np(outs[0][1]).astype(np.float64)
    assert np.all(np.isfinite(got_g))
    assert not got_g[:, V:].any(), "pad columns must be 0"
    assert not got_g[1].any() and not got_g[n:].any(), "rows without a target / beyond the count must be 0"
    assert np.all(got_l[R:] == 5.0), "row_loss beyond the chunk was written"
    assert got_l[1] == 0.0 and np.all(got_l[n:R] == 0.0)
    live = [r for r in range(R) if r < n and targets[r] >= 0]
    err_l = np.abs(got_l[live] - want_l[live]) / np.abs(want_l[live])
    top = np.abs(want_g).max()
    err_g = np.abs(got_g - want_g)
    bound = 2.0 ** -22 * top + (0.5 * _ulp_bf16(want_g) if dtype == torch.bfloat16 else 0.0)
    print(f"V={V} {dtype} weighted={weighted}: row_loss rel err {err_l.max():.2e}; gradient max err {err_g.max():.2e} (max|ref| {top:.2e}, "
          f"worst err / bound {np.max(err_g / bound):.2f})")
    assert err_l.max() < 1e-5
    assert np.all(err_g <= bound)


def test_loss_grad_rows_chunk_offset():
    """`first`: a chunk in the middle of the list reads its own entries and writes its own row_loss slots."""
    V, R = 300, 4
    xt, rows, targets, count, _, want_g, want_l, n, cap = _row_case(R, V, torch.float32, False, seed=9)
    first = 128
    pad = lambda a: np.concatenate([np.full(first, -1, dtype=np.int32), a])
    rows2, targets2 = pad(rows), pad(targets)
    rows2[:first], targets2[:first] = np.arange(first), 0
    count2 = np.array([first + n, 0], dtype=np.int32)
    rl = torch.full((first + cap,), 5.0, dtype=torch.float32, device=dev())
    ops.lm_loss_grad_rows(xt, V, to_dev(rows2), to_dev(targets2), to_dev(count2), rl, first=first)
    got_l = to_np(rl)
    assert np.all(got_l[:first] == 5.0) and np.all(got_l[first + R:] == 5.0)
    scale = n / (first + n)                                        # the token mean now counts first + n targets
    assert np.max(np.abs(to_np(xt).astype(np.float64) - want_g * scale)) <= 2.0 ** -22 * np.abs(want_g * scale).max()
    assert np.allclose(got_l[first:first + R], want_l[:R], rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------
# reduce
def test_reduce():
    rng = np.random.default_rng(4)
    cap, n, M = 384, 300, 1000
    rl = rng.uniform(0.0, 9.0, cap).astype(np.float32)
    rows = np.full(cap, -1, dtype=np.int32)
    rows[:n] = np.sort(rng.choice(M - 1, n, replace=False))
    w = rng.uniform(0.0, 0.1, M).astype(np.float32)
    rld, rd, wd = to_dev(rl), to_dev(rows), to_dev(w)
    cnt = lambda a, b: to_dev(np.array([a, b], dtype=np.int32))
    mean = float(ops.lm_loss_reduce(rld, rd, cnt(n, 0))[0])
    assert abs(mean - rl[:n].astype(np.float64).mean()) < 1e-6 * mean
    ws = float(ops.lm_loss_reduce(rld, rd, cnt(n, 0), weights=wd)[0])
    want = float((w[rows[:n] + 1].astype(np.float64) * rl[:n]).sum())
    assert abs(ws - want) < 1e-6 * want
    again = ops.lm_loss_reduce(rld, rd, cnt(n, 0), weights=wd)
    assert float(again[0]) == ws
    assert np.isnan(float(ops.lm_loss_reduce(rld, rd, cnt(0, 0))[0]))                    # no target: the mean over nothing
    assert np.isnan(float(ops.lm_loss_reduce(rld, rd, cnt(cap + 9, 1))[0]))              # overflow
    assert np.isnan(float(ops.lm_loss_reduce(rld, rd, cnt(cap + 9, 1), weights=wd)[0]))
