"""p2t_lora_wgrad (csrc/lora_wgrad.hip) on its own: G[c, j] = sum_m X'[m, c] U[m, j] against the fp64 product of the values the inputs
hold (bf16 inputs rounded first), both dtypes, both store orientations.

The bound is the fp32 summation bound, which holds for ANY order of the sum (so for every split of the token axis):
    |G - ref| <= M 2^-24 sum_m |X'[m, c] U[m, j]| + the smallest fp32 normal
(products of two bf16 values are exact in fp32; an fp32 product adds one rounding, inside the same bound).  The padding columns of X
and U hold NaN -- the kernel must not read them into a sum -- and G lies in a larger buffer of sentinels that must survive.
Shapes: token counts around the 64-token tile (1, 63, 64, 65), several tiles and several splits (200, 4 864), column counts below / not
a multiple of / many times the 128-column block (8, 24, 136, 4 096), ranks 4 / 16 / 64 (one and two 32-column MFMA blocks)."""
import numpy as np
import pytest
import torch

from gpu_util import SENT, _assert_sentinel, _q, _sentinel, dev
from p2t_hip import _lib, ops
from p2t_hip.ops import ptr, stream

pytestmark = pytest.mark.gpu
LD_U = 64
TINY = float(np.finfo(np.float32).tiny)
SHAPES = [(1, 8, 4), (63, 24, 16), (64, 136, 64), (65, 136, 4), (200, 8, 16), (200, 136, 64), (65, 4096, 64), (4864, 24, 4), (4864, 4096, 16)]
_CACHE = {}


def _inputs(M, C, R, dtype):
    """X [M, C + 8], U [M, 64] on the device (NaN outside [:, :C] / [:, :R]) and their fp64 values [M, C], [M, R] -- built once per shape."""
    key = (M, C, R, dtype)
    if key not in _CACHE:
        rs = np.random.RandomState(M * 7 + C * 3 + R)
        xv, uv = _q(rs.standard_normal((M, C)), dtype), _q(rs.standard_normal((M, R)), dtype)
        x = torch.full((M, C + 8), float("nan"), dtype=dtype, device=dev())
        u = torch.full((M, LD_U), float("nan"), dtype=dtype, device=dev())
        x[:, :C] = torch.from_numpy(xv).to(dev()).to(dtype)
        u[:, :R] = torch.from_numpy(uv).to(dev()).to(dtype)
        _CACHE.clear()                                  # one shape's tensors at a time
        _CACHE[key] = (x, u)
    return _CACHE[key]


def _reference(x, u, C, R):
    """fp64 on the device: (the product [C, R], the sum of the absolute products [C, R])."""
    xd, ud = x[:, :C].double(), u[:, :R].double()
    return (xd.T @ ud).cpu().numpy(), (xd.abs().T @ ud.abs()).cpu().numpy()


def _run(x, u, C, R, transposed, p=0.0, seed=0):
    buf = _sentinel((R + 2, C + 3) if transposed else (C + 2, R + 3), torch.float32)
    ops.lora_wgrad(x, u, c=C, r=R, transposed=transposed, p=p, seed=seed, out=buf)
    torch.cuda.synchronize()
    if transposed:
        _assert_sentinel(buf, cols=C, rows=R)
        return buf[:R, :C].T.contiguous().cpu().numpy(), buf
    _assert_sentinel(buf, cols=R, rows=C)
    return buf[:C, :R].cpu().numpy(), buf


def _assert_within_summation_bound(got, ref, mag, M, what):
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    err, bound = np.abs(got.astype(np.float64) - ref), M * 2.0 ** -24 * mag + TINY
    worst = float(np.max(err / bound))
    print(f"{what}: worst error / bound {worst:.3f}, max abs error {float(err.max()):.3e}")
    assert worst <= 1.0, f"{what}: {int((err > bound).sum())} elements past the fp32 summation bound, worst ratio {worst:.3f}"


@pytest.mark.parametrize("transposed", [False, True], ids=["c_major", "r_major"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,C,R", SHAPES)
def test_token_axis_product_within_the_fp32_summation_bound(M, C, R, dtype, transposed):
    x, u = _inputs(M, C, R, dtype)
    ref, mag = _reference(x, u, C, R)
    got, _ = _run(x, u, C, R, transposed)
    _assert_within_summation_bound(got, ref, mag, M, f"M {M} C {C} R {R}")


def test_the_token_axis_is_split_where_columns_alone_would_not_fill_the_device():
    """Read off the sizing function (f32 [splits, C, R]): one tile cannot split, 200 tokens under 8 columns do; both shapes run above."""
    size = lambda C, R, M: _lib.call("p2t_lora_wgrad_workspace_bytes", C, R, M)
    assert size(8, 4, 1) == 8 * 4 * 4
    assert size(8, 16, 200) == 4 * 8 * 16 * 4                  # 4 tiles of 64 tokens, one per split
    assert size(4096, 16, 4864) > 4096 * 16 * 4 and size(14336, 16, 4864) > 14336 * 16 * 4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_cfg3_decoder_shape(dtype):
    """4 x 1 216 tokens against the FFN width of Llama-3.1-8B at rank 16: dB of gate / up (stored [N, r]) and dA of down (stored [r, K])."""
    M, C, R = 4864, 14336, 16
    x, u = _inputs(M, C, R, dtype)
    ref, mag = _reference(x, u, C, R)
    for transposed in (False, True):
        got, _ = _run(x, u, C, R, transposed)
        _assert_within_summation_bound(got, ref, mag, M, f"cfg3 transposed {transposed}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,C,R", [(200, 136, 16), (4864, 24, 4), (65, 4096, 64)])
def test_dropout_on_the_fly_equals_p2t_dropout_rows_output(M, C, R, dtype):
    """p = 0.1: the product must be that of p2t_dropout_rows' own output for the same (p, seed) -- same mask, same scaling, same rounding."""
    p, seed = 0.1, 0x1234567 + M
    x, u = _inputs(M, C, R, dtype)
    xd = torch.full((M, C + 8), float("nan"), dtype=dtype, device=dev())
    _lib.call("p2t_dropout_rows", ptr(x), ops.dt_of(x), x.stride(0), ptr(xd), ops.dt_of(xd), xd.stride(0), M, C, p, seed, 0, stream())
    kept = float((xd[:, :C] != 0).float().mean())
    assert 0.8 < kept < 0.97 or M * C < 2000, kept
    ref, mag = _reference(xd, u, C, R)
    got, _ = _run(x, u, C, R, True, p=p, seed=seed)
    _assert_within_summation_bound(got, ref, mag, M, f"dropout M {M} C {C} R {R}")
    plain, _ = _run(x, u, C, R, True)
    assert not np.array_equal(plain, got)                    # the mask did something


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_same_call_twice_is_bit_identical(dtype):
    M, C, R = 4864, 4096, 16
    x, u = _inputs(M, C, R, dtype)
    a, _ = _run(x, u, C, R, False, p=0.1, seed=7)
    b, _ = _run(x, u, C, R, False, p=0.1, seed=7)
    assert np.array_equal(a, b)
    assert SENT not in a
