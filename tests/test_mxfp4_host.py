"""CPU: the MXFP4 weight format's rule (tests/mxfp4_reference.py, the fp64 restatement of include/p2t_hip.h "MXFP4 decoder weights"):
the tie table, the scale rule at its boundary, the clamp and what it is for -- `quant_rows_e4m3(W~) == W~` bit for bit, which fails
without it -- zero blocks and rows, K that is no multiple of 32 / 128, value idempotence and the per-element error bound."""
import numpy as np
import pytest

import mxfp4_reference as R
from oracle import p2t_oracle as O


def _bf16_up(x):
    """the next bf16 above a positive bf16-exact f32"""
    return (np.float32(x).view(np.uint32) + np.uint32(0x10000)).view(np.float32)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_ties_go_to_the_even_code(sign):
    ties = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}
    for e in (-3, 0, 5):
        row = np.zeros((1, 32))
        row[0, 0] = 6.0 * 2.0 ** e                                   # pins the block scale at e
        row[0, 1:8] = sign * np.array(list(ties)) * 2.0 ** e
        codes, sc, val = R.quantise(row)
        assert sc[0, 0] == 127 + e
        assert np.array_equal(val[0, 1:8], sign * np.array(list(ties.values())) * 2.0 ** e)
        assert np.array_equal(codes[0, 1:8] >> 3, np.full(7, int(sign < 0)))
    # just off a tie goes to the nearer value, on both sides
    eps = 2.0 ** -20
    row = np.zeros((1, 32)); row[0, 0] = 6.0
    row[0, 1:5] = sign * np.array([0.25 + eps, 0.75 - eps, 2.5 + eps, 5.0 + eps])
    assert np.array_equal(R.quantise(row)[2][0, 1:5], sign * np.array([0.5, 0.5, 3.0, 6.0]))


def test_scale_rule_at_the_boundary_and_the_next_bf16_above_it():
    for e in (-20, -1, 0, 7):
        amax = np.float32(6.0 * 2.0 ** e)
        row = np.zeros((2, 32), np.float32)
        row[0, 3], row[1, 3] = amax, _bf16_up(amax)
        codes, sc, val = R.quantise(row)
        assert sc[:, 0].tolist() == [127 + e, 127 + e + 1]           # 6 * 2^e still fits e; one bf16 step more does not
        assert val[0, 3] == float(amax) and val[1, 3] == 3.0 * 2.0 ** (e + 1)
    rs = np.random.RandomState(0)
    amax = np.exp(rs.uniform(-30, 30, 4000))
    e = R.block_exponent(amax)
    assert np.all(amax / np.ldexp(1.0, e) <= 6.0) and np.all(amax / np.ldexp(1.0, e - 1) > 6.0)


def test_clamp_zero_blocks_and_zero_rows():
    row = np.zeros((3, 128))
    row[0, 0:32] = 5.0                                               # e = 0
    row[0, 32:64] = 2.0 ** -20                                       # far below: clamped to E_row - 8, rounds to zero
    row[0, 64:96] = 3.0 * 2.0 ** -10                                 # natural e = -11 -> clamped to -8: 0.75 * 2^-8 -> 1 * 2^-8 (tie to even)
    row[1, 40] = -1.0                                                # one non-zero block; the rest are zero blocks
    codes, sc, val = R.quantise(row)
    assert sc[0].tolist() == [127, 119, 119, 119]
    assert not val[0, 32:64].any() and np.all(val[0, 64:96] == 2.0 ** -8)
    assert sc[1].tolist() == [127 - 2 - 8, 127 - 2, 127 - 2 - 8, 127 - 2 - 8] and val[1, 40] == -1.0
    assert sc[2].tolist() == [127] * 4 and not val[2].any() and not (codes[2] & 7).any()
    # without the clamp the tiny block keeps its own scale
    assert R.quantise(row, clamp=False)[1][0, 1] == 127 - 22


@pytest.mark.parametrize("K", [32, 100, 128, 1000])
def test_shapes_padding_and_packing(K):
    w = R.adversarial_rows(K, 9, K)
    codes, sc, val = R.quantise(w)
    Kq = (K + 127) // 128 * 128
    assert codes.shape == (9, Kq) and sc.shape == (9, Kq // 32) and val.shape == (9, K)
    assert not (codes[:, K:] & 7).any()                              # columns at or beyond K count as zeros
    packed = R.pack(codes)
    assert packed.shape == (9, Kq // 2) and np.array_equal(R.unpack(packed), codes)
    assert np.array_equal(packed[:, 0] & 15, codes[:, 0]) and np.array_equal(packed[:, 0] >> 4, codes[:, 1])   # even column: low nibble
    assert np.array_equal(R.dequantise(packed, sc, K), val + 0.0)
    # per element |w - w~| <= 2^e_j
    bound = np.repeat(np.ldexp(1.0, sc.astype(np.int64) - 127), 32, axis=1)[:, :K]
    assert np.all(np.abs(w.astype(np.float64) - val) <= bound)
    # value idempotence (the scale bytes may differ)
    assert np.array_equal(R.quantise(val)[2], val)


@pytest.mark.parametrize("K", [100, 128, 1000, 4096])
def test_e4m3_row_quantisation_of_the_values_is_lossless_and_needs_the_clamp(K):
    """quant_rows_e4m3(W~) == W~ bit for bit on 200 adversarial row sets; with the clamp removed the property fails on the same family."""
    fails_without = 0
    sets = 200 if K <= 1000 else 20
    for seed in range(sets):
        w = R.adversarial_rows(1000 * K + seed, 6, K)
        val = R.quantise(w)[2].astype(np.float32)
        assert np.array_equal(val.astype(np.float64), R.quantise(w)[2])                 # the values are f32-exact
        assert np.array_equal(O.quant_rows_e4m3(val)[0], val), (K, seed)
        loose = R.quantise(w, clamp=False)[2].astype(np.float32)
        fails_without += not np.array_equal(O.quant_rows_e4m3(loose)[0], loose)
    assert fails_without > sets // 2, fails_without
