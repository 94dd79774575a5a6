"""fp64 / numpy restatement of the MXFP4 weight format of the decode step (include/p2t_hip.h, "MXFP4 decoder weights"): e2m1 codes
times one power-of-two scale per block of 32 consecutive K columns, K padded with zeros to a multiple of 128.

Scale rule: e_j = smallest integer with amax_j / 2^e_j <= 6; E_row = max_j e_j; clamp e_j <- max(e_j, E_row - 8); a zero block gets
E_row - 8, an all-zero row byte 127 everywhere; stored byte 127 + e_j.  Codes: round-to-nearest onto GRID * 2^e_j, ties to the even code.
Everything here is exact: powers of two through ldexp / frexp, comparisons of fp64 values that hold the f32 / bf16 inputs exactly."""
import numpy as np

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
CLAMP = 8


def block_exponent(amax: np.ndarray) -> np.ndarray:
    """Smallest integer e with amax <= 6 * 2^e (amax > 0): amax = m 2^x with m in [0.5, 1) -> e = x - 3 + (m > 0.75)."""
    m, x = np.frexp(np.asarray(amax, dtype=np.float64))
    return (x - 3 + (m > 0.75)).astype(np.int64)


def round_codes(v: np.ndarray) -> np.ndarray:
    """Index of the grid value nearest to v in [0, 6]; of two equally near ones, the even index."""
    d = np.abs(np.asarray(v, dtype=np.float64)[..., None] - GRID)
    lo = d.argmin(-1)                                                # the lower index of a tied pair
    hi = np.minimum(lo + 1, 7)
    tie = (np.take_along_axis(d, hi[..., None], -1)[..., 0] == np.take_along_axis(d, lo[..., None], -1)[..., 0]) & (hi != lo)
    return np.where(tie & (lo % 2 == 1), hi, lo).astype(np.uint8)


def quantise(w: np.ndarray, clamp: bool = True):
    """w [rows, K] -> (codes uint8 [rows, Kq] = sign << 3 | grid index, scale bytes uint8 [rows, Kq / 32], values fp64 [rows, K]).
    clamp=False: the rule without the E_row - 8 floor (zero blocks then take E_row), to show what the floor is for."""
    w = np.asarray(w, dtype=np.float64)
    rows, K = w.shape
    Kq = (K + 127) // 128 * 128
    x = np.zeros((rows, Kq))
    x[:, :K] = w
    blocks = x.reshape(rows, Kq // 32, 32)
    amax = np.abs(blocks).max(-1)
    nz = amax > 0
    e = np.where(nz, block_exponent(np.where(nz, amax, 1.0)), np.iinfo(np.int64).min)
    e_row = e.max(-1, keepdims=True)
    zero_row = ~nz.any(-1, keepdims=True)
    floor = np.where(zero_row, 0, e_row - (CLAMP if clamp else 0))
    e = np.where(nz, np.maximum(e, floor) if clamp else e, floor)
    e = np.where(zero_row, 0, e)
    idx = round_codes(np.abs(blocks) / np.ldexp(1.0, e)[..., None])
    codes = (idx | (np.signbit(blocks).astype(np.uint8) << 3)).reshape(rows, Kq)
    values = (np.copysign(GRID[idx], blocks) * np.ldexp(1.0, e)[..., None]).reshape(rows, Kq)[:, :K]
    return codes, (e + 127).astype(np.uint8), values


def pack(codes: np.ndarray) -> np.ndarray:
    """codes [rows, Kq] -> bytes [rows, Kq / 2]: the even column in the low nibble."""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack(packed: np.ndarray) -> np.ndarray:
    out = np.empty((packed.shape[0], packed.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2], out[:, 1::2] = packed & 15, packed >> 4
    return out


def dequantise(packed: np.ndarray, scales: np.ndarray, K: int) -> np.ndarray:
    """bytes [rows, >= Kq / 2] + scale bytes [rows, Kq / 32] -> values fp64 [rows, K] (a negative zero reads as zero)."""
    Kq = (K + 127) // 128 * 128
    c = unpack(np.asarray(packed)[:, : Kq // 2])
    mag = GRID[c & 7] * np.repeat(np.ldexp(1.0, scales.astype(np.int64) - 127), 32, axis=1)
    return (np.where(c & 8, -mag, mag) + 0.0)[:, :K]


def adversarial_rows(seed: int, rows: int, K: int, bf16: bool = True) -> np.ndarray:
    """Rows that stress the scale rule: blocks 2^-5 .. 2^-29 below the rest, zero blocks, a zero row, per-row magnitudes; f32 values that
    are bf16-exact when asked (so that a bf16 copy holds the same numbers)."""
    rs = np.random.RandomState(seed)
    w = rs.randn(rows, K) * np.exp(rs.randn(rows, 1) * 2.0)
    nb = (K + 31) // 32
    for r in range(rows):
        for j in rs.choice(nb, size=max(1, nb // 4), replace=False):
            w[r, 32 * j: 32 * j + 32] *= 2.0 ** -rs.randint(5, 30)
        if nb > 1:
            j = rs.randint(nb)
            w[r, 32 * j: 32 * j + 32] = 0.0
    if rows > 2:
        w[rows // 2] = 0.0
    w = w.astype(np.float32)
    if bf16:
        u = w.view(np.uint32)
        w = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return w
