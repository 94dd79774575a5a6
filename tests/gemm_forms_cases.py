"""The case table of tests/test_gpu_gemm_forms.py: the smallest shapes that reach each four-wave form of the bf16 GEMM under the
default policy on 256 CUs with the full split-K fix-up workspace (plan_default, csrc/gemm_mfma.hip), every epilogue that form is
built for, and the plan (form, grid, n_full, n_tail, half_tail) each case gets under the default policy and under policy 9 (the
eight-wave forms).  tests/test_gemm_plan.py asserts the plans without a GPU, so the GPU test verifiably runs the form its name says;
the GPU test reads from the plans whether the two policies split K the same way.  Nothing in here needs a GPU."""
from collections import namedtuple

from helpers import EPI_GELU, EPI_QKV_ROPE, EPI_RESID, EPI_STORE, EPI_STORE_F32, EPI_SWIGLU

F32, BF16 = 0, 1
# epilogue name (as in the observe() key) -> (code, out dtype) that p2t_gemm_nt gets; gelu_z (GELU with the pre-activation copy) and f32
# (EPI_STORE_F32) are no cases of the table: the argument tests use them.  Every other name is a qkv_* one of p2t_gemm_qkv_rope
EPILOGUES = {"store_bf16": (EPI_STORE, BF16), "store_f32": (EPI_STORE, F32), "resid": (EPI_RESID, F32), "gelu": (EPI_GELU, BF16),
             "gelu_z": (EPI_GELU, BF16), "swiglu": (EPI_SWIGLU, BF16), "f32": (EPI_STORE_F32, F32)}

# qkv: (head_dim, nh, nkv, seq) of p2t_gemm_qkv_rope; p0 / p9: the plan under the default policy / policy 9
Case = namedtuple("Case", "form epi code out M N K qkv p0 p9")


def _c(form, epi, shape, p0, p9, qkv=None):
    return Case(form, epi, *EPILOGUES.get(epi, (EPI_QKV_ROPE, BF16)), *shape, qkv, p0, p9)


def _qkv(d, nh, nkv, seq):
    return f"qkv_d{d}_s{seq}", (d, nh, nkv, seq)


CASES = []
# w4_persist, one whole round: 256 tiles; K = 384 is the 12-stage minimum of persist_fits
for K in (384, 512):
    p0, p9 = ("w4_persist", 256, 256, 0, 0), ("persist", 256, 256, 0, 0)
    for epi in ("store_bf16", "store_f32", "resid", "gelu", "swiglu"):
        CASES.append(_c("w4_persist", epi, (4096, 4096, K), p0, p9))
    for name, q in (_qkv(64, 32, 16, 512), _qkv(128, 16, 8, 512)):
        CASES.append(_c("w4_persist", name, (4096, 4096, K), p0, p9, q))
# w4_persist, a partial round as whole tiles (272 tiles, rem 16): persist_pays takes it for the read-modify-write epilogue only;
# the eight-wave kernel runs the 16 leftover tiles as 128-row halves
CASES.append(_c("w4_persist", "resid", (4096, 4352, 384), ("w4_persist", 256, 272, 0, 0), ("persist", 256, 256, 16, 1)))
# w4_persist + in-stream split-K pairs: rem 16, K at the pairs_pay threshold
for epi in ("store_bf16", "resid", "gelu"):
    CASES.append(_c("w4_persist_pairs", epi, (4096, 4352, 6144), ("w4_persist", 256, 256, 16, 0), ("persist", 256, 256, 16, 0)))
# w4_tile: 192 tiles = three quarters of a round; K = 256 is its minimum.  seq 256 at M = 2048: every 256-row tile is one sequence;
# seq 512: two tiles per sequence
for K in (256, 384):
    p0, p9 = ("w4_tile", 192, 192, 0, 0), ("tile256", 192, 192, 0, 0)
    CASES.append(_c("w4_tile", "store_bf16", (2048, 6144, K), p0, p9))
    for name, q in (_qkv(128, 32, 8, 512), _qkv(128, 32, 8, 256), _qkv(64, 32, 32, 512), _qkv(64, 32, 32, 256)):
        CASES.append(_c("w4_tile", name, (2048, 6144, K), p0, p9, q))
# w4_pairs: 96 tiles, the lower bound items * 8 >= cus * 3; every tile as a split-K pair
for epi in ("store_bf16", "store_f32", "resid"):
    CASES.append(_c("w4_pairs", epi, (2048, 3072, 8192), ("w4_pairs", 192, 0, 96, 0), ("splitk", 192, 0, 96, 0)))
# rotary rows wrapping INSIDE a tile: seq 384 at 4608 rows = 288 tiles.  Without a read-modify-write epilogue persist_pays does not
# take a partial round this short, and 288 tiles are more than a round, so both policies run it on the eight-wave per-tile kernel
for name, q in (_qkv(64, 32, 16, 384), _qkv(128, 16, 8, 384)):
    CASES.append(_c("tile256", name, (4608, 4096, 384), ("tile256", 288, 288, 0, 0), ("tile256", 288, 288, 0, 0), q))


def case_id(c):
    return f"{c.form}-{c.epi}-{c.M}x{c.N}x{c.K}"


def k_split_tiles(plan):
    """How many tiles a plan runs as two K halves (the tail tiles, unless they are 128-row halves).  Both kernel families cut such a tile
    at the same K element (half the 32- resp. 64-wide stages, rounded down to even: K = 6144 -> 3072, 8192 -> 4096) and the consumer adds
    the producer's partial sums in a fixed order, so two plans with the same count here associate every fp32 sum the same way."""
    _, _, _, n_tail, half_tail = plan
    return 0 if half_tail else n_tail
