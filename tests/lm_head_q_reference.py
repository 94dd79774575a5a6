"""fp64 restatement of the quantised LM head (include/p2t_hip.h, p2t_lm_head_q / p2t_lm_head_logits_q): de-quantise the codes and scales
of both operands, take the dot products in fp64, round once to the model dtype (bf16).  The quantiser restatements are the repository's
own: tests/mxfp4_reference.py for MXFP4, oracle/p2t_oracle.py quant_rows_e4m3 (the fp8 rule of the host tests) for e4m3."""
import numpy as np
import torch

import mxfp4_reference as R
from oracle import p2t_oracle as O


def e4m3_values(codes: np.ndarray, scales: np.ndarray, K: int) -> np.ndarray:
    """e4m3 bytes [rows, >= K] + one E8M0 byte per row -> the values they stand for, fp64 [rows, K]."""
    v = torch.from_numpy(np.ascontiguousarray(codes)).view(torch.float8_e4m3fn).to(torch.float64).numpy()[:, :K]
    return v * np.ldexp(1.0, scales.astype(np.int64).reshape(-1) - 127)[:, None]


def head_values(fmt: str, codes: np.ndarray, scales: np.ndarray, K: int) -> np.ndarray:
    """The head W~ [vocab, K] in fp64 from its codes and scales: "fp8" (row scales) or "mxfp4" (one scale byte per 32 columns)."""
    return e4m3_values(codes, scales, K) if fmt == "fp8" else R.dequantise(codes, scales, K)


def quantise_head(fmt: str, w: np.ndarray):
    """The quantisers restated on a bf16-exact head w [vocab, K] -> (values fp64 [vocab, K], scale bytes)."""
    if fmt == "fp8":
        deq, E, _ = O.quant_rows_e4m3(np.asarray(w, dtype=np.float32))
        return deq.astype(np.float64), E
    _, sc, val = R.quantise(w)
    return val + 0.0, sc


def bf16_round(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def logits(act: np.ndarray, w: np.ndarray):
    """act fp64 [M, K] (the de-quantised e4m3 rows), w fp64 [V, K] -> (exact products summed in fp64 [M, V], sum of |a w| [M, V])."""
    return act @ w.T, np.abs(act) @ np.abs(w).T


def bound(ref: np.ndarray, abs_sum: np.ndarray, Kq: int) -> np.ndarray:
    """|stored bf16 logit - ref|: every product of an e4m3 and an e4m3 / e2m1 value is exact in f32 and the power-of-two scales are
    exact, so the kernel's only errors are its f32 additions -- at most Kq of them per output, each within 2^-24 of a partial sum that
    is at most sum |a w| -- and ONE rounding of the f32 result to bf16: half a step (2^-8 relative) of a value within that distance."""
    acc = Kq * 2.0 ** -24 * abs_sum
    return acc + 2.0 ** -8 * (np.abs(ref) + acc)
