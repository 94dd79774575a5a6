"""Shared test helpers: rebuild a golden case's specs, inputs and synthetic weights."""
import numpy as np
from scipy.special import erf

from oracle import p2t_oracle as O
from p2t_hip import specs, synth

EPI_STORE, EPI_GELU, EPI_RESID, EPI_SWIGLU, EPI_STORE_F32, EPI_GELU_BWD = range(6)      # the epilogue codes of include/p2t_hip.h
EPI_QKV_ROPE = 6


def case_setup(meta):
    esm = specs.EsmSpec(**meta["esm"])
    llama = specs.LlamaSpec(**meta["llama"])
    ad = specs.AdapterSpec(**meta["adapter"])
    pid, pmask = synth.protein_batch(meta["seed_in"], meta["B"], meta["T_p"], meta["p_lens"])
    tid, tmask = synth.text_batch(meta["seed_in"], meta["B"], meta["T_t"], meta["id_high"], meta["t_lens"],
                                  meta["pad_id"], meta["eos_id"])
    return esm, llama, ad, pid, pmask, tid, tmask


from oracle.weights import LazyWeights, model_weights  # noqa: E402,F401  (kept importable from helpers)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def gemm_epilogue_ref(acc, bias, epi, resid=None, z=None):
    """The epilogue of p2t_gemm_nt on the product acc [M, N], in acc's precision (fp32: the oracle's GELU; fp64: the same formula in fp64)."""
    if epi == EPI_SWIGLU:
        F = acc.shape[1] // 2
        v = acc.reshape(acc.shape[0], F // 32, 2, 32)
        g, u = v[:, :, 0, :].reshape(-1, F), v[:, :, 1, :].reshape(-1, F)
        return (g / (1 + np.exp(-g))) * u
    if bias is not None:
        acc = acc + bias
    if epi == EPI_GELU:
        return O.gelu_erf(acc) if acc.dtype != np.float64 else acc * 0.5 * (1.0 + erf(acc / np.sqrt(2.0)))
    if epi == EPI_RESID:
        return resid + acc
    if epi == EPI_GELU_BWD:
        return acc * O.gelu_erf_grad(z)
    return acc


def gemm_ref(a, w, bias, epi, resid=None, z=None):
    return gemm_epilogue_ref(a.astype(np.float32) @ w.astype(np.float32).T, bias, epi, resid, z)


def qkv_rope_ref(acc, pos, nh, nkv, d, q_scale, inv_freq):
    """EPI_QKV_ROPE on rows of the product acc [R, (nh + 2 nkv) * d] (natural channel order) that sit at sequence positions pos [R], in
    acc's precision: query scale BEFORE the rotation, rotate-half rotary on q and k -> q [R, nh, d], k, v [R, nkv, d]."""
    x = acc.reshape(acc.shape[0], nh + 2 * nkv, d)
    cos, sin = O.rope_cos_sin(inv_freq, np.asarray(pos))
    cos, sin = cos[:, None, :].astype(acc.dtype), sin[:, None, :].astype(acc.dtype)
    q = x[:, :nh] * acc.dtype.type(np.float32(q_scale))
    k, v = x[:, nh:nh + nkv], x[:, nh + nkv:]
    return q * cos + O.rotate_half(q) * sin, k * cos + O.rotate_half(k) * sin, v


def pack_d128(w, heads):
    """[heads * 128, K] -> the per-head row order 0..31, 64..95, 32..63, 96..127 of include/p2t_hip.h (p2t_llama_layer).  Its own inverse."""
    K = w.shape[1]
    return np.ascontiguousarray(w.reshape(heads, 2, 2, 32, K).transpose(0, 2, 1, 3, 4).reshape(heads * 128, K))
