"""The kernels of the padding-free prefill one by one against numpy (tests/prefill_packed_reference.py), exact comparisons only:
p2t_prompt_index + p2t_pack_rows (and p2t_doc_prepare on their result), p2t_kv_store_packed in fp32 / bf16 and into the fp8 prompt
segment, where p2t_kv_quant_store on the same keys laid out one prompt per row is the independent oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import kv8_reference as K8
import prefill_packed_reference as PR
from gpu_util import SENT, _sentinel, dev, rnd, to_dev, to_np
from p2t_hip import _lib, generation as G, ops
from p2t_hip.ops import ptr, stream

pytestmark = pytest.mark.gpu


def _place(place):
    return (C.c_int32 * (3 * len(place)))(*[v for p in place for v in p])


def _masks(T):
    rs = np.random.RandomState(11)
    m = np.zeros((5, T), dtype=np.int64)
    m[0, T - 90:] = 1                                     # left padding
    m[1, :60] = 1                                         # right padding
    m[2] = rs.rand(T) < 0.5                               # holes
    m[3] = 1                                              # a full row
    m[4, 77] = 1                                          # one token
    return m


@pytest.mark.parametrize("H", [64, 256])
def test_prompt_index_and_pack_rows_vs_numpy(H):
    """Left pad, right pad, holes, a full row and a one-token row of 150 tokens into two packed rows of 256 with padded tails: index, lens,
    embeddings, mask and position ids bit-equal to numpy, nothing written outside the outputs, and p2t_doc_prepare on the result finds
    well-formed rows whose documents are the prompts."""
    T = 150
    mask = _masks(T)
    B = mask.shape[0]
    x = rnd(21, f"pp.x{H}", (B, T, H), 1.0)
    xd, md = to_dev(x), to_dev(mask)
    idx = torch.full((B * T + 8,), -7, dtype=torch.int32, device=dev())
    lens = torch.full((B + 8,), -7, dtype=torch.int32, device=dev())
    _lib.call("p2t_prompt_index", ptr(md), B, T, ptr(idx), ptr(lens), stream())
    ridx, rlens = PR.prompt_index(mask)
    assert np.array_equal(to_np(idx)[: B * T].reshape(B, T), ridx) and np.array_equal(to_np(lens)[:B], rlens)
    assert (to_np(idx)[B * T:] == -7).all() and (to_np(lens)[B:] == -7).all()
    R, Tpk, place = G.plan_prompt_rows(rlens.tolist(), 256)
    PR.check_plan(rlens, 256, R, Tpk, place)
    assert (R, Tpk) == (2, 256) and all(sum(n for r, _, n in place if r == row) < Tpk for row in range(R))        # two rows, each with a padded tail
    out = _sentinel((R * Tpk + 3, H), torch.float32)
    om = torch.full((R * Tpk + 3,), 99, dtype=torch.int64, device=dev())
    pos = torch.full((R * Tpk + 3,), 99, dtype=torch.int32, device=dev())
    _lib.call("p2t_pack_rows", ptr(xd), ptr(idx), ptr(lens), B, T, H, _place(place), R, Tpk, ptr(out), ptr(om), ptr(pos), stream())
    rout, rom, rpos = PR.pack_rows(x, mask, R, Tpk, place)
    assert np.array_equal(to_np(out)[: R * Tpk].reshape(R, Tpk, H), rout) and (to_np(out)[R * Tpk:] == SENT).all()
    assert np.array_equal(to_np(om)[: R * Tpk].reshape(R, Tpk), rom) and (to_np(om)[R * Tpk:] == 99).all()
    assert np.array_equal(to_np(pos)[: R * Tpk].reshape(R, Tpk), rpos) and (to_np(pos)[R * Tpk:] == 99).all()
    assert np.array_equal(PR.unpack_rows(to_np(out)[: R * Tpk].reshape(R, Tpk, H), place, T), PR.compact_rows(x, mask))
    docs = torch.full((2, R, Tpk), -1, dtype=torch.int32, device=dev())
    flags = torch.full((1,), 77, dtype=torch.int32, device=dev())
    _lib.call("p2t_doc_prepare", ptr(pos), 0, ptr(om), R, Tpk, ptr(docs), ptr(flags), stream())
    assert int(flags.item()) & 1 == 0 and int(flags.item()) & 2
    d = to_np(docs)
    for row, start, n in place:
        assert (d[0, row, start:start + n] == start).all() and (d[1, row, start:start + n] == start + n).all()
    for row in range(R):
        used = sum(n for r, _, n in place if r == row)
        assert np.array_equal(d[0, row, used:], np.arange(used, Tpk)) and np.array_equal(d[1, row, used:], np.arange(used, Tpk) + 1)


def test_a_single_unpadded_prompt_packs_to_an_ordinary_row():
    """One prompt of 64 tokens under a full mask: the packed row is the row itself, and p2t_doc_prepare reports neither malformed input
    (bit 0) nor documents (bit 1)."""
    B, T, H = 1, 64, 64
    x = rnd(22, "pp.one", (B, T, H), 1.0)
    xd, md = to_dev(x), torch.ones((B, T), dtype=torch.int64, device=dev())
    idx, lens = torch.empty((T,), dtype=torch.int32, device=dev()), torch.empty((1,), dtype=torch.int32, device=dev())
    _lib.call("p2t_prompt_index", ptr(md), B, T, ptr(idx), ptr(lens), stream())
    R, Tpk, place = G.plan_prompt_rows(lens.tolist())
    assert (R, Tpk, place) == (1, 64, [(0, 0, 64)])
    out, om, pos = torch.empty((1, 64, H), device=dev()), torch.empty((1, 64), dtype=torch.int64, device=dev()), torch.empty((1, 64), dtype=torch.int32, device=dev())
    _lib.call("p2t_pack_rows", ptr(xd), ptr(idx), ptr(lens), B, T, H, _place(place), R, Tpk, ptr(out), ptr(om), ptr(pos), stream())
    assert np.array_equal(to_np(out), x) and to_np(om).all() and np.array_equal(to_np(pos)[0], np.arange(64))
    docs, flags = torch.empty((2, 1, 64), dtype=torch.int32, device=dev()), torch.empty((1,), dtype=torch.int32, device=dev())
    _lib.call("p2t_doc_prepare", ptr(pos), 0, ptr(om), 1, 64, ptr(docs), ptr(flags), stream())
    assert int(flags.item()) == 0


# ---------------------------------------------------------------------------------------------
LENS = [1, 7, 63, 64, 65, 100, 129, 200]
NKV, LAYERS, TP = 2, 2, 256


def _store_case(d, dt, seed):
    """-> (cfg, R, Tpk, place, k, v as numpy in the values `dt` holds): the eight prompts in rows of 320 tokens."""
    R, Tpk, place = G.plan_prompt_rows(LENS, 320)
    PR.check_plan(LENS, 320, R, Tpk, place)
    starts = sorted(s for _, s, _ in place)
    assert R == 3 and Tpk == 320 and any(s % 64 for s in starts) and max(LENS) > 128       # several rows, starts off the tile grid, two tile edges crossed
    dp = ops.head_dim_padded(d)
    cfg = _lib.LlamaConfigC(n_layers=LAYERS, hidden=2 * d, ffn=64, heads=2, kv_heads=NKV, head_dim=d, vocab=64, dtype=ops.dt_of(dt), rms_norm_eps=1e-5,
                            rope_theta=1e4)
    q = lambda a: to_np(to_dev(a, dt)).astype(np.float32)
    k, v = q(rnd(seed, f"ks.k{d}", (R, NKV, Tpk, dp), 2.0)), q(rnd(seed, f"ks.v{d}", (R, NKV, Tpk, dp), 2.0))
    return cfg, R, Tpk, place, dp, k, v


def _cache(kp, vtp, ks=None, vs=None):
    """A p2t_kv_cache over the given prompt segment; the generated segment and the counters are never touched (small live buffers)."""
    gen = torch.zeros((64,), dtype=torch.float32, device=dev())
    cnt = torch.zeros((len(LENS) + 1,), dtype=torch.int32, device=dev())
    c = _lib.KvCacheC(k_prompt=kp.data_ptr(), vt_prompt=vtp.data_ptr(), k_gen=gen.data_ptr(), vt_gen=gen.data_ptr(), prompt_len=cnt.data_ptr(),
                      step=cnt[len(LENS):].data_ptr(), B0=len(LENS), group=1, Tp=TP, G=64, k_prompt_scale=ks.data_ptr() if ks is not None else None,
                      v_prompt_scale=vs.data_ptr() if vs is not None else None)
    return c, (gen, cnt)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [16, 64, 128])
def test_kv_store_packed_vs_numpy_placement(d, dt):
    """Layer 1 of a sentinel-filled two-layer cache: K rows and V^T columns [0, len) of every prompt bit-equal to the numpy placement,
    everything else -- positions >= len, layer 0 -- still the sentinel."""
    cfg, R, Tpk, place, dp, k, v = _store_case(d, dt, 31)
    n = len(LENS)
    kp, vtp = _sentinel((LAYERS, n, NKV, TP, dp), dt), _sentinel((LAYERS, n, NKV, dp, TP), dt)
    cache, keep = _cache(kp, vtp)
    kd, vd = to_dev(k, dt), to_dev(v, dt)
    _lib.call("p2t_kv_store_packed", C.byref(cfg), C.byref(cache), 1, ptr(kd), ptr(vd), R, Tpk, _place(place), n, stream())
    rk, rvt = np.full((n, NKV, TP, dp), SENT, dtype=np.float32), np.full((n, NKV, dp, TP), SENT, dtype=np.float32)
    PR.kv_store(k, v, place, TP, rk, rvt)
    gk, gvt = to_np(kp).astype(np.float32), to_np(vtp).astype(np.float32)
    assert np.array_equal(gk[1], rk) and np.array_equal(gvt[1], rvt)
    assert (gk[0] == SENT).all() and (gvt[0] == SENT).all()
    for i, (_, _, ln) in enumerate(place):                # (what the two comparisons above imply, said once more for the reader)
        assert (gk[1, i, :, ln:] == SENT).all() and (gvt[1, i, :, :, ln:] == SENT).all() and not (gk[1, i, :, :ln] == SENT).any()


@pytest.mark.parametrize("d", [16, 64, 128])
def test_kv_store_packed_fp8_vs_kv_quant_store_and_numpy(d):
    """The fp8 prompt segment: codes and both scale arrays of every prompt's [0, len) bit-equal to p2t_kv_quant_store run on the same keys
    laid out one prompt per row (an existing entry point: the independent oracle) and to kv8_reference; 0xA5 everywhere else."""
    dt = torch.bfloat16
    cfg, R, Tpk, place, dp, k, v = _store_case(d, dt, 32)
    n, S = len(LENS), 0xA5
    u8 = lambda *shape: torch.full(shape, S, dtype=torch.uint8, device=dev())
    kq, vtq, ks, vs = u8(LAYERS, n, NKV, TP, dp), u8(LAYERS, n, NKV, dp, TP), u8(LAYERS, n, NKV, TP), u8(LAYERS, n, NKV, TP)
    cache, keep = _cache(kq, vtq, ks, vs)
    kd, vd = to_dev(k, dt), to_dev(v, dt)
    _lib.call("p2t_kv_store_packed", C.byref(cfg), C.byref(cache), 1, ptr(kd), ptr(vd), R, Tpk, _place(place), n, stream())
    got = [to_np(t) for t in (kq, vtq, ks, vs)]
    for t in got:
        assert (t[0] == S).all()
    # numpy: kv8_reference's bytes at the numpy placement
    ref = [np.full(t.shape[1:], S, dtype=np.uint8) for t in got]
    PR.kv_store_fp8(k, v, place, d, *ref)
    for name, a, b in zip(("k codes", "v codes", "k scales", "v scales"), got, ref):
        assert np.array_equal(a[1], b), name
    # the oracle kernel on one prompt per row
    T = max(LENS)
    k1, v1 = np.zeros((n, NKV, T, dp), dtype=np.float32), np.zeros((n, NKV, T, dp), dtype=np.float32)
    for i, (row, start, ln) in enumerate(place):
        k1[i, :, :ln], v1[i, :, :ln] = k[row, :, start:start + ln], v[row, :, start:start + ln]
    okq, ovtq, oks, ovs = u8(n, NKV, TP, dp), u8(n, NKV, dp, TP), u8(n, NKV, TP), u8(n, NKV, TP)
    k1d, v1d = to_dev(k1, dt), to_dev(v1, dt)
    _lib.call("p2t_kv_quant_store", ptr(k1d), ptr(v1d), n, NKV, T, d, TP, ptr(okq), ptr(ovtq), ptr(oks), ptr(ovs), stream())
    okq, ovtq, oks, ovs = (to_np(t) for t in (okq, ovtq, oks, ovs))
    for i, (_, _, ln) in enumerate(place):
        assert np.array_equal(got[0][1, i, :, :ln], okq[i, :, :ln]) and np.array_equal(got[1][1, i, :, :, :ln], ovtq[i, :, :, :ln]), i
        assert np.array_equal(got[2][1, i, :, :ln], oks[i, :, :ln]) and np.array_equal(got[3][1, i, :, :ln], ovs[i, :, :ln]), i
        assert (got[0][1, i, :, ln:] == S).all() and (got[1][1, i, :, :, ln:] == S).all() and (got[2][1, i, :, ln:] == S).all() and (got[3][1, i, :, ln:] == S).all()
