#!/usr/bin/env python3
"""Kernel micro-benchmarks on the GPU box (HIP-event timed, random data): GEMM shapes of the
cfg-3 towers, attention, norms.  Usage: python tools/microbench.py [gemm] [attn] [norm]
`attn_decode` [m8] [m32]: the decode step's attention alone over the bf16 and the fp8 prompt segment of the KV cache.
`attn_decode beams`: the attention of a beam group alone, the (row, kv head) kernel against the (prompt, kv head) kernel that reads an ancestry
table, 8 x 4 and 32 x 4 beams, bf16 and fp8 prompt segment, 33 and 250 generated keys; then p2t_kv_reorder against p2t_kv_ancestry_update.
`attn_decode multi`: the attention of a step of Q tokens per row alone (p2t_attention_decode_multi, prompt-lookup decoding), 1 / 2 / 4 / 8 rows x
Q = 2 / 4 / 8, bf16 and fp8 prompt segment, against Q launches of p2t_attention_decode_rows and against one.
`choice_rows` [m8] [m32]: the per-row choice kernels of continuous batching alone (p2t_sample_select_rows, p2t_logits_process_rows) on
[rows, 128256] bf16 logits next to their lock-step twins, with no row and with half of the rows finished (the per-row kernels leave a
finished row before they read it; the lock-step ones do its whole work).

`kv_store` [m8] [m32]: the prefill's store of one layer's keys and values alone, p2t_kv_store_packed (bf16 and fp8 prompt segment) from a packed
row of ragged prompts next to p2t_kv_quant_store on the padded batch.

The `gemm` / `cold` / `ksweep` modes force launch forms through p2t_set_gemm_policy, and `fp8abl` runs the fp8 K-loop ablations
(tile 1001-1003): run them against the LAB build (P2T_HIP_LIB=tools/build/libp2t_lab.so, `make -C prot2text-v2-esm3_amd/csrc lab`);
the product library only knows policies 0 and 9 and fp8 tiles 0, 4, 128 and 256."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prot2text-v2-esm3_amd"))
from p2t_hip import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")


def timeit(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def rand(shape, dtype=torch.bfloat16, scale=1.0):
    t = torch.empty(shape, dtype=dtype, device=dev)
    ops.fill_hash_(t, 1, f"mb{shape}", scale)
    return t


def bench_gemm():
    shapes = [  # name, M, N, K, epilogue
        ("esm qkv", 16384, 7680, 2560, 0), ("esm o", 16384, 2560, 2560, 2), ("esm fc1", 16384, 10240, 2560, 1),
        ("esm fc2", 16384, 2560, 10240, 2), ("llama qkv", 2048, 6144, 4096, 0), ("llama o", 2048, 4096, 4096, 2),
        ("llama gu", 2048, 28672, 4096, 3), ("llama down", 2048, 4096, 14336, 2), ("adapter fc1", 16384, 2048, 2560, 1),
        ("adapter fc2", 16384, 4096, 2048, 1), ("square 4k", 4096, 4096, 4096, 0), ("square 8k", 8192, 8192, 8192, 0),
    ]
    for name, M, N, K, epi in shapes:
        a, w = rand((M, K)), rand((N, K), scale=0.05)
        bias = None if epi == 3 else rand((N,), torch.float32, 0.1)
        out = torch.zeros((M, N), dtype=torch.float32, device=dev) if epi == 2 else None
        ws, ep = ops.gemm_fix_workspace(dev), [0]

        def with_tail():
            ep[0] += 1
            ops.gemm_nt(a, w, bias, epilogue=epi, out=out, use_mfma=1, fix_ws=ws, fix_epoch=ep[0])
        res = []
        for env, fn in (("2", lambda: ops.gemm_nt(a, w, bias, epilogue=epi, out=out, use_mfma=1)), ("2", with_tail),
                        ("4", with_tail), ("3", with_tail), (None, with_tail), ("7", with_tail), ("8", with_tail)):
            _lib.call("p2t_set_gemm_policy", int(env or 0))
            res.append(timeit(fn))
        _lib.call("p2t_set_gemm_policy", 0)
        fl = 2.0 * M * N * K / 1e9
        print(f"gemm {name:12s} M={M:6d} N={N:6d} K={K:6d} epi={epi}: TF/s per-tile {fl / res[0]:7.1f} | per-tile+splitK {fl / res[1]:7.1f} | "
              f"persistent {fl / res[2]:7.1f} | persistent+splitK {fl / res[3]:7.1f} | default {fl / res[4]:7.1f} ({res[4]:.3f} ms) | four-wave per-tile {fl / res[5]:7.1f} | four-wave persistent {fl / res[6]:7.1f}", flush=True)


def bench_cold():
    """Encoder GEMMs with their operands / residual stream COLD (a 768 MB fill between launches evicts the 256 MB Infinity
    Cache), as they are inside a step; each launch timed on its own with events."""
    shapes = [("esm qkv", 16384, 7680, 2560, 0), ("esm o", 16384, 2560, 2560, 2), ("esm fc1", 16384, 10240, 2560, 1),
              ("esm fc2", 16384, 2560, 10240, 2)]
    flush = torch.empty((768 << 20,), dtype=torch.uint8, device=dev)
    for name, M, N, K, epi in shapes:
        a, w = rand((M, K)), rand((N, K), scale=0.05)
        bias = rand((N,), torch.float32, 0.1)
        out = torch.zeros((M, N), dtype=torch.float32, device=dev) if epi == 2 else None
        ws, ep = ops.gemm_fix_workspace(dev), [0]
        fl = 2.0 * M * N * K / 1e9
        res = []
        for env in ("2", "4", "3", "5", "9", "7", "8", "10", "12"):
            _lib.call("p2t_set_gemm_policy", int(env or 0))
            tot = 0.0
            for i in range(6):
                flush.fill_(i)
                s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ep[0] += 1
                s0.record()
                ops.gemm_nt(a, w, bias, epilogue=epi, out=out, use_mfma=1, fix_ws=ws, fix_epoch=ep[0])
                e0.record()
                torch.cuda.synchronize()
                if i > 0:
                    tot += s0.elapsed_time(e0)
            res.append(tot / 5)
        _lib.call("p2t_set_gemm_policy", 0)
        print(f"cold {name:8s}: per-tile(+splitK) {res[0] * 1e3:7.1f} us {fl / res[0]:7.1f} TF/s | persistent {res[1] * 1e3:7.1f} us {fl / res[1]:7.1f} | "
              f"persistent+splitK {res[2] * 1e3:7.1f} us {fl / res[2]:7.1f} | persistent+half-tiles {res[3] * 1e3:7.1f} us {fl / res[3]:7.1f} | "
              f"eight-wave default {res[4] * 1e3:7.1f} us {fl / res[4]:7.1f} | four-wave per-tile {res[5] * 1e3:7.1f} us {fl / res[5]:7.1f} | four-wave persistent + split-K tail {res[6] * 1e3:7.1f} us {fl / res[6]:7.1f} | "
              f"four-wave persistent, whole tiles only {res[7] * 1e3:7.1f} us {fl / res[7]:7.1f} | same, other order {res[8] * 1e3:7.1f} us {fl / res[8]:7.1f}", flush=True)


def bench_ksweep():
    """Per-tile fixed cost vs steady-state rate: time = rounds * (a + b*K)."""
    for epi in (0, 1, 2):
        for M, N in ((16384, 10240), (16384, 2560)):
            for K in (256, 512, 1024, 2560, 5120, 10240):
                a, w = rand((M, K)), rand((N, K), scale=0.05)
                bias = rand((N,), torch.float32, 0.1)
                out = torch.zeros((M, N), dtype=torch.float32, device=dev) if epi == 2 else None
                ms = timeit(lambda: ops.gemm_nt(a, w, bias, epilogue=epi, out=out, use_mfma=1))
                rounds = (M // 256) * (N // 256) / 256.0
                print(f"ksweep epi={epi} M={M} N={N} K={K:6d}: {ms * 1e3:8.1f} us  {2.0 * M * N * K / ms / 1e9:7.1f} TF/s  "
                      f"per-round {ms * 1e3 / rounds:7.2f} us", flush=True)


def bench_attn():
    for name, B, T, nh, nkv, d, causal in [("esm3b", 16, 1024, 40, 40, 64, False), ("llama8b", 16, 128, 32, 8, 128, True),
                                            ("esm35m", 32, 512, 20, 20, 24, False)]:
        qkv = rand((B * T, (nh + 2 * nkv) * d))
        inv = torch.ones((d // 2,), dtype=torch.float32, device=dev)
        mask = torch.ones((B, T), dtype=torch.int64, device=dev)
        km, kv, _ = ops.mask_prepare(mask)
        q, k, v = ops.qkv_post(qkv, inv, B, T, nh, nkv, d, 1.0)
        ms_post = timeit(lambda: ops.qkv_post(qkv, inv, B, T, nh, nkv, d, 1.0))
        ms = timeit(lambda: ops.attention(q, k, v, km, kv, d, d ** -0.5, causal, use_mfma=1))
        ms2 = timeit(lambda: ops.attention(q, k, v, km, kv, d, 1.0, causal, use_mfma=1, log2_scores=True))     # timing only: q not re-scaled
        fl = 4.0 * B * nh * T * T * d * (0.5 if causal else 1.0)
        print(f"attn {name:8s} B={B} T={T} nh={nh}/{nkv} d={d}: {ms:7.3f} ms {fl / ms / 1e9:7.1f} TF/s | log2-scores form {ms2:7.3f} ms "
              f"{fl / ms2 / 1e9:7.1f} TF/s | qkv_post {ms_post:7.3f} ms", flush=True)


def bench_norm():
    for rows, cols in ((16384, 2560), (2048, 4096)):
        x = rand((rows, cols), torch.float32)
        w, b = rand((cols,), torch.float32), rand((cols,), torch.float32)
        ms = timeit(lambda: ops.layernorm(x, w, b, 1e-5, torch.bfloat16))
        print(f"layernorm {rows}x{cols}: {ms * 1e3:7.1f} us  {rows * cols * 6 / ms / 1e6:7.1f} GB/s", flush=True)


def bench_blas():
    """Vendor-library reference point (NOT used by the product): torch.matmul (hipBLASLt / rocBLAS) on the encoder GEMM
    shapes, plain bf16 store, same cold-cache protocol as `cold`."""
    shapes = [("esm qkv", 16384, 7680, 2560), ("esm o", 16384, 2560, 2560), ("esm fc1", 16384, 10240, 2560),
              ("esm fc2", 16384, 2560, 10240), ("square", 8192, 8192, 8192)]
    flush = torch.empty((768 << 20,), dtype=torch.uint8, device=dev)
    for name, M, N, K in shapes:
        a, w = rand((M, K)), rand((N, K), scale=0.05)
        out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        fl = 2.0 * M * N * K / 1e9
        res = []
        for which in ("blas", "ours"):
            tot = 0.0
            for i in range(6):
                flush.fill_(i)
                s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                if which == "blas":
                    torch.matmul(a, w.t(), out=out)
                else:
                    ops.gemm_nt(a, w, None, epilogue=0, out=out, use_mfma=1)
                e0.record()
                torch.cuda.synchronize()
                if i > 0:
                    tot += s0.elapsed_time(e0)
            res.append(tot / 5)
        print(f"blas {name:8s} M={M} N={N} K={K}: torch.matmul {res[0] * 1e3:7.1f} us {fl / res[0]:7.1f} TF/s | p2t gemm_nt (store epilogue) "
              f"{res[1] * 1e3:7.1f} us {fl / res[1]:7.1f} TF/s", flush=True)


def bench_fp8():
    """fp8 MFMA GEMM (cfg5) on the tower shapes, operands cold (a 768 MB fill between launches), per tile height; beside it
    the bf16 kernel's default policy on the same shape, and the cost of the quantise pass that feeds FFN-down / o-proj."""
    shapes = [("esm qkv", 16384, 7680, 2560, 0), ("esm o", 16384, 2560, 2560, 2), ("esm fc1", 16384, 10240, 2560, 1),
              ("esm fc2", 16384, 2560, 10240, 2), ("esm qkv b64", 65536, 7680, 2560, 0), ("esm fc2 b64", 65536, 2560, 10240, 2),
              ("llama qkv", 8192, 6144, 4096, 0), ("llama gu", 8192, 28672, 4096, 3), ("llama down", 8192, 4096, 14336, 2)]
    flush = torch.empty((768 << 20,), dtype=torch.uint8, device=dev)
    for name, M, N, K, epi in shapes:
        a, w = rand((M, K)), rand((N, K), scale=0.05)
        a8, sa = ops.quant_rows_fp8(a)
        w8, sw = ops.quant_rows_fp8(w)
        bias = None if epi == 3 else rand((N,), torch.float32, 0.1)
        out = torch.zeros((M, N), dtype=torch.float32, device=dev) if epi == 2 else None
        fl = 2.0 * M * N * K / 1e9
        res = []
        for which in (256, 128, "bf16", "quant", 0):
            if which == 0 and epi == 1:
                res.append(float("nan"))                     # plain GELU has no four-wave form (the towers use GELU -> e4m3)
                continue
            tot = 0.0
            for i in range(5):
                flush.fill_(i)
                s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                if which == "bf16":
                    ops.gemm_nt(a, w, bias, epilogue=epi, out=out, use_mfma=1)
                elif which == "quant":
                    ops.quant_rows_fp8(a)
                else:
                    ops.gemm_nt_fp8(a8, sa, w8, sw, bias, n=N, k=K, epilogue=epi, out=out, tile=which)
                e0.record()
                torch.cuda.synchronize()
                if i > 0:
                    tot += s0.elapsed_time(e0)
            res.append(tot / 4)
        print(f"fp8 {name:12s} M={M:6d} N={N:6d} K={K:6d} epi={epi}: 256-row {res[0] * 1e3:7.1f} us {fl / res[0]:7.1f} TF/s | 128-row "
              f"{res[1] * 1e3:7.1f} us {fl / res[1]:7.1f} | bf16 kernel {res[2] * 1e3:7.1f} us {fl / res[2]:7.1f} | quantise A [{M}x{K}] "
              f"{res[3] * 1e3:6.1f} us {M * K * 3 / res[3] / 1e6:6.0f} GB/s | four-wave persistent {res[4] * 1e3:7.1f} us {fl / res[4]:7.1f}", flush=True)


def bench_skinny():
    """The decode step's weight-streaming GEMM (p2t_gemm_nt_skinny) on the Llama-3.1-8B projections: every call reads another copy
    of the weights (a ring of copies > 1 GB, so neither the L2s nor the 256 MB memory-side cache serve them) -> GB/s of W."""
    from p2t_hip.ops import ptr, stream
    shapes = [("o-proj", 4096, 4096, _lib.EPI_RESID), ("qkv", 6144, 4096, _lib.EPI_STORE_F32), ("gate/up", 28672, 4096, _lib.EPI_SWIGLU),
              ("down", 4096, 14336, _lib.EPI_RESID), ("lm head", 128256, 4096, _lib.EPI_STORE)]
    Ms = [int(a[1:]) for a in sys.argv if a.startswith("m") and a[1:].isdigit()] or [8, 32]
    if "head" in sys.argv:              # `skinny head`: the LM head shape alone, bf16 / fp8 / mxfp4 (generate(lm_head_dtype=))
        shapes = shapes[-1:]
    for M in Ms:
        for name, N, K, epi in shapes:
            copies = max(2, min(40, int(1.3e9 // (N * K * 2)) + 1))
            ws = [rand((N, K), scale=0.02) for _ in range(copies)]
            x = rand((M, K))
            if epi == _lib.EPI_SWIGLU:
                out, ldc, odt = torch.zeros((M, N // 2), dtype=torch.bfloat16, device=dev), N // 2, _lib.BF16
            elif epi == _lib.EPI_STORE:
                out, ldc, odt = torch.zeros((M, N), dtype=torch.bfloat16, device=dev), N, _lib.BF16
            else:
                out, ldc, odt = torch.zeros((M, N), dtype=torch.float32, device=dev), N, _lib.F32
            from p2t_hip.generation import preshuffle
            res = []
            for pre in (0, 1):
                if pre:
                    ws = [preshuffle(w, N) for w in ws]
                i = [0]

                def run():
                    w = ws[i[0] % copies]
                    i[0] += 1
                    _lib.call("p2t_gemm_nt_skinny", ptr(x), K, ptr(w), K, pre, ptr(out), ldc, M, N, K, odt, epi, stream())
                ms = timeit(run, iters=max(20, copies), warm=copies)
                res.append(f"{'stream copy' if pre else 'row-major W'} {ms * 1e3:7.1f} us {N * K * 2 / ms / 1e6:6.0f} GB/s")
            print(f"skinny M={M:2d} {name:8s} N={N:6d} K={K:5d}: " + " | ".join(res), flush=True)
            del ws
            # the same projection on quantised weights: e4m3 + row scales (p2t_gemm_nt_skinny_fp8) and MXFP4 codes + block scales
            # (p2t_gemm_nt_skinny_mxfp4, 4.25 bits per weight), cold weights from a ring of copies as above
            from p2t_hip.generation import preshuffle_mxfp4
            w0 = rand((N, K), scale=0.02)
            a8, sa = ops.quant_rows_fp8(x)
            w8, sw = ops.quant_rows_fp8(w0)
            codes, bs = ops.quant_rows_mxfp4(w0)
            del w0
            for fmt, wbytes in (("fp8", N * K), ("mxfp4", N * K * 17 // 32)):
                copies = max(2, min(40, int(1.3e9 // wbytes) + 1))
                res = []
                for pre in (0, 1):
                    if fmt == "fp8":
                        ring = [(preshuffle(w8, N) if pre else w8.clone(), sw) for _ in range(copies)]
                    else:
                        ring = [(preshuffle_mxfp4(codes, bs, N), None) if pre else (codes.clone(), bs.clone()) for _ in range(copies)]
                    i = [0]

                    def run():
                        w, sc = ring[i[0] % copies]
                        i[0] += 1
                        _lib.call("p2t_gemm_nt_skinny_" + fmt, ptr(a8), K, ptr(sa), ptr(w), K if fmt == "fp8" else K // 2, ptr(sc) if sc is not None else None,
                                  pre, ptr(out), ldc, M, N, K, odt, epi, stream())
                    ms = timeit(run, iters=max(20, copies), warm=copies)
                    res.append(f"{'stream copy' if pre else 'row-major W'} {ms * 1e3:7.1f} us {wbytes / ms / 1e6:6.0f} GB/s")
                    del ring
                print(f"skinny M={M:2d} {name:8s} N={N:6d} K={K:5d} {fmt:5s}: " + " | ".join(res), flush=True)


def bench_attn_decode():
    """The decode step's attention alone at Llama-3.1-8B sizes (8 kv heads x 4 query heads x head_dim 128) over 1088 prompt keys + 33
    generated ones: p2t_attention_decode (bf16 prompt segment) and p2t_attention_decode_prompt_fp8 (e4m3 codes + one scale byte per key)
    in the same loop, alternating, each on a ring of cache copies so that nothing is served from a cache; five rounds, median and range."""
    import numpy as np
    from p2t_hip.ops import ptr, stream
    nh, nkv, d, T, S = 32, 8, 128, 1088, 32
    Tp, G, copies, rounds, n = ops.round_up(T, 64), 64, 24, 5, 96
    for B in [int(a[1:]) for a in sys.argv if a.startswith("m") and a[1:].isdigit()] or [8, 32]:
        kp, vtp = [rand((B, nkv, Tp, d), scale=0.5) for _ in range(copies)], [rand((B, nkv, d, Tp), scale=0.5) for _ in range(copies)]
        kg, vtg, q = rand((B, nkv, G, d), scale=0.5), rand((B, nkv, d, G), scale=0.5), rand((B, nh, d), scale=0.5)
        k8, v8, ks, vs = [], [], [], []
        for c in range(copies):                                   # the same keys and values through the prefill's store
            k8.append(torch.empty((B, nkv, Tp, d), dtype=torch.uint8, device=dev)); v8.append(torch.empty((B, nkv, d, Tp), dtype=torch.uint8, device=dev))
            ks.append(torch.empty((B, nkv, Tp), dtype=torch.uint8, device=dev)); vs.append(torch.empty((B, nkv, Tp), dtype=torch.uint8, device=dev))
            _lib.call("p2t_kv_quant_store", ptr(kp[c]), ptr(vtp[c].transpose(2, 3).contiguous()), B, nkv, Tp, d, Tp, ptr(k8[c]), ptr(v8[c]), ptr(ks[c]),
                      ptr(vs[c]), stream())
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        step = torch.tensor([S], dtype=torch.int32, device=dev)
        out = torch.zeros((B, nh * d), dtype=torch.bfloat16, device=dev)
        i = [0]

        def run(fp8):
            c = i[0] % copies
            i[0] += 1
            if fp8:
                _lib.call("p2t_attention_decode_prompt_fp8", ptr(q), ptr(k8[c]), ptr(v8[c]), ptr(kg), ptr(vtg), ptr(lens), ptr(step), B, 1, nh, nkv, d, Tp, G,
                          1.0, 1, _lib.BF16, 1, ptr(out), nh * d, ptr(ks[c]), ptr(vs[c]), stream())
            else:
                _lib.call("p2t_attention_decode", ptr(q), ptr(kp[c]), ptr(vtp[c]), ptr(kg), ptr(vtg), ptr(lens), ptr(step), B, 1, nh, nkv, d, Tp, G, 1.0, 1,
                          _lib.BF16, 1, ptr(out), nh * d, stream())
        res = {0: [], 1: []}
        for _ in range(rounds):
            for fp8 in (0, 1):
                res[fp8].append(timeit(lambda: run(fp8), iters=n, warm=copies) * 1e3)
        for fp8, name in ((0, "bf16 prompt segment"), (1, "fp8 prompt segment ")):
            nbytes = 2 * B * nkv * ((d * (1 if fp8 else 2) + fp8) * T + 2 * d * (S + 1))         # keys + values (+ one scale byte per key each)
            r = res[fp8]
            print(f"attn_decode B={B:2d} {T}+{S + 1} keys, {name}: median {np.median(r):5.1f} us (min {min(r):.1f}, max {max(r):.1f}; {rounds} rounds of {n}), "
                  f"{nbytes / np.median(r) / 1e3:5.0f} GB/s of cache bytes ({nbytes / 1e6:.1f} MB)", flush=True)


def bench_attn_decode_beams():
    """`attn_decode beams`: the attention of a beam group alone at Llama-3.1-8B sizes, 8 x 4 and 32 x 4 beams over 1088 prompt keys and 33 /
    250 generated ones, bf16 and fp8 prompt segment: p2t_attention_decode[_prompt_fp8] (one block per (row, kv head), the copy path) and
    p2t_attention_decode_beams (one block per (prompt, kv head), identity table) alternating on a ring of cache copies; then
    p2t_kv_reorder against p2t_kv_ancestry_update over 32 layers at both lengths."""
    import ctypes as C
    import numpy as np
    from p2t_hip.ops import ptr, stream
    nh, nkv, d, T, group, L = 32, 8, 128, 1088, 4, 32
    Tp, G, copies, rounds, n = ops.round_up(T, 64), 256, 12, 5, 48
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    for B0 in (8, 32):
        BB = B0 * group
        kp, vtp = [rand((B0, nkv, Tp, d), scale=0.5) for _ in range(copies)], [rand((B0, nkv, d, Tp), scale=0.5) for _ in range(copies)]
        kg, vtg, q = rand((BB, nkv, G, d), scale=0.5), rand((BB, nkv, d, G), scale=0.5), rand((BB, nh, d), scale=0.5)
        k8, v8, ks, vs = [], [], [], []
        for c in range(copies):
            k8.append(u8(B0, nkv, Tp, d)); v8.append(u8(B0, nkv, d, Tp)); ks.append(u8(B0, nkv, Tp)); vs.append(u8(B0, nkv, Tp))
            _lib.call("p2t_kv_quant_store", ptr(kp[c]), ptr(vtp[c].transpose(2, 3).contiguous()), B0, nkv, Tp, d, Tp, ptr(k8[c]), ptr(v8[c]), ptr(ks[c]),
                      ptr(vs[c]), stream())
        lens = torch.full((B0,), T, dtype=torch.int32, device=dev)
        anc = (torch.arange(BB, device=dev) % group).to(torch.uint8)[:, None].repeat(1, G).contiguous()      # every beam its own row's keys
        out = torch.zeros((BB, nh * d), dtype=torch.bfloat16, device=dev)
        for S in (32, 249):
            step = torch.tensor([S], dtype=torch.int32, device=dev)
            i = [0]

            def run(fp8, beams):
                c = i[0] % copies
                i[0] += 1
                a = (ptr(q), ptr(k8[c] if fp8 else kp[c]), ptr(v8[c] if fp8 else vtp[c]), ptr(kg), ptr(vtg), ptr(lens), ptr(step), B0, group, nh, nkv, d, Tp, G,
                     1.0, 1, _lib.BF16, 1, ptr(out), nh * d)
                sc = (ptr(ks[c]), ptr(vs[c])) if fp8 else (None, None)
                if beams:
                    _lib.call("p2t_attention_decode_beams", *a, *sc, ptr(anc), stream())
                elif fp8:
                    _lib.call("p2t_attention_decode_prompt_fp8", *a, *sc, stream())
                else:
                    _lib.call("p2t_attention_decode", *a, stream())
            res = {(f, b): [] for f in (0, 1) for b in (0, 1)}
            for _ in range(rounds):
                for key in res:
                    res[key].append(timeit(lambda: run(*key), iters=n, warm=copies) * 1e3)
            for (f, b), r in res.items():
                print(f"attn_decode {B0:2d} x {group} beams {T}+{S + 1} keys, {'fp8 ' if f else 'bf16'} prompt segment, "
                      f"{'(prompt, kv head) blocks + ancestry table' if b else '(row, kv head) blocks                    '}: median {np.median(r):5.1f} us "
                      f"(min {min(r):.1f}, max {max(r):.1f}; {rounds} rounds of {n})", flush=True)
        del kp, vtp, k8, v8
    # the per-step maintenance: the copy of every layer's generated keys and values against one byte per row and token
    B0, BB = 8, 32
    cfg = _lib.LlamaConfigC(n_layers=L, hidden=4096, ffn=14336, heads=nh, kv_heads=nkv, head_dim=d, vocab=128256, dtype=_lib.BF16)
    bufs = [torch.zeros((L, BB, nkv, G, d), dtype=torch.bfloat16, device=dev) for _ in range(4)]
    lens, step = torch.full((B0,), T, dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    src = (torch.arange(BB, device=dev) // group * group + torch.tensor([1, 1, 0, 2], device=dev).repeat(B0)).to(torch.int64)
    anc = torch.zeros((BB, G), dtype=torch.uint8, device=dev)
    cache = _lib.KvCacheC(k_prompt=bufs[0].data_ptr(), vt_prompt=bufs[0].data_ptr(), k_gen=bufs[0].data_ptr(), vt_gen=bufs[1].data_ptr(),
                          prompt_len=lens.data_ptr(), step=step.data_ptr(), B0=B0, group=group, Tp=Tp, G=G)
    for S in (30, 250):
        step.fill_(S)
        t_copy = timeit(lambda: _lib.call("p2t_kv_reorder", C.byref(cfg), C.byref(cache), ptr(src), ptr(bufs[2]), ptr(bufs[3]), stream()), iters=20) * 1e3
        t_tab = timeit(lambda: _lib.call("p2t_kv_ancestry_update", C.byref(cache), ptr(src), ptr(anc), stream()), iters=20) * 1e3
        print(f"beam maintenance at {S} generated tokens, {BB} rows x {L} layers: p2t_kv_reorder {t_copy:.1f} us, p2t_kv_ancestry_update {t_tab:.1f} us", flush=True)


def bench_attn_decode_multi():
    """`attn_decode multi`: p2t_attention_decode_multi alone at Llama-3.1-8B sizes (8 kv heads x 4 query heads x head_dim 128: 4 queries per
    block) over 1088 prompt keys + 65 .. generated ones, next to Q launches of p2t_attention_decode_rows on the same cache with the counters
    at s + j (what Q one-token steps run) and to ONE such launch (what a one-token step runs), alternating on a ring of cache copies."""
    import numpy as np
    from p2t_hip.ops import ptr, stream
    nh, nkv, d, T, S = 32, 8, 128, 1088, 64
    Tp, G, copies, rounds, n = ops.round_up(T, 64), 128, 24, 5, 48
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    for B in (1, 2, 4, 8):
        kp, vtp = [rand((B, nkv, Tp, d), scale=0.5) for _ in range(copies)], [rand((B, nkv, d, Tp), scale=0.5) for _ in range(copies)]
        k8, v8, ks, vs = [], [], [], []
        for c in range(copies):
            k8.append(u8(B, nkv, Tp, d)); v8.append(u8(B, nkv, d, Tp)); ks.append(u8(B, nkv, Tp)); vs.append(u8(B, nkv, Tp))
            _lib.call("p2t_kv_quant_store", ptr(kp[c]), ptr(vtp[c].transpose(2, 3).contiguous()), B, nkv, Tp, d, Tp, ptr(k8[c]), ptr(v8[c]), ptr(ks[c]),
                      ptr(vs[c]), stream())
        kg, vtg = rand((B, nkv, G, d), scale=0.5), rand((B, nkv, d, G), scale=0.5)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        for Q in (2, 4, 8):
            q, out = rand((B * Q, nh, d), scale=0.5), torch.zeros((B * Q, nh * d), dtype=torch.bfloat16, device=dev)
            steps = [torch.full((B,), S + j, dtype=torch.int32, device=dev) for j in range(Q)]
            qj = [q.view(B, Q, nh, d)[:, j].contiguous() for j in range(Q)]
            i = [0]

            def run(fp8, what):
                c = i[0] % copies
                i[0] += 1
                seg = (ptr(k8[c] if fp8 else kp[c]), ptr(v8[c] if fp8 else vtp[c]), ptr(kg), ptr(vtg), ptr(lens))
                sc = (ptr(ks[c]), ptr(vs[c])) if fp8 else (None, None)
                tail = (B, nh, nkv, d, Tp, G, 1.0, 1, _lib.BF16, 1)
                if what == "multi":
                    _lib.call("p2t_attention_decode_multi", ptr(q), *seg, ptr(steps[0]), *tail, ptr(out), nh * d, *sc, Q, stream())
                else:
                    for j in range(Q if what == "rows x Q" else 1):
                        _lib.call("p2t_attention_decode_rows", ptr(qj[j]), *seg, ptr(steps[j]), *tail, ptr(out), nh * d, *sc, stream())
            res = {(f, w): [] for f in (0, 1) for w in ("multi", "rows x Q", "rows x 1")}
            for _ in range(rounds):
                for key in res:
                    res[key].append(timeit(lambda: run(*key), iters=n, warm=copies) * 1e3)
            for (f, w), r in res.items():
                print(f"attn_decode multi B={B} Q={Q} {T}+{S + 1}..{S + Q} keys, {'fp8 ' if f else 'bf16'} prompt segment, "
                      f"{dict(multi='p2t_attention_decode_multi     ', **{'rows x Q': 'Q x p2t_attention_decode_rows  ', 'rows x 1': 'one p2t_attention_decode_rows  '})[w]}: "
                      f"median {np.median(r):5.1f} us (min {min(r):.1f}, max {max(r):.1f}; {rounds} rounds of {n})", flush=True)
        del kp, vtp, k8, v8


def bench_choice_rows():
    """p2t_sample_select / p2t_sample_select_rows (top_k 50, top_p 0.9, temperature 0.7) and p2t_logits_process / p2t_logits_process_rows
    (every stage on, 64 history tokens) on randn * 3 bf16 logits [rows, 128256] at pitch 128320, alternating, five rounds of 200 launches,
    median and range; `finished`: 0 or every second row (the lock-step processors take no finished array: they process every row)."""
    import numpy as np
    from p2t_hip.ops import ptr, stream
    V, G, hist, rounds, n = 128256, 256, 64, 5, 200
    ld = ops.round_up(V, 64)
    gen = torch.Generator(device=dev).manual_seed(0)
    for B in [int(a[1:]) for a in sys.argv if a.startswith("m") and a[1:].isdigit()] or [8, 32]:
        lg = (torch.randn((B, ld), device=dev, generator=gen) * 3).to(torch.bfloat16)
        out_tokens = torch.randint(0, 1000, (B, G), device=dev, generator=gen)
        nxt, flags = torch.zeros((B,), dtype=torch.int64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
        step, row_step = torch.full((1,), hist, dtype=torch.int32, device=dev), torch.full((B,), hist, dtype=torch.int32, device=dev)
        row_limit, row_key = torch.full((B,), G, dtype=torch.int32, device=dev), torch.arange(B, device=dev)
        processed = torch.zeros((B, ld), dtype=torch.float32, device=dev)
        eos = torch.tensor([128001, 128009], dtype=torch.int64, device=dev)
        words = [[11, 12], [13, 14, 15], [16]] * 8 + [[t] for t in range(100, 132)]
        word_ids = torch.tensor([t for w in words for t in w], dtype=torch.int64, device=dev)
        offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(w) for w in words])]), dtype=torch.int32, device=dev)
        proc = (1.3, 3, G, ptr(eos), 2, ptr(word_ids), ptr(offsets), len(words), word_ids.numel())
        for half in (False, True):
            fin = torch.zeros((B,), dtype=torch.int32, device=dev)
            if half:
                fin[1::2] = 2
            kernels = {
                "p2t_sample_select      ": lambda: _lib.call("p2t_sample_select", ptr(lg), _lib.BF16, ld, V, B, None, 0, 0, ptr(fin), ptr(nxt), ptr(out_tokens), G,
                                                             ptr(step), G, 0.7, 50, 0.9, 1, 0, None, 0, ptr(flags), stream()),
                "p2t_sample_select_rows ": lambda: _lib.call("p2t_sample_select_rows", ptr(lg), _lib.BF16, ld, V, B, None, 0, 0, ptr(fin), ptr(nxt),
                                                             ptr(out_tokens), G, ptr(row_step), ptr(row_limit), None, ptr(row_key), B, G, 0.7, 50, 0.9, 1, None, 0,
                                                             ptr(flags), stream()),
                "p2t_logits_process     ": lambda: _lib.call("p2t_logits_process", ptr(lg), _lib.BF16, ld, V, B, ptr(out_tokens), G, ptr(step), G, ptr(processed), ld,
                                                             *proc, stream()),
                "p2t_logits_process_rows": lambda: _lib.call("p2t_logits_process_rows", ptr(lg), _lib.BF16, ld, V, B, ptr(out_tokens), G, ptr(row_step), None,
                                                             ptr(fin), B, G, ptr(processed), ld, *proc, stream())}
            res = {k: [] for k in kernels}
            for _ in range(rounds):
                for k, go in kernels.items():
                    res[k].append(timeit(go, iters=n, warm=10) * 1e3)
            for k, r in res.items():
                print(f"choice_rows rows={B:2d} [{B}, {V}] bf16, {hist} history tokens, {B // 2 if half else 0:2d} rows finished, {k}: median {np.median(r):6.1f} us "
                      f"(min {min(r):.1f}, max {max(r):.1f}; {rounds} rounds of {n})", flush=True)


def bench_kv_store():
    """The prefill's store of ONE layer's keys and values at cfg3 shape (8 kv heads, head_dim 128), 8 and 32 prompts of bench.py's ragged
    lengths (+ 64 chat tokens): p2t_kv_store_packed from one packed row, bf16 and into the fp8 prompt segment, next to p2t_kv_quant_store on
    the padded batch (the padded path's fp8 store; its bf16 pair -- a 2-D copy + a transpose kernel -- has no entry point of its own and is
    not timed alone).  Bytes: what a store must read and write for the VALID keys."""
    import ctypes as C
    import numpy as np
    from p2t_hip import generation
    from p2t_hip.ops import ptr, stream
    nkv, d, L = 8, 128, 1
    for B in [int(a[1:]) for a in sys.argv if a.startswith("m") and a[1:].isdigit()] or [8, 32]:
        lens = (np.clip(np.round(np.random.RandomState(0).lognormal(5.75, 0.6, B)), 16, 1024).astype(int) + 64).tolist()
        T, Tp = max(lens), ops.round_up(max(lens), 64)
        R, Tpk, place = generation.plan_prompt_rows(lens)
        c_place = (C.c_int32 * (3 * B))(*[v for p in place for v in p])
        cfg = _lib.LlamaConfigC(n_layers=L, hidden=4096, ffn=14336, heads=32, kv_heads=nkv, head_dim=d, vocab=128256, dtype=_lib.BF16, rms_norm_eps=1e-5,
                                rope_theta=5e5)
        k, v = rand((R, nkv, Tpk, d)), rand((R, nkv, Tpk, d))
        kpad, vpad = rand((B, nkv, T, d)), rand((B, nkv, T, d))
        gen, cnt = torch.zeros((64,), device=dev), torch.zeros((B + 1,), dtype=torch.int32, device=dev)
        z = lambda dt, *s: torch.zeros(s, dtype=dt, device=dev)
        kp, vtp = z(torch.bfloat16, L, B, nkv, Tp, d), z(torch.bfloat16, L, B, nkv, d, Tp)
        kq, vtq, ks, vs = z(torch.uint8, L, B, nkv, Tp, d), z(torch.uint8, L, B, nkv, d, Tp), z(torch.uint8, L, B, nkv, Tp), z(torch.uint8, L, B, nkv, Tp)
        base = dict(k_gen=gen.data_ptr(), vt_gen=gen.data_ptr(), prompt_len=cnt.data_ptr(), step=cnt[B:].data_ptr(), B0=B, group=1, Tp=Tp, G=64)
        c16 = _lib.KvCacheC(k_prompt=kp.data_ptr(), vt_prompt=vtp.data_ptr(), **base)
        c8 = _lib.KvCacheC(k_prompt=kq.data_ptr(), vt_prompt=vtq.data_ptr(), k_prompt_scale=ks.data_ptr(), v_prompt_scale=vs.data_ptr(), **base)
        packed = lambda cache: _lib.call("p2t_kv_store_packed", C.byref(cfg), C.byref(cache), 0, ptr(k), ptr(v), R, Tpk, c_place, B, stream())
        runs = {"p2t_kv_store_packed, bf16": (lambda: packed(c16), 8.0),
                "p2t_kv_store_packed, fp8 prompt segment": (lambda: packed(c8), 6.0),
                f"p2t_kv_quant_store, padded {B} x {T} (fp8 prompt segment)": (
                    lambda: _lib.call("p2t_kv_quant_store", ptr(kpad), ptr(vpad), B, nkv, T, d, Tp, ptr(kq), ptr(vtq), ptr(ks), ptr(vs), stream()), 6.0)}
        res = {n: [] for n in runs}
        for _ in range(5):
            for n, (go, _) in runs.items():
                res[n].append(timeit(go, iters=50, warm=5) * 1e3)
        valid = sum(lens)
        for n, r in res.items():
            gb = runs[n][1] * valid * nkv * d / 1e9
            print(f"kv_store prompts={B:2d} ({valid} valid keys x {nkv} kv heads x {d}, one layer; {R} packed row(s) of {Tpk}), {n}: median {np.median(r):6.1f} us "
                  f"(min {min(r):.1f}, max {max(r):.1f}; 5 rounds of 50) = {gb / np.median(r) * 1e6 / 1e3:.2f} TB/s of valid-key traffic", flush=True)


def bench_fp8abl():
    """Lab ablations of the fp8 K loop (per-tile kernel, garbage results; lab build only): full / no DMA / no fragment reloads / neither."""
    for name, M, N, K in (("esm qkv b64", 65536, 7680, 2560), ("esm fc2 b64", 65536, 2560, 10240), ("square 8k", 8192, 8192, 8192)):
        a, w = rand((M, K)), rand((N, K), scale=0.05)
        a8, sa = ops.quant_rows_fp8(a)
        w8, sw = ops.quant_rows_fp8(w)
        fl = 2.0 * M * N * K / 1e9
        res = [timeit(lambda t=t: ops.gemm_nt_fp8(a8, sa, w8, sw, None, n=N, k=K, epilogue=0, tile=t), iters=5, warm=2) for t in (256, 1001, 1002, 1003)]
        print(f"fp8abl {name:12s}: full {fl / res[0]:7.1f} TF/s | no DMA {fl / res[1]:7.1f} | no LDS reads {fl / res[2]:7.1f} | neither {fl / res[3]:7.1f}", flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["gemm", "attn", "norm"]
    print(torch.cuda.get_device_name(0), flush=True)
    if "gemm" in which:
        bench_gemm()
    if "cold" in which:
        bench_cold()
    if "ksweep" in which:
        bench_ksweep()
    if "attn" in which:
        bench_attn()
    if "norm" in which:
        bench_norm()
    if "blas" in which:
        bench_blas()
    if "fp8" in which:
        bench_fp8()
    if "skinny" in which:
        bench_skinny()
    if "kv_store" in which:
        bench_kv_store()
    if "attn_decode" in which and "multi" in which:
        bench_attn_decode_multi()
    elif "attn_decode" in which and "beams" in which:
        bench_attn_decode_beams()
    elif "attn_decode" in which:
        bench_attn_decode()
    if "choice_rows" in which:
        bench_choice_rows()
    if "fp8abl" in which:
        bench_fp8abl()
