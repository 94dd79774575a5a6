"""The GEMM launch policy without a GPU: the lab build's p2t_lab_gemm_plan returns the plan (kernel form, grid, whole tiles,
split-K / 128-row-half tail tiles) that p2t_gemm_nt / p2t_gemm_nt_fp8 would launch, from pure host code.  The rows below pin the
forms on 256 CUs with the towers' full split-K fix-up workspace: every GEMM of a cfg3 step (batch 16 and 64), bf16 under the
default policy and under policy 9 (no four-wave kernels), fp8 at tile 0, and each forced lab policy on the shapes of
lab_forms_cases.py::test_gemm_mfma_splitk_tail, and every case of tests/test_gpu_gemm_forms.py (gemm_forms_cases.py).  The lab
library is loaded in a child process, so this process never maps it."""
import json
import os
import subprocess
import sys

from gemm_forms_cases import CASES as FORMS_CASES, case_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB = os.path.join(ROOT, "tools", "build", "libp2t_lab.so")

F32, BF16, FP8 = 0, 1, 2
STORE, GELU, RESID, SWIGLU, QKV_ROPE, GELU_FP8 = 0, 1, 2, 3, 6, 7
FORMS = ["none", "tile128", "tile256", "splitk", "persist", "w4_tile", "w4_persist", "w4_pairs", "k64", "fp8_tile128", "fp8_tile256", "fp8_w4"]
CUS = 256
FIX_BYTES = 2048 + 128 * 256 * 256 * 4          # p2t_gemm_fix_workspace_bytes()

# name, N, K, bf16 (epilogue, out dtype), fp8 (epilogue, out dtype)
ESM = [("esm qkv", 7680, 2560, (QKV_ROPE, BF16), (QKV_ROPE, BF16)), ("esm o", 2560, 2560, (RESID, F32), (RESID, F32)),
       ("esm fc1", 10240, 2560, (GELU, BF16), (GELU_FP8, BF16)), ("esm fc2", 2560, 10240, (RESID, F32), (RESID, F32))]
TEXT = [("text qkv", 6144, 4096, (QKV_ROPE, BF16), (QKV_ROPE, BF16)), ("text o", 4096, 4096, (RESID, F32), (RESID, F32)),
        ("text gate-up", 28672, 4096, (SWIGLU, BF16), (SWIGLU, BF16)), ("text down", 4096, 14336, (RESID, F32), (RESID, F32))]
STEP = [(name, 16384, N, K, b, f) for name, N, K, b, f in ESM] + [(name, 65536, N, K, b, f) for name, N, K, b, f in ESM] + \
       [(name, 2048, N, K, b, f) for name, N, K, b, f in TEXT]

# (name, M) -> (policy 0, policy 9, fp8 tile 0); a row is (form, grid, n_full, n_tail, half_tail)
STEP_PLANS = {
    ("esm qkv", 16384): (("w4_persist", 256, 1920, 0, 0), ("persist", 256, 1792, 128, 1), ("fp8_w4", 256, 1920, 0, 0)),
    ("esm o", 16384): (("w4_persist", 256, 640, 0, 0), ("persist", 256, 512, 128, 1), ("fp8_w4", 256, 640, 0, 0)),
    ("esm fc1", 16384): (("w4_persist", 256, 2560, 0, 0), ("persist", 256, 2560, 0, 0), ("fp8_w4", 256, 2560, 0, 0)),
    ("esm fc2", 16384): (("w4_persist", 256, 512, 128, 0), ("persist", 256, 512, 128, 0), ("fp8_w4", 256, 640, 0, 0)),
    ("esm qkv", 65536): (("w4_persist", 256, 7680, 0, 0), ("persist", 256, 7680, 0, 0), ("fp8_w4", 256, 7680, 0, 0)),
    ("esm o", 65536): (("w4_persist", 256, 2560, 0, 0), ("persist", 256, 2560, 0, 0), ("fp8_w4", 256, 2560, 0, 0)),
    ("esm fc1", 65536): (("w4_persist", 256, 10240, 0, 0), ("persist", 256, 10240, 0, 0), ("fp8_w4", 256, 10240, 0, 0)),
    ("esm fc2", 65536): (("w4_persist", 256, 2560, 0, 0), ("persist", 256, 2560, 0, 0), ("fp8_w4", 256, 2560, 0, 0)),
    ("text qkv", 2048): (("w4_tile", 192, 192, 0, 0), ("tile256", 192, 192, 0, 0), ("fp8_tile256", 192, 192, 0, 0)),
    ("text o", 2048): (("tile128", 256, 256, 0, 0), ("tile128", 256, 256, 0, 0), ("fp8_tile128", 256, 256, 0, 0)),
    ("text gate-up", 2048): (("w4_persist", 256, 896, 0, 0), ("persist", 256, 768, 128, 1), ("fp8_w4", 256, 896, 0, 0)),
    ("text down", 2048): (("w4_pairs", 256, 0, 128, 0), ("splitk", 256, 0, 128, 0), ("fp8_tile128", 256, 256, 0, 0)),
}

# forced lab policies on the split-K tail shapes (the same plan for the bf16 store and the fp32 residual epilogue)
FORCED_POLICIES = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 128, 256)
FORCED_PLANS = {
    (16384, 2560, 4096): (("tile256", 640, 640, 0, 0), ("splitk", 768, 512, 128, 0), ("persist", 256, 512, 128, 0), ("persist", 256, 640, 0, 0),
                          ("persist", 256, 512, 128, 1), ("k64", 640, 640, 0, 0), ("w4_tile", 640, 640, 0, 0), ("w4_persist", 256, 512, 128, 0),
                          ("w4_persist", 256, 640, 0, 0), ("w4_persist", 256, 640, 0, 0), ("tile128", 1280, 1280, 0, 0), ("tile256", 640, 640, 0, 0)),
    (4096, 5376, 4096): (("tile256", 336, 336, 0, 0), ("splitk", 416, 256, 80, 0), ("persist", 256, 256, 80, 0), ("persist", 256, 336, 0, 0),
                         ("persist", 256, 256, 80, 1), ("k64", 336, 336, 0, 0), ("w4_tile", 336, 336, 0, 0), ("w4_persist", 256, 256, 80, 0),
                         ("w4_persist", 256, 336, 0, 0), ("w4_persist", 256, 336, 0, 0), ("tile128", 672, 672, 0, 0), ("tile256", 336, 336, 0, 0)),
    (2048, 4096, 8192): (("tile128", 256, 256, 0, 0), ("splitk", 256, 0, 128, 0), ("splitk", 256, 0, 128, 0), ("splitk", 256, 0, 128, 0),
                         ("splitk", 256, 0, 128, 0), ("k64", 128, 128, 0, 0), ("w4_tile", 128, 128, 0, 0), ("splitk", 256, 0, 128, 0),
                         ("splitk", 256, 0, 128, 0), ("splitk", 256, 0, 128, 0), ("tile128", 256, 256, 0, 0), ("tile256", 128, 128, 0, 0)),
}

CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.p2t_lab_gemm_plan.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 6 + [ctypes.c_int] * 4 + [ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64)]
lib.p2t_is_lab_build.restype = ctypes.c_int
assert lib.p2t_is_lab_build() == 1
plans = []
for q in json.loads(sys.stdin.read()):
    out = (ctypes.c_int64 * 5)()
    rc = lib.p2t_lab_gemm_plan(*q, out)
    plans.append([rc] + list(out))
print(json.dumps(plans))
"""


def _plans(queries):
    """queries: (dtype, M, N, K, n_cover, lda, ldw, epilogue, out_dtype, policy, cus, fix_bytes) -> [(form, grid, n_full, n_tail, half_tail)]"""
    assert os.path.exists(LAB), f"{LAB} missing: __graft_entry__.build() / `make -C prot2text-v2-esm3_amd/csrc lab` builds it"
    r = subprocess.run([sys.executable, "-c", CHILD, LAB], input=json.dumps(queries), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(rc == 0 for rc, *_ in res), res
    return [(FORMS[f],) + tuple(rest) for _, f, *rest in res]


def test_cfg3_step_plans():
    queries, expect = [], []
    for name, M, N, K, (e16, o16), (e8, o8) in STEP:
        p0, p9, f8 = STEP_PLANS[(name, M)]
        queries += [(BF16, M, N, K, N, K, K, e16, o16, 0, CUS, FIX_BYTES), (BF16, M, N, K, N, K, K, e16, o16, 9, CUS, FIX_BYTES),
                    (FP8, M, N, K, N, K, K, e8, o8, 0, CUS, 0)]
        expect += [(name, M, "policy 0", p0), (name, M, "policy 9", p9), (name, M, "fp8", f8)]
    got = _plans(queries)
    assert got == [e[3] for e in expect], [(e[:3], e[3], g) for e, g in zip(expect, got) if e[3] != g]


def test_forced_policy_plans():
    queries, expect = [], []
    for (M, N, K), rows in FORCED_PLANS.items():
        for epi, od in ((STORE, BF16), (RESID, F32)):
            for policy, row in zip(FORCED_POLICIES, rows):
                queries.append((BF16, M, N, K, N, K, K, epi, od, policy, CUS, FIX_BYTES))
                expect.append(((M, N, K), epi, policy, row))
    got = _plans(queries)
    assert got == [e[3] for e in expect], [(e[:3], e[3], g) for e, g in zip(expect, got) if e[3] != g]


def test_plan_without_fixup_workspace():
    """No workspace: the split-K forms give way (FFN-down of the text tower: 128-row tiles; ESM fc2: 128-row halves on the
    eight-wave kernel, whole tiles on the four-wave one)."""
    got = _plans([(BF16, 2048, 4096, 14336, 4096, 14336, 14336, RESID, F32, 0, CUS, 0),
                  (BF16, 16384, 2560, 10240, 2560, 10240, 10240, RESID, F32, 9, CUS, 0),
                  (BF16, 16384, 2560, 10240, 2560, 10240, 10240, RESID, F32, 0, CUS, 0)])
    assert got == [("tile128", 256, 256, 0, 0), ("persist", 256, 512, 128, 1), ("w4_persist", 256, 640, 0, 0)]


def test_gemm_forms_case_plans():
    """Every (shape, epilogue, out dtype) of tests/test_gpu_gemm_forms.py plans to the form its case names, under the default policy and
    under policy 9: a policy change that moves a shape off its form fails here instead of hollowing out the GPU test."""
    queries, expect = [], []
    for c in FORMS_CASES:
        for policy, row in ((0, c.p0), (9, c.p9)):
            queries.append((BF16, c.M, c.N, c.K, c.N, c.K, c.K, c.code, c.out, policy, CUS, FIX_BYTES))
            expect.append((case_id(c), policy, row))
        assert c.p0[0] == {"w4_persist_pairs": "w4_persist"}.get(c.form, c.form), c
    got = _plans(queries)
    assert got == [e[2] for e in expect], [(e[:2], e[2], g) for e, g in zip(expect, got) if e[2] != g]
    # every four-wave form, with and without in-stream pairs and with a partial round of whole tiles, is in the table
    assert {(c.p0[0], c.p0[3] > 0, c.p0[2] % CUS != 0) for c in FORMS_CASES} >= {("w4_persist", False, False), ("w4_persist", False, True),
                                                                                ("w4_persist", True, False), ("w4_tile", False, True), ("w4_pairs", True, False)}
