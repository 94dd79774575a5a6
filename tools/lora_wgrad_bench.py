"""dA / dB of one LoRA target at the seven decoder shapes of cfg3 (Llama-3.1-8B, 4 x 1 216 tokens, r = 16, dropout 0.1), two routes:

    transposes   LoraLinear._wgrad_transposed: the dropped copy of x, four p2t_transpose, two p2t_gemm_nt over the padded token axis
    token axis   two p2t_lora_wgrad calls on the activations as they lie

HIP events, the routes alternating, `rounds` rounds of `reps` calls each: median and min .. max of the per-round means.
python tools/lora_wgrad_bench.py [rounds] > profiles/<name>.log"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prot2text-v2-esm3_amd"))
from p2t_hip import ops                                          # noqa: E402
from p2t_hip.lora_linear import LoraLinear                       # noqa: E402

M, R, P_DROP = 4 * 1216, 16, 0.1
SHAPES = [("q_proj", 4096, 4096), ("k_proj", 1024, 4096), ("v_proj", 1024, 4096), ("o_proj", 4096, 4096), ("gate_proj", 14336, 4096),
          ("up_proj", 14336, 4096), ("down_proj", 4096, 14336)]   # (target, N = out, K = in)


def main():
    rounds, reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5, 10
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: (torch.randn(s, generator=g) * 0.3).to(dev, torch.bfloat16)
    print(f"LoRA weight gradients, M = {M} tokens, r = {R}, dropout {P_DROP}, bf16; ms per (dA, dB) pair, median [min .. max] of {rounds} rounds x {reps}")
    for name, N, K in SHAPES:
        lin = LoraLinear.__new__(LoraLinear)
        lin.N, lin.K, lin.r, lin.rp, lin.p, lin.seed, lin.dt = N, K, R, R, P_DROP, 12345, torch.bfloat16
        dy, x, u, du = rnd(M, N), rnd(M, K), rnd(M, 64), rnd(M, 64)
        routes = {"transposes": lambda: lin._wgrad_transposed(dy, x, u, du),
                  "token axis": lambda: (ops.lora_wgrad(x, du, c=K, r=R, transposed=True, p=P_DROP, seed=lin.seed), ops.lora_wgrad(dy, u, c=N, r=R))}
        dA0, dB0 = routes["transposes"]()
        dA1, dB1 = routes["token axis"]()
        err = max(float((dA1 - dA0).norm() / dA0.norm()), float((dB1 - dB0).norm() / dB0.norm()))
        ms = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / reps)
        med = lambda v: sorted(v)[len(v) // 2]
        a, b = ms["transposes"], ms["token axis"]
        print(f"{name:>10} N {N:>5} K {K:>5}: transposes {med(a):.3f} [{min(a):.3f} .. {max(a):.3f}]  token axis {med(b):.3f} [{min(b):.3f} .. {max(b):.3f}]  "
              f"= {med(a) / med(b):.2f}x; routes differ by {err:.1e}", flush=True)


if __name__ == "__main__":
    main()
