"""Stage-2 trainer (p2t_hip/instruct.py) and its flat clip + AdamW step (p2t_clip_adamw_flat, csrc/optim.hip) on the GPU:
the kernel against torch's clip_grad_norm_ + AdamW, the trainer against a torch twin on the LoRA golden cases
(tests/golden/sft_lora_tiny.npz), eval loss without dropout, GEMM-operand reuse, checkpoint resume, two ranks, the epoch loop."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import p2t_hip as P
from gpu_util import build_model, dev, to_dev
from p2t_hip import instruct, specs, synth
from p2t_hip.training_state import CosineWarmupSchedule

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(HERE, "golden", "sft_lora_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


def _model(g, case, dtype, dropout=0.0):
    """The golden case's model with LoRA (the matrices from the golden's seed, B != 0), adapter trainable, eval mode."""
    meta = g["meta"]
    m = meta["cases"][case]
    model = build_model(specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"]), dtype, 0)
    model.config.placeholder_id = meta["placeholder_id"]
    model.eval()
    model.requires_grad_(False)
    lora = model.add_lora(meta["r"], meta["alpha"], dropout, meta["targets"])
    P_ = dict(model.llama_decoder.model.named_parameters())
    with torch.no_grad():
        for i in range(model.llama_decoder.spec.num_hidden_layers):
            for t in meta["targets"]:
                a, b = lora.get(i, t)
                w = P_[f"layers.{i}.{t}.weight"]
                a.copy_(to_dev(synth.uniform_f32(meta["lora_seed"], f"lora.{i}.{t}.A", (meta["r"], w.shape[1]), 0.25)))
                b.copy_(to_dev(synth.uniform_f32(meta["lora_seed"], f"lora.{i}.{t}.B", (w.shape[0], meta["r"]), 0.25)))
    model.adapter.requires_grad_(True)
    return model, lora


def _batch(g, rows=None):
    sl = slice(None) if rows is None else rows
    f = lambda k: to_dev(np.ascontiguousarray(g[k][sl]))
    return dict(input_ids=f("input_ids"), attention_mask=f("attention_mask"), labels=f("labels"),
                protein_input_ids=f("protein_input_ids"), protein_attention_mask=f("protein_attention_mask"))


def _flip(b):
    return {k: v.flip(0).contiguous() for k, v in b.items()}


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the flat kernel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 0.05])
def test_flat_step_matches_torch_clip_and_adamw(max_norm):
    rs = np.random.RandomState(1)
    sizes = [int(v) for v in rs.randint(1, 3000, size=500)]
    sizes[:4] = [16 * 200, 4 * 64, 7 * 33, 5000 * 3 + 1]                     # a16-like, bs16-like, odd, > one chunk
    shapes = [(s,) for s in sizes]
    shapes[0], shapes[1], shapes[2], shapes[3] = (16, 200), (64, 4), (7, 33), (1, 15001)
    d = dev()
    sentinel = 7.0
    # shadows: A as a16 [rp, K8] bf16, (alpha / r) B as bs16 [N, 64] bf16, an adapter-like w copy [rows, round_up(cols, 64)] f32,
    # a bf16 matrix with odd columns (the scalar path)
    sh = [torch.full((16, 200), sentinel, dtype=torch.bfloat16, device=d), torch.full((64, 64), sentinel, dtype=torch.bfloat16, device=d),
          torch.full((9, 64), sentinel, dtype=torch.float32, device=d), torch.full((1, 15008), sentinel, dtype=torch.bfloat16, device=d)]
    shadows = [(sh[0], 16, 200, 1.0), (sh[1], 64, 4, 2.0), (sh[2], 7, 33, 1.0), (sh[3], 1, 15001, 0.5)] + [None] * (len(sizes) - 4)
    runs = []
    for _ in range(2):
        opt = instruct.FlatAdamW(sizes, d, shadows)
        init = [torch.from_numpy(rs_i.standard_normal(s).astype(np.float32)).to(d) for rs_i, s in
                zip([np.random.RandomState(10 + k) for k in range(len(sizes))], sizes)]
        for k, t in enumerate(init):
            opt.view(opt.flat_p, k).copy_(t)
        runs.append(opt)
    ref = [torch.nn.Parameter(opt.view(opt.flat_p, k).clone().view(shapes[k])) for k in range(len(sizes))]
    topt = torch.optim.AdamW(ref, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
    gnorms = [[], []]
    for step in range(1, 6):
        lr = 1e-3 * (1.0 - 0.15 * step)
        gs = [torch.from_numpy(np.random.RandomState(100 * step + k).standard_normal(s).astype(np.float32) * (0.01 + k % 7)).to(d)
              for k, s in enumerate(sizes)]
        for j, opt in enumerate(runs):
            for k, t in enumerate(gs):
                opt.view(opt.flat_g, k).copy_(t)
            opt.step(step, lr=lr, eps=1e-6, weight_decay=0.01, max_norm=max_norm)
            gnorms[j].append(opt.grad_norm.clone())
        for q, t in zip(ref, gs):
            q.grad = t.view(q.shape).clone()
        tn = torch.nn.utils.clip_grad_norm_(ref, max_norm=float("inf") if max_norm is None else max_norm)
        for pg in topt.param_groups:
            pg["lr"] = lr
        topt.step()
        assert abs(float(gnorms[0][-1]) - float(tn)) <= 1e-5 * float(tn)
    opt = runs[0]
    got_p = torch.cat([opt.view(opt.flat_p, k) for k in range(len(sizes))])
    got_m = torch.cat([opt.view(opt.flat_m, k) for k in range(len(sizes))])
    got_v = torch.cat([opt.view(opt.flat_v, k) for k in range(len(sizes))])
    st = topt.state
    assert _rel(got_p, torch.cat([q.detach().reshape(-1) for q in ref])) <= 1e-6
    assert _rel(got_m, torch.cat([st[q]["exp_avg"].reshape(-1) for q in ref])) <= 1e-6
    assert _rel(got_v, torch.cat([st[q]["exp_avg_sq"].reshape(-1) for q in ref])) <= 1e-6
    # padding of the flat buffers is never written
    mask = torch.ones(opt.total, dtype=torch.bool, device=d)
    for k in range(len(sizes)):
        mask[int(opt.offsets[k]): int(opt.offsets[k]) + sizes[k]] = False
    for flat in (opt.flat_p, opt.flat_m, opt.flat_v):
        assert int(torch.count_nonzero(flat[mask])) == 0
    # shadows: RNE(scale * p) bit for bit, padding untouched
    for k, (t, rows, cols, scale) in enumerate(shadows[:4]):
        want = (opt.view(opt.flat_p, k).view(rows, cols) * scale).to(t.dtype)
        assert torch.equal(t[:rows, :cols].view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32),
                           want.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)), k
        pad = torch.ones_like(t, dtype=torch.bool)
        pad[:rows, :cols] = False
        assert bool((t[pad] == sentinel).all()), k
    # the norm is bit-identical from run to run
    for a, b in zip(*gnorms):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_flat_step_handles_more_than_64k_segments():
    sizes = [1 + (k % 5) for k in range(70000)]
    opt = instruct.FlatAdamW(sizes, dev())
    opt.flat_g.normal_()
    mask = torch.zeros(opt.total, dtype=torch.bool, device=dev())
    idx = np.concatenate([np.arange(o, o + n) for o, n in zip(opt.offsets, sizes)])
    mask[torch.from_numpy(idx).to(dev())] = True
    opt.flat_g[~mask] = 0.0
    g = opt.flat_g[mask].clone()
    opt.step(1, lr=1e-2, weight_decay=0.0)
    # step 1 of Adam moves every element by lr * g / (|g| + eps') ~ lr * sign(g)
    moved = opt.flat_p[mask]
    assert bool(((moved * g) <= 0).all()) and float(moved.abs().max()) <= 1e-2 * 1.001
    assert int(torch.count_nonzero(opt.flat_p[~mask])) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the trainer against torch's AdamW on a twin model (fp32)
# ------------------------------------------------------------------------------------------------------------------------------
def _trained(model, lora):
    out = []
    for i in range(model.llama_decoder.spec.num_hidden_layers):
        for t in lora.targets:
            out += list(lora.get(i, t))
    ad = model.adapter
    return out + [ad.fc1.weight, ad.fc1.bias, ad.fc2.weight, ad.fc2.bias]


@pytest.mark.parametrize("case", ["d16", "d64"])
def test_trainer_matches_torch_adamw_fp32(g, case):
    model, lora = _model(g, case, torch.float32)
    tw, tw_lora = _model(g, case, torch.float32)
    sched = CosineWarmupSchedule(2e-3, 1, 4)
    tr = P.InstructTrainer(model, lr=2e-3, max_norm=1.0, gradient_accumulation_steps=2, schedule=sched)
    lo, hi = tr.flat_g.data_ptr(), tr.flat_g.data_ptr() + tr.flat_g.numel() * 4
    p_lo, p_hi = tr.flat_p.data_ptr(), tr.flat_p.data_ptr() + tr.flat_p.numel() * 4
    for q in lora.parameters():
        assert lo <= q.grad.data_ptr() < hi and p_lo <= q.data_ptr() < p_hi
    params = _trained(tw, tw_lora)
    topt = torch.optim.AdamW(params, lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
    tsched = torch.optim.lr_scheduler.LambdaLR(topt, lambda s: CosineWarmupSchedule(2e-3, 1, 4).factor(s))
    batches = [_batch(g), _flip(_batch(g))]
    for step in range(4):
        for micro in range(2):
            b = batches[micro]
            l_tr = float(tr.step(b))
            out = tw(**b)
            (out.loss / 2).backward()
            assert abs(l_tr - float(out.loss.detach())) <= 1e-5 * abs(float(out.loss.detach())), (step, micro)
        torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
        topt.step()
        tsched.step()
        topt.zero_grad(set_to_none=True)
    assert tr.step_count == 4 and sched.last_epoch == 4
    for q_tr, q_tw in zip(_trained(model, lora), params):
        assert _rel(q_tr.detach(), q_tw.detach()) <= 1e-5
    for q in lora.parameters():                                  # still views of the flat buffers after the steps
        assert lo <= q.grad.data_ptr() < hi


# ------------------------------------------------------------------------------------------------------------------------------
# 3. eval loss without dropout
# ------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_runs_lora_without_dropout(g):
    model, lora = _model(g, "d16", torch.float32, dropout=0.1)
    tr = P.InstructTrainer(model)
    sc = lora.step_count
    loss = float(tr.evaluate(_batch(g)))
    assert abs(loss - float(g["d16.loss"])) < 2e-5 * max(1.0, float(g["d16.loss"]))
    assert lora.step_count == sc


# ------------------------------------------------------------------------------------------------------------------------------
# 4. operand reuse (bf16)
# ------------------------------------------------------------------------------------------------------------------------------
def test_registered_operands_are_bit_identical_to_the_rebuild(g):
    model, lora = _model(g, "d64", torch.bfloat16)
    tr = P.InstructTrainer(model, lr=1e-3)
    b = _batch(g)
    for _ in range(2):
        tr.step(b)
    t0 = lora.targets[0]
    assert lora.operands(0, t0, torch.bfloat16) is not None

    def loss(registered=True):
        saved = lora._operands, lora._operand_key
        if not registered:                                       # as without a trainer: every operand rebuilt from the masters
            lora._operands, lora._operand_key = {}, {}
        try:
            with torch.no_grad():
                return model(**b).loss.clone()
        finally:
            lora._operands, lora._operand_key = saved

    l_reg, l_fresh = loss(), loss(False)
    assert torch.equal(l_reg.view(torch.int32), l_fresh.view(torch.int32))
    a = lora.get(1, "mlp.up_proj")[0]
    with torch.no_grad():
        a.copy_(a * 1.5)                                         # a write behind the trainer's back
    assert lora.operands(1, "mlp.up_proj", torch.bfloat16) is None
    assert lora.operands(0, t0, torch.bfloat16) is not None
    l_copy, l_copy_fresh = loss(), loss(False)
    assert torch.equal(l_copy.view(torch.int32), l_copy_fresh.view(torch.int32))
    assert not torch.equal(l_copy, l_reg)
    tr.step(b)                                                   # the step writes the operands from the copied master
    assert lora.operands(1, "mlp.up_proj", torch.bfloat16) is not None
    a16 = tr._operands[(1, "mlp.up_proj")][0]
    assert torch.equal(a16[:a.shape[0], :a.shape[1]], a.detach().to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. resume
# ------------------------------------------------------------------------------------------------------------------------------
def test_resume_is_bit_identical_and_the_directory_merges(g, tmp_path):
    b = _batch(g)

    def trainer():
        model, lora = _model(g, "d16", torch.float32, dropout=0.1)
        model.train()
        return P.InstructTrainer(model, lr=1e-3, max_norm=1.0, schedule=CosineWarmupSchedule(1e-3, 1, 4))

    full = trainer()
    for _ in range(4):
        full.step(b)
    first = trainer()
    for _ in range(2):
        first.step(b)
    adir, opath = P.save_instruct_checkpoint(first, str(tmp_path), 2)
    assert os.path.basename(adir) == "adapter_checkpoint_2" and os.path.basename(opath) == "optimizer_scheduler_checkpoint_2.pt"
    second = trainer()
    P.load_instruct_checkpoint(second, adir, opath)
    assert second.step_count == 2 and second.schedule.last_epoch == 2 and second.lora.step_count == first.lora.step_count
    for _ in range(2):
        second.step(b)
    assert torch.equal(second.flat_p.view(torch.int32), full.flat_p.view(torch.int32))
    assert torch.equal(second.opt.flat_v.view(torch.int32), full.opt.flat_v.view(torch.int32))
    # the directory through the inference-time merge gives the loss evaluate() gives
    want = float(first.evaluate(b))
    merged, _ = _model(g, "d16", torch.float32)
    merged.llama_decoder.lora = None
    rep = P.load_and_merge_adapter(merged, adir)
    assert rep["merged"] == 3 * 7 and rep["replaced"] == 4
    with torch.no_grad():
        got = float(merged(**b).loss)
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want))


# ------------------------------------------------------------------------------------------------------------------------------
# 6. two ranks on one GPU (gloo)
# ------------------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import json, os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.path.join(ROOT, "prot2text-v2-esm3_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_instruct_trainer as T
import p2t_hip as P
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
if world > 1:
    dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
z = np.load(os.path.join(ROOT, "tests", "golden", "sft_lora_tiny.npz"))
g = {k: z[k] for k in z.files}
g["meta"] = json.loads(bytes(g.pop("meta_json")).decode())
model, lora = T._model(g, "d16", torch.float32)
halves = [slice(0, 2), slice(2, 3)]
tr = P.InstructTrainer(model, lr=1e-3, max_norm=1.0, gradient_accumulation_steps=1 if world > 1 else 2)
for _ in range(2):
    if world > 1:
        tr.step(T._batch(g, halves[rank]))
    else:
        for h in halves:
            tr.step(T._batch(g, h))
if rank == 0:
    json.dump({"p": tr.flat_p.cpu().numpy().tolist(), "steps": tr.step_count}, open(os.environ["P2T_TEST_OUT"], "w"))
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
'''


def _run(world, tmp_path):
    out = str(tmp_path / f"instruct_w{world}.json")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   P2T_TEST_OUT=out, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + WORKER], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=300)[0].decode(errors="replace") for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-3000:]
    return json.load(open(out))


def test_two_ranks_equal_one_process_accumulating_both_shares(tmp_path):
    """DDP averages the ranks' gradients of their own mean losses: one process accumulating the two shares with GA 2 computes
    exactly that (the shares have different token counts, so it is not the full-batch mean)."""
    two, one = _run(2, tmp_path), _run(1, tmp_path)
    assert two["steps"] == one["steps"] == 2
    p2, p1 = np.array(two["p"]), np.array(one["p"])
    assert np.linalg.norm(p2 - p1) <= 1e-5 * np.linalg.norm(p1)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the epoch loop
# ------------------------------------------------------------------------------------------------------------------------------
def test_train_and_eval_epoch_drive_the_trainer(g):
    model, lora = _model(g, "d16", torch.float32, dropout=0.1)
    tr = P.InstructTrainer(model, gradient_accumulation_steps=2, schedule=P.instruct_schedule(2e-4, 1, 3, 2))
    logs = []
    rec = P.train_epoch(tr, [_batch(g), _flip(_batch(g)), _batch(g)], log=logs.append)
    assert set(rec) >= {"train_loss", "epoch_lr", "epoch_gradnorm"} and rec["batches"] == 3 and rec["optimizer_steps"] == 1
    assert np.isfinite(rec["train_loss"]) and np.isfinite(rec["epoch_gradnorm"]) and tr.step_count == 1
    ev = P.eval_epoch(tr, [_batch(g)], log=logs.append)
    assert abs(ev["eval_loss"] - float(tr.evaluate(_batch(g)))) < 1e-6 and any("eval_loss=" in s for s in logs)
    last = model.llama_decoder.spec.num_hidden_layers - 1     # a NaN on the residual stream (NaN scores would be masked away)
    k = tr.names.index(f"llama_decoder.model.layers.{last}.mlp.down_proj.lora_B.weight")
    with torch.no_grad():
        tr.opt.view(tr.flat_p, k).fill_(float("nan"))
    tr.sync_from_masters()
    with pytest.raises(ValueError, match="NaN"):
        P.train_epoch(tr, [_batch(g)], log=logs.append)
