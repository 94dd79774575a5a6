"""`python bench.py --gpus N` without an outer launcher must start its N ranks itself (the driver runs exactly that) and
fail CLEANLY, with the failing rank's message and a non-zero exit code, on a node with fewer GPUs -- not with a usage text.
A plain run prints the headline line alone; `--full` adds the other measurements; `--dump-outputs` writes the last step's outputs."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(180)
def test_self_launch_fails_cleanly_without_enough_gpus():
    if torch.cuda.device_count() >= 2:
        pytest.skip("this node has the GPUs: the launch would succeed")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=170, env=env)
    assert r.returncode != 0
    assert "needs 2 GPUs on this node" in r.stderr and "rank 1" in r.stderr       # the child's own message
    assert "stopping the other ranks" in r.stderr and "torch.distributed.run" not in r.stderr
    assert r.stdout.strip() == ""                                                  # no half-written JSON line


def test_launched_rank_rejects_world_size_mismatch():
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True,
                       text=True, timeout=170, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr


def test_dump_outputs_are_float32_seeded_and_bounded(tmp_path):
    """bench.dump_outputs at the cfg3 adapter's sizes (the largest the benchmark runs): float32 files, the same sample in two
    calls, at most 64 MB in all, small arrays whole."""
    import bench
    from p2t_hip import specs
    esm_name, llama_name = specs.CONFIGS["cfg3"][:2]
    ad = specs.adapter_spec(specs.esm_spec(esm_name), specs.llama_spec(llama_name))
    shapes = [(ad.intermediate_dim, ad.input_dim), (ad.intermediate_dim,), (ad.output_dim, ad.intermediate_dim), (ad.output_dim,)]
    g = torch.Generator().manual_seed(0)
    trainer = types.SimpleNamespace(p=[torch.randn(s, generator=g) for s in shapes], g=[torch.randn(s, generator=g) for s in shapes])
    for d in ("a", "b"):
        bench.dump_outputs(trainer, torch.tensor([0.25]), str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and len(files) == 9
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [0.25]
    assert np.array_equal(np.load(tmp_path / "a" / "adapter_fc2_bias_grad.npy"), trainer.g[3].numpy())
    w = np.load(tmp_path / "a" / "adapter_fc1_weight.npy")
    assert w.size == bench.DUMP_SAMPLE and np.isin(w, trainer.p[0].numpy().ravel()).all()


def _bench_line(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_dumps_the_last_step(tmp_path):
    d = _bench_line(["--config", "cfg1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["unit"] == "samples/s" and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(4 * 1e3 / d["ms_per_step"], rel=2e-3)
    assert "roofline" not in d and "cpu_baseline" not in d and "one_stream_check" not in d["config"]
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float32 and float(loss[0]) == pytest.approx(d["config"]["loss"], abs=1e-5)
    for name in ("fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias"):
        for f in (f"adapter_{name}.npy", f"adapter_{name}_grad.npy"):
            a = np.load(tmp_path / f)
            assert a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0, f


@pytest.mark.gpu
def test_full_run_adds_the_roofline_block():
    d = _bench_line(["--config", "cfg1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert d["roofline"]["event_steps"] == 2 and d["roofline"]["kernel_src_sha16"]
    assert d["config"]["one_stream_check"]["samples_per_s"] > 0
