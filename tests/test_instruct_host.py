"""CPU: host side of the stage-2 trainer (p2t_hip/instruct.py) -- the segment / chunk planner of p2t_clip_adamw_flat, the table
layouts against the library's structs, the schedule stepped once per optimizer step against train_instruct.py's arithmetic, the
checkpoint names and key set, argument validation.  Nothing is launched."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from p2t_hip import _lib, instruct
from p2t_hip.training_state import CosineWarmupSchedule


def _check_plan(sizes):
    offs, total = instruct.plan_segments(sizes)
    assert (offs % 16 == 0).all() and total % 16 == 0
    ends = offs + np.asarray(sizes)
    assert (ends[:-1] <= offs[1:]).all() and ends[-1] <= total and total - ends[-1] < 16
    ch = instruct.plan_chunks(offs, sizes)
    assert (ch["count"] >= 1).all() and (ch["count"] <= _lib.FLAT_CHUNK).all() and (ch["start"] % 16 == 0).all()
    covered = np.zeros(total, dtype=np.int64)
    for s, seg, c in zip(ch["start"], ch["segment"], ch["count"]):
        assert offs[seg] <= s and s + c <= offs[seg] + sizes[seg]
        covered[s:s + c] += 1
    want = np.zeros(total, dtype=np.int64)
    for o, n in zip(offs, sizes):
        want[o:o + n] = 1
    assert (covered == want).all()                               # every element once, padding never
    return offs, total, ch


def test_planner_alignment_coverage_and_tails():
    rs = np.random.RandomState(0)
    sizes = [int(v) for v in rs.randint(1, 20000, size=300)] + [4096, 4097, 1, 15, 16, 17, 3 * 4096]
    _, _, ch = _check_plan(sizes)
    assert len(set(ch["segment"].tolist())) == len(sizes) > 64
    _check_plan([7])                                             # one odd-sized segment: tail chunk of 7


def test_planner_scales_to_64k_segments_and_2_pow_31_elements():
    offs, total, ch = _check_plan([1 + k % 33 for k in range(65537)])
    assert len(offs) == 65537
    big = [2 ** 30 + 3, 2 ** 30 + 5, 100]
    offs, total = instruct.plan_segments(big)
    assert total >= 2 ** 31 and offs.dtype == np.int64
    ch = instruct.plan_chunks(offs, big)
    assert int(ch["count"].sum()) == sum(big) and ch["start"].max() + ch["count"][-1] <= total


def test_tables_match_the_library_structs():
    assert instruct.SEGMENT_DTYPE.itemsize == ctypes.sizeof(_lib.FlatSegmentC) == _lib.lib.p2t_struct_size(12)
    assert instruct.CHUNK_DTYPE.itemsize == ctypes.sizeof(_lib.FlatChunkC) == _lib.lib.p2t_struct_size(13)
    for name, _ in _lib.FlatSegmentC._fields_:
        assert instruct.SEGMENT_DTYPE.fields[name][1] == getattr(_lib.FlatSegmentC, name).offset
    for name, _ in _lib.FlatChunkC._fields_:
        assert instruct.CHUNK_DTYPE.fields[name][1] == getattr(_lib.FlatChunkC, name).offset
    a16 = torch.zeros((16, 72), dtype=torch.bfloat16)            # LoRA A [r = 4 of rp = 16 rows, K = 70]
    bs16 = torch.zeros((40, 64), dtype=torch.bfloat16)           # LoRA B [N = 40, r = 4 of 64 cols], scale alpha / r
    w1 = torch.zeros((24, 64), dtype=torch.float32)              # adapter w1 copy [I, round_up(in, 64)]
    opt = instruct.FlatAdamW([280, 160, 24 * 50, 24], "cpu", [(a16, 4, 70, 1.0), (bs16, 40, 4, 2.0), (w1, 24, 50, 1.0), None])
    seg = opt.segment_table.numpy().view(instruct.SEGMENT_DTYPE)
    assert seg["offset"].tolist() == [0, 288, 448, 1648] and opt.total == 1680
    assert seg["ld"].tolist() == [72, 64, 64, 1] and seg["cols"].tolist() == [70, 4, 50, 1] and seg["rows"].tolist()[:3] == [4, 40, 24]
    assert seg["shadow"][3] == 0 and seg["scale"][1] == 2.0 and seg["shadow_dtype"].tolist()[:3] == [_lib.BF16, _lib.BF16, _lib.F32]
    with pytest.raises(ValueError):
        instruct.FlatAdamW([280], "cpu", [(a16, 4, 71, 1.0)])   # [4, 71] does not hold 280 elements
    with pytest.raises(ValueError):
        instruct.FlatAdamW([280], "cpu", [(a16.t(), 4, 70, 1.0)])
    with pytest.raises(ValueError):
        instruct.plan_segments([3, 0])


def test_flat_entry_point_rejects_bad_arguments_without_a_gpu():
    with pytest.raises(ValueError, match="null"):
        _lib.call("p2t_clip_adamw_flat", None, None, None, None, 16, None, None, 1, 1, 1e-3, 0.9, 0.999, 1e-6, 0.01, 0.0, None, None, None)
    buf = ctypes.create_string_buffer(1024)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("p2t_clip_adamw_flat", p, p, p, p, 17, p, p, 1, 1, 1e-3, 0.9, 0.999, 1e-6, 0.01, 0.0, None, p, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("p2t_clip_adamw_flat", p, p, p, p, 16, p, p, 1, 0, 1e-3, 0.9, 0.999, 1e-6, 0.01, 0.0, None, p, None)


def test_schedule_steps_once_per_optimizer_step_like_train_instruct():
    """train_instruct.py:241-294 + 436-447: total = len(loader) * epochs // GA, warmup int(0.06 total), optimizer step when
    (batch_idx + 1) % GA == 0 (the window restarts every epoch: zero_grad at its start), scheduler.step() after every optimizer
    step -- against torch's LambdaLR over the same lambda, for GA 32 over a 7-batch epoch (no step at all) and GA 2."""
    from p2t_hip import sharding
    for ga, batches, epochs in ((32, 7, 40), (2, 7, 3), (1, 5, 2)):
        sched = instruct.instruct_schedule(2e-4, epochs, batches, ga)
        total = batches * epochs // ga
        assert (sched.num_training_steps, sched.num_warmup_steps) == (total, int(0.06 * total))
        ref_sched = CosineWarmupSchedule(2e-4, int(0.06 * total), total)
        topt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=2e-4)
        tsched = torch.optim.lr_scheduler.LambdaLR(topt, ref_sched.factor)
        want, got, micro = [], [], 0
        for _ in range(epochs):
            micro = 0                                            # loop.train_epoch: trainer._micro = 0
            for batch_idx in range(batches):
                if (batch_idx + 1) % ga == 0:
                    want.append(topt.param_groups[0]["lr"])
                    topt.step()
                    tsched.step()
                _, _, _, do_step = sharding.micro_step_plan(micro, ga)
                micro += 1
                if do_step:
                    got.append(sched.lr())
                    sched.step()
                    micro = 0
        assert len(got) == len(want) == epochs * (batches // ga)
        assert np.allclose(got, want, rtol=1e-12, atol=0)
        if ga == 32:
            assert got == [] and sched.last_epoch == 0


class _StubDecoder(torch.nn.Module):
    """The parameter names DecoderLora reads (model.layers.{i}.{target}.weight, every projection [12, 8]), on the CPU (no engine)."""

    def __init__(self, n_layers=2):
        super().__init__()
        from p2t_hip.decoder_train import TARGETS
        self.spec = types.SimpleNamespace(num_hidden_layers=n_layers)
        self.model = torch.nn.Module()
        self.model.layers = torch.nn.ModuleList()
        for _ in range(n_layers):
            layer = torch.nn.ModuleDict({"self_attn": torch.nn.ModuleDict(), "mlp": torch.nn.ModuleDict()})
            for t in TARGETS:
                block, proj = t.split(".")
                layer[block][proj] = torch.nn.Linear(8, 12, bias=False)
            self.model.layers.append(layer)


def _decoder_lora():
    from p2t_hip.decoder_train import DecoderLora
    return DecoderLora(_StubDecoder(), 4)


def test_checkpoint_names_config_and_safetensors_keys_of_a_decoder_lora(tmp_path):
    from safetensors.torch import load_file, save_file
    adir, opath = instruct.checkpoint_paths(str(tmp_path), 3)
    assert adir.endswith("adapter_checkpoint_3") and opath.endswith("optimizer_scheduler_checkpoint_3.pt")
    lora = _decoder_lora()
    ad = {k: torch.randn(5) for k in instruct.ADAPTER_KEYS}
    t = instruct.adapter_tensors(lora, ad)
    os.makedirs(adir)
    save_file(t, os.path.join(adir, "adapter_model.safetensors"))
    keys = set(load_file(os.path.join(adir, "adapter_model.safetensors")))
    want = {f"base_model.model.llama_decoder.model.layers.{i}.{tg}.lora_{w}.weight" for i in range(2) for tg in lora.targets for w in "AB"}
    want |= {f"base_model.model.adapter.{m}.{w}" for m in ("fc1", "fc2") for w in ("weight", "bias")}
    assert keys == want
    cfg = instruct.adapter_config(lora)
    assert cfg["peft_type"] == "LORA" and cfg["r"] == 4 and cfg["lora_alpha"] == 8.0 and cfg["lora_dropout"] == 0.1
    assert cfg["target_modules"] == list(lora.targets) and cfg["modules_to_save"] == ["adapter.fc1", "adapter.fc2"]
    assert instruct.adapter_config(lora, train_adapter=False)["modules_to_save"] is None
    json.dumps(cfg)


def test_trainer_argument_validation():
    class _Dec:
        lora = None

    class _M:
        llama_decoder = _Dec()

    with pytest.raises(ValueError, match="add_lora"):
        instruct.InstructTrainer(_M())
    _Dec.lora = _decoder_lora()
    for kw in (dict(gradient_accumulation_steps=0), dict(gradient_accumulation_steps=1.5), dict(lr=0.0), dict(eps=0.0),
               dict(weight_decay=-1.0), dict(betas=(0.9, 1.0)), dict(max_norm=0.0)):
        with pytest.raises(ValueError):
            instruct.InstructTrainer(_M(), **kw)
