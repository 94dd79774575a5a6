"""Continuous batching, kernel by kernel (csrc/llama_decode.hip, csrc/attn_decode.hip, csrc/kv_cache.hip, csrc/gemm_skinny.hip; include/p2t_hip.h "continuous batching";
reference restated in tests/continuous_reference.py):

* the decode step's attention with one counter PER ROW against numpy -- one row past the 64-key tile of its generated segment while
  another sits at 0 -- in every kernel form, under the lock-step tests' own tolerances;
* the fused QKV + rotation + append == the unfused pair bit for bit under per-row counters, and the appended keys at each row's own
  position against numpy;
* p2t_greedy_select_rows (ties, finished rows, eos and limit bits, a row_map subset) and p2t_kv_slot_load (bf16 and fp8 + scales)
  against the state the reference leaves behind;
* equal counters == lock-step: p2t_llama_decode_step_rows gives p2t_llama_decode_step_q's logits and cache contents bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import continuous_reference as R
import kv8_reference as K
from gpu_util import attn_o_bound, build_model, check_rows, dev, observe, rel, rnd, to_dev, to_np
from oracle import p2t_oracle as O
from p2t_hip import specs, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
LENS, STEPS = np.array([100, 7, 64], dtype=np.int32), np.array([0, 3, 70], dtype=np.int32)      # row 2 is past its 64-key tile, row 0 at 0
NAN8, NOSCALE = 0x7F, 0xFF


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(HERE, "golden", "generate_tiny.npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d.pop("meta_json")).decode())
    return d


def _model(g, case, dtype):
    m = g["meta"]["cases"][case]
    model = build_model(specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"]), dtype, m["weight_seed"])
    model.config.placeholder_id = g["meta"]["placeholder_id"]
    model.eval()
    return model


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev())


def _i32(a):
    return torch.tensor(np.asarray(a).tolist(), dtype=torch.int32, device=dev())


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32", "bf16", "bf16_mfma", "kv8"])
@pytest.mark.parametrize("d", [16, 64, 128])
def test_attention_with_per_row_counters_vs_numpy(d, form):
    """p2t_attention_decode_rows: 3 rows, 4 heads over 2 kv heads, prompt lengths {100, 7, 64}, row_step {0, 3, 70}.  Behind every row's
    OWN valid prefix the buffers hold NaN (fp8: 0x7F codes, 0xFF scale bytes): a row that read its neighbour's counter returns NaN or
    misses its bound.  Tolerances: test_decode_attention_vs_numpy's (f32: 3e-6 of the norm; bf16: 1.2e-2 of the norm and the row bound of
    gpu_util.attn_o_bound) and tests/test_gpu_kv8.py's (the same row bound against fp64 on the dequantised operands)."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    nh, nkv, B = 4, 2, 3
    dp, Tp, G = ops.head_dim_padded(d), 128, 128
    bf = form != "f32"
    dt = torch.bfloat16 if bf else torch.float32
    rs = np.random.RandomState(100 + d)
    rd = (lambda a: synth.bf16_round(a.astype(F32))) if bf else (lambda a: a.astype(F32))
    f = lambda *s: rd(rs.randn(*s) * 0.7)
    q, kp, vp, kg, vg = f(B, nh, d), f(B, nkv, Tp, d), f(B, nkv, Tp, d), f(B, nkv, G, d), f(B, nkv, G, d)
    padf = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (dp - d,), F32)], -1)
    kgn, vgn = kg.copy(), vg.copy()
    for b in range(B):
        kgn[b, :, STEPS[b] + 1:] = np.nan; vgn[b, :, STEPS[b] + 1:] = np.nan
    qd, kgd = to_dev(padf(q), dt), to_dev(padf(kgn), dt)
    vtg = to_dev(np.ascontiguousarray(padf(vgn).transpose(0, 1, 3, 2)), dt)
    QO = ops.round_up(nh * d, 64)
    out = torch.zeros((B, QO), dtype=dt, device=dev())
    lens_d, step_d = _i32(LENS), _i32(STEPS)
    if form == "kv8":
        (kc, ks, kdq), (vc, vs, vdq) = K.quant_keys(kp), K.quant_keys(vp)
        kc, ks, vc, vs = (np.array(a, copy=True) for a in (kc, ks, vc, vs))
        for b in range(B):
            kc[b, :, LENS[b]:] = NAN8; vc[b, :, LENS[b]:] = NAN8
            ks[b, :, LENS[b]:] = NOSCALE; vs[b, :, LENS[b]:] = NOSCALE
        pad8 = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (dp - d,), np.uint8)], -1)
        kpd, vtp, ksd, vsd = _u8(pad8(kc)), _u8(pad8(vc).transpose(0, 1, 3, 2)), _u8(ks), _u8(vs)
        kp, vp = kdq, vdq
    else:
        kpn, vpn = kp.copy(), vp.copy()
        for b in range(B):
            kpn[b, :, LENS[b]:] = np.nan; vpn[b, :, LENS[b]:] = np.nan
        kpd, vtp = to_dev(padf(kpn), dt), to_dev(np.ascontiguousarray(padf(vpn).transpose(0, 1, 3, 2)), dt)
        ksd = vsd = None
    _lib.call("p2t_attention_decode_rows", ptr(qd), ptr(kpd), ptr(vtp), ptr(kgd), ptr(vtg), ptr(lens_d), ptr(step_d), B, nh, nkv, d, Tp, G, float(d ** -0.5),
              int(bf), ops.dt_of(dt), {"f32": 0, "bf16": 0}.get(form, 1), ptr(out), QO, ptr(ksd) if ksd is not None else None,
              ptr(vsd) if vsd is not None else None, stream())
    got = to_np(out).astype(F32)[:, : nh * d].reshape(B, nh, d)
    assert np.isfinite(got).all()
    c_s = np.log(2.0) if bf else d ** -0.5                      # bf16: q holds scale * log2(e) already (log2_scores)
    ref, _ = R.decode_attention_rows(q, kp, vp, kg, vg, LENS, STEPS, c_s)
    if form == "f32":
        assert rel(got, ref) < 3e-6
    elif form != "kv8":
        observe(f"decode_attn_rows[d{d}].{form}", rel(got, ref), 1.2e-2)
    o64, A64 = R.decode_attention_rows(*(a.astype(np.float64) for a in (q, kp, vp, kg, vg)), LENS, STEPS, c_s)
    r64 = dict(o=o64[:, :, None], A=A64[:, :, None])
    bound = attn_o_bound(r64, bf, bf)
    check_rows(f"attn_rows[decode_rows,{form},d{d}]", [("o", got[:, :, None], r64["o"], bound)])
    # the check tells the counters apart: the lock-step reading of the same buffers (every row at row 0's counter) misses row 2's bound
    wrong, _ = R.decode_attention_rows(*(a.astype(np.float64) for a in (q, kp, vp, kg, vg)), LENS, np.full(3, STEPS[0]), c_s)
    assert (np.abs(wrong - o64)[2] > bound[2, :, 0]).any()


# ---------------------------------------------------------------------------------------------
def _rows_engine(model, g, slots=3, cap=128, **kw):
    from p2t_hip.continuous import ContinuousEngine
    return ContinuousEngine(model.llama_decoder, slots, cap, cap, [], g["meta"]["pad_id"], use_graph=False, **kw)


@pytest.mark.parametrize("case", ["d64", "d128"])
def test_fused_rotation_and_append_equal_the_unfused_pair_at_per_row_positions(g, case):
    """One p2t_llama_decode_step_rows on a bf16 model with prompt_len {100, 7, 64} and row_step {0, 3, 70}, the generated segment full of a
    sentinel: (a) the fused QKV + rotation + append epilogue and the unfused pair (P2T_DECODE_NO_ROPE_FUSION) leave the same cache and
    logits bit for bit; (b) exactly one key and one value per (layer, row, kv head) were written, at index row_step[row]; (c) layer 0's
    key of row r is the rotation to position prompt_len[r] + row_step[r] of what the same step appends at position 0 (its unrotated
    key, rounded to bf16), under continuous_reference.rotate_bound_bf16, and its value is that step's value bit for bit."""
    model = _model(g, case, torch.bfloat16)
    spec = model.llama_decoder.spec
    e = _rows_engine(model, g)
    x = to_dev(rnd(11, "cont.x", (3, spec.hidden_size), 1.0))
    SENT = 3.0

    def step(lens, steps, flags):
        e.lens.copy_(_i32(lens)); e.row_step.copy_(_i32(steps))
        e.k_gen.fill_(SENT); e.vt_gen.fill_(SENT)
        e.x.copy_(x)
        e.flags = flags
        e._step_rows(frozen=False)
        assert to_np(e.row_step).tolist() == [int(s) + 1 for s in steps]
        return e.k_gen.clone(), e.vt_gen.clone(), e.logits.clone()

    kf, vf, lf = step(LENS, STEPS, 0)
    ku, vu, lu = step(LENS, STEPS, 1)
    assert torch.equal(kf, ku) and torch.equal(vf, vu) and torch.equal(lf, lu)
    k0, v0, _ = step([0, 0, 0], [0, 0, 0], 0)
    kf, vf, k0, v0 = (to_np(t.float()) for t in (kf, vf, k0, v0))
    L, nkv, d = spec.num_hidden_layers, spec.num_key_value_heads, spec.head_dim
    written_k, written_v = kf != SENT, vf != SENT
    for r in range(3):
        s = int(STEPS[r])
        assert not np.delete(written_k[:, r], s, axis=2).any() and not np.delete(written_v[:, r], s, axis=3).any(), r
        assert written_k[:, r, :, s].any(axis=-1).all() and written_v[:, r, :, :, s].any(axis=-1).all(), r
    inv_freq = np.asarray(O.llama_inv_freq(spec), dtype=F32)
    parts = []
    for r in range(3):
        s, pos = int(STEPS[r]), int(LENS[r]) + int(STEPS[r])
        ref, S = R.rotate(k0[0, r, :, 0, :d], inv_freq, pos)
        parts.append((f"k[row {r}]", kf[0, r, :, s, :d][None, None], ref[None, None], R.rotate_bound_bf16(ref, S)[None, None]))
        assert np.array_equal(vf[0, r, :, :, s], v0[0, r, :, :, 0]), r
        assert (np.abs(k0[0, r, :, 0, :d] - ref) > R.rotate_bound_bf16(ref, S)).any(), r       # the check tells positions apart: position 0 misses it
    check_rows(f"rope_append_rows[{case}]", parts)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_greedy_select_rows(dt):
    """Ties go to the lowest index; a finished row emits pad and writes NOTHING (its counter no longer moves: the token at it is its
    last one); eos bit 1, limit bit 2, both; columns >= V are padding; a row_map subset leaves every other row's state untouched."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    V, ld, BB, G, PAD = 1000, 1024, 5, 64, 555
    eos_ids = [5, 77]
    lg = np.full((BB, ld), -5.0, dtype=F32)
    lg[0, [900, 17, 400]] = 3.0                       # three-way tie -> 17
    lg[1, 8] = 4.0                                    # finished before: pad, nothing written
    lg[2, 5] = 2.0                                    # an eos id -> bit 1
    lg[3, 999] = 1.0; lg[3, 1001] = 9.0               # columns >= V are padding; at its limit -> bit 2
    lg[4, 77] = 1.0                                   # eos at the limit -> bits 1 | 2, at the table's last column
    state = dict(finished=np.array([0, 1, 0, 0, 0], np.int32), next_tokens=np.full(BB, -7, np.int64), out_tokens=np.full((BB, G), -1, np.int64),
                 row_step=np.array([3, 9, 0, 6, 63], np.int32), row_limit=np.array([10, 64, 4, 7, 64], np.int32))

    def run(logits, row_map):
        t = {k: to_dev(v) for k, v in state.items()}
        eos = torch.tensor(eos_ids, dtype=torch.int64, device=dev())
        lgd = to_dev(logits, dt)
        rm = _i32(row_map) if row_map is not None else None
        _lib.call("p2t_greedy_select_rows", ptr(lgd), ops.dt_of(dt), ld, V, logits.shape[0], ptr(eos), 2, PAD, ptr(t["finished"]), ptr(t["next_tokens"]),
                  ptr(t["out_tokens"]), G, ptr(t["row_step"]), ptr(t["row_limit"]), ptr(rm) if rm is not None else None, BB, G, stream())
        want = {k: v.copy() for k, v in state.items()}
        R.greedy_select_rows(logits, V, want["finished"], want["next_tokens"], want["out_tokens"], want["row_step"], want["row_limit"], eos_ids, PAD, row_map)
        for k in want:
            assert np.array_equal(to_np(t[k]), want[k]), k
        return want

    w = run(lg, None)
    assert w["next_tokens"].tolist() == [17, PAD, 5, 999, 77] and w["finished"].tolist() == [0, 1, 1, 2, 3]
    assert w["out_tokens"][0, 3] == 17 and (w["out_tokens"][1] == -1).all() and w["out_tokens"][4, 63] == 77
    assert (w["out_tokens"] != -1).sum() == 4
    w = run(lg[[3, 1]], [3, 1])                       # logits row 0 -> engine row 3, row 1 -> engine row 1 (finished)
    assert w["next_tokens"].tolist() == [-7, PAD, -7, 999, -7] and w["finished"].tolist() == [0, 1, 0, 2, 0]
    assert (w["out_tokens"] != -1).sum() == 1 and w["out_tokens"][3, 6] == 999
    w = run(lg[[0]], [7])                             # a row the engine does not have: nothing is touched
    assert all(np.array_equal(w[k], state[k]) for k in state)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,d,Tp", [("bf16", 64, 1088), ("f32", 16, 64), ("fp8", 48, 128)])
def test_kv_slot_load(fmt, d, Tp):
    """2 of 4 slots loaded (slots 3 and 1, in that order) from a staging cache of 2 rows: the loaded slots' prompt segments -- K, V^T and,
    for fp8, both scale arrays, all Tp entries of every layer -- equal the staging rows bit for bit, the other slots and the whole
    generated segment are unchanged, and prompt_len / row_step / finished / row_limit are set for the loaded slots only.  Tp = 1088 with
    bf16: more 16-byte pieces than one sweep of the grid covers."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    C = __import__("ctypes")
    L, B0, k, nkv, G = 2, 4, 2, 2, 64
    dp = ops.head_dim_padded(d)
    rs = np.random.RandomState(Tp + d)
    esz = dict(bf16=2, f32=4, fp8=1)[fmt]
    raw = lambda *shape: rs.randint(0, 256, size=shape + (esz,), dtype=np.uint8).reshape(shape[:-1] + (shape[-1] * esz,))
    stage = dict(k=raw(L, k, nkv, Tp, dp), vt=raw(L, k, nkv, dp, Tp), lens=np.array([9, 33], np.int32))
    cache = dict(k=raw(L, B0, nkv, Tp, dp), vt=raw(L, B0, nkv, dp, Tp), lens=np.array([5, 6, 7, 8], np.int32), row_step=np.array([4, 40, 2, 63], np.int32),
                 finished=np.array([0, 1, 0, 3], np.int32), row_limit=np.array([64, 64, 10, 64], np.int32))
    if fmt == "fp8":
        stage.update(ks=raw(L, k, nkv, Tp), vs=raw(L, k, nkv, Tp))
        cache.update(ks=raw(L, B0, nkv, Tp), vs=raw(L, B0, nkv, Tp))
    gen = raw(L, B0, nkv, G, dp * (2 if fmt == "fp8" else 1))
    sd, cd = {n: to_dev(v) for n, v in stage.items()}, {n: to_dev(v) for n, v in cache.items()}
    kg, vtg = to_dev(gen), to_dev(gen[::-1].copy())
    cfg = _lib.LlamaConfigC(n_layers=L, hidden=128, ffn=256, heads=4, kv_heads=nkv, head_dim=d, vocab=512, dtype=0 if fmt == "f32" else 1)
    sc = lambda t: dict(k_prompt_scale=t["ks"].data_ptr(), v_prompt_scale=t["vs"].data_ptr()) if "ks" in t else {}
    st = _lib.KvCacheC(k_prompt=sd["k"].data_ptr(), vt_prompt=sd["vt"].data_ptr(), k_gen=kg.data_ptr(), vt_gen=vtg.data_ptr(), prompt_len=sd["lens"].data_ptr(),
                       step=None, B0=k, group=1, Tp=Tp, G=G, **sc(sd))
    ca = _lib.KvCacheC(k_prompt=cd["k"].data_ptr(), vt_prompt=cd["vt"].data_ptr(), k_gen=kg.data_ptr(), vt_gen=vtg.data_ptr(), prompt_len=cd["lens"].data_ptr(),
                       step=None, B0=B0, group=1, Tp=Tp, G=G, **sc(cd))
    slots, limits = [3, 1], [17, 1]
    _lib.call("p2t_kv_slot_load", C.byref(cfg), C.byref(st), C.byref(ca), (C.c_int32 * k)(*slots), (C.c_int32 * k)(*limits), k, ptr(cd["row_step"]),
              ptr(cd["finished"]), ptr(cd["row_limit"]), stream())
    before = {n: v.copy() for n, v in cache.items()}
    R.kv_slot_load(cache, stage, slots, limits)
    for n in cache:
        assert np.array_equal(to_np(cd[n]), cache[n]), n
    for n in ("k", "vt") + (("ks", "vs") if fmt == "fp8" else ()):
        assert np.array_equal(cache[n][:, [0, 2]], before[n][:, [0, 2]]) and np.array_equal(cache[n][:, 3], stage[n][:, 0]), n
    assert cache["lens"].tolist() == [5, 33, 7, 9] and cache["row_step"].tolist() == [4, 0, 2, 0]
    assert cache["finished"].tolist() == [0, 0, 0, 0] and cache["row_limit"].tolist() == [64, 1, 10, 17]
    assert np.array_equal(to_np(kg), gen) and np.array_equal(to_np(vtg), gen[::-1])
    for n, v in stage.items():
        assert np.array_equal(to_np(sd[n]), v), n


# ---------------------------------------------------------------------------------------------
EQUAL_CASES = {
    "bf16_d64_stream": ("d64", torch.bfloat16, "model", dict(stream_copy=True)),
    "bf16_d64_row_major": ("d64", torch.bfloat16, "model", dict(stream_copy=False)),
    "f32_d16": ("d16", torch.float32, "model", dict()),
    "mxfp4_d64": ("d64", torch.bfloat16, "mxfp4", dict()),
    "fp8_weights_d128": ("d128", torch.bfloat16, "fp8", dict()),
    "kv8_d64": ("d64", torch.bfloat16, "model", dict(prompt_kv_dtype="fp8")),
    "head_fp8_d64": ("d64", torch.bfloat16, "model", dict(lm_head_dtype="fp8")),
    "head_mxfp4_d64": ("d64", torch.bfloat16, "model", dict(lm_head_dtype="mxfp4")),
    "qwen3_bf16": ("qwen3", torch.bfloat16, "model", dict()),
}


@pytest.mark.parametrize("name", list(EQUAL_CASES))
def test_equal_counters_equal_lock_step_bit_for_bit(g, name):
    """The golden prompts prefilled into a lock-step DecodeEngine and, through the staging cache and p2t_kv_slot_load, into a
    ContinuousEngine; then 6 steps on the same fed tokens: p2t_llama_decode_step[_q / _mxfp4] against p2t_llama_decode_step_rows with every
    row_step[r] equal and frozen == NULL.  First-token logits, every step's logits, both cache segments (and the scale arrays), the
    prompt lengths and the counters are equal bit for bit."""
    from p2t_hip.generation import DecodeEngine
    case, dt, gemm, kw = EQUAL_CASES[name]
    model = _model(g, case, dt)
    if gemm != "model":
        model.set_gemm_dtype(gemm)
    with torch.no_grad():
        emb, mask = model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                          protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)
    B, T, _ = emb.shape
    V = model.llama_decoder.spec.vocab_size
    e1 = DecodeEngine(model.llama_decoder, B, 1, T, 8, **kw)
    first1 = e1.prefill(*e1.compact(emb, mask))
    e2 = _rows_engine(model, g, slots=B, cap=T, **kw)
    assert (e2.Tp, e2.G) == (e1.Tp, e1.G)
    first2 = e2.load(list(range(B)), [(emb[b], mask[b]) for b in range(B)], [e2.G] * B)
    assert torch.equal(first1, first2)
    assert to_np(e2.row_step).tolist() == [0] * B and to_np(e2.finished).tolist() == [0] * B
    for s in range(6):
        tok = torch.tensor([(7 * s + 13 * r + 5) % V for r in range(B)], dtype=torch.int64, device=dev())
        e1.feed(tok); e1.decode_step()
        e2.feed(tok); e2._step_rows(frozen=False)
        assert torch.equal(e1.logits, e2.logits), s
    assert int(e1.step.item()) == 6 and to_np(e2.row_step).tolist() == [6] * B
    names = ["k_prompt", "vt_prompt", "k_gen", "vt_gen", "lens"] + (["k_prompt_scale", "v_prompt_scale"] if kw.get("prompt_kv_dtype") else [])
    for n in names:
        assert torch.equal(getattr(e1, n), getattr(e2, n)), n
