"""Beam search without the cache copy, kernel by kernel (csrc/kv_cache.hip, csrc/attn_decode.hip, csrc/llama_decode.hip; include/p2t_hip.h
"beam search without the cache copy"; reference restated in tests/beam_ancestry_reference.py):

* p2t_kv_ancestry_update against numpy, bit for bit, in place, with sentinels behind the counter;
* p2t_attention_decode_beams in every kernel form against the fp64 gather reference under gpu_util.attn_o_bound -- tables from a chain
  of beam selections with dying beams, dead-branch entries of magnitude 1e4, NaN behind every valid prefix, slots that see no key of a
  tile;
* p2t_llama_decode_step_beams over a table against p2t_llama_decode_step over the segment that p2t_kv_reorder materialises, each against
  the bf16 oracle on the same tokens."""
import numpy as np
import pytest
import torch

import beam_ancestry_reference as A
import kv8_reference as K
from gpu_util import attn_o_bound, check_rows, dev, observe, rel, to_dev, to_np
from helpers import model_weights
from oracle import p2t_oracle as O
from p2t_hip import specs, synth
from test_gpu_generate import _model, g  # noqa: F401  (g: the module-scoped golden fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32
LENS = np.array([100, 7], dtype=np.int32)
NAN8, NOSCALE = 0x7F, 0xFF


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev())


def _i32(a):
    return torch.tensor(np.asarray(a).tolist(), dtype=torch.int32, device=dev())


def _cache(step_d, B0, group, G):
    from p2t_hip import _lib
    return _lib.KvCacheC(step=step_d.data_ptr(), B0=B0, group=group, Tp=64, G=G)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B0,group", [(2, 3), (1, 16), (3, 2)])
def test_ancestry_update_vs_numpy(B0, group):
    """src_rows: the identity, duplicates ([1, 1, 0]-style: a beam dies), a full permutation inside every prompt; counters 0, 1, 63, 64,
    70 (and past the capacity: clamped to the last column).  In place on a table of valid bytes in front of the counter and 0xFF behind it."""
    import ctypes as C
    from p2t_hip import _lib
    from p2t_hip.ops import ptr, stream
    BB, G = B0 * group, 128
    rs = np.random.RandomState(group)
    base = np.repeat(np.arange(B0) * group, group)
    srcs = dict(identity=np.arange(BB), duplicates=base + np.tile(np.r_[[1, 1, 0], rs.randint(0, group, size=group)][:group] % group, B0),
                permutation=base + np.concatenate([rs.permutation(group) for _ in range(B0)]))
    assert len(set(srcs["duplicates"].tolist())) < BB and sorted(srcs["permutation"].tolist()) == list(range(BB))
    for name, src in srcs.items():
        for step in (0, 1, 63, 64, 70, 500):
            s = min(step, G - 1)
            anc = np.full((BB, G), 0xFF, dtype=np.uint8)
            anc[:, :s] = rs.randint(0, group, size=(BB, s))
            anc_d, src_d, step_d = _u8(anc), torch.from_numpy(src.astype(np.int64)).to(dev()), _i32([step])
            _lib.call("p2t_kv_ancestry_update", C.byref(_cache(step_d, B0, group, G)), ptr(src_d), ptr(anc_d), stream())
            want = A.ancestry_update(anc, src, step, group)
            assert np.array_equal(to_np(anc_d), want), (name, step)
            assert (want[:, s + 1:] == 0xFF).all() and (want[:, : s + 1] < group).all()


# ---------------------------------------------------------------------------------------------
def _table(B0, group, step, G, seed):
    """The table after `step` + 1 updates along a chain of random selections with repeated sources, as a search leaves it."""
    rs = np.random.RandomState(seed)
    anc = np.zeros((B0 * group, G), dtype=np.uint8)
    for s in range(step + 1):
        src = np.concatenate([b * group + rs.randint(0, group, size=group) for b in range(B0)])
        anc = A.ancestry_update(anc, src, s, group)
    return anc


def _blind(anc, n1, group):
    """(row, physical row, tile) where the row sees NO key of a tile that is the first its wave runs: tile t of the list (the prompt's
    tiles, then the generated tiles of physical row 0, 1, ...) goes to wave t mod NW, NW >= 8, so the first 8 of the list qualify."""
    tiles1, out = (n1 + 63) // 64, []
    for r in range(anc.shape[0]):
        tiles0 = (int(LENS[r // group]) + 63) // 64
        for p in range(group):
            for tt in range(tiles1):
                if tiles0 + p * tiles1 + tt < 8 and not (anc[r, 64 * tt: min(n1, 64 * tt + 64)] == p).any():
                    out.append((r, p, tt))
    return out


HEADS = {"nh4_g3": (4, 2, 3), "nh8_g4": (8, 2, 4), "nh8_g5": (8, 2, 5), "nh10_g4": (10, 2, 4)}      # (nh, nkv, group)


@pytest.mark.parametrize("form", ["f32", "bf16", "bf16_mfma", "kv8"])
@pytest.mark.parametrize("d", [16, 64, 128])
@pytest.mark.parametrize("heads", list(HEADS))
def test_attention_through_the_table_vs_numpy(heads, d, form):
    """p2t_attention_decode_beams: 2 prompts of lengths {100, 7}; 6 head slots (no power of two), exactly 16, two chunks with a partial
    last one, and 5 heads per kv head (15 slots per chunk); counters 0 and 70 (the generated segment crosses a 64-key tile).  Behind the
    counter and behind each prompt length the buffers hold NaN (fp8: 0x7F codes, 0xFF scale bytes); the keys inside the counter that no
    beam's table references hold +-1e4 in K and V -- finite, as the dead branches of a search are.  Tolerances: those of
    test_attention_with_per_row_counters_vs_numpy (f32: 3e-6 of the norm; the row bound of gpu_util.attn_o_bound against fp64)."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    nh, nkv, group = HEADS[heads]
    B0, BB = 2, 2 * group
    dp, Tp, G = ops.head_dim_padded(d), 128, 128
    bf = form != "f32"
    dt = torch.bfloat16 if bf else torch.float32
    rs = np.random.RandomState(1000 + d + nh + group)
    rd = (lambda a: synth.bf16_round(a.astype(F32))) if bf else (lambda a: a.astype(F32))
    f = lambda *s: rd(rs.randn(*s) * 0.7)
    padf = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (dp - d,), F32)], -1)
    q, kp, vp = f(BB, nh, d), f(B0, nkv, Tp, d), f(B0, nkv, Tp, d)
    QO = ops.round_up(nh * d, 64)
    lens_d = _i32(LENS)
    if form == "kv8":
        (kc, ks, kdq), (vc, vs, vdq) = K.quant_keys(kp), K.quant_keys(vp)
        kc, ks, vc, vs = (np.array(a, copy=True) for a in (kc, ks, vc, vs))
        for b in range(B0):
            kc[b, :, LENS[b]:] = NAN8; vc[b, :, LENS[b]:] = NAN8
            ks[b, :, LENS[b]:] = NOSCALE; vs[b, :, LENS[b]:] = NOSCALE
        pad8 = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (dp - d,), np.uint8)], -1)
        kpd, vtp, ksd, vsd = _u8(pad8(kc)), _u8(pad8(vc).transpose(0, 1, 3, 2)), _u8(ks), _u8(vs)
        kp, vp = kdq, vdq
    else:
        kpn, vpn = kp.copy(), vp.copy()
        for b in range(B0):
            kpn[b, :, LENS[b]:] = np.nan; vpn[b, :, LENS[b]:] = np.nan
        kpd, vtp = to_dev(padf(kpn), dt), to_dev(np.ascontiguousarray(padf(vpn).transpose(0, 1, 3, 2)), dt)
        ksd = vsd = None
    c_s = np.log(2.0) if bf else d ** -0.5                      # bf16: q holds scale * log2(e) already (log2_scores)
    qd = to_dev(padf(q), dt)
    for step in (0, 70):
        n1 = step + 1
        anc = _table(B0, group, step, G, 7 * step + group)
        kg, vg = f(BB, nkv, G, d), f(BB, nkv, G, d)
        # dead branches: keys inside the counter that no beam's table names
        used = np.zeros((BB, G), dtype=bool)
        for r in range(BB):
            used[r // group * group + anc[r, :n1].astype(int), np.arange(n1)] = True
        dead = ~used[:, :n1]
        if step:
            assert dead.any()
        sign = np.where(rs.rand(BB, nkv, n1, d) < 0.5, -1e4, 1e4).astype(F32)
        for a in (kg, vg):
            a[:, :, :n1] = np.where(dead[:, None, :, None], rd(sign), a[:, :, :n1])
        assert _blind(anc, n1, group), "the table leaves no slot without a visible key in a wave's first tile"
        kgn, vgn = kg.copy(), vg.copy()
        kgn[:, :, n1:] = np.nan; vgn[:, :, n1:] = np.nan
        kgd, vtg = to_dev(padf(kgn), dt), to_dev(np.ascontiguousarray(padf(vgn).transpose(0, 1, 3, 2)), dt)
        out = torch.zeros((BB, QO), dtype=dt, device=dev())
        step_d, anc_d = _i32([step]), _u8(anc)
        _lib.call("p2t_attention_decode_beams", ptr(qd), ptr(kpd), ptr(vtp), ptr(kgd), ptr(vtg), ptr(lens_d), ptr(step_d), B0, group, nh, nkv, d, Tp, G,
                  float(d ** -0.5), int(bf), ops.dt_of(dt), {"f32": 0, "bf16": 0}.get(form, 1), ptr(out), QO, ptr(ksd) if ksd is not None else None,
                  ptr(vsd) if vsd is not None else None, ptr(anc_d), stream())
        got = to_np(out).astype(F32)[:, : nh * d].reshape(BB, nh, d)
        assert np.isfinite(got).all(), step
        if form == "f32":
            ref, _ = A.decode_attention_beams(q, kp, vp, kg, vg, LENS, step, anc, group, c_s)
            assert rel(got, ref) < 3e-6
        to64 = lambda *a: (x.astype(np.float64) for x in a)
        o64, A64 = A.decode_attention_beams(*to64(q, kp, vp, kg, vg), LENS, step, anc, group, c_s)
        r64 = dict(o=o64[:, :, None], A=A64[:, :, None])
        bound = attn_o_bound(r64, bf, bf)
        check_rows(f"attn_rows[decode_beams,{form},d{d},{heads},s{step}]", [("o", got[:, :, None], r64["o"], bound)])
        if step:        # the check tells tables apart: the identity reading of the same buffers misses the bound on some row
            ident = np.tile(np.arange(group, dtype=np.uint8), B0)[:, None].repeat(G, 1)
            wrong, _ = A.decode_attention_beams(*to64(q, kp, vp, kg, vg), LENS, step, ident, group, c_s)
            assert (np.abs(wrong - o64) > bound[:, :, 0]).any(-1).any(-1).any()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d64", "d128"])
def test_step_over_the_table_vs_step_over_the_copied_segment(g, case):
    """Two engines on the same bf16 model, prompts, fed tokens and beam selections (3 beams, 7 steps, repeated sources): one re-orders
    its generated segment with p2t_kv_reorder and steps with p2t_llama_decode_step, the other updates the table and steps with
    p2t_llama_decode_step_beams.  Each path's last logits against the bf16 oracle teacher-forced with every row's own history, under
    test_bf16_steps_vs_bf16_oracle_and_own_forward's bound (4e-2 of the norm); the difference between the two paths is recorded."""
    from p2t_hip.generation import DecodeEngine
    model = _model(g, case, torch.bfloat16)
    m = g["meta"]["cases"][case]
    emb, mask = model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                      protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)
    B0, nb, n = emb.shape[0], 3, 7
    V = model.llama_decoder.spec.vocab_size
    rs = np.random.RandomState(3)
    toks = rs.randint(0, V, size=(n, B0 * nb))
    srcs = [np.concatenate([b * nb + rs.randint(0, nb, size=nb) for b in range(B0)]) for _ in range(n)]
    hist = [[] for _ in range(B0 * nb)]
    for s in range(n):
        hist = [hist[srcs[s][r]] + [int(toks[s][r])] for r in range(B0 * nb)]
    logits = {}
    for path in ("copy", "ancestry"):
        eng = DecodeEngine(model.llama_decoder, B0, nb, emb.shape[1], 64, beam_cache="ancestry" if path == "ancestry" else None)
        eng.prefill(*eng.compact(emb, mask))
        for s in range(n):
            src = torch.from_numpy(srcs[s].astype(np.int64)).to(dev())
            eng.ancestry_update(src) if path == "ancestry" else eng.reorder(src)
            eng.next_tokens.copy_(torch.from_numpy(toks[s].astype(np.int64)).to(dev()))
            eng.feed(eng.next_tokens)
            eng.decode_step()
        logits[path] = to_np(eng.logits[:, :V].float())
        assert (eng.k_alt is None) == (path == "ancestry")
    esm, llama, ad = specs.EsmSpec(**m["esm"]), specs.LlamaSpec(**m["llama"]), specs.AdapterSpec(**m["adapter"])
    W = model_weights(esm, llama, ad, m["weight_seed"], lm_head=True)
    rep = lambda a: np.repeat(to_np(a), nb, axis=0)
    forced = np.concatenate([np.array(hist, dtype=np.int64), np.zeros((B0 * nb, 1), dtype=np.int64)], 1)
    _, ref = O.generate_greedy(llama, W, rep(emb), rep(mask), n + 1, (), g["meta"]["pad_id"], prec=O.BF16, forced=forced)
    for path in ("copy", "ancestry"):
        print(f"{case} {path}: rel error of the last step's logits against the bf16 oracle {rel(logits[path], ref[n]):.3g}")
        observe(f"beam_ancestry_step[{case}].{path}_vs_bf16oracle.logits", rel(logits[path], ref[n]), 4e-2)
    observe(f"beam_ancestry_step[{case}].ancestry_vs_copy.logits", rel(logits["ancestry"], logits["copy"]), 4e-2)
