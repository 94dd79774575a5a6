"""The kernels of prompt-lookup decoding, one by one (csrc/attn_decode.hip, csrc/llama_decode.hip, csrc/gemm_skinny.hip, csrc/lookup.hip):

* p2t_attention_decode_multi: for every (row, query j) the bits of p2t_attention_decode_rows on the same cache with the row's counter at
  s + j -- the matrix-pipe form (bf16; the fp8 prompt segment) and the lane-per-key form (f32, bf16); counters on both sides of the 64-key
  tile and prompt lengths 0 .. 100 mixed in one launch; NaN behind the step's last token changes nothing, and a large value in what a
  LATER token of the same step wrote reaches no earlier query;
* the rotation + append and the whole p2t_llama_decode_step_multi against Q sequential p2t_llama_decode_step_rows fed the same tokens;
* p2t_lookup_draft_rows / p2t_lookup_verify_rows against tests/lookup_reference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lookup_reference as R
from gpu_util import build_model, dev, observe, rel, to_dev, to_np
from p2t_hip import specs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = [0, 5, 57, 60, 63, 64, 100]            # the rows' counters, one launch: G = 128
LENS = [0, 1, 63, 64, 65, 100, 64]             # their prompt lengths: Tp = 128
G_CAP, TP = 128, 128


class AttnCase:
    """q / caches for B0 = len(STEPS) rows and Q tokens per row, as device tensors of `dt`; NaN behind every valid prefix (the prompt's
    and, in the generated segment, behind the step's last token s + Q - 1)."""

    def __init__(self, d, nh, nkv, Q, dt, fp8=False, seed=0):
        from p2t_hip import ops
        self.d, self.nh, self.nkv, self.Q, self.dt, self.dp = d, nh, nkv, Q, dt, ops.head_dim_padded(d)
        B0, dp = len(STEPS), self.dp
        rs = np.random.RandomState(seed + d + nh + 7 * Q)
        f = lambda *s: (rs.randn(*s) * 0.7).astype(np.float32)
        pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (dp - d,), np.float32)], -1)
        q, kp, vp, kg, vg = f(B0 * Q, nh, d), f(B0, nkv, TP, d), f(B0, nkv, TP, d), f(B0, nkv, G_CAP, d), f(B0, nkv, G_CAP, d)
        kp, vp = pad(kp), pad(vp)
        self.kg_np, self.vg_np = pad(kg), pad(vg)
        for b in range(B0):
            self.kg_np[b, :, STEPS[b] + Q:] = np.nan
            self.vg_np[b, :, STEPS[b] + Q:] = np.nan
        self.q = to_dev(pad(q), dt)
        self.lens, self.steps = to_dev(np.array(LENS, np.int32)), to_dev(np.array(STEPS, np.int32))
        self.ks = self.vs = None
        if fp8:                                  # the prefill's store (p2t_kv_quant_store) writes positions < T only: NaN bytes (0x7f) behind them
            from p2t_hip import _lib
            from p2t_hip.ops import ptr, stream
            z8 = lambda *s: torch.full(s, 0x7F, dtype=torch.uint8, device=dev())
            self.kp, self.vtp, self.ks, self.vs = z8(B0, nkv, TP, dp), z8(B0, nkv, dp, TP), z8(B0, nkv, TP), z8(B0, nkv, TP)
            for b in range(B0):
                if LENS[b] == 0:
                    continue
                args = [t[b:b + 1] for t in (self.kp, self.vtp, self.ks, self.vs)]
                kb, vb = to_dev(kp[b:b + 1, :, :LENS[b]], dt).contiguous(), to_dev(vp[b:b + 1, :, :LENS[b]], dt).contiguous()
                _lib.call("p2t_kv_quant_store", ptr(kb), ptr(vb), 1, nkv, LENS[b], d, TP, *[ptr(a) for a in args], stream())
        else:
            for b in range(B0):
                kp[b, :, LENS[b]:] = np.nan
                vp[b, :, LENS[b]:] = np.nan
            self.kp, self.vtp = to_dev(kp, dt), to_dev(np.ascontiguousarray(vp.transpose(0, 1, 3, 2)), dt)
        self.set_gen(self.kg_np, self.vg_np)

    def set_gen(self, kg, vg):
        self.kg, self.vtg = to_dev(kg, self.dt), to_dev(np.ascontiguousarray(vg.transpose(0, 1, 3, 2)), self.dt)

    def _call(self, name, q, steps, rows, use_mfma, *more):
        from p2t_hip import _lib, ops
        from p2t_hip.ops import ptr, stream
        QO = ops.round_up(self.nh * self.d, 64)
        out = torch.full((rows, QO), 7.0, dtype=self.dt, device=dev())
        bf = self.dt == torch.bfloat16
        _lib.call(name, ptr(q), ptr(self.kp), ptr(self.vtp), ptr(self.kg), ptr(self.vtg), ptr(self.lens), ptr(steps), len(STEPS), self.nh, self.nkv, self.d,
                  TP, G_CAP, float(self.d ** -0.5), int(bf), ops.dt_of(self.dt), use_mfma, ptr(out), QO, ptr(self.ks) if self.ks is not None else None,
                  ptr(self.vs) if self.vs is not None else None, *more, stream())
        return out[:, : self.nh * self.d]

    def multi(self, use_mfma):
        return self._call("p2t_attention_decode_multi", self.q, self.steps, len(STEPS) * self.Q, use_mfma, self.Q)

    def rows(self, j, use_mfma):
        """p2t_attention_decode_rows for token j of every row: the counters at s + j"""
        q = self.q.view(len(STEPS), self.Q, self.nh, self.dp)[:, j].contiguous()
        return self._call("p2t_attention_decode_rows", q, (self.steps + j).contiguous(), len(STEPS), use_mfma)


SHAPES = [(64, 4, 2, 8), (128, 8, 2, 8), (128, 8, 2, 3), (128, 5, 1, 3), (128, 5, 1, 4), (64, 4, 2, 1), (48, 4, 2, 3), (16, 4, 2, 5), (64, 16, 1, 3)]


@pytest.mark.parametrize("form", ["bf16_mfma", "f32", "bf16_lanes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d-nh%d-nkv%d-q%d" % s)
def test_attention_multi_is_the_per_row_attention_bit_for_bit(shape, form):
    """(d, heads, kv heads, Q): 8 queries of GQA 2 in one chunk; GQA 4 in two chunks; a last chunk with idle slots; GQA 5 (16 % 5 idle
    slots) with a whole and a cut chunk; Q = 1; head_dim 48 / 16 through their padded forms; 16 heads per kv head (one query per chunk)."""
    d, nh, nkv, Q = shape
    dt, use_mfma = (torch.float32, 0) if form == "f32" else (torch.bfloat16, int(form == "bf16_mfma"))
    c = AttnCase(d, nh, nkv, Q, dt)
    got = c.multi(use_mfma).view(len(STEPS), Q, -1)
    assert torch.isfinite(got.float()).all()                           # the NaN behind every prefix reached nothing
    for j in range(Q):
        want = c.rows(j, use_mfma)
        assert torch.equal(got[:, j], want), (j, (got[:, j].float() - want.float()).abs().max().item())
    # what a later token of the SAME step wrote must not reach an earlier query: 1e4 in the entries behind token j0
    base = got.clone()
    for j0 in sorted({0, Q // 2}):
        if j0 == Q - 1:
            continue
        kg, vg = c.kg_np.copy(), c.vg_np.copy()
        for b, s in enumerate(STEPS):
            kg[b, :, s + j0 + 1:s + Q, :d] = 1e4
            vg[b, :, s + j0 + 1:s + Q, :d] = 1e4
        c.set_gen(kg, vg)
        again = c.multi(use_mfma).view(len(STEPS), Q, -1)
        assert torch.equal(again[:, : j0 + 1], base[:, : j0 + 1]), j0
        assert not torch.equal(again[:, j0 + 1:], base[:, j0 + 1:])   # ... and does reach the later ones


@pytest.mark.parametrize("shape", [(64, 4, 2, 8), (128, 5, 1, 4)], ids=lambda s: "d%d-nh%d-nkv%d-q%d" % s)
def test_attention_multi_over_the_fp8_prompt_segment(shape):
    d, nh, nkv, Q = shape
    c = AttnCase(d, nh, nkv, Q, torch.bfloat16, fp8=True)
    got = c.multi(1).view(len(STEPS), Q, -1)
    assert torch.isfinite(got.float()).all()
    for j in range(Q):
        assert torch.equal(got[:, j], c.rows(j, 1)), j


# ---------------------------------------------------------------------------------------------
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


STEP_CASES = [("d64", "bf16", True), ("d64", "bf16", False), ("d128", "bf16", True), ("qwen3", "bf16", True), ("d16", "bf16", True),
              ("d64", "f32", True), ("qwen3", "f32", True), ("d128", "f32", True), ("d64", "fp8", True), ("d64", "mxfp4", True), ("d64", "bf16_head_fp8", True)]


@pytest.mark.parametrize("case,form,fuse", STEP_CASES)
def test_step_multi_is_q_sequential_row_steps(g, case, form, fuse):
    """Q = 4 tokens per row through ONE p2t_llama_decode_step_multi against 4 sequential p2t_llama_decode_step_rows fed the same tokens, from
    the same cache (the prompt prefilled; the rows' counters at 0, 5 and 62 over the same generated entries, so one row crosses the
    64-key tile inside the step): the cache entries s .. s + 3 of every layer and the logits.  Every launch computes its rows
    independently of how many rows it has -- the weight-streaming GEMMs for up to 64 rows, the norms, the quantisers, the attention --
    so the bf16 / fp8 / MXFP4 forms are held to EQUAL BITS; the fp32 model runs the general GEMM, whose launch form may depend on the row
    count: 2e-4 on the logits (the project's logits bound), 1e-5 on the cache entries (|entries| < 8, f32 sums of a few hundred terms).
    Measured: equal bits in fp32 as well (3 against 12 rows take the same form); the test prints what it finds."""
    from p2t_hip import lookup
    from p2t_hip.generation import DecodeEngine
    from p2t_hip.ops import ptr, stream
    from p2t_hip._lib import call
    f32 = form == "f32"
    model = _model(g, case, torch.float32 if f32 else torch.bfloat16)
    if form in ("fp8", "mxfp4"):
        model.set_gemm_dtype(form)
    dec, Q, B = model.llama_decoder, 4, 3
    emb, mask = model(input_ids=to_dev(g["input_ids"]), attention_mask=to_dev(g["attention_mask"]), protein_input_ids=to_dev(g["protein_input_ids"]),
                      protein_attention_mask=to_dev(g["protein_attention_mask"]), return_decoder_inputs=True)
    V, pad = dec.spec.vocab_size, g["meta"]["pad_id"]
    head = "fp8" if form == "bf16_head_fp8" else None
    em = lookup.LookupEngine(dec, B, emb.shape[1], 100, Q - 1, 2, (), pad, fuse_rope=fuse, lm_head_dtype=head)
    er = DecodeEngine(dec, B, 1, emb.shape[1], 128, True, fuse, lm_head_dtype=head)
    assert em.G == er.G == 128 and em.k_gen.shape == er.k_gen.shape
    torch.manual_seed(5)
    fill_k, fill_v = torch.randn_like(em.k_gen.float()) * 0.5, torch.randn_like(em.vt_gen.float()) * 0.5
    steps0 = torch.tensor([0, 5, 62], dtype=torch.int32, device=dev())
    toks = torch.randint(0, V, (B, Q), device=dev(), dtype=torch.int64)
    for e in (em, er):
        e.prompt(emb, mask)
        e.k_gen.copy_(fill_k)
        e.vt_gen.copy_(fill_v)
    em.row_step.copy_(steps0)
    em.step_tokens.copy_(toks)
    call("p2t_llama_embed_tokens", C.byref(em.e["cfg"]), C.byref(em.e["w"]), ptr(em.step_tokens), B * Q, ptr(em.x), stream())
    em.step_multi()
    assert torch.equal(em.row_step, steps0)                            # read only
    got = em.logits.view(B, Q, -1)[:, :, :V].float()
    row_step, want = steps0.clone(), []
    for j in range(Q):
        er.feed(toks[:, j].contiguous())
        call("p2t_llama_decode_step_rows", C.byref(er.e["cfg"]), C.byref(er.e["w"]), *er.step_weights(), C.byref(er.cache), ptr(er.x), ptr(er.logits),
             er.ld_logits, er.flags, ptr(er.ws), er.ws.numel(), ptr(row_step), None, stream())
        want.append(er.logits[:, :V].float().clone())
    want = torch.stack(want, 1)
    assert torch.equal(row_step, steps0 + Q)
    # the generated segment: entries s .. s + Q - 1 of every layer from the step, everything else as it was
    same_k, same_v = torch.equal(em.k_gen, er.k_gen), torch.equal(em.vt_gen, er.vt_gen)
    dk, dv = (em.k_gen.float() - er.k_gen.float()).abs().max().item(), (em.vt_gen.float() - er.vt_gen.float()).abs().max().item()
    dl = (got - want).abs().max().item()
    print(f"step_multi[{case},{form},fuse={fuse}] cache bit-equal: {same_k and same_v} (max |dK| {dk:.2e}, |dV| {dv:.2e}); logits bit-equal: "
          f"{torch.equal(got, want)} (max |d| {dl:.2e}, rel {rel(to_np(got), to_np(want)):.2e})")
    for b, s in enumerate(steps0.tolist()):
        assert not torch.equal(em.k_gen[:, b, :, s:s + Q].float(), fill_k[:, b, :, s:s + Q].to(em.k_gen.dtype).float())      # ... were written
        keep = torch.ones(em.G, dtype=torch.bool, device=dev())
        keep[s:s + Q] = False
        assert torch.equal(em.k_gen[:, b][:, :, keep], fill_k.to(em.k_gen.dtype)[:, b][:, :, keep])
        assert torch.equal(em.vt_gen[:, b][:, :, :, keep], fill_v.to(em.vt_gen.dtype)[:, b][:, :, :, keep])
    assert torch.isfinite(got).all()
    if f32:
        assert dk < 1e-5 and dv < 1e-5 and dl < 2e-4
    else:
        # (bounds the issue names, recorded; the assertion that holds is the stronger one: equal bits)
        observe(f"lookup_step_multi[{case},{form}].vs_sequential_rows.logits", rel(to_np(got), to_np(want)), 8e-2 if form in ("fp8", "mxfp4") else 3e-2)
        assert same_k and same_v and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------
def _histories(rs, BB, G, vocab):
    """random rows over a small vocabulary (n-grams repeat); counters 0, 1, G - 2, G - 1 among them; some rows finished"""
    out = rs.randint(0, vocab, size=(BB, G)).astype(np.int64)
    steps = rs.randint(0, G - 1, size=BB).astype(np.int32)
    steps[:4] = [0, 1, G - 2, G - 1]
    fin = (rs.rand(BB) < 0.2).astype(np.int32) * rs.randint(1, 4, size=BB).astype(np.int32)
    fin[:3] = 0
    fin[3] = R.LIMIT_BIT                           # the row at G - 1 has written its last token
    return out, steps, fin


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_draft_kernel_vs_numpy(k, n):
    from p2t_hip import _lib
    from p2t_hip.ops import ptr, stream
    BB, G, pad, Q = 40, 64, 99, k + 1
    rs = np.random.RandomState(10 * k + n)
    out, steps, fin = _histories(rs, BB, G, 5)
    out[5, :40] = np.arange(40) + 7                 # no repeat at all: c = 0
    steps[5], fin[5] = 39, 0
    od, sd, fd = to_dev(out), to_dev(steps), to_dev(fin)
    toks, lens = torch.full((BB + 1, Q), -7, dtype=torch.int64, device=dev()), torch.full((BB + 1,), -7, dtype=torch.int32, device=dev())
    _lib.call("p2t_lookup_draft_rows", ptr(od), G, ptr(sd), ptr(fd), BB, G, k, n, pad, ptr(toks), ptr(lens), stream())
    got_t, got_c = to_np(toks), to_np(lens)
    assert (got_t[BB] == -7).all() and got_c[BB] == -7 and np.array_equal(to_np(od), out)
    seen = set()
    for r in range(BB):
        want_t, want_c = ([pad] * Q, 0) if fin[r] else R.step_tokens(out[r, : steps[r] + 1], k, n, pad)
        assert got_t[r].tolist() == want_t and got_c[r] == want_c, (r, steps[r], fin[r])
        seen.add(want_c)
    assert {0, k} <= seen


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_verify_kernel_vs_numpy(k, dt):
    """Random rows: full accepts, rejects at every place, eos ids inside runs, limits inside runs, finished rows, a row at G - 2 with room
    for one token, a row whose counter says G - 1 without its limit bit (nothing may be written behind the table), two- and three-way
    ties between the draft's token and a lower / higher index, a larger value in a column behind V."""
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    BB, G, V, ld, pad, Q = 48, 64, 300, 320, 299, k + 1
    rs = np.random.RandomState(k)
    out, steps, fin = _histories(rs, BB, G, 6)
    fin[4], steps[4] = 0, G - 1                     # inconsistent on purpose: live at the table's last index
    limits = np.where(rs.rand(BB) < 0.5, G, np.minimum(G, steps + 1 + rs.randint(1, Q + 1, size=BB))).astype(np.int32)
    limits[2] = G
    eos = [3, 5]
    toks = np.full((BB, Q), pad, np.int64)
    clen = np.zeros(BB, np.int32)
    choice = rs.randint(0, 6, size=(BB, Q)).astype(np.int64)
    for r in range(BB):
        t, c = R.step_tokens(out[r, : steps[r] + 1], k, 2, pad)
        toks[r], clen[r] = t, c
        agree = rs.randint(0, Q + 1)                # the model agrees with the first `agree` draft tokens (then whatever it drew)
        choice[r, :min(agree, c)] = toks[r, 1:1 + min(agree, c)]
    lg = rs.randn(BB * Q, ld).astype(np.float32)
    lg[:, V:] = 50.0                                # padding columns: never chosen
    for i in range(BB * Q):
        tok = int(choice.reshape(-1)[i])
        lg[i, tok] = 9.0
        if i % 3 == 0:
            lg[i, tok + 1 + i % 200] = 9.0          # a tie with a higher index: the lowest wins
        if i % 5 == 0 and tok > 0:
            lg[i, rs.randint(0, tok)] = 8.75        # a near miss below it (exact in bf16)
    want_choice = R.argmax_rows(to_np(to_dev(lg, dt)), V).reshape(BB, Q)
    assert np.array_equal(want_choice, choice)
    table = np.full((BB + 1, G), -1, np.int64)
    table[:BB] = out
    d = dict(lg=to_dev(lg, dt), toks=to_dev(toks), clen=to_dev(clen), eos=to_dev(np.array(eos, np.int64)), fin=to_dev(fin), steps=to_dev(steps),
             limits=to_dev(limits), out=to_dev(table), nxt=torch.full((BB,), -5, dtype=torch.int64, device=dev()),
             stats=torch.zeros((BB, 3), dtype=torch.int32, device=dev()) + 100, scratch=torch.zeros((BB * Q,), dtype=torch.int32, device=dev()))
    _lib.call("p2t_lookup_verify_rows", ptr(d["lg"]), ops.dt_of(dt), ld, V, BB, Q, ptr(d["toks"]), ptr(d["clen"]), ptr(d["eos"]), len(eos), pad, ptr(d["fin"]),
              ptr(d["nxt"]), ptr(d["out"]), G, ptr(d["steps"]), ptr(d["limits"]), G, ptr(d["stats"]), ptr(d["scratch"]), stream())
    assert np.array_equal(to_np(d["scratch"]).reshape(BB, Q), choice)
    got_out, got_steps, got_fin, got_next, got_stats = (to_np(d[x]) for x in ("out", "steps", "fin", "nxt", "stats"))
    assert (got_out[BB] == -1).all()
    kinds = set()
    for r in range(BB):
        new, bits, a = R.verify(choice[r], toks[r], int(clen[r]), int(steps[r]), int(limits[r]), eos, finished=int(fin[r]))
        row = out[r].copy()
        row[steps[r] + 1:steps[r] + 1 + len(new)] = new
        assert got_out[r].tolist() == row.tolist(), r
        assert got_steps[r] == steps[r] + len(new) and got_fin[r] == (fin[r] | bits), (r, got_fin[r], bits)
        assert got_next[r] == (pad if (fin[r] or not new) else new[-1])
        assert got_stats[r].tolist() == ([100, 100, 100] if fin[r] else [101, 100 + clen[r], 100 + a]), r
        if not fin[r]:
            kinds.add(("full" if a == clen[r] and clen[r] else "part" if a else "none", bits))
    assert got_steps[4] == G - 1 and got_fin[4] == R.LIMIT_BIT                # nothing behind the table
    assert {b for _, b in kinds} >= {0, R.EOS_BIT, R.LIMIT_BIT} and {m for m, _ in kinds} == ({"full", "none"} if k == 1 else {"full", "part", "none"})
