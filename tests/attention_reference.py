"""What the row-by-row attention tests (tests/test_gpu_attention_rows.py, tests/test_attention_reference_host.py) are built from, plain
numpy / torch on the CPU:

* `reference`: encoder_ops_reference.attention_fwd_bwd64 (the one fp64 implementation; documents and the bound terms live there);
* the cases: shapes, masks and packed-row layouts at which each kernel's structure is crossed, as data (`Case`);
* the inputs: two witnesses (q = 0, so every visible probability is exactly 1 / n_visible, and v names the key that was read), peaked
  random inputs whose boundary keys dominate a partner row, and the lazy-rescale cases;
* `restate_forward`: the MFMA kernels' forward arithmetic restated in numpy (64-key tiles, fp32 scores, P rounded to bf16 for the PV
  product, lazy rescale with slack 8 per 32-query group, bf16 output), with switches for the forms the kernels differ in and a list of
  deliberate corruptions the row check has to flag.

Flat random inputs cannot carry these tests: with a flat softmax one key is worth 1 / n and no metric sees it dropped."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from encoder_ops_reference import attention_fwd_bwd64
from p2t_hip.synth import bf16_round

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
# a dominant key is BETA * (its partner query).  diag: every key is one, the other scores of a row are BETA q[i].q[j] ~ d^-1/2 of the diagonal one
# and the diagonal key holds 0.4 to 0.9 of its row; boundary: the other keys are uniform(-4, 4) (scores of sigma 5.3, maximum near 17) and the
# chosen key's score is 7.7 BETA
BETA = {"diag": 0.875, "boundary": 3.0}
P_MIN = 0.25                                             # ... and holds at least this much of the partner row's probability


def bf16(a):
    """a rounded to bf16 (round to nearest even), as fp32."""
    return bf16_round(np.asarray(a, dtype=np.float32))


# ---- cases ----------------------------------------------------------------------------------------------------------------------
G_T, G_LENS = 321, [321, 320, 257, 256, 193, 129, 128, 65, 64, 63, 33, 1]
H_T, H_LENS = 641, [641, 640, 577, 576, 513, 512, 449, 385, 384, 321, 257, 256, 255, 193, 129, 65, 1]
DOC_T = 641
DOC_ROWS = ([1, 63, 1, 130, 301, 1, 65], [512, 1, 128], [1] * DOC_T, [DOC_T])     # test_gpu_packed_sft.ROW_LENS cut to 641; 1-token documents; one document
MASK_KINDS = ("full", "hole", "tile", "first", "key0", "single")
SHAPES = {  # name: (T, nh, nkv, d)
    "g64": (G_T, 4, 1, 64), "g128": (G_T, 2, 2, 128), "g24": (G_T, 4, 1, 24), "g40": (G_T, 3, 3, 40), "h64": (H_T, 6, 2, 64),
    "doc64": (DOC_T, 4, 1, 64), "doc128": (DOC_T, 2, 2, 128),
}
FLAVOURS = ("v_pos", "v_tile", "diag", "boundary")
RESCALE = ("rescale12", "rescale40")
RESCALE_ROWS, RESCALE_KEYS = 192, 128                   # the 32-query group 192..223 and its partner keys 128..159


def mask_row(kind: str, T: int) -> np.ndarray:
    m = np.ones(T, dtype=np.int64)
    if kind == "hole":
        m[60:71] = 0                                     # crosses the edge of key tile 0
    elif kind == "tile":
        m[192:256] = 0                                   # a wholly hidden 64-key tile in the middle
    elif kind == "first":
        m[0:70] = 0                                      # a hidden first tile and a bit: the left-padded SFT prompt (causal: rows 0..69 see nothing)
    elif kind == "key0":
        m[0] = 0
    elif kind == "single":
        m[:] = 0
        m[T - 1] = 1
    else:
        assert kind == "full", kind
    return m


@dataclass(frozen=True)
class Case:
    shape: str
    layout: str                                          # "lens" (right-padded rows of G_LENS / H_LENS), "masks" (one row per MASK_KINDS), "docs"
    causal: bool
    flavour: str
    T: int = field(init=False)
    nh: int = field(init=False)
    nkv: int = field(init=False)
    d: int = field(init=False)

    def __post_init__(self):
        for nm, val in zip(("T", "nh", "nkv", "d"), SHAPES[self.shape]):
            object.__setattr__(self, nm, val)

    @property
    def name(self):
        return f"{self.shape}-{self.layout}-{'causal' if self.causal else 'full'}-{self.flavour}"

    @property
    def witness(self):
        return self.flavour in ("v_pos", "v_tile")

    def mask(self) -> np.ndarray:
        T = self.T
        if self.layout == "masks":
            return np.stack([mask_row(k, T) for k in MASK_KINDS])
        if self.layout == "docs":
            return np.stack([(np.arange(T) < sum(lens)).astype(np.int64) for lens in DOC_ROWS])
        lens = H_LENS if T == H_T else G_LENS
        return np.stack([(np.arange(T) < n).astype(np.int64) for n in lens])

    def docs(self):
        """-> (start [B, T] (a padding token: a document of its own), position_ids [B, T]) or (None, None)."""
        if self.layout != "docs":
            return None, None
        start = np.tile(np.arange(self.T, dtype=np.int64), (len(DOC_ROWS), 1))
        for b, lens in enumerate(DOC_ROWS):
            t = 0
            for n in lens:
                start[b, t:t + n] = t
                t += n
        return start, np.arange(self.T, dtype=np.int64)[None] - start


def forward_cases():
    """Every input set of the GPU file's forward tests."""
    out = []
    for shape in ("g64", "g128", "g24", "h64"):
        for causal in (False, True):
            for layout in ("lens", "masks"):
                out += [Case(shape, layout, causal, f) for f in FLAVOURS]
            if shape in ("g64", "h64"):
                out += [Case(shape, "lens", causal, f) for f in RESCALE]
    out += [Case("g40", "lens", causal, f) for causal in (False, True) for f in ("v_pos", "boundary")]
    out += [Case(shape, "docs", True, f) for shape in ("doc64", "doc128") for f in FLAVOURS]
    return out


def backward_cases():
    """The input sets of the backward tests: the general set at each head dim, with and without documents."""
    out = [Case(shape, layout, causal, f) for shape in ("g64", "g128", "g24") for causal in (False, True) for layout in ("lens", "masks")
           for f in FLAVOURS]
    return out + [Case(shape, "docs", True, f) for shape in ("doc64", "doc128") for f in FLAVOURS]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def partner_head(j, g, rep):
    """The query head of kv head g whose row j the dominant key j is built from: the heads of a group take turns."""
    return g * rep + j % rep


def chosen_keys(mask_b, start_b) -> np.ndarray:
    """The `boundary` keys of one batch row: the last valid key, both sides of every 64-key tile edge, and the first visible key after
    each hole or document start -- visible keys only."""
    T = mask_b.shape[0]
    vis = mask_b != 0
    pick = np.zeros(T, bool)
    if vis.any():
        pick[np.flatnonzero(vis)[-1]] = True
    edges = np.arange(64, T, 64)
    pick[edges] = True
    pick[edges - 1] = True
    pick[1:] |= vis[1:] & ~vis[:-1]
    pick[0] = True
    if start_b is not None:
        pick |= start_b == np.arange(T)
    return np.flatnonzero(pick & vis)


def inputs(case: Case, seed: int = 0):
    """-> dict(q [B, nh, T, d], k, v [B, nkv, T, d], d_o [B, nh, T, d]) fp32 arrays of bf16-exact values (so the bf16 and the fp32 routes read
    the same numbers and share one reference), logits = ln 2 * q k^T: q carries d^-0.5 log2(e), the towers' form for bf16 models, and
    the scale form is run on the same q with scale = ln 2.  partners: list of (b, h, j), the rows whose key j must dominate."""
    mask = case.mask()
    start, _ = case.docs()
    B, (T, nh, nkv, d) = mask.shape[0], (case.T, case.nh, case.nkv, case.d)
    rep = nh // nkv
    rng = np.random.default_rng([seed, T, nh, nkv, d, int(case.causal), len(case.layout)])
    u = lambda h: rng.uniform(-4.0, 4.0, (B, h, T, d))
    uq = u(nh)
    if case.flavour in ("diag", "boundary"):
        # every query row at the norm a uniform(-4, 4) row has on average: key j = BETA q[j] then outscores key j' in row j unless q[j] and
        # q[j'] are nearly parallel, whatever their lengths drew (at d = 24 a short row among 320 longer ones is otherwise outscored)
        uq *= np.sqrt(16.0 * d / 3.0) / np.linalg.norm(uq, axis=-1, keepdims=True)
    q, k, v = bf16(uq * (d ** -0.5 * LOG2E)), bf16(u(nkv)), bf16(u(nkv))
    d_o = bf16(rng.standard_normal((B, nh, T, d)))
    d_o[d_o == 0] = 1.0                                   # non-zero on every row (every element)
    partners = []
    if case.witness:
        q[:] = 0.0
        c = min(d, 64)
        j = np.arange(T)
        idx = j % c if case.flavour == "v_pos" else (j // 64) % c
        v[:] = 0.0
        for b in range(B):
            for g in range(nkv):
                v[b, g, j, idx] = 1 + g + nkv * b         # small integers: exact in bf16
    elif case.flavour in ("diag", "boundary"):
        for b in range(B):
            keys = np.flatnonzero(mask[b]) if case.flavour == "diag" else chosen_keys(mask[b], None if start is None else start[b])
            for g in range(nkv):
                hs = partner_head(keys, g, rep)
                k[b, g, keys] = bf16(BETA[case.flavour] * q[b, hs, keys])
                partners += [(b, int(h), int(j)) for h, j in zip(hs, keys)]
    elif case.flavour in RESCALE:
        big = 14.0 if case.flavour == "rescale12" else 44.0
        rows = RESCALE_ROWS + np.arange(32)
        for g in range(nkv):
            k[0, g, RESCALE_KEYS:RESCALE_KEYS + 64] = 0.0
            qi = q[0, g * rep, rows].astype(np.float64)                                   # [32, d]
            m_before = (qi @ k[0, g, :RESCALE_KEYS].astype(np.float64).T).max(-1)          # log2 units: q carries log2(e)
            excess = np.where(np.arange(32) < 16, big, 4.0)
            beta = (m_before + excess) / (qi * qi).sum(-1)
            k[0, g, RESCALE_KEYS + np.arange(32)] = bf16(beta[:, None] * qi)
    else:
        raise ValueError(case.flavour)
    return dict(q=q, k=k, v=v, d_o=d_o, partners=partners)


def rescale_excess(case: Case, x):
    """The rescale cases' condition, from the fp64 scores (log2 units) of batch row 0, the first head of each group, rows 192..223:
    max over keys 128..191 minus max over keys 0..127.  -> [nkv, 32]."""
    rep = case.nh // case.nkv
    rows = RESCALE_ROWS + np.arange(32)
    out = []
    for g in range(case.nkv):
        s = x["q"][0, g * rep, rows].astype(np.float64) @ x["k"][0, g, :RESCALE_KEYS + 64].astype(np.float64).T
        out.append(s[:, RESCALE_KEYS:].max(-1) - s[:, :RESCALE_KEYS].max(-1))
    return np.stack(out)


def assert_conditions(case: Case, x, ref):
    """The conditions the inputs are built to meet, checked on the fp64 reference: they are conditions of the tests, not of the kernels."""
    if x["partners"]:
        b, h, j = (np.array(t) for t in zip(*x["partners"]))
        p = ref["p_diag"][b, h, j]
        assert p.min() >= P_MIN, f"{case.name}: key {j[p.argmin()]} holds only {p.min():.3f} of row (b {b[p.argmin()]}, h {h[p.argmin()]})"
    if case.flavour in RESCALE:
        e = rescale_excess(case, x)
        lo = 12.0 if case.flavour == "rescale12" else 40.0
        assert (e[:, :16] >= lo).all(), (case.name, e[:, :16].min())
        if case.flavour == "rescale12":
            assert ((e[:, 16:] > 1.0) & (e[:, 16:] < 7.0)).all(), (case.name, e[:, 16:].min(), e[:, 16:].max())
    if case.witness:
        n = ref["n_visible"]
        seen = n > 0
        assert np.abs(ref["lse"][seen] - np.log(n[seen])).max() < 1e-12


def reference(case: Case, x, backward: bool):
    """The fp64 reference of one input set with its bound terms.  The backward takes D = rowsum(dO o O) from O rounded to bf16 when the
    operands are (`o16`: what the bf16 routes are handed), else from the fp64 O: both are returned, as ref and ref["f32"]."""
    start, _ = case.docs()
    kw = dict(mask=case.mask(), causal=case.causal, c_s=LN2, docs=start, bounds=True)
    if not backward:
        return attention_fwd_bwd64(x["q"], x["k"], x["v"], None, **kw)
    ref = attention_fwd_bwd64(x["q"], x["k"], x["v"], x["d_o"], o_stored=bf16, **kw)
    ref["o16"] = bf16(ref["o"])
    ref["f32"] = attention_fwd_bwd64(x["q"], x["k"], x["v"], x["d_o"], o_stored=lambda o: o.astype(np.float32), **kw)
    return ref


# ---- the kernels' forward arithmetic, restated ---------------------------------------------------------------------------------------
CORRUPTIONS = ("drop_diag", "drop_last", "leak_end", "key_plus_64", "kv_head", "rescale_l")


def restate_forward(q, k, v, mask, causal: bool, c_s: float, docs=None, sum_rounded: bool = False, p_bf16: bool = True, out_bf16: bool = True,
                    corrupt=()):
    """The flash forward as the MFMA kernels run it, in numpy fp32: 64-key tiles; scores q k^T accumulated in fp32, in log2 units; the
    reference point m of a row set at its first visible tile and moved only when a row of its 32-query group sees a score more than 8 above it
    (every row of the group then moves to max(m, tile max)); p = exp2(s - m); row sums over p (the general kernel) or over p rounded to
    bf16 (`sum_rounded`: the hand-placed kernel sums on the matrix pipe); PV from p rounded to bf16 (`p_bf16`; False: the fp32-softmax
    kernels), fp32 accumulation; o = acc / l rounded to bf16 (`out_bf16`); lse = ln 2 (m + log2 l).
    corrupt: names from CORRUPTIONS, defects of the kind a kernel can have:
      drop_diag    rows 32 k + 31 lose their diagonal key;        drop_last   the last valid key of every batch row is hidden;
      leak_end     the hidden key `end` (1 + the last valid key) is let through for the 32 rows that start at the next multiple of 32
                   (row 0 on, where there is none);               key_plus_64 key 5 is read from key 69 (a ring slot one tile off);
      kv_head      kv head h / rep + 1 (mod nkv) is read;         rescale_l   a rescale multiplies o by alpha but not l.
    -> dict(o [B, nh, T, d], lse [B, nh, T]) fp64 arrays of the values a kernel would store."""
    f32 = np.float32
    q, k, v = (np.asarray(t, dtype=f32) for t in (q, k, v))
    B, nh, T, d = q.shape
    nkv = k.shape[1]
    rep = nh // nkv
    assert not set(corrupt) - set(CORRUPTIONS), corrupt
    fac = f32(c_s * LOG2E)
    o_out, lse_out = np.zeros((B, nh, T, d)), np.full((B, nh, T), np.inf)
    tri = np.tril(np.ones((T, T), bool))
    n_grp = -(-T // 32)
    pad = n_grp * 32 - T
    for b in range(B):
        allowed = np.broadcast_to(np.asarray(mask[b] != 0)[None, :], (T, T)).copy()
        if causal or docs is not None:
            allowed &= tri
        if docs is not None:
            allowed &= np.arange(T)[None, :] >= np.asarray(docs[b])[:, None]
        valid = np.flatnonzero(mask[b])
        end = int(valid[-1]) + 1 if valid.size else 0
        if "drop_diag" in corrupt:
            r = np.arange(31, T, 32)
            allowed[r, r] = False
        if "drop_last" in corrupt and end:
            allowed[:, end - 1] = False
        if "leak_end" in corrupt and end < T:
            r0 = -(-end // 32) * 32 if causal else 0
            r0 = r0 if r0 < T else 0
            allowed[r0:r0 + 32, end] = True
            if causal:
                allowed[r0:r0 + 32] &= tri[r0:r0 + 32]
        for h in range(nh):
            g = (h // rep + 1) % nkv if "kv_head" in corrupt else h // rep
            kk, vv = k[b, g], v[b, g]
            if "key_plus_64" in corrupt and T > 69:
                kk, vv = kk.copy(), vv.copy()
                kk[5], vv[5] = kk[69], vv[69]
            S = q[b, h] @ kk.T
            if fac != f32(1.0):
                S = S * fac
            S = np.where(allowed, S, f32(-np.inf)).astype(f32)
            m = np.full(T, -np.inf, f32)
            l = np.zeros(T, f32)
            acc = np.zeros((T, d), f32)
            for t0 in range(0, T, 64):
                st = S[:, t0:t0 + 64]
                mloc = st.max(-1)
                first = np.isneginf(m)
                grow = np.isfinite(mloc) & (first | (mloc - np.where(first, f32(0), m) > f32(8.0)))
                grp = np.pad(grow, (0, pad)).reshape(n_grp, 32).any(-1).repeat(32)[:T]
                move = grp & np.isfinite(mloc)
                m_new = np.where(move, np.where(first, mloc, np.maximum(m, mloc)), m).astype(f32)
                with np.errstate(invalid="ignore"):
                    alpha = np.where(np.isneginf(m), f32(0), np.exp2(m - m_new)).astype(f32)
                alpha = np.where(move, alpha, f32(1)).astype(f32)
                if "rescale_l" not in corrupt:
                    l = l * alpha
                acc = acc * alpha[:, None]
                m = m_new
                with np.errstate(invalid="ignore"):
                    p = np.where(np.isneginf(st), f32(0), np.exp2(st - np.where(np.isneginf(m), f32(0), m)[:, None])).astype(f32)
                pr = bf16(p) if p_bf16 else p
                l = (l + (pr if sum_rounded else p).sum(-1, dtype=f32)).astype(f32)
                acc = (acc + pr @ vv[t0:t0 + 64]).astype(f32)
            seen = l > 0
            inv = np.where(seen, f32(1) / np.where(seen, l, f32(1)), f32(0)).astype(f32)
            o = (acc * inv[:, None]).astype(f32)
            o_out[b, h] = bf16(o) if out_bf16 else o
            with np.errstate(divide="ignore", invalid="ignore"):
                lse = (f32(LN2) * (m + np.log2(l).astype(f32))).astype(f32)
            lse_out[b, h] = np.where(seen, lse, np.inf)
    return dict(o=o_out, lse=lse_out)
