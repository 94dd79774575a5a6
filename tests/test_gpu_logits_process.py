"""p2t_logits_process (csrc/logits_process.hip) against tests/logits_process_reference.py, bit for bit: every operation of the contract
is one IEEE f32 operation, so there is no tolerance.  Shapes: the scalar path (a pitch that is no multiple of 16 bytes), the 16-byte
path in bf16 with a tail and with more columns than one pass of the block, a bf16 view and an output view offset by one element
(unaligned bases).  BB = 3, G = 64; step counters 0, 1, 2, 3, 17, 63 and two outside [0, G] (clamped); every processor alone and all
together; n-gram sizes 1, 2, 3; histories from a small alphabet (duplicates, repeated n-grams) holding an id >= V and a negative id,
which name no column; columns V .. ld_out keep a sentinel; a second launch gives the same bits."""
import numpy as np
import pytest
import torch

import logits_process_reference as LR
from gpu_util import SENT, dev, to_dev, to_np

pytestmark = pytest.mark.gpu
BB, G = 3, 64
STEPS = (0, 1, 2, 3, 17, 63)
# (V, ld, dtype, element offset of the logits view, ld_out, element offset of the output view)
SHAPES = {
    "f32-scalar": (33, 33, torch.float32, 0, 40, 0),
    "bf16-vec": (300, 320, torch.bfloat16, 0, 320, 0),
    "bf16-vec-2051": (2051, 2056, torch.bfloat16, 0, 2064, 0),
    "bf16-view+1": (300, 320, torch.bfloat16, 1, 320, 0),
    "f32-vec-out+1": (300, 320, torch.float32, 0, 320, 1),
}


def _alphabet(V):
    return [0, 4, 9, V // 2, V - 2, V - 1]


def _setting(V, which):
    a = _alphabet(V)
    words = [[a[1], a[2]], [a[2], a[1], a[3]], [a[5]], [a[0], V + 1], [a[3], a[3], a[3], a[4]], [21]]
    full = dict(penalty=1.3, ngram=2, min_new=3, eos_ids=[a[0], V - 3, V], words=words)
    return {"penalty": dict(penalty=1.3), "penalty<1": dict(penalty=0.75), "ngram1": dict(ngram=1), "ngram2": dict(ngram=2), "ngram3": dict(ngram=3),
            "words": dict(words=words), "min_new": dict(min_new=3, eos_ids=full["eos_ids"]), "all-n1": dict(full, ngram=1), "all-n2": full,
            "all-n3": dict(full, ngram=3)}[which]


def _data(shape):
    V, ld, dt, off, ld_out, _ = SHAPES[shape]
    rs = np.random.RandomState(V + off)
    x = (rs.randn(BB, ld) * 3).astype(np.float32)
    x[:, 4] = 0.0
    x[:, 9] = -np.inf
    x[0, V - 1] = x[0, V - 2]
    x[1, :8] = -np.abs(x[1, :8])
    flat = torch.zeros((BB * ld + 8,), dtype=dt, device=dev())
    lg = flat[off: off + BB * ld].view(BB, ld)
    lg.copy_(to_dev(x))
    xs = to_np(lg)[:, :V].astype(np.float32)                   # the stored values (bf16-rounded where the row is bf16)
    a = _alphabet(V)
    tok = np.array(a, dtype=np.int64)[rs.randint(0, len(a), size=(BB, G))]
    tok[0, 1], tok[1, 2], tok[2, 0], tok[0, 30] = V + 3, -4, V, 2 ** 40
    tok[1, 10:16] = [a[1], a[2], a[1], a[2], a[1], a[2]]       # a repeated 2- and 3-gram for certain
    tok[2, 14:17] = a[3]
    return lg, xs, tok


def _launch(lg, V, tok_d, ld_tok, step, out, s):
    from p2t_hip import _lib, ops
    from p2t_hip.ops import ptr, stream
    ids, offs = LR.pack_words(s.get("words", []))
    eos = np.array(s.get("eos_ids", []), dtype=np.int64)
    ids_d, offs_d, eos_d = to_dev(ids), to_dev(offs), to_dev(eos)
    step_d = torch.tensor([step], dtype=torch.int32, device=dev())
    opt = lambda t: ptr(t) if t.numel() else None
    _lib.call("p2t_logits_process", ptr(lg), ops.dt_of(lg), lg.stride(0), V, BB, ptr(tok_d), ld_tok, ptr(step_d), G, ptr(out), out.stride(0),
              float(s.get("penalty", 1.0)), int(s.get("ngram", 0)), int(s.get("min_new", 0)), opt(eos_d), eos.size, opt(ids_d),
              ptr(offs_d) if len(ids) else None, len(offs) - 1 if len(ids) else 0, len(ids), stream())
    torch.cuda.synchronize()


def _out(shape):
    _, _, _, _, ld_out, off = SHAPES[shape]
    flat = torch.full((BB * ld_out + 8,), SENT, dtype=torch.float32, device=dev())
    return flat, flat[off: off + BB * ld_out].view(BB, ld_out)


@pytest.mark.parametrize("which", ["penalty", "penalty<1", "ngram1", "ngram2", "ngram3", "words", "min_new", "all-n1", "all-n2", "all-n3"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_the_restatement_bitwise(shape, which):
    V = SHAPES[shape][0]
    lg, xs, tok = _data(shape)
    s = _setting(V, which)
    ld_tok = G + 6 if which == "all-n2" else G                 # a token table wider than G
    tok_w = np.full((BB, ld_tok), 7, dtype=np.int64)
    tok_w[:, :G] = tok
    tok_d = to_dev(tok_w)
    before = to_np(lg).copy()
    changed = 0
    for step, cur in [(n, n) for n in STEPS] + [(G + 136, G), (-5, 0)]:
        flat, out = _out(shape)
        _launch(lg, V, tok_d, ld_tok, step, out, s)
        got = to_np(out)
        want = LR.process(xs, [tok[r, :cur] for r in range(BB)], **s)
        assert np.array_equal(got[:, :V].view(np.uint32), want.view(np.uint32)), (shape, which, step)
        assert (got[:, V:] == SENT).all(), (shape, which, step)                       # columns V .. ld_out are never written
        f = to_np(flat)
        off = SHAPES[shape][5]
        assert (f[:off] == SENT).all() and (f[off + got.size:] == SENT).all()
        flat2, out2 = _out(shape)
        _launch(lg, V, tok_d, ld_tok, step, out2, s)
        assert torch.equal(flat.view(torch.int32), flat2.view(torch.int32)), (shape, which, step)
        changed += int((want.view(np.uint32) != xs.view(np.uint32)).sum())
    assert changed > 0                                                                # the setting did something at these histories
    assert np.array_equal(to_np(lg).view(np.uint32), before.view(np.uint32))          # the stored logits are never edited
    assert np.array_equal(to_np(tok_d), tok_w)


def test_nothing_active_is_a_copy():
    lg, xs, tok = _data("bf16-vec")
    flat, out = _out("bf16-vec")
    _launch(lg, 300, to_dev(tok), G, 17, out, {})
    assert np.array_equal(to_np(out)[:, :300].view(np.uint32), xs.view(np.uint32)) and (to_np(out)[:, 300:] == SENT).all()
