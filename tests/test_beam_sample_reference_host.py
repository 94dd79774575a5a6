"""CPU: the fp64 restatement of a beam-sampling step (tests/beam_sample_reference.py):
  (a) against the torch step of the torch path (p2t_hip.generation.beam_step_torch(do_sample=True): HF's two lines) in everything that
      does not depend on the random numbers -- the processed scores, and, handed torch's own draws, the whole bookkeeping;
  (b) the law of its draws: first draws against softmax(acc), ordered pairs against the without-replacement law;
  (c) the uniform number never reaches 0 or 1 and the noise stays finite at the hash's two extremes;
  (d) the share of undecidable (prompt, step) cases among the synthetic cases of tests/test_gpu_beam_sample_select.py -- bounded here,
      by the restatement alone, so that the GPU test cannot hide a failure behind undecidable cases."""
import numpy as np
import pytest
import torch

import beam_sample_reference as R
from p2t_hip import synth


def _np_state(st, done=False):
    return dict(running=st["running"].numpy().copy(), running_idx=st["running_idx"].numpy().copy(), running_scores=st["running_scores"].numpy().copy(),
                sequences=st["sequences"].numpy().copy(), beam_idx=st["beam_idx_tab"].numpy().copy(), beam_scores=st["beam_scores"].numpy().copy(),
                is_finished=st["is_finished"].numpy().copy(), heuristic_open=st["heuristic_open"].numpy()[:, 0].copy(), done=done, steps=0)


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_eos,early_stopping,length_penalty,temperature,top_k,top_p",
                         [(0, False, 1.0, 0.7, 8, 1.0), (1, True, 0.8, 1.3, 12, 0.95), (2, "never", 2.0, 1.0, 0, 1.0), (1, False, 0.0, 2.0, 20, 0.9)])
def test_bookkeeping_of_torch_draws_equals_the_torch_step(n_eos, early_stopping, length_penalty, temperature, top_k, top_p):
    """torch.multinomial draws from torch's own stream; the restatement is handed those draws (`draws=`) and must then agree with the torch
    step in every table, and in the processed scores whatever the draws are."""
    from p2t_hip import generation as G
    B, nb, V, L, pad = 2, 3, 61, 7, 0
    eos_ids = R.case_eos(V, n_eos)
    eos = torch.tensor(eos_ids, dtype=torch.int64)
    gen = torch.Generator().manual_seed(5)
    st = G.beam_state_init(B, nb, L, pad, "cpu")
    steps = 0
    for cur in range(L):
        logits = R.case_logits(31 + n_eos, cur, B * nb, V, "f32", eos_ids)
        new, scores, src_rows, hits, go_on = G.beam_step_torch(st, torch.from_numpy(logits), cur, nb, eos, length_penalty, early_stopping, L,
                                                               do_sample=True, generator=gen, temperature=temperature, top_k=top_k, top_p=top_p)
        drawn = new.pop("drawn").numpy()
        assert drawn.shape == (B, max(2, 1 + n_eos) * nb)
        ref = R.step(logits, _np_state(st), cur, nb, eos_ids, length_penalty, early_stopping, L, pad, temperature, top_k, top_p, draws=drawn)
        r = ref["state"]
        sc = scores.numpy().astype(np.float64)
        cut = np.isinf(ref["scores"])
        assert np.array_equal(np.isinf(sc), cut), cur                                  # the kept sets
        assert (np.abs(sc[~cut] - ref["scores"][~cut]) <= ref["e_scores"][~cut] + 1e-6).all(), cur
        if not ref["decidable"].all():                                                  # a tie torch's f32 arithmetic may take either way
            break
        fin = r["is_finished"]
        assert np.array_equal(new["is_finished"].numpy(), fin)
        assert np.array_equal(new["sequences"].numpy()[fin], r["sequences"][fin]) and np.array_equal(new["beam_idx_tab"].numpy()[fin], r["beam_idx"][fin])
        assert np.allclose(new["beam_scores"].numpy()[fin], r["beam_scores"][fin], rtol=1e-6, atol=1e-5)
        if ref["running_decidable"].all():
            assert np.array_equal(new["running"].numpy(), r["running"]) and np.array_equal(new["running_idx"].numpy(), r["running_idx"])
            assert np.array_equal(src_rows.numpy(), ref["src_rows"])
            assert np.array_equal(new["running"].numpy()[:, :, cur].reshape(-1), ref["next_tokens"])
            assert np.array_equal(new["heuristic_open"].numpy()[:, 0], r["heuristic_open"])
            assert np.allclose(new["running_scores"].numpy(), r["running_scores"], rtol=1e-6, atol=1e-4)
        went_on = bool(go_on) and cur + 1 < L
        assert r["done"] == (not went_on), cur
        steps += 1
        st = new
        for k, v in (("sequences", r["sequences"]), ("beam_idx_tab", r["beam_idx"]), ("beam_scores", r["beam_scores"])):
            st[k] = torch.where(torch.from_numpy(fin).reshape(fin.shape + (1,) * (st[k].dim() - 2)), st[k], torch.from_numpy(v))
        if not went_on:
            break
    assert steps >= 3


def test_forced_draws_equal_the_torch_step_entirely():
    """One candidate with all the mass per beam and as many beams as draws: nothing is left to the random numbers.  (top_k = 1 with one
    beam, the other forced form, asks for two draws from one candidate: torch.multinomial raises there and the kernel raises bit 1;
    tests/test_gpu_beam_sample_select.py covers it.)  Here every beam has one dominant column, 80 above the rest, and keep = 2 nb draws
    over nb live beams take each beam's dominant column first."""
    from p2t_hip import generation as G
    B, nb, V, L, pad = 2, 2, 61, 4, 0
    gen = torch.Generator().manual_seed(9)
    st = G.beam_state_init(B, nb, L, pad, "cpu")
    st["running_scores"][:] = torch.tensor([[-1.0, -3.0], [-2.0, -2.5]])                  # two live beams each
    logits = R.case_logits(40, 0, B * nb, V, "f32", [])
    for r in range(B * nb):
        logits[r, 5 + r] = logits[r].max() + np.float32(80.0)
    new, scores, src_rows, hits, go_on = G.beam_step_torch(st, torch.from_numpy(logits), 0, nb, torch.tensor([], dtype=torch.int64), 1.0, False, L,
                                                           do_sample=True, generator=gen, temperature=1.0, top_k=2, top_p=1.0)
    ref = R.step(logits, _np_state(st), 0, nb, [], 1.0, False, L, pad, 1.0, 2, 1.0, seed=77)
    assert not ref["flagged"].any() and ref["decidable"].all() and ref["running_decidable"].all()
    # the first nb draws are the dominant columns (in either order), so the running rows are those two, best first
    assert np.array_equal(new["running"].numpy(), ref["state"]["running"]) and np.array_equal(src_rows.numpy(), ref["src_rows"])
    assert list(ref["next_tokens"]) == [5, 6, 7, 8]
    assert np.allclose(new["running_scores"].numpy(), ref["state"]["running_scores"], atol=1e-5)


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
def test_draws_follow_the_without_replacement_law():
    nb, V, T, k, N, keep = 3, 61, 0.7, 8, 20000, 6
    rows = R.case_logits(51, 0, nb, V, "f32", [])
    run = np.array([-1.0, -1.7, -2.4], dtype=np.float32)
    c = R.prompt_candidates(rows, run, T, k, 1.0)
    n = c["flat"].size
    assert n == nb * k
    p = np.exp(c["acc"] - c["acc"].max())
    p /= p.sum()
    first, pairs = np.zeros(n), np.zeros((n, n))
    for prompt in range(N):
        top = R.draw(c, 12345, prompt, 3, keep)["top"]
        first[top[0]] += 1
        pairs[top[0], top[1]] += 1
    sd = np.sqrt(N * p * (1 - p))
    dev = np.abs(first - N * p) / sd
    print("first draws: worst deviation %.2f binomial standard deviations over %d bins" % (dev.max(), n))
    assert (dev <= 4.5).all(), dev
    law = p[:, None] * p[None, :] / (1 - p[:, None])
    np.fill_diagonal(law, 0.0)
    best = np.argsort(-law, axis=None)[:10]
    q, got = law.reshape(-1)[best], pairs.reshape(-1)[best]
    dev2 = np.abs(got - N * q) / np.sqrt(N * q * (1 - q))
    print("ordered pairs: worst deviation %.2f binomial standard deviations over the 10 likeliest" % dev2.max())
    assert (dev2 <= 4.5).all(), dev2
    assert abs(law.sum() - 1.0) < 1e-12


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
def test_uniform_is_strictly_inside_the_unit_interval_and_the_noise_finite():
    for h23 in (0, 2 ** 23 - 1):
        u = (2 * h23 + 1) * 2.0 ** -24
        u32 = np.float32(u)
        assert float(u32) == u and 0.0 < float(u32) < 1.0                                # exact in f32, never an end point
        t = -np.log(u32, dtype=np.float32)
        g = -np.log(t, dtype=np.float32)
        assert np.isfinite(t) and t > 0 and np.isfinite(g)
        g64, e_g = R.gumbel(u)
        assert abs(float(g) - float(g64)) <= float(e_g)
    # the chain: one more link than the sampler's, 23 hash bits
    h = synth.mix64((9 + 0x9E3779B97F4A7C15) & (2 ** 64 - 1))
    h = synth.mix64(h ^ 4)
    h = synth.mix64(h ^ 2)
    h = synth.mix64(h ^ 1234567)
    assert synth.beam_sample_uniform(9, 4, 2, 1234567) == (2 * (h >> 41) + 1) * 2.0 ** -24
    us = synth.beam_sample_uniforms(9, 4, 2, np.arange(1234560, 1234570))
    assert us[7] == synth.beam_sample_uniform(9, 4, 2, 1234567) and ((us > 0) & (us < 1)).all()
    assert all(us[i] == synth.beam_sample_uniform(9, 4, 2, 1234560 + i) for i in range(10))
    assert synth.beam_sample_uniform(9, 4, 2, 1234567) != synth.beam_sample_uniform(9, 4, 3, 1234567)
    assert synth.beam_sample_uniform(2 ** 64 - 1, 2 ** 40, 0, 2 ** 31) > 0


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
def run_case(case):
    """The restatement chained on its own states -> [(decidable, flagged) per (prompt, step)].  A chain ends where a prompt is flagged:
    its state is unspecified from there (the GPU test goes on from the state the kernel left)."""
    name, V, ld, B0, nb, n_eos, dtype, steps, L, lp, es, T, k, p = case
    eos_ids = R.case_eos(V, n_eos)
    st = R.fresh_state(B0, nb, L, 0)
    out = []
    for cur in range(steps):
        if st["done"]:
            break
        vals = R.case_logits(R.case_seed(name), cur, B0 * nb, V, dtype, eos_ids)
        ref = R.step(vals, st, cur, nb, eos_ids, lp, es, L, 0, T, k, p, R.SEED, 0)
        out += list(zip(ref["decidable"], ref["flagged"]))
        if ref["flagged"].any():
            break
        st = ref["state"]
    return out


def test_undecidable_share_of_the_gpu_cases():
    per = {"f32": [], "bf16": []}
    for case in R.CASES:
        res = run_case(case)
        print(f"{case[0]}: {len(res)} cases, {sum(not d for d, _ in res)} undecidable, {sum(f for _, f in res)} flagged")
        per[case[6]] += res
    for dtype, res in per.items():
        n, bad = len(res), sum(not d for d, _ in res)
        print(f"{dtype}: {bad} undecidable of {n}")
        assert n > 20 and bad <= 0.05 * n, (dtype, bad, n)
        assert sum(1 for d, f in res if d and not f) > 20, dtype                          # and enough of them compare whole tables
