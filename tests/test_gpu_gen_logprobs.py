"""GPU: the log-probabilities of the tokens the device picks RETURN (pgv_kv_set_logprobs, generate(output_logprobs=True)), from the building
block (pgv_sample_logits_lp) up to model.generate / generate_continuous.

Two values per token (include/pgv.h): `model` = x[t] - logsumexp(x) on the raw logits, `pick` = the log of the probability the pick used.
Yardsticks: fp64 log-softmax, and HF's own processors in fp64 in HF's order (test_gpu_warpers.hf_chain).
Tolerance, from tests/test_gpu_score.py::ref64: 5e-5 + 2^-21 * max |finite score| of the row -- `model`: the raw logits; `pick`: the scores after
penalty and temperature.  The kernels use the same v_exp_f32 / v_log_f32 on max-subtracted arguments and fp32 sums as pgv_logprob_rows; the largest
processed score of the building-block inputs is 88.5 (temperature 0.2), which gives 9.2e-5.
A nucleus whose boundary lies within 1e-5 of top_p in fp64 ("open": n_lo != n_hi, test_gpu_warpers.band) has several legitimate kept counts: there the
reference is the log-softmax over the `kept` largest entries, `kept` inside the band.  How many rows are open is a property of the inputs and the
fp64 reference, computed without the device result: at most 5 % of each building-block case (the cap and the one exempt family of
tests/test_gpu_warpers.py: V = 32003, top_k 0, top_p 0.9, whose CDF steps are ~3e-5 apart) and at most 10 % of the 72 steps of the sampled model run.
"""
import numpy as np
import pytest
import torch

from test_gpu_warpers import PARAMS, _prompts, _tiny, band, hf_chain, top_n_scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def row_tol(scores: torch.Tensor) -> torch.Tensor:
    """5e-5 + 2^-21 * max |finite entry| per row of [R, V]."""
    s = scores.double()
    finite = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s))
    return 5e-5 + 2.0 ** -21 * finite.max(dim=-1).values


def bits(t) -> torch.Tensor:
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


def padded(logits: torch.Tensor) -> torch.Tensor:
    R, V = logits.shape
    out = torch.full((R, (V + 15) // 16 * 16 + 16), float("nan"), dtype=torch.float32, device=logits.device)
    out[:, :V] = logits
    return out


def lsm_at(scores: torch.Tensor, tok: torch.Tensor) -> torch.Tensor:
    """fp64 log-softmax of [R, V] scores at tok [R]."""
    return torch.log_softmax(scores.double(), -1).gather(1, tok.long()[:, None])[:, 0]


def assert_within(got, want, tol, what):
    got, want, tol = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1), torch.as_tensor(tol).double().reshape(-1)
    err = (got - want).abs()
    assert not torch.isnan(err).any(), (what, got.tolist(), want.tolist())
    worst = int(torch.argmax(err - tol))
    assert bool((err <= tol).all()), (what, float(got[worst]), float(want[worst]), float(err[worst]), float(tol[worst]))
    return float(err.max()) if err.numel() else 0.0


# ---- 1. building block vs fp64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,B", [(32003, 8), (515, 16), (1000, 3), (50, 2)])
@pytest.mark.parametrize("temp,top_k,top_p,pen", PARAMS)
def test_building_block_matches_fp64_hf_chain(ctx, V, B, temp, top_k, top_p, pen):
    """The inputs of test_warped_pick_and_kept_set_match_hf_chain.  Tokens and kept counts: bitwise pgv_sample_logits_ex.  `model`: bitwise
    pgv_logprob_rows of the same row and token, and within the tolerance of the fp64 log-softmax (a NaN in the row: NaN, as there).  `pick`: the
    fp64 log-softmax of HF's filtered scores on closed rows, of the `kept` largest entries on open ones."""
    g = torch.Generator().manual_seed(V * 7 + B)
    n_open = total = 0
    worst_m = worst_p = 0.0
    for r in range(40):
        logits = torch.randn(B, V, generator=g) * (1.5 + (r % 3))
        if r == 5:
            logits[-1, V // 2] = float("nan")
        seen = torch.randint(0, V, (B, 30), generator=g)
        u = torch.rand(B, generator=g)
        if r == 7:
            u[0] = 0.0
        x2, y = hf_chain(logits, seen, temp, top_k, top_p, pen)
        n_lo, n_hi, order = band(x2, top_p)
        closed = n_lo == n_hi
        n_open += int((~closed).sum()); total += B
        lg_d, u_d, seen_d = logits.to(DEV), u.to(DEV), seen.int().to(DEV)
        tok_ex, kept_ex = ctx.sample_logits_ex(lg_d, u_d, temp, top_k, top_p, pen, seen_d, want_kept=True)
        tok, kept, lpm, lpp = ctx.sample_logits_lp(lg_d, u_d, temp, top_k, top_p, pen, seen_d)
        assert torch.equal(tok, tok_ex) and torch.equal(kept, kept_ex), r
        lp_rows, _lse, _am = ctx.logprob_rows(padded(lg_d), tok, V)
        assert torch.equal(bits(lpm), bits(lp_rows)), (r, lpm.tolist(), lp_rows.tolist())
        tok, kept, lpm, lpp = tok.cpu().long(), kept.cpu().long(), lpm.cpu(), lpp.cpu()
        has_nan = torch.isnan(logits).any(-1)
        assert bool(torch.isnan(lpm[has_nan]).all())
        ok = ~has_nan
        worst_m = max(worst_m, assert_within(lpm[ok], lsm_at(logits[ok], tok[ok]), row_tol(logits[ok]), f"model r={r}"))
        assert bool(((n_lo <= kept) & (kept <= n_hi)).all()), (r, n_lo.tolist(), kept.tolist(), n_hi.tolist())
        want = lsm_at(y, tok)
        for b in torch.nonzero(~closed)[:, 0].tolist():
            want[b] = lsm_at(top_n_scores(x2[b], order[b], int(kept[b]))[None], tok[b:b + 1])[0]
        assert bool(torch.isfinite(lpp).all()), (r, lpp.tolist())
        worst_p = max(worst_p, assert_within(lpp, want, row_tol(x2), f"pick r={r}"))
    print(f"V={V} B={B} {temp, top_k, top_p, pen}: open rows {n_open}/{total}, max |err| model {worst_m:.3e} pick {worst_p:.3e}")
    if not (V == 32003 and top_k == 0 and top_p == 0.9):
        assert n_open <= 0.05 * total, (n_open, total)


@pytest.mark.parametrize("V,B", [(32003, 8), (515, 16), (1000, 3), (50, 2)])
@pytest.mark.parametrize("pen", [1.0, 1.3])
def test_building_block_greedy(ctx, V, B, pen):
    """greedy = 1: the arg-max of the penalised logits in fp64 where the top-two margin exceeds the tolerance; `pick` = the log-softmax of the penalised
    scores over the whole vocabulary (not the top-1 value 0); penalty 1.0: the same float as `model`; temperature / top_k / top_p / u are ignored."""
    g = torch.Generator().manual_seed(V * 11 + B)
    for r in range(10):
        logits = torch.randn(B, V, generator=g) * (1.5 + (r % 3))
        if r == 5:
            logits[-1, V // 2] = float("nan")
        seen = torch.randint(0, V, (B, 30), generator=g)
        x, _ = hf_chain(logits, seen, 1.0, 0, 1.0, pen)                     # the penalised scores (NaN -> -inf: weight 0)
        lg_d, seen_d = logits.to(DEV), seen.int().to(DEV)
        tok, kept, lpm, lpp = ctx.sample_logits_lp(lg_d, None, 0.3, 7, 0.4, pen, seen_d, greedy=True)
        tok_ex, kept_ex = ctx.sample_logits_ex(lg_d, torch.zeros(B, device=DEV), 1.0, 1, 1.0, pen, seen_d, want_kept=True)
        assert torch.equal(tok, tok_ex) and torch.equal(kept, kept_ex)
        tok, lpm, lpp = tok.cpu().long(), lpm.cpu(), lpp.cpu()
        top2 = x.topk(2, dim=-1).values
        sure = (top2[:, 0] - top2[:, 1]) > row_tol(x)
        assert torch.equal(tok[sure], x.argmax(-1)[sure]), r
        has_nan = torch.isnan(logits).any(-1)
        if pen == 1.0:
            assert torch.equal(bits(lpp), bits(lpm)), r
            ok = ~has_nan
        else:
            ok = torch.ones(B, dtype=torch.bool)
            assert bool((lpp < 0).all())
        assert_within(lpp[ok], lsm_at(x[ok], tok[ok]), row_tol(x[ok]), f"greedy pick r={r}")
        assert_within(lpm[~has_nan], lsm_at(logits[~has_nan], tok[~has_nan]), row_tol(logits[~has_nan]), f"greedy model r={r}")


# ---- 2. edges on caller logits -----------------------------------------------------------------------------------------------------------
def test_edges_on_caller_logits(ctx):
    g = torch.Generator().manual_seed(4)
    for V in (515, 32003, 50):
        B = 3
        u = torch.rand(B, generator=g).to(DEV)
        # all entries equal: -ln V, sampled over the whole vocabulary and greedy
        flat = torch.full((B, V), 0.7, device=DEV)
        for greedy in (False, True):
            tok, kept, lpm, lpp = ctx.sample_logits_lp(flat, u, 1.0, 0, 1.0, 1.0, greedy=greedy)
            assert_within(lpm.cpu(), torch.full((B,), -np.log(V)), torch.full((B,), 5e-5 + 2.0 ** -21 * 0.7), f"flat model V={V}")
            assert_within(lpp.cpu(), torch.full((B,), -np.log(V)), torch.full((B,), 5e-5 + 2.0 ** -21 * 0.7), f"flat pick V={V}")
        # one dominant logit: <= 0 and ~ 0
        dom = torch.randn(B, V, generator=g)
        dom[torch.arange(B), torch.tensor([0, V // 2, V - 1])] = 60.0
        tok, kept, lpm, lpp = ctx.sample_logits_lp(dom.to(DEV), u, 1.0, 50, 0.9, 1.0)
        assert tok.tolist() == [0, V // 2, V - 1]
        for v in (lpm.cpu(), lpp.cpu()):
            assert bool((v <= 0).all()) and bool((v > -1e-6).all()), v.tolist()
        # -inf everywhere but one entry: exactly 0
        one = torch.full((B, V), float("-inf"))
        one[torch.arange(B), torch.tensor([V - 1, 3, V // 3])] = torch.tensor([-7.5, 0.0, 1e4])
        for top_k, top_p in ((50, 0.8), (0, 1.0)):
            tok, kept, lpm, lpp = ctx.sample_logits_lp(one.to(DEV), u, 0.7, top_k, top_p, 1.0)
            assert tok.tolist() == [V - 1, 3, V // 3] and kept.tolist() == [1] * B
            assert lpm.tolist() == [0.0] * B and lpp.tolist() == [0.0] * B
        # a NaN entry: never picked, `pick` finite; `model` is what pgv_logprob_rows gives (NaN: it poisons the sum, as in torch)
        nan = torch.randn(B, V, generator=g) * 2
        nan[:, [1, V // 2]] = float("nan")
        for uu in (0.0, 0.37, 1.0 - 2.0 ** -24):
            for pen, greedy in ((1.0, False), (1.4, False), (1.4, True)):
                seen = torch.tensor([[1, V // 2, 5, 9]] * B).int().to(DEV)
                tok, kept, lpm, lpp = ctx.sample_logits_lp(nan.to(DEV), torch.full((B,), uu, device=DEV), 1.0, 0, 0.999, pen, seen, greedy=greedy)
                assert not torch.isin(tok.cpu(), torch.tensor([1, V // 2], dtype=torch.int32)).any()
                assert bool(torch.isfinite(lpp).all())
                lp_rows, _, _ = ctx.logprob_rows(padded(nan.to(DEV)), tok, V)
                assert torch.equal(bits(lpm), bits(lp_rows)) and bool(torch.isnan(lpm).all())
                x, y = hf_chain(nan, seen.cpu().long(), 1.0, 0, 1.0 if greedy else 0.999, pen)
                n_lo, n_hi, order = band(x, 1.0 if greedy else 0.999)
                if greedy:
                    assert_within(lpp.cpu(), lsm_at(x, tok.cpu()), row_tol(x), "NaN greedy pick")
                else:
                    assert bool(((n_lo <= kept.cpu()) & (kept.cpu() <= n_hi)).all())
                    want = torch.stack([lsm_at(top_n_scores(x[b], order[b], int(kept[b]))[None], tok[b:b + 1].cpu())[0] for b in range(B)])
                    assert_within(lpp.cpu(), want, row_tol(x), "NaN pick")
        # greedy WITHOUT a penalty on such a row: `pick` is `model`, the same float -- NaN (include/pgv.h); the token is still never the NaN
        tok, kept, lpm, lpp = ctx.sample_logits_lp(nan.to(DEV), None, 1.0, 0, 1.0, 1.0, greedy=True)
        assert not torch.isin(tok.cpu(), torch.tensor([1, V // 2], dtype=torch.int32)).any()
        assert tok.cpu().tolist() == torch.nan_to_num(nan, nan=float("-inf")).argmax(-1).tolist()
        assert bool(torch.isnan(lpp).all()) and torch.equal(bits(lpp), bits(lpm))
        # u = 0 and u just below 1 over the whole vocabulary: the first / the last entry; no processor: `pick` is `model` within the tolerance
        x = torch.randn(B, V, generator=g) * 2
        x[:, -1] = 3.0                                                       # the last entry's probability is far above the 2^-24 that u leaves
        for uu, want_tok in ((0.0, 0), (1.0 - 2.0 ** -24, V - 1)):
            tok, kept, lpm, lpp = ctx.sample_logits_lp(x.to(DEV), torch.full((B,), uu, device=DEV), 1.0, 0, 1.0, 1.0)
            assert tok.tolist() == [want_tok] * B and kept.tolist() == [V] * B
            ref = lsm_at(x, tok.cpu())
            assert_within(lpp.cpu(), ref, row_tol(x), f"u={uu} pick")
            assert_within(lpm.cpu(), ref, row_tol(x), f"u={uu} model")


# ---- through the model -------------------------------------------------------------------------------------------------------------------
def replay_logits(m, prompts, feats, new_ids, max_seq=128):
    """The device logits of every step when the generated ids are fed back one by one (prefill + decode_step): list of [B, V] fp32 on the host."""
    B, n = len(prompts), len(new_ids[0])
    kv, _nxt, logits = m.prefill(prompts, feats, max_seq, want_logits=True)
    out = []
    for i in range(n):
        out.append(logits.cpu().clone())
        if i + 1 < n:
            _nxt, logits = m.decode_step(kv, torch.tensor([new_ids[b][i] for b in range(B)], dtype=torch.int32, device=DEV), want_logits=True)
    return out


def check_replay(steps, prompts, new_ids, model, pick, mode, what):
    """`model` / `pick` [B, n] against fp64 on the replayed logits `steps`, the ids so far as the seen-set.  mode: ("sample", T, top_k, top_p, pen) or
    ("greedy", pen).  Returns the number of open-boundary steps; there lp(n_hi) - tol <= pick <= lp(n) + tol with n the smallest legitimate count
    that keeps the token, max(n_lo, rank + 1)."""
    B, n = len(prompts), len(new_ids[0])
    n_open = 0
    worst_m = worst_p = 0.0
    for i in range(n):
        logits = steps[i]
        tok = torch.tensor([new_ids[b][i] for b in range(B)])
        worst_m = max(worst_m, assert_within(model[:, i], lsm_at(logits, tok), row_tol(logits), f"{what}: model step {i}"))
        for b in range(B):
            seen = torch.tensor([list(prompts[b]) + list(new_ids[b][:i])])
            if mode[0] == "greedy":
                x, _ = hf_chain(logits[b:b + 1], seen, 1.0, 0, 1.0, mode[1])
                worst_p = max(worst_p, assert_within(pick[b, i], lsm_at(x, tok[b:b + 1]), row_tol(x), f"{what}: greedy pick step {i} seq {b}"))
                continue
            _, temp, top_k, top_p, pen = mode
            x2, y = hf_chain(logits[b:b + 1], seen, temp, top_k, top_p, pen)
            n_lo, n_hi, order = band(x2, top_p)
            tol = row_tol(x2)
            if top_p >= 1.0 or int(n_lo) == int(n_hi):              # no nucleus filter: no boundary to be open
                worst_p = max(worst_p, assert_within(pick[b, i], lsm_at(y, tok[b:b + 1]), tol, f"{what}: pick step {i} seq {b}"))
            else:
                n_open += 1
                rank = int(torch.nonzero(order[0] == tok[b])[0, 0])
                assert rank < int(n_hi), (what, i, b, rank, int(n_hi))
                hi = float(lsm_at(top_n_scores(x2[0], order[0], max(int(n_lo), rank + 1))[None], tok[b:b + 1])[0])
                lo = float(lsm_at(top_n_scores(x2[0], order[0], int(n_hi))[None], tok[b:b + 1])[0])
                assert lo - float(tol) <= float(pick[b, i]) <= hi + float(tol), (what, i, b, lo, float(pick[b, i]), hi)
    print(f"{what}: max |err| model {worst_m:.3e} pick {worst_p:.3e}, open steps {n_open}/{B * n}")
    return n_open


def new_ids_of(out, prompts, n):
    return [out[b, len(prompts[b]):len(prompts[b]) + n].tolist() for b in range(len(prompts))]


# ---- 3. sampled ----------------------------------------------------------------------------------------------------------------------------
def test_generate_sampled_logprobs(ctx):
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(2), 20, (3, 40, 0))
    n, temp, top_k, top_p, pen, B = 24, 0.9, 50, 0.7, 1.2, 3
    gen = torch.Generator(device=DEV).manual_seed(11)
    kw = dict(video_spatio_temporal_features=feats_t, do_sample=True, temperature=temp, max_new_tokens=n, generator=gen, eos_token_id=None,
              top_p=top_p, repetition_penalty=pen)
    plain = m.generate(prompts, chunk=7, **kw)
    gen.manual_seed(11)
    a = m.generate(prompts, chunk=7, output_logprobs=True, **kw)
    gen.manual_seed(11)
    b_ = m.generate(prompts, chunk=32, output_logprobs=True, **kw)
    assert torch.is_tensor(plain) and torch.equal(a.sequences, plain) and torch.equal(b_.sequences, plain)
    assert a.token_logprobs.shape == (B, n) and a.transition_scores.shape == (B, n) and a.token_logprobs.dtype == torch.float32
    assert torch.equal(bits(a.token_logprobs), bits(b_.token_logprobs)) and torch.equal(bits(a.transition_scores), bits(b_.transition_scores))
    assert a.sequence_logprob.dtype == torch.float64 and torch.allclose(a.sequence_logprob, a.token_logprobs.double().sum(1), rtol=0, atol=1e-12)
    new = new_ids_of(plain, prompts, n)
    steps = replay_logits(m, prompts, feats_t, new)
    n_open = check_replay(steps, prompts, new, a.token_logprobs, a.transition_scores, ("sample", temp, top_k, top_p, pen), "sampled")
    assert n_open <= 0.1 * B * n, n_open
    # the keyword off again: the plain tensor, the same ids
    gen.manual_seed(11)
    assert torch.equal(m.generate(prompts, chunk=7, **kw), plain)


def test_generate_sampled_neutral_processors_keep_the_ids(ctx):
    """do_sample with a temperature and nothing else set (top_k 50, and the whole vocabulary): without the keyword the pick is the kernel without
    the two processors, with it the kernel that carries them and the two values -- the ids must not change, and `pick` is the fp64 log-softmax
    of the temperature / top-k scores."""
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(12), 20, (5, 0, 23))
    n, B = 18, 3
    for temp, tk in ((0.2, {}), (0.9, {}), (1.0, {"top_k": 0})):
        gen = torch.Generator(device=DEV).manual_seed(23)
        kw = dict(video_spatio_temporal_features=feats_t, do_sample=True, temperature=temp, max_new_tokens=n, generator=gen, eos_token_id=None, chunk=5, **tk)
        plain = m.generate(prompts, **kw)
        gen.manual_seed(23)
        out = m.generate(prompts, output_logprobs=True, **kw)
        assert torch.equal(out.sequences, plain), (temp, tk)
        new = new_ids_of(plain, prompts, n)
        steps = replay_logits(m, prompts, feats_t, new)
        check_replay(steps, prompts, new, out.token_logprobs, out.transition_scores, ("sample", temp, tk.get("top_k", 50), 1.0, 1.0), f"neutral T={temp} {tk}")
        gen.manual_seed(23)
        assert torch.equal(m.generate(prompts, **kw), plain)


def test_switch_is_off_again_when_generate_ends_early(ctx):
    """A stopping criterion that raises ends generate(output_logprobs=True) in the middle of the decode loop: the cache the model hands out again
    must not keep recording."""
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(5), 20, (4,))

    def boom(ids, scores):
        raise KeyError("criterion failed")

    with pytest.raises(KeyError):
        m.generate(prompts, video_spatio_temporal_features=feats_t, max_new_tokens=8, eos_token_id=None, output_logprobs=True, stopping_criteria=[boom])
    kv, nxt, _ = m.prefill(prompts, feats_t, 64)                       # the same cache shape: the same handle, switch untouched by this call
    m.decode_greedy(kv, nxt, 3)
    with pytest.raises(RuntimeError, match="pgv_kv_set_logprobs"):
        m.logprobs_last(kv, 1)
    # ... and a generate_continuous generator that is closed after its first answer
    from video_llava_amd.continuous import Task, generate_continuous
    tasks = [Task(i, prompts[0], feats_t[0].to(DEV), max_new_tokens=4 + i) for i in range(3)]
    it = generate_continuous(m, iter(tasks), 2, 8, eos_token_id=None, logprobs={}, max_seq=64)
    next(it)
    it.close()
    kv, nxt, _ = m.prefill([prompts[0], prompts[0]], torch.cat([feats_t, feats_t]), 64)
    with pytest.raises(RuntimeError, match="pgv_kv_set_logprobs"):
        m.logprobs_last(kv, 2)


# ---- 4. greedy -----------------------------------------------------------------------------------------------------------------------------
def test_generate_greedy_logprobs(ctx):
    cfg, m = _tiny(seed=8)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(4), 20, (2, 17))
    n = 20
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=None, chunk=6)
    for pen in (1.0, 1.3):
        pk = {} if pen == 1.0 else {"repetition_penalty": pen}
        plain = m.generate(prompts, **kw, **pk)
        out = m.generate(prompts, output_logprobs=True, **kw, **pk)
        assert torch.equal(out.sequences, plain)
        if pen == 1.0:
            assert torch.equal(bits(out.transition_scores), bits(out.token_logprobs))
        else:
            assert not torch.equal(out.transition_scores, out.token_logprobs) and bool((out.transition_scores < 0).all())
        new = new_ids_of(plain, prompts, n)
        steps = replay_logits(m, prompts, feats_t, new)
        check_replay(steps, prompts, new, out.token_logprobs, out.transition_scores, ("greedy", pen), f"greedy pen {pen}")


# ---- 5. EOS and cuts -------------------------------------------------------------------------------------------------------------------------
def test_eos_step_is_real_later_steps_are_zero_and_cuts_follow_the_ids(ctx):
    from helpers import SynthTokenizer
    cfg, m = _tiny(seed=8)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(4), 20, (2, 17))
    n, B = 20, 2
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, chunk=4)
    free = m.generate(prompts, eos_token_id=None, output_logprobs=True, **kw)
    new = new_ids_of(free.sequences, prompts, n)
    # an id the greedy run emits mid-answer for the first time
    k = next(j for j in range(3, n - 3) if new[0][j] not in new[0][:j])
    eos = new[0][k]
    out = m.generate(prompts, eos_token_id=eos, output_logprobs=True, **kw)
    ends = [new[b].index(eos) + 1 if eos in new[b] else n for b in range(B)]
    assert ends[0] == k + 1
    for b in range(B):
        e = ends[b]
        assert out.sequences[b, len(prompts[b]):len(prompts[b]) + e].tolist() == new[b][:e]
        for got, ref in ((out.token_logprobs, free.token_logprobs), (out.transition_scores, free.transition_scores)):
            assert torch.equal(bits(got[b, :e]), bits(ref[b, :e])), b                  # up to and including the EOS step: the real values
            assert bool((got[b, e:] == 0).all())
        assert float(out.token_logprobs[b, e - 1]) < 0
        assert float(out.sequence_logprob[b]) == pytest.approx(float(out.token_logprobs[b, :e].double().sum()), abs=1e-12)
    # on the device: the EOS step carries its values, the sticky steps after it 0.0 (a row sum is the answer's log-probability)
    kv, nxt, _ = m.prefill(prompts, feats_t, 128, logprobs=True)
    first = m.logprobs_last(kv, B).cpu()
    assert torch.equal(bits(first[0]), bits(free.token_logprobs[:, 0])) and torch.equal(bits(first[1]), bits(free.transition_scores[:, 0]))
    toks = m.decode_greedy(kv, nxt, n - 1, eos).cpu()
    lp = m.logprobs_steps(kv, B, n - 1).cpu()
    m.set_logprobs(kv, False)
    for b in range(B):
        rest = new[b][1:]                                                              # the device learns of EOS in the decode steps only
        e = rest.index(eos) + 1 if eos in rest else n - 1                              # decode steps up to and including the EOS step
        assert toks[b, :e].tolist() == new[b][1:e + 1] and bool((toks[b, e:] == eos).all())
        assert torch.equal(bits(lp[0, b, :e]), bits(free.token_logprobs[b, 1:e + 1])) and torch.equal(bits(lp[1, b, :e]), bits(free.transition_scores[b, 1:e + 1]))
        assert bool((lp[:, b, e:] == 0).all())
    # a stop-string cut: the value arrays end where the ids end
    j = next(j for j in range(2, n - 2) if new[1][j] not in new[1][:j])
    stop_id = new[1][j]

    class StopTok(SynthTokenizer):
        def batch_decode(self, ids, skip_special_tokens=True):
            return [" ".join("###" if int(t) == stop_id else str(int(t)) for t in row) for row in ids]

    cut = m.generate(prompts, eos_token_id=None, output_logprobs=True, stop_strings=["###", "###"], tokenizer=StopTok(cfg.vocab), **kw)
    es = [max(new[b].index(stop_id) + 1, 2) if stop_id in new[b] else n for b in range(B)]      # the criterion looks from the second token on
    assert es[1] == j + 1 and cut.token_logprobs.shape == (B, max(es)) == cut.transition_scores.shape
    for b in range(B):
        e = es[b]
        assert cut.sequences[b, len(prompts[b]):len(prompts[b]) + e].tolist() == new[b][:e]
        assert torch.equal(bits(cut.token_logprobs[b, :e]), bits(free.token_logprobs[b, :e])) and bool((cut.token_logprobs[b, e:] == 0).all())
        assert torch.equal(bits(cut.transition_scores[b, :e]), bits(free.transition_scores[b, :e])) and bool((cut.transition_scores[b, e:] == 0).all())


# ---- 6. agreement with score() -----------------------------------------------------------------------------------------------------------------
def test_generate_logprobs_agree_with_score(ctx):
    """|generate.token_logprobs - score.token_logprobs| <= 2 d + tol per position, d the largest |decode-path logit - prefill-path logit| of that
    position: log-softmax at an index moves by at most twice the sup-norm change of its input."""
    from video_llava_amd.scoring import continuation_labels
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(6), 20, (11,))
    n = 20
    out = m.generate(prompts, video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=None, output_logprobs=True)
    answer = new_ids_of(out.sequences, prompts, n)[0]
    full = list(prompts[0]) + answer
    P = len(prompts[0])
    dec = torch.stack([s[0] for s in replay_logits(m, prompts, feats_t, [answer])])            # [n, V]: row i predicts answer[i]
    _kv, _nxt, _lg, all_lg = m.prefill([full], feats_t, 128, want_all_logits=True)
    pre = all_lg[P - 1:P - 1 + n].cpu().float().clone()
    sc = m.score([full], [continuation_labels(prompts[0], full)], video_spatio_temporal_features=feats_t)
    assert sc.scored[0].tolist() == [False] * P + [True] * n
    d = (dec.double() - pre.double()).abs().max(dim=1).values
    diff = (out.token_logprobs[0].double() - sc.token_logprobs[0][P:].double()).abs()
    bound = 2.0 * d + row_tol(dec)
    print(f"generate vs score: largest |difference| {float(diff.max()):.3e} (bound there {float(bound[int(torch.argmax(diff))]):.3e}); largest decode-vs-prefill "
          f"logit distance {float(d.max()):.3e}")
    assert bool((diff <= bound).all()), (int(torch.argmax(diff - bound)), float((diff - bound).max()))


# ---- 7. width and slot independence ------------------------------------------------------------------------------------------------------------
def test_logprobs_are_width_and_slot_independent(ctx):
    """The setup of test_warped_task_is_width_and_slot_independent: the same task alone in generate(), inside a wider generate() group and in
    generate_continuous at widths 1, 2 and 4 with refills (sampled and greedy alike) gives bitwise the same ids AND the same two value arrays -- the first token of a refilled
    slot included (pgv_llm_prefill_slots picks in scratch rows; the values land at the slot)."""
    from video_llava_amd.continuous import Task, generate_continuous
    cfg, m = _tiny()
    rng = np.random.default_rng(9)
    n_tasks, Vr = 10, 20
    prompts, feats_t = _prompts(cfg, rng, Vr, [int(x) for x in rng.integers(0, 30, n_tasks)])
    budgets = [int(x) for x in rng.integers(3, 20, n_tasks)]
    tasks = [Task(i, prompts[i], feats_t[i].to(DEV), max_new_tokens=budgets[i], seed=1000 + i) for i in range(n_tasks)]

    def same(lp, want):
        for tid, (ids, tl, ts) in want.items():
            assert len(lp[tid]["token_logprobs"]) == len(lp[tid]["transition_scores"]) == len(ids), tid
            assert torch.equal(bits(torch.tensor(lp[tid]["token_logprobs"], dtype=torch.float32)), bits(tl)), tid
            assert torch.equal(bits(torch.tensor(lp[tid]["transition_scores"], dtype=torch.float32)), bits(ts)), tid

    # sampled, per-task seeds
    skw = dict(do_sample=True, temperature=0.9, top_k=50, top_p=0.7, repetition_penalty=1.2, eos_token_id=None)
    want = {}
    for t in tasks:
        gen = torch.Generator(device=DEV).manual_seed(t.seed)
        o = m.generate([t.ids], video_spatio_temporal_features=t.feats[None], max_new_tokens=t.max_new_tokens, generator=gen, output_logprobs=True, **skw)
        want[t.task_id] = (o.sequences[0, len(t.ids):].tolist(), o.token_logprobs[0].clone(), o.transition_scores[0].clone())
        assert len(want[t.task_id][0]) == t.max_new_tokens == o.token_logprobs.shape[1]
    for W in (1, 2, 4):
        lp = {}
        got = dict(generate_continuous(m, iter(tasks), W, 32, refill_min=1, chunk=5, logprobs=lp, **skw))
        assert got == {k: v[0] for k, v in want.items()}, W
        same(lp, want)
        assert dict(generate_continuous(m, iter(tasks), W, 32, refill_min=1, chunk=5, **skw)) == got, W
    # greedy, under a penalty and without one: alone, at width 3 in generate(), refilled at width 2
    for pk in ({"repetition_penalty": 1.3}, {}):
        alone = {}
        for t in tasks[:6]:
            o = m.generate([t.ids], video_spatio_temporal_features=t.feats[None], max_new_tokens=12, eos_token_id=None, output_logprobs=True, **pk)
            alone[t.task_id] = (o.sequences[0, len(t.ids):].tolist(), o.token_logprobs[0].clone(), o.transition_scores[0].clone())
        wide = m.generate([t.ids for t in tasks[:3]], video_spatio_temporal_features=torch.stack([t.feats for t in tasks[:3]]), max_new_tokens=12,
                          eos_token_id=None, output_logprobs=True, **pk)
        for b, t in enumerate(tasks[:3]):
            assert wide.sequences[b, len(t.ids):len(t.ids) + 12].tolist() == alone[t.task_id][0]
            assert torch.equal(bits(wide.token_logprobs[b]), bits(alone[t.task_id][1])) and torch.equal(bits(wide.transition_scores[b]), bits(alone[t.task_id][2]))
        g_tasks = [Task(t.task_id, t.ids, t.feats, max_new_tokens=12) for t in tasks[:6]]
        for W in (1, 2, 4):
            lp = {}
            got = dict(generate_continuous(m, iter(g_tasks), W, 12, refill_min=1, chunk=5, eos_token_id=None, logprobs=lp, **pk))
            assert got == {k: v[0] for k, v in alone.items()}, W
            same(lp, alone)
            assert dict(generate_continuous(m, iter(g_tasks), W, 12, refill_min=1, chunk=5, eos_token_id=None, **pk)) == got, W


# ---- 8. switch hygiene ---------------------------------------------------------------------------------------------------------------------------
def test_switch_off_on_off_rebuilds_the_graphs(ctx):
    """One cache: decode_greedy with the switch off, on, off again (12 steps: one eager, one 8-step graph, three single-step graphs).  The ids are
    the same all three times; the step values exist only after the run with the switch on."""
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(5), 20, (4, 9))
    B, n = 2, 12
    runs, handles = [], []
    for on in (False, True, False):
        kv, nxt, _ = m.prefill(prompts, feats_t, 128, logprobs=on)
        handles.append(kv.value)
        runs.append(m.decode_greedy(kv, nxt, n).cpu())
        if on:
            lp = m.logprobs_steps(kv, B, n).cpu()
            assert lp.shape == (2, B, n) and bool((lp < 0).all()) and torch.equal(bits(lp[0]), bits(lp[1]))
            with pytest.raises(ValueError):
                m.logprobs_steps(kv, B, n + 1)
        else:
            with pytest.raises(RuntimeError, match="pgv_kv_set_logprobs"):
                m.logprobs_steps(kv, B, n)
            with pytest.raises(RuntimeError, match="pgv_kv_set_logprobs"):
                m.logprobs_last(kv, B)
    assert len(set(handles)) == 1
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    # switched on between two stepping calls: the values of the earlier call are not handed out
    kv, nxt, _ = m.prefill(prompts, feats_t, 128, logprobs=False)
    m.decode_greedy(kv, nxt, 3)
    m.set_logprobs(kv, True)
    with pytest.raises(RuntimeError, match="pgv_kv_set_logprobs"):
        m.logprobs_steps(kv, B, 3)
    m.set_logprobs(kv, False)


# (temperature, top_k, top_p, repetition_penalty) of a sampled run, or ("greedy", repetition_penalty): neighbours differ in exactly one field
PICK_SETS = [(0.7, 50, 0.9, 1.0), (1.3, 50, 0.9, 1.0), (1.3, 5, 0.9, 1.0), (1.3, 5, 0.5, 1.0), (1.3, 5, 0.5, 1.5), ("greedy", 1.5), ("greedy", 1.0)]


def test_one_cache_rebuilds_the_graphs_for_every_pick_parameter(ctx):
    """One cache, the same prompts (B = 2) and the same uniforms throughout; every call is a prefill and 10 steps (the cache's first call: one eager
    step, the 8-step graph, one single-step graph; later ones: the 8-step graph and two single steps).  PICK_SETS forwards, then backwards: every
    set returns bitwise the same ids both times, and no two sets return the same ids -- a captured graph that kept a neighbour's temperature,
    top_k, top_p, penalty or greedy flag would repeat the neighbour's ids."""
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(5), 20, (4, 9))
    B, n = 2, 10
    u = torch.rand(n, B, generator=torch.Generator().manual_seed(23)).to(DEV)
    runs, handles = {}, set()
    for ps in PICK_SETS + PICK_SETS[::-1]:
        kv, nxt, _ = m.prefill(prompts, feats_t, 128, logprobs=False)
        handles.add(kv.value)
        if ps[0] == "greedy":
            ids = m.decode_greedy(kv, nxt, n, repetition_penalty=ps[1]).cpu()
        else:
            ids = m.decode_sample(kv, nxt, n, -1, ps[0], ps[1], u, top_p=ps[2], repetition_penalty=ps[3]).cpu()
        print(ps, ids.tolist())
        runs.setdefault(ps, []).append(ids)
    assert len(handles) == 1
    for ps, (fwd, back) in runs.items():
        assert torch.equal(fwd, back), (ps, fwd.tolist(), back.tolist())
    for i, a in enumerate(PICK_SETS):
        for b in PICK_SETS[i + 1:]:
            assert not torch.equal(runs[a][0], runs[b][0]), (a, b, runs[a][0].tolist())


# ---- 9. real vocabulary --------------------------------------------------------------------------------------------------------------------------
_REAL = {}


def real_model():
    if "m" not in _REAL:
        from oracle import synth
        from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
        from video_llava_amd.random_init import iter_llama_tensors, load_streaming
        cfg = synth.LlamaCfg(layers=2)
        m = VideoChatGPTLlamaForCausalLM(VideoChatGPTConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2,
                                                            num_attention_heads=cfg.heads, eos_token_id=None), VisionConfig(), torch.bfloat16)
        load_streaming(m, iter_llama_tensors(vocab=cfg.vocab, hidden=cfg.hidden, inter=cfg.inter, layers=2, dtype=torch.bfloat16, seed=5, head_std=0.05))
        _REAL["m"] = m
    return _REAL["m"]


@pytest.mark.parametrize("B,n", [(2, 16), (17, 3)])
def test_real_vocabulary_bf16(ctx, B, n):
    """A two-layer 7B-shaped bf16 model: the 32003-wide logit row (odd: no 16-byte alignment between rows); B = 17 takes the logits of the last
    sequence from the second MFMA column tile of the decode GEMVs."""
    m = real_model()
    assert m.vocab_size == 32003
    rng = np.random.default_rng(13)
    prompts = [[1] + rng.integers(3, 32000, 6 + 3 * (b % 4)).tolist() for b in range(B)]
    temp, top_k, top_p, pen = 0.9, 50, 0.7, 1.2
    gen = torch.Generator(device=DEV).manual_seed(17)
    kw = dict(do_sample=True, temperature=temp, top_k=top_k, top_p=top_p, repetition_penalty=pen, max_new_tokens=n, generator=gen, eos_token_id=None, chunk=9)
    plain = m.generate(prompts, **kw)
    gen.manual_seed(17)
    out = m.generate(prompts, output_logprobs=True, **kw)
    assert torch.equal(out.sequences, plain)
    new = new_ids_of(plain, prompts, n)
    steps = replay_logits(m, prompts, None, new, max_seq=64)
    check_replay(steps, prompts, new, out.token_logprobs, out.transition_scores, ("sample", temp, top_k, top_p, pen), f"7B-shaped bf16 B={B}")
    g = m.generate(prompts, max_new_tokens=n, eos_token_id=None, output_logprobs=True)
    assert torch.equal(bits(g.transition_scores), bits(g.token_logprobs))
    gnew = new_ids_of(g.sequences, prompts, n)
    check_replay(replay_logits(m, prompts, None, gnew, max_seq=64), prompts, gnew, g.token_logprobs, g.transition_scores, ("greedy", 1.0), f"7B-shaped bf16 greedy B={B}")


# ---- the inference entry ---------------------------------------------------------------------------------------------------------------------------
def test_video_chatgpt_infer_logprobs(ctx):
    """inference.video_chatgpt_infer_logprobs on the tiny tower + decoder of test_video_chatgpt_score: the text of video_chatgpt_infer, its ids, and
    the values generate(output_logprobs=True) gives for the same prompt."""
    from helpers import make_tower
    from oracle import synth
    from test_gpu_score import _RoundTripTok
    from video_llava_amd.inference import video_chatgpt_infer, video_chatgpt_infer_logprobs
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    ccfg, lcfg = synth.CLIP_TINY, synth.LLAMA_TINY
    tower = make_tower(ccfg, synth.make_clip_weights(ccfg, seed=21))
    model = VideoChatGPTLlamaForCausalLM(VideoChatGPTConfig(vocab_size=lcfg.vocab, hidden_size=lcfg.hidden, intermediate_size=lcfg.inter,
                                                            num_hidden_layers=lcfg.layers, num_attention_heads=lcfg.heads, eos_token_id=None,
                                                            max_position_embeddings=2048), VisionConfig(frame_size=ccfg.image), torch.float16)
    model.load_state_dict(synth.make_llama_weights(lcfg, seed=22, head_std=0.08))
    vc = model.get_model().vision_config
    vc.vid_patch_token, vc.vid_start_token, vc.vid_end_token, vc.use_vid_start_end = lcfg.vocab - 3, lcfg.vocab - 2, lcfg.vocab - 1, True
    tok = _RoundTripTok(lcfg.vocab)

    class IP:
        crop_size = {"height": ccfg.image, "width": ccfg.image}
    V = 100 + (ccfg.image // ccfg.patch) ** 2
    frames = synth.make_frames(5, ccfg.image, seed=30)
    q, mode = "what happens 0?", "pg-video-llava"
    text = video_chatgpt_infer(frames, q, mode, model, tower, tok, IP(), V, do_sample=False, max_new_tokens=6)
    res = video_chatgpt_infer_logprobs(frames, q, mode, model, tower, tok, IP(), V, do_sample=False, max_new_tokens=6)
    assert set(res) == {"text", "ids", "token_logprobs", "transition_scores", "logprob"}
    assert res["text"] == text and len(res["ids"]) == len(res["token_logprobs"]) == len(res["transition_scores"]) == 6
    assert res["transition_scores"] == res["token_logprobs"] and all(v < 0 for v in res["token_logprobs"])
    assert res["logprob"] == float(torch.tensor(res["token_logprobs"], dtype=torch.float32).double().sum())
    warm = video_chatgpt_infer_logprobs(frames, q, mode, model, tower, tok, IP(), V, do_sample=True, temperature=0.8, max_new_tokens=6, top_p=0.8)
    assert len(warm["ids"]) == len(warm["token_logprobs"]) == len(warm["transition_scores"]) >= 1
    assert warm["logprob"] == pytest.approx(sum(warm["token_logprobs"]), abs=1e-4)
