"""GPU: nucleus (top-p) filtering and the repetition penalty inside the device pick (csrc/sampling.hip sample_kernel<true>), from the kernel
(pgv_sample_logits_ex) up to model.generate / generate_continuous.

Yardstick: HF's own processors from the installed transformers (generation/logits_process.py: RepetitionPenaltyLogitsProcessor,
TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper), run in fp64 in HF's order.  The kernel sums in fp32 in a fixed order and decides
the nucleus on 2^-40 fixed-point sums, the reference in fp64; the project's allowance for that is 1e-5 on a cumulative probability
(tests/test_gpu_sampling.py), used here twice:
  * kept set: with c = HF's ascending cumulative sums after penalty / temperature / top-k, n_lo = #(c > 1 - top_p + 1e-5) and
    n_hi = max(1, #(c > 1 - top_p - 1e-5)): n_lo <= kept <= n_hi always, and kept == HF's count when n_lo == n_hi;
  * pick: equal to the fp64 inverse-CDF pick over HF's filtered distribution when n_lo == n_hi and u is farther than 1e-5 from every CDF
    step; otherwise the pick has non-zero probability under the n_hi set and sits next to the step of the distribution over the `kept`
    largest entries (any count inside the band is a legitimate nucleus, and each has its own renormalised CDF).
The share of rows outside the exact rule is a property of the inputs and the fp64 reference: it is computed without the device result and
capped at 5 % (except the whole-vocabulary top_p = 0.9 family at V = 32003, whose CDF steps are ~3e-5 apart).
"""
import numpy as np
import pytest
import torch
from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                    TopPLogitsWarper)

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def hf_chain(logits, seen, temp, top_k, top_p, pen):
    """HF's processors in HF's order on fp64 scores [B, V] (seen: LongTensor [B, n] or None) -> (scores after penalty / temperature / top-k,
    scores after top-p)."""
    x = torch.nan_to_num(torch.as_tensor(logits).double(), nan=float("-inf"))
    if pen != 1.0 and seen is not None:
        x = RepetitionPenaltyLogitsProcessor(float(pen))(seen.long(), x)
    x = TemperatureLogitsWarper(float(temp))(None, x)
    if 0 < top_k < x.shape[-1]:
        x = TopKLogitsWarper(int(top_k))(None, x)
    y = TopPLogitsWarper(float(top_p))(None, x) if top_p < 1.0 else x
    return x, y


def band(x2, top_p):
    """(n_lo, n_hi, descending order of the entries) per row of the pre-top-p scores."""
    srt, order = torch.sort(x2, descending=False, dim=-1)
    c = srt.softmax(-1).cumsum(-1)
    n_lo = (c > 1 - top_p + TOL).sum(-1)
    n_hi = (c > 1 - top_p - TOL).sum(-1).clamp_min(1)
    return n_lo, n_hi, order.flip(-1)


def cdf_of(scores):
    return torch.softmax(scores, -1).cumsum(-1)


def top_n_scores(x2_row, order_row, n):
    out = torch.full_like(x2_row, float("-inf"))
    idx = order_row[:n]
    out[idx] = x2_row[idx]
    return out


PARAMS = [(0.2, 50, 0.6, 1.0), (0.9, 50, 0.6, 1.0), (1.0, 7, 0.5, 1.0), (0.2, 50, 0.95, 1.3), (0.7, 0, 0.6, 1.2), (1.0, 0, 0.9, 1.0)]


@pytest.mark.parametrize("V,B", [(32003, 8), (515, 16), (1000, 3), (50, 2)])
@pytest.mark.parametrize("temp,top_k,top_p,pen", PARAMS)
def test_warped_pick_and_kept_set_match_hf_chain(ctx, V, B, temp, top_k, top_p, pen):
    g = torch.Generator().manual_seed(V * 7 + B)
    inexact = total = 0
    for r in range(40):
        logits = torch.randn(B, V, generator=g) * (1.5 + (r % 3))
        if r == 5:
            logits[-1, V // 2] = float("nan")                            # a NaN is never picked
        seen = torch.randint(0, V, (B, 30), generator=g)
        u = torch.rand(B, generator=g)
        if r == 7:
            u[0] = 0.0
        # ---- the reference alone: which rows fall under the exact rule ----
        x2, y = hf_chain(logits, seen, temp, top_k, top_p, pen)
        n_lo, n_hi, order = band(x2, top_p)
        hf_count = (y > float("-inf")).sum(-1)
        cdf = cdf_of(y)
        ud = u.double()[:, None]
        want = (cdf <= ud).sum(-1).clamp_max(V - 1)
        dist = (cdf - ud).abs().min(-1).values
        closed = n_lo == n_hi
        sure = closed & (dist > TOL)
        inexact += int((~sure).sum()); total += B
        # ---- the device ----
        got, kept = ctx.sample_logits_ex(logits.to(DEV), u.to(DEV), temp, top_k, top_p, pen, seen.int().to(DEV), want_kept=True)
        got, kept = got.cpu().long(), kept.cpu().long()
        print(f"r={r} n_lo={n_lo.tolist()} n_hi={n_hi.tolist()} hf={hf_count.tolist()} kept={kept.tolist()} got={got.tolist()} want={want.tolist()}")
        assert bool(((n_lo <= kept) & (kept <= n_hi)).all()), (r, n_lo.tolist(), kept.tolist(), n_hi.tolist())
        assert torch.equal(kept[closed], hf_count[closed]), (r, kept.tolist(), hf_count.tolist())
        assert torch.equal(got[sure], want[sure]), (r, got.tolist(), want.tolist(), dist.tolist())
        for b in torch.nonzero(~sure)[:, 0].tolist():
            t = int(got[b])
            p_hi = torch.softmax(top_n_scores(x2[b], order[b], int(n_hi[b])), -1)
            assert float(p_hi[t]) > 0, (r, b, t)
            p_k = torch.softmax(top_n_scores(x2[b], order[b], int(kept[b])), -1)
            c_k = p_k.cumsum(-1)
            assert float(p_k[t]) > 0 and abs(float(c_k[t] - u[b].double())) < 1e-4 + float(p_k[t]), (r, b, t, float(c_k[t]), float(u[b]))
    print(f"rows outside the exact rule: {inexact}/{total}")
    if not (V == 32003 and top_k == 0 and top_p == 0.9):
        assert inexact <= 0.05 * total, (inexact, total)


def test_neutral_values_equal_the_plain_pick_bitwise(ctx):
    g = torch.Generator().manual_seed(5)
    for V, B in ((32003, 8), (515, 16), (50, 2)):
        for temp, top_k in ((0.2, 50), (1.0, 0), (0.7, 7)):
            for _ in range(6):
                logits = (torch.randn(B, V, generator=g) * 2).to(DEV)
                u = torch.rand(B, generator=g).to(DEV)
                seen = torch.randint(0, V, (B, 9), generator=g).int().to(DEV)
                plain = ctx.sample_logits(logits, u, temp, top_k)
                assert torch.equal(ctx.sample_logits_ex(logits, u, temp, top_k, 1.0, 1.0, seen), plain)
                # ... and through the kernel that carries the two processors (asking for the kept count selects it)
                got, kept = ctx.sample_logits_ex(logits, u, temp, top_k, 1.0, 1.0, seen, want_kept=True)
                assert torch.equal(got, plain)
                assert kept.tolist() == [min(top_k, V) if top_k > 0 else V] * B


def test_edges_greedy_limit_ties_nan_penalty_direction_and_refusals(ctx):
    g = torch.Generator().manual_seed(2)
    V = 32003
    logits = (torch.randn(4, V, generator=g) * 2).to(DEV)
    u = torch.rand(4, generator=g).to(DEV)
    # top_p -> 0 is greedy, with and without a top-k mask
    for top_k in (50, 0):
        got, kept = ctx.sample_logits_ex(logits, u, 0.8, top_k, 1e-6, 1.0, want_kept=True)
        assert got.tolist() == logits.argmax(-1).tolist() and kept.tolist() == [1] * 4
    # tie rule: equal logits are kept or removed together.  Four tied maxima: HF's sort would cut between them at top_p = 0.3; here all four stay
    row = torch.full((1, 64), -4.0)
    row[0, [3, 17, 40, 41]] = 6.0
    picks = set()
    for i in range(40):
        got, kept = ctx.sample_logits_ex(row.to(DEV), torch.tensor([(i + 0.5) / 40], device=DEV), 1.0, 0, 0.3, 1.0, want_kept=True)
        assert kept.tolist() == [4]
        picks.add(int(got[0]))
    assert picks == {3, 17, 40, 41}
    # a tied group below the top: {5, 5} carry 2 * e^5 / Z = 0.833 of the mass, the three 3s 0.169: at top_p = 0.9 HF keeps one of the 3s
    # (the mass above the first is 0.833 < 0.9, above the second 0.889 < 0.9, above the third 0.946) -- the rule here keeps all three, since
    # the mass STRICTLY greater than 3 is 0.833 < 0.9; at top_p = 0.8 the 3s go together
    row = torch.full((1, 50), -20.0)
    row[0, [7, 8]] = 5.0
    row[0, [20, 30, 31]] = 3.0
    for top_p, n in ((0.9, 5), (0.8, 2)):
        _, kept = ctx.sample_logits_ex(row.to(DEV), torch.tensor([0.5], device=DEV), 1.0, 0, top_p, 1.0, want_kept=True)
        assert kept.tolist() == [n], (top_p, kept.tolist())
    # NaN logits are never picked, seen or not, whatever u
    lg = torch.randn(16, 515, generator=g)
    lg[:, [0, 100, 514]] = float("nan")
    seen = torch.tensor([[0, 100, 7, 9]] * 16).int()
    for i in range(8):
        uu = torch.rand(16, generator=g)
        if i == 0:
            uu[:] = 0.0
        if i == 1:
            uu[:] = 1.0 - 2 ** -24
        got = ctx.sample_logits_ex(lg.to(DEV), uu.to(DEV), 1.0, 0, 0.999, 1.5, seen.to(DEV)).cpu()
        assert not torch.isin(got, torch.tensor([0, 100, 514], dtype=got.dtype)).any()
    # the penalty moves a positive and a negative logit the right way: [2, -1, 0.5] with penalty 2 -> seen {0}: [1, -1, 0.5]; seen {1}: [2, -2, 0.5]
    hand = torch.tensor([[2.0, -1.0, 0.5]])
    n = 400
    us = (torch.arange(n) + 0.5) / n
    counts = {}
    for name, ids in (("none", None), ("pos", [0]), ("neg", [1]), ("both", [0, 1])):
        seen_t = torch.tensor([ids] * n).int().to(DEV) if ids else None
        got = ctx.sample_logits_ex(hand.expand(n, 3).contiguous().to(DEV), us.to(DEV), 1.0, 0, 1.0, 2.0 if ids else 1.0, seen_t, want_kept=ids is None)
        got = (got[0] if ids is None else got).cpu().long()
        _, y = hf_chain(hand.expand(n, 3), torch.tensor([ids] * n) if ids else None, 1.0, 0, 1.0, 2.0 if ids else 1.0)
        cdf = cdf_of(y)
        want = (cdf <= us.double()[:, None]).sum(-1).clamp_max(2)
        sure = (cdf - us.double()[:, None]).abs().min(-1).values > TOL
        assert torch.equal(got[sure], want[sure]), name
        counts[name] = torch.bincount(got, minlength=3).tolist()
    assert counts["pos"][0] < counts["none"][0] and counts["neg"][1] < counts["none"][1]
    assert counts["both"][0] < counts["none"][0] and counts["both"][1] <= counts["none"][1] and counts["both"][2] > counts["none"][2]
    # refused values, HF's wording
    for top_p, pen, word in ((0.0, 1.0, "top_p"), (1.5, 1.0, "top_p"), (-0.1, 1.0, "top_p"), (0.5, 0.0, "penalty"), (0.5, -1.0, "penalty")):
        with pytest.raises(ValueError, match=word):
            ctx.sample_logits_ex(logits, u, 0.8, 50, top_p, pen)


def test_nucleus_distribution_chi_square(ctx):
    g = torch.Generator().manual_seed(1)
    V = 32003
    logits = (torch.randn(1, V, generator=g) * 2)
    _, y = hf_chain(logits, None, 0.8, 50, 0.6, 1.0)
    p = torch.softmax(y[0], -1)
    keep = p > 0
    k = int(keep.sum())
    assert 2 <= k < 50
    row = logits.expand(16, V).contiguous().to(DEV)
    counts = torch.zeros(V, dtype=torch.float64)
    n = 0
    for i in range(4000):
        uu = torch.rand(16, generator=g).to(DEV)
        counts += torch.bincount(ctx.sample_logits_ex(row, uu, 0.8, 50, 0.6, 1.0).cpu().long(), minlength=V).double()
        n += 16
    assert float(counts[~keep].sum()) == 0.0
    chi2 = float((((counts[keep] - n * p[keep]) ** 2) / (n * p[keep])).sum())
    print(f"kept {k}, chi2 {chi2:.1f}")
    assert chi2 < 100.0 / 49.0 * (k - 1), (chi2, k)          # the existing test's bound per degree of freedom (100 for 49)


# ---- through the model -------------------------------------------------------------------------------------------------------------
def _prompts(cfg, rng, Vr, extras):
    PATCH, START, END = cfg.vocab - 3, cfg.vocab - 2, cfg.vocab - 1
    prompts, feats = [], []
    for extra in extras:
        prompts.append([1] + rng.integers(3, cfg.vocab - 3, 5 + extra).tolist() + [START] + [PATCH] * Vr + [END] + rng.integers(3, cfg.vocab - 3, 4).tolist())
        feats.append(torch.from_numpy(rng.standard_normal((Vr, 1024), dtype=np.float32)))
    return prompts, torch.stack(feats).half()


def _tiny(seed=3):
    from helpers import make_model
    cfg = synth.LLAMA_TINY
    return cfg, make_model(cfg, synth.make_llama_weights(cfg, seed=seed, head_std=0.08), torch.float16)


def test_generate_with_top_p_and_penalty_equals_stepwise_hf_chain(ctx):
    """Every sampled token equals the fp64 HF chain's inverse-CDF pick on THAT step's device logits with the ids so far (prompt as given,
    placeholder ids included, plus the tokens generated before), for a ragged batch; the chunk size does not matter."""
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(2), 20, (3, 40, 0))
    n, temp, top_k, top_p, pen, B = 24, 0.9, 50, 0.7, 1.2, 3
    gen = torch.Generator(device=DEV).manual_seed(11)
    kw = dict(video_spatio_temporal_features=feats_t, do_sample=True, temperature=temp, max_new_tokens=n, generator=gen, eos_token_id=None,
              top_p=top_p, repetition_penalty=pen)
    out = m.generate(prompts, chunk=7, **kw)
    gen.manual_seed(11)
    out2 = m.generate(prompts, chunk=32, **kw)
    assert torch.equal(out, out2)
    gen.manual_seed(11)
    plain = m.generate(prompts, chunk=32, **dict(kw, top_p=1.0, repetition_penalty=1.0))
    assert not torch.equal(out, plain)                                   # the two processors change the draw at these settings
    gen.manual_seed(11)
    u = torch.rand(n, B, device=DEV, generator=gen).cpu()
    kv, nxt, logits = m.prefill(prompts, feats_t, 128, want_logits=True)
    n_exact = 0
    for i in range(n):
        got = torch.tensor([int(out[b, len(prompts[b]) + i]) for b in range(B)])
        for b in range(B):
            seen = torch.tensor([prompts[b] + out[b, len(prompts[b]):len(prompts[b]) + i].tolist()])
            x2, y = hf_chain(logits[b:b + 1].cpu(), seen, temp, top_k, top_p, pen)
            n_lo, n_hi, _ = band(x2, top_p)
            cdf = cdf_of(y)[0]
            want = int((cdf <= u[i, b].double()).sum().clamp_max(cfg.vocab - 1))
            dist = float((cdf - u[i, b].double()).abs().min())
            if int(n_lo) == int(n_hi) and dist > TOL:
                assert int(got[b]) == want, (i, b, int(got[b]), want)
                n_exact += 1
            else:
                assert float(torch.softmax(x2[0], -1)[int(got[b])]) > 0
        nxt, logits = m.decode_step(kv, got.to(torch.int32).to(DEV), want_logits=True)
    assert n_exact > 0.9 * n * B, n_exact
    for b in range(B):
        assert out[b, :len(prompts[b])].tolist() == prompts[b]


def test_greedy_with_penalty_equals_host_loop(ctx):
    cfg, m = _tiny(seed=8)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(4), 20, (2, 17))
    n, pen = 20, 1.3
    out = m.generate(prompts, video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=None, repetition_penalty=pen, chunk=6)
    free = m.generate(prompts, video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=None)
    assert not torch.equal(out, free)
    kv, nxt, logits = m.prefill(prompts, feats_t, 128, want_logits=True)
    ids = [list(p) for p in prompts]
    for i in range(n):
        step = []
        for b in range(2):
            x = RepetitionPenaltyLogitsProcessor(pen)(torch.tensor([ids[b]]), logits[b:b + 1].cpu().double())
            step.append(int(x.argmax(-1)))
            ids[b].append(step[-1])
        assert [int(out[b, len(prompts[b]) + i]) for b in range(2)] == step, (i, step)
        nxt, logits = m.decode_step(kv, torch.tensor(step, dtype=torch.int32, device=DEV), want_logits=True)


def test_warped_task_is_width_and_slot_independent(ctx):
    """The same task gives the same ids alone, inside a wider generate() group, and in generate_continuous at widths 1, 2 and 4 with refills:
    a task that enters a refilled slot starts from a seen-set of its own prompt."""
    from video_llava_amd.continuous import Task, generate_continuous
    cfg, m = _tiny()
    rng = np.random.default_rng(9)
    n_tasks, Vr = 10, 20
    prompts, feats_t = _prompts(cfg, rng, Vr, [int(x) for x in rng.integers(0, 30, n_tasks)])
    budgets = [int(x) for x in rng.integers(3, 20, n_tasks)]
    tasks = [Task(i, prompts[i], feats_t[i].to(DEV), max_new_tokens=budgets[i], seed=1000 + i) for i in range(n_tasks)]
    top_p, pen = 0.7, 1.2
    # sampled: alone, with the task's own seeded stream
    want = {}
    for t in tasks:
        gen = torch.Generator(device=DEV).manual_seed(t.seed)
        o = m.generate([t.ids], video_spatio_temporal_features=t.feats[None], do_sample=True, temperature=0.9, top_k=50, top_p=top_p,
                       repetition_penalty=pen, max_new_tokens=t.max_new_tokens, generator=gen, eos_token_id=None)
        want[t.task_id] = o[0, len(t.ids):].tolist()
    for W in (1, 2, 4):
        got = dict(generate_continuous(m, iter(tasks), W, 32, do_sample=True, temperature=0.9, top_k=50, top_p=top_p, repetition_penalty=pen,
                                       refill_min=1, chunk=5, eos_token_id=None))
        assert got == want, W
    # greedy under the penalty: alone, at width 3 in generate(), refilled at width 2
    alone = {t.task_id: m.generate([t.ids], video_spatio_temporal_features=t.feats[None], max_new_tokens=12, eos_token_id=None,
                                   repetition_penalty=1.3)[0, len(t.ids):].tolist() for t in tasks[:6]}
    wide = m.generate([t.ids for t in tasks[:3]], video_spatio_temporal_features=torch.stack([t.feats for t in tasks[:3]]), max_new_tokens=12,
                      eos_token_id=None, repetition_penalty=1.3)
    for b, t in enumerate(tasks[:3]):
        assert wide[b, len(t.ids):len(t.ids) + 12].tolist() == alone[t.task_id]
    g_tasks = [Task(t.task_id, t.ids, t.feats, max_new_tokens=12) for t in tasks[:6]]
    got = dict(generate_continuous(m, iter(g_tasks), 2, 12, repetition_penalty=1.3, refill_min=1, chunk=5, eos_token_id=None))
    assert got == alone
    # neutral values: the call without them
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = m.generate(prompts[:2], video_spatio_temporal_features=feats_t[:2], do_sample=True, temperature=0.9, max_new_tokens=16, generator=gen,
                   top_p=1.0, repetition_penalty=1.0)
    gen.manual_seed(5)
    b_ = m.generate(prompts[:2], video_spatio_temporal_features=feats_t[:2], do_sample=True, temperature=0.9, max_new_tokens=16, generator=gen)
    assert torch.equal(a, b_)


REFUSED_CASES = [("num_beams", 4, 1), ("min_p", 0.05, None), ("typical_p", 0.9, 1.0), ("penalty_alpha", 0.6, None), ("no_repeat_ngram_size", 3, 0),
                 ("bad_words_ids", [[5]], None), ("min_length", 4, 0), ("min_new_tokens", 2, 0), ("num_return_sequences", 2, 1),
                 ("epsilon_cutoff", 3e-4, 0.0), ("eta_cutoff", 3e-4, 0.0), ("encoder_repetition_penalty", 1.5, 1.0)]


def test_generate_refuses_what_it_does_not_implement(ctx):
    cfg, m = _tiny()
    ids = [1, 17, 230, 9, 44]
    base = m.generate([ids], max_new_tokens=3, eos_token_id=None)
    for name, bad, neutral in REFUSED_CASES:
        with pytest.raises(ValueError, match=name):
            m.generate([ids], max_new_tokens=3, eos_token_id=None, **{name: bad})
        assert torch.equal(m.generate([ids], max_new_tokens=3, eos_token_id=None, **{name: neutral}), base), name
    # inert arguments stay ignored
    assert torch.equal(m.generate([ids], max_new_tokens=3, eos_token_id=None, use_cache=True, pad_token_id=0, output_scores=False,
                                  return_dict_in_generate=False, attention_mask=torch.ones(1, len(ids))), base)
    for top_p, pen, word in ((0.0, 1.0, "top_p"), (1.2, 1.0, "top_p"), (0.5, 0.0, "penalty")):
        with pytest.raises(ValueError, match=word):
            m.generate([ids], max_new_tokens=3, do_sample=True, top_p=top_p, repetition_penalty=pen)
    # a generation config is honoured below the call's own arguments and refused fields raise at generate()
    from video_llava_amd.generation import GenerationDefaults
    gen = torch.Generator(device=DEV).manual_seed(3)
    want = m.generate([ids], max_new_tokens=12, eos_token_id=None, do_sample=True, temperature=0.9, top_p=0.6, generator=gen)
    m.generation_config = GenerationDefaults(temperature=0.3, top_p=0.6)
    gen.manual_seed(3)
    assert torch.equal(m.generate([ids], max_new_tokens=12, eos_token_id=None, do_sample=True, temperature=0.9, generator=gen), want)
    m.generation_config = GenerationDefaults(num_beams=4)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate([ids], max_new_tokens=3)
    m.generation_config = None
