"""GPU: HF's min_p / typical_p / epsilon_cutoff / eta_cutoff warpers inside the device pick (csrc/sampling.hip sample_kernel<true, LP, true>), from
the kernel (pgv_sample_logits_filtered) up to model.generate(filters=), generate_continuous and the refill runner.

Yardstick: video_llava_amd/sample_filters.filter_chain, the fp64 numpy rules that tests/test_filters_cpu.py holds against the installed HF warper
classes, behind HF's own repetition penalty / temperature / top-k / top-p in fp64 (test_gpu_warpers.hf_chain).

The kernel computes its weights and sums in fp32, the rules in fp64, so a decision boundary that sits within rounding distance of an entry may fall
either way.  Which rows those are is decided from the reference ALONE: a row is EXACT when filter_chain returns the same set under all eight sign
combinations of (rel, dH, dmass) = (1e-4, 1e-4, 1e-5) -- the probability thresholds scaled, the entropies shifted, the typical mass shifted -- and
its nucleus is closed under the project's 1e-5 allowance on a cumulative probability (test_gpu_warpers.band).  Where the band comes from: a weight
is exp2 of an fp32 product with |argument| <~ 60, about 5e-6 relative; the fixed-order sums have depth ~150, about 1e-5 relative, which gives about
1e-5 * H <= 1e-4 absolute on an entropy; 1e-5 on a cumulative probability is the existing allowance.
  * exact rows: d_kept and d_kept_range equal the rule's set (count, smallest and largest kept fp32 logit), and for u farther than 1e-5 from every
    CDF step the token equals the fp64 inverse-CDF pick;
  * other rows: kept lies between the smallest and the largest perturbed set, and the token has non-zero probability under their union.
The share of inexact rows is a property of the inputs (seed V * 7 + B), capped at 5 % per family -- 15 % for the three whole-vocabulary
single-warper families at V = 32003 (typical 0.9, epsilon 3e-4, eta 2e-3), whose boundary sits among thousands of probabilities about 1e-5 apart.
"""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

from filters_hf import FAMILIES, filters_of, hf_tail
from helpers import SynthTokenizer as _Tok
from oracle import synth
from test_gpu_gen_logprobs import assert_within, bits, lsm_at, new_ids_of, replay_logits, row_tol
from test_gpu_warpers import band, cdf_of, hf_chain, top_n_scores
from video_llava_amd.sample_filters import SampleFilters, filter_chain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SIGNS = [(sr * 1e-4, sh * 1e-4, sm * 1e-5) for sr, sh, sm in itertools.product((1, -1), repeat=3)]


def penalised32(logits, seen, pen):
    """The fp32 logits the kernel sees: x < 0 ? x * pen : x / pen on the seen ids (IEEE fp32, as __fmul_rn / __fdiv_rn)."""
    x = logits.clone().float()
    if pen != 1.0 and seen is not None:
        p = torch.tensor(pen, dtype=torch.float32)
        for b in range(x.shape[0]):
            idx = torch.unique(seen[b].long())
            v = x[b, idx]
            x[b, idx] = torch.where(v < 0, v * p, v / p)
    return x


def rule_sets(x2_row, order_row, n_lo, n_hi, n_hf, top_p, f):
    """(nominal kept mask, list of perturbed masks) for one row of pre-top-p fp64 scores.  Nominal: the rules behind HF's own nucleus of n_hf
    entries.  Perturbed: the eight sign combinations, behind every nucleus size the 1e-5 allowance admits (n_lo .. n_hi) -- an open nucleus makes a
    row inexact only where the tail does not cut above it anyway.  None for the nominal mask: the nucleus band is too wide to enumerate."""
    def nucleus(n):
        return (top_n_scores(x2_row, order_row, n) if top_p < 1.0 else x2_row).numpy()
    n_lo, n_hi = max(1, int(n_lo)), max(1, int(n_hi))
    counts = range(n_lo, n_hi + 1) if n_hi - n_lo <= 8 else (n_lo, n_hi)
    sets = [filter_chain(nucleus(n), f, rel=a, dH=h, dmass=m) for n in counts for a, h, m in SIGNS]
    nominal = filter_chain(nucleus(max(1, int(n_hf))), f) if n_hi - n_lo <= 8 else None
    return nominal, sets


CASES = [(i, 1.0) for i in range(len(FAMILIES))] + [(1, 1.3)]


@pytest.mark.parametrize("V,B", [(32003, 8), (515, 16), (50, 2)])
@pytest.mark.parametrize("fam,pen", CASES)
def test_filtered_pick_and_kept_set_match_the_rules(ctx, V, B, fam, pen):
    temp, top_k, top_p = FAMILIES[fam][:3]
    f = filters_of(FAMILIES[fam])
    g = torch.Generator().manual_seed(V * 7 + B)
    sigma0 = 3.0 if V == 32003 else 1.5
    inexact = total = 0
    for r in range(8 if V == 32003 else 40):
        logits = torch.randn(B, V, generator=g) * (sigma0 + (r % 3))
        if r == 5:
            logits[-1, V // 2] = float("nan")                            # a NaN is never kept
        seen = torch.randint(0, V, (B, 30), generator=g)
        u = torch.rand(B, generator=g)
        if r == 7:
            u[0] = 0.0
        # ---- the reference alone ----
        x2, y = hf_chain(logits, seen, temp, top_k, top_p, pen)
        n_lo, n_hi, order = band(x2, top_p)
        n_hf = torch.isfinite(y).sum(-1)
        if top_p >= 1.0:
            n_lo = n_hi = n_hf
        x32 = penalised32(logits, seen, pen)
        rows = []
        for b in range(B):
            nominal, sets = rule_sets(x2[b], order[b], n_lo[b], n_hi[b], n_hf[b], top_p, f)
            exact = nominal is not None and all((s == nominal).all() for s in sets)
            rows.append((nominal, sets, exact))
            inexact += not exact; total += 1
        # ---- the device ----
        got, kept, _model, _pick, rng = ctx.sample_logits_filtered(logits.to(DEV), u.to(DEV), temp, top_k, top_p, pen, seen.int().to(DEV), filters=f)
        got, kept, rng = got.cpu().long(), kept.cpu().long(), rng.cpu()
        for b, (nominal, sets, exact) in enumerate(rows):
            t = int(got[b])
            counts = [int(s.sum()) for s in sets]
            print(f"r={r} b={b} exact={exact} kept={int(kept[b])} rule={int(nominal.sum()) if nominal is not None else None} band=[{min(counts)}, {max(counts)}] tok={t}")
            if exact:
                assert int(kept[b]) == int(nominal.sum()), (r, b, int(kept[b]), int(nominal.sum()))
                vals = x32[b][torch.from_numpy(nominal)]
                assert (float(rng[b, 0]), float(rng[b, 1])) == (float(vals.min()), float(vals.max())), (r, b, rng[b].tolist(), float(vals.min()), float(vals.max()))
                y = torch.where(torch.from_numpy(nominal), x2[b], torch.full_like(x2[b], float("-inf")))
                cdf = cdf_of(y)
                ud = u[b].double()
                if float((cdf - ud).abs().min()) > TOL:
                    assert t == int((cdf <= ud).sum().clamp_max(V - 1)), (r, b, t)
                else:
                    assert nominal[t], (r, b, t)
            else:
                assert min(counts) <= int(kept[b]) <= max(counts), (r, b, int(kept[b]), min(counts), max(counts))
                assert np.logical_or.reduce(sets)[t], (r, b, t)
    print(f"rows outside the exact rule: {inexact}/{total} = {100.0 * inexact / total:.1f} %")
    wide = V == 32003 and fam in (2, 4, 5)
    assert inexact <= (0.15 if wide else 0.05) * total, (inexact, total)


def test_neutral_record_equals_the_pick_without_it_bitwise(ctx):
    g = torch.Generator().manual_seed(5)
    for V, B in ((32003, 8), (515, 16), (50, 2)):
        for temp, top_k, top_p, pen in ((0.2, 50, 1.0, 1.0), (1.0, 0, 1.0, 1.0), (0.7, 7, 0.6, 1.0), (0.9, 0, 0.9, 1.3), (0.8, 50, 0.95, 1.2)):
            for _ in range(3):
                logits = (torch.randn(B, V, generator=g) * 2).to(DEV)
                u = torch.rand(B, generator=g).to(DEV)
                seen = torch.randint(0, V, (B, 9), generator=g).int().to(DEV)
                want = ctx.sample_logits_lp(logits, u, temp, top_k, top_p, pen, seen)
                # no record / a neutral record, without the range: the launches of before; with the range: the kernel that carries the tail, no stage on
                for filters, want_range in ((None, False), (SampleFilters(), False), (SampleFilters(min_p=0.0), False), (None, True), (SampleFilters(), True)):
                    got = ctx.sample_logits_filtered(logits, u, temp, top_k, top_p, pen, seen, filters=filters, want_range=want_range)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (V, temp, top_k, top_p, pen, filters, want_range)
                    assert torch.equal(bits(got[2]), bits(want[2])) and torch.equal(bits(got[3]), bits(want[3])), (V, temp, top_k, top_p, pen, filters, want_range)
                # greedy ignores a record
                gw = ctx.sample_logits_lp(logits, None, repetition_penalty=pen, seen_ids=seen, greedy=True)
                gg = ctx.sample_logits_filtered(logits, None, repetition_penalty=pen, seen_ids=seen, greedy=True, filters=SampleFilters(min_p=0.5, typical_p=0.3),
                                                want_range=False)
                assert torch.equal(gg[0], gw[0]) and torch.equal(bits(gg[3]), bits(gw[3]))


def test_edges_ties_band_top_only_nan_and_refusals(ctx):
    def run(row, u, **f):
        got, kept, _m, _p, rng = ctx.sample_logits_filtered(row.to(DEV), torch.tensor([u], device=DEV), 1.0, 0, 1.0, 1.0, filters=SampleFilters(**f))
        return int(got[0]), int(kept[0]), rng[0].tolist()
    # min_p = 1 keeps exactly the maxima: four tied maxima all stay
    row = torch.full((1, 64), -4.0)
    row[0, [3, 17, 40, 41]] = 6.0
    picks = set()
    for i in range(40):
        t, kept, rng = run(row, (i + 0.5) / 40, min_p=1.0)
        assert kept == 4 and rng == [6.0, 6.0]
        picks.add(t)
    assert picks == {3, 17, 40, 41}
    # typical_p tiny keeps exactly the entry nearest the entropy -- here not the maximum
    row = torch.log(torch.tensor([[0.5, 0.25, 0.15, 0.06, 0.04]]))
    near = filter_chain(row[0].double().numpy(), SampleFilters(typical_p=1e-6))
    assert near.sum() == 1 and int(near.argmax()) != 0
    for u in (0.0, 0.5, 0.999):
        t, kept, rng = run(row, u, typical_p=1e-6)
        assert (t, kept) == (int(near.argmax()), 1) and rng == [float(row[0, t])] * 2
    # ... and the two stages behind it keep the top of what is LEFT
    t, kept, rng = run(row, 0.5, typical_p=1e-6, epsilon_cutoff=0.9, eta_cutoff=0.9)
    assert (t, kept) == (int(near.argmax()), 1)
    # epsilon = 0.999 keeps the top only
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(1, 32003, generator=g) * 2
    t, kept, rng = run(wide, 0.7, epsilon_cutoff=0.999)
    assert (t, kept) == (int(wide.argmax()), 1) and rng == [float(wide.max())] * 2
    # an all-NaN row returns token 0 and keeps nothing
    t, kept, rng = run(torch.full((1, 515), float("nan")), 0.3, min_p=0.1, typical_p=0.5, epsilon_cutoff=1e-3, eta_cutoff=1e-3)
    assert (t, kept) == (0, 0) and rng == [float("inf"), float("-inf")]
    # every refusal of the C layer comes back with the value in the message
    logits, u = wide.to(DEV), torch.tensor([0.5], device=DEV)
    for f, msg in (({"min_p": 1.5}, r"`min_p` has to be a float in the \[0, 1\] interval, but is 1.5"), ({"min_p": -0.25}, "`min_p` .* but is -0.25"),
                   ({"typical_p": 0.0}, "`typical_p` has to be a float > 0 and < 1, but is 0"), ({"typical_p": 1.25}, "`typical_p` .* but is 1.25"),
                   ({"epsilon_cutoff": 1.0}, "`epsilon_cutoff` has to be a float > 0 and < 1, but is 1"), ({"epsilon_cutoff": -0.5}, "`epsilon_cutoff` .* but is -0.5"),
                   ({"eta_cutoff": 1.0}, "`eta_cutoff` has to be a float > 0 and < 1, but is 1"), ({"eta_cutoff": -0.5}, "`eta_cutoff` .* but is -0.5")):
        with pytest.raises(ValueError, match=msg):
            ctx.sample_logits_filtered(logits, u, 1.0, 0, 1.0, 1.0, filters=f)


# ---- through the model -------------------------------------------------------------------------------------------------------------------
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


FILT = SampleFilters(min_p=0.02, typical_p=0.9, epsilon_cutoff=1e-4, eta_cutoff=1e-3)


def _step_rule(logits_row, seen, temp, top_k, top_p, pen, f):
    """(nominal mask or None, perturbed masks, x2 row, HF's scores behind top-p [1, V]) of one step's device logits under HF's chain with the ids
    so far."""
    x2, y = hf_chain(logits_row[None], torch.tensor([seen]), temp, top_k, top_p, pen)
    n_lo, n_hi, order = band(x2, top_p)
    n_hf = torch.isfinite(y).sum(-1)
    if top_p >= 1.0:
        n_lo = n_hi = n_hf
    nominal, sets = rule_sets(x2[0], order[0], n_lo[0], n_hi[0], n_hf[0], top_p, f)
    return nominal, sets, x2[0], y


def test_set_filters_refuses_in_the_c_layer_and_leaves_warpers_alone(ctx):
    from video_llava_amd import _lib
    cfg, m = _tiny()
    kv, _nxt, _ = m.prefill([[1, 17, 230, 9, 44]], None, 64)
    for bad, msg in (((1.5, 1.0, 0.0, 0.0), "pgv_kv_set_filters: `min_p` .* but is 1.5"), ((0.0, 0.0, 0.0, 0.0), "`typical_p` .* but is 0"),
                     ((0.0, 1.0, 1.0, 0.0), "`epsilon_cutoff` .* but is 1"), ((0.0, 1.0, 0.0, 2.0), "`eta_cutoff` .* but is 2")):
        with pytest.raises(ValueError, match=msg):
            _lib.check(m.ctx.lib.pgv_kv_set_filters(kv, C.byref(_lib.FilterConfig(*bad))), "pgv_kv_set_filters")
    # the record stays through set_warpers (sample_last sets them on every call) and is dropped by None
    u = torch.tensor([0.9], device=DEV)
    plain = int(m.sample_last(kv, u, 1.0, 0)[0])
    m.set_filters(kv, SampleFilters(epsilon_cutoff=0.999))
    top = int(m.greedy_last(kv, 1)[0])
    assert int(m.sample_last(kv, u, 1.0, 0)[0]) == top and int(m.sample_last(kv, u, 1.0, 0, top_p=0.99)[0]) == top
    m.set_filters(kv, None)
    assert int(m.sample_last(kv, u, 1.0, 0)[0]) == plain


def test_generate_with_filters_equals_stepwise_hf_chain(ctx):
    """Every sampled token equals the fp64 inverse-CDF pick over HF's whole warper chain on THAT step's device logits with the ids so far, for a
    ragged batch, on the steps whose kept set is exact; the chunk size does not matter; the filters change the draw."""
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(2), 20, (3, 40, 0))
    n, temp, top_k, top_p, pen, B = 24, 0.9, 0, 0.95, 1.2, 3
    gen = torch.Generator(device=DEV).manual_seed(11)
    kw = dict(video_spatio_temporal_features=feats_t, do_sample=True, temperature=temp, top_k=top_k, max_new_tokens=n, generator=gen, eos_token_id=None,
              top_p=top_p, repetition_penalty=pen)
    out = m.generate(prompts, chunk=8, filters=FILT, **kw)
    for chunk in (1, 32):
        gen.manual_seed(11)
        assert torch.equal(m.generate(prompts, chunk=chunk, filters=FILT, **kw), out), chunk
    gen.manual_seed(11)
    plain = m.generate(prompts, chunk=32, **kw)
    assert not torch.equal(out, plain)
    # a dict of the same fields, and the fields from a generation config, are the same call
    gen.manual_seed(11)
    assert torch.equal(m.generate(prompts, chunk=32, filters={"min_p": 0.02, "typical_p": 0.9, "epsilon_cutoff": 1e-4, "eta_cutoff": 1e-3}, **kw), out)
    from video_llava_amd.generation import GenerationDefaults
    m.generation_config = GenerationDefaults(typical_p=0.9, epsilon_cutoff=1e-4, eta_cutoff=1e-3, min_p=0.5)
    try:
        gen.manual_seed(11)
        assert torch.equal(m.generate(prompts, chunk=32, filters={"min_p": 0.02}, **kw), out)
        with pytest.raises(ValueError, match="generation_config field `min_p`"):
            m.generate(prompts, chunk=32, **kw)
    finally:
        m.generation_config = None
    gen.manual_seed(11)
    u = torch.rand(n, B, device=DEV, generator=gen).cpu()
    kv, nxt, logits = m.prefill(prompts, feats_t, 128, want_logits=True)
    n_exact = 0
    for i in range(n):
        got = torch.tensor([int(out[b, len(prompts[b]) + i]) for b in range(B)])
        for b in range(B):
            seen = prompts[b] + out[b, len(prompts[b]):len(prompts[b]) + i].tolist()
            nominal, sets, x2, y = _step_rule(logits[b].cpu(), seen, temp, top_k, top_p, pen, FILT)
            t = int(got[b])
            if nominal is not None and all((s == nominal).all() for s in sets):
                mask = torch.from_numpy(nominal)
                # the rules ARE HF's classes on this row too
                assert torch.equal(torch.isfinite(hf_tail(y, FILT))[0], mask), (i, b)
                cdf = cdf_of(torch.where(mask, x2, torch.full_like(x2, float("-inf"))))
                ud = u[i, b].double()
                if float((cdf - ud).abs().min()) > TOL:
                    assert t == int((cdf <= ud).sum().clamp_max(cfg.vocab - 1)), (i, b, t)
                    n_exact += 1
                else:
                    assert nominal[t]
            else:
                assert np.logical_or.reduce(sets)[t], (i, b, t)
        nxt, logits = m.decode_step(kv, got.to(torch.int32).to(DEV), want_logits=True)
    print(f"exact steps: {n_exact}/{n * B}")
    assert n_exact > 0.8 * n * B, n_exact


def test_generate_filters_samples_logprobs_slot_and_width(ctx):
    """samples_per_prompt = 3 with output_logprobs: the ids equal the prompts repeated, transition_scores are the log-softmax of the FILTERED fp64
    scores (HF's compute_transition_scores on `scores`), token_logprobs stay the raw model's.  The same task gives the same ids alone, in a wider
    group and refilled into a slot of generate_continuous.  do_sample=False ignores the record; None / neutral is the call without it."""
    from video_llava_amd.continuous import Task, generate_continuous
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(2), 20, (3, 40, 0))
    n, temp, top_k, top_p, pen = 12, 0.9, 50, 1.0, 1.1
    gen = torch.Generator(device=DEV).manual_seed(3)
    kw = dict(do_sample=True, temperature=temp, top_k=top_k, top_p=top_p, repetition_penalty=pen, max_new_tokens=n, eos_token_id=None, generator=gen, filters=FILT)
    s = m.generate(prompts, video_spatio_temporal_features=feats_t, samples_per_prompt=3, output_logprobs=True, chunk=5, **kw)
    rep = [p for p in prompts for _ in range(3)]
    rep_f = feats_t.repeat_interleave(3, 0)
    gen.manual_seed(3)
    assert torch.equal(m.generate(rep, video_spatio_temporal_features=rep_f, **kw), s.sequences)
    new = new_ids_of(s.sequences, rep, n)
    steps = replay_logits(m, rep, rep_f, new)
    checked = differ = 0
    for i in range(n):
        tok = torch.tensor([new[b][i] for b in range(len(rep))])
        assert_within(s.token_logprobs[:, i], lsm_at(steps[i], tok), row_tol(steps[i]), f"model step {i}")
        for b in range(len(rep)):
            nominal, sets, x2, _y = _step_rule(steps[i][b], rep[b] + new[b][:i], temp, top_k, top_p, pen, FILT)
            if nominal is None or not all((s_ == nominal).all() for s_ in sets):
                continue
            y = torch.where(torch.from_numpy(nominal), x2, torch.full_like(x2, float("-inf")))[None]
            assert_within(s.transition_scores[b, i], lsm_at(y, tok[b:b + 1]), row_tol(x2[None]), f"pick step {i} seq {b}")
            checked += 1
            differ += abs(float(s.transition_scores[b, i]) - float(lsm_at(x2[None], tok[b:b + 1]))) > 2 * float(row_tol(x2[None]))
    assert checked > 0.8 * n * len(rep) and differ >= 1, (checked, differ)
    # slot and group width
    rng = np.random.default_rng(9)
    more, more_f = _prompts(cfg, rng, 20, [int(x) for x in rng.integers(0, 30, 5)])
    all_p, all_f = prompts + more, torch.cat([feats_t, more_f])
    tasks = [Task(i, all_p[i], all_f[i].to(DEV), max_new_tokens=n, seed=500 + i) for i in range(8)]
    ckw = dict(do_sample=True, temperature=temp, top_k=top_k, top_p=top_p, repetition_penalty=pen, eos_token_id=None, filters=FILT)
    alone = {}
    for t in tasks:
        g1 = torch.Generator(device=DEV).manual_seed(t.seed)
        alone[t.task_id] = m.generate([t.ids], video_spatio_temporal_features=t.feats[None], max_new_tokens=n, generator=g1, **ckw)[0, len(t.ids):].tolist()
    for W in (1, 3):
        assert dict(generate_continuous(m, iter(tasks), W, n, refill_min=1, chunk=5, **ckw)) == alone, W
    without = dict(generate_continuous(m, iter(tasks), 3, n, refill_min=1, chunk=5, **dict(ckw, filters=None)))
    assert without != alone
    # greedy ignores the record; None / neutral is the call without the keyword, and a filtered call leaves nothing behind on a kept cache
    gkw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=None)
    assert torch.equal(m.generate(prompts, filters=FILT, **gkw), m.generate(prompts, **gkw))
    skw = dict(gkw, do_sample=True, temperature=temp, generator=gen)
    gen.manual_seed(2)
    s_plain = m.generate(prompts, output_logprobs=True, **skw)
    for neutral in (None, SampleFilters(), {}, {"min_p": 0.0}):
        gen.manual_seed(2)
        got = m.generate(prompts, output_logprobs=True, filters=neutral, **skw)
        assert torch.equal(got.sequences, s_plain.sequences) and torch.equal(bits(got.transition_scores), bits(s_plain.transition_scores))
    one = dict(video_spatio_temporal_features=feats_t[:1], do_sample=True, temperature=temp, max_new_tokens=n, eos_token_id=None, generator=gen, kv_reuse_key="clip")
    gen.manual_seed(4)
    a = m.generate(prompts[:1], **one)
    gen.manual_seed(4)
    m.generate(prompts[:1], filters=FILT, **one)
    gen.manual_seed(4)
    assert torch.equal(m.generate(prompts[:1], **one), a)
    with pytest.raises(ValueError, match="`filters` cannot be combined with `beams`=2"):
        m.generate(prompts[:1], max_new_tokens=4, eos_token_id=None, beams=2, filters=FILT)


def test_runner_refill_with_min_p_equals_the_one_question_wrapper(ctx, tmp_path):
    from test_gpu_runners import _tiny_components
    from video_llava_amd.continuous import sample_seed
    from video_llava_amd.eval import run_inference_qa_activitynet as qa
    from video_llava_amd.inference import video_chatgpt_infer_logprobs
    ccfg, lcfg, cw, lw, tower, model, ip, Vt = _tiny_components()
    tok = _Tok(lcfg.vocab)
    vd = tmp_path / "v"; vd.mkdir()
    for i, n in enumerate(["a", "b", "c"]):
        np.save(vd / f"v_{n}.npy", synth.make_frames(5 + i, ccfg.image, seed=80 + i))
    order = ["a", "b", "c", "a", "b"]
    qs = [{"video_name": n, "question": f"question {'x' * i} {i}?", "question_id": f"q{i}"} for i, n in enumerate(order)]
    (tmp_path / "q.json").write_text(json.dumps(qs)); (tmp_path / "a.json").write_text(json.dumps([{"answer": "x"}] * len(qs)))
    base = ["--video_dir", str(vd), "--gt_file_question", str(tmp_path / "q.json"), "--gt_file_answers", str(tmp_path / "a.json"),
            "--output_dir", str(tmp_path / "out"), "--model-name", "x", "--projection_path", "y", "--max_new_tokens", "16",
            "--schedule", "refill", "--do_sample", "--seed", "7", "--samples_per_prompt", "2"]
    comps = (model, tower, tok, ip, Vt)
    so = tmp_path / "s.jsonl"
    got = qa.run_inference(qa.parse_args(base + ["--output_name", "f", "--batch", "4", "--min_p", "0.1", "--samples_out", str(so)]), components=comps)
    lines = {x["task"]: x for x in (json.loads(x) for x in so.read_text().splitlines())}
    assert len(got) == len(order) == len(lines)
    for i, q in enumerate(qs):
        for j in range(2):
            gen = torch.Generator(device=DEV).manual_seed(sample_seed(7 * 1000003 + i, j))
            ref = video_chatgpt_infer_logprobs(np.load(vd / f"v_{q['video_name']}.npy"), q["question"], "pg-video-llava", model, tower, tok, ip, Vt,
                                               max_new_tokens=16, filters={"min_p": 0.1}, generator=gen)
            assert lines[i]["samples"][j]["text"] == ref["text"], (i, j)
        assert got[i]["pred"] == lines[i]["samples"][lines[i]["picked"]]["text"]
    so2 = tmp_path / "s2.jsonl"
    qa.run_inference(qa.parse_args(base + ["--output_name", "p", "--batch", "4", "--samples_out", str(so2)]), components=comps)
    off = {x["task"]: x for x in (json.loads(x) for x in so2.read_text().splitlines())}
    assert any(off[i]["samples"] != lines[i]["samples"] for i in range(len(order)))          # the flag changes the draw
