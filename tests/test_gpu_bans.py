"""GPU: HF's -inf processors on the device (csrc/logit_ban.hip), from the kernel (pgv_ban_logits) and the per-slot id record (pgv_kv_ids_peek) up to
model.generate(bans=) / generate_continuous(bans=).

Yardsticks: video_llava_amd.logit_bans.banned_ids for the kernel (itself held to the installed HF by tests/test_bans_cpu.py), and HF's own processors
(tests/bans_hf.py) applied on the CPU to the stepped device logits for the runs.  A ban is a set of indices: every comparison of ban sets and tokens
is exact.  The only float comparisons are log-probabilities against values recomputed on the host from the same device logits, with the bound of
tests/test_gpu_gen_logprobs.py (row_tol: 5e-5 + 2^-21 * max |finite score| of the row).
"""
import numpy as np
import pytest
import torch

from bans_hf import hf_scores
from oracle import synth
from test_gpu_gen_logprobs import assert_within, bits, lsm_at, new_ids_of, replay_logits, row_tol
from test_gpu_warpers import band, cdf_of
from test_gpu_warpers import hf_chain as warp_chain
from video_llava_amd.logit_bans import LogitBans, banned_ids

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = float("-inf")
STRIDE = 4096


def _tiny(seed=3):
    from helpers import make_model
    cfg = synth.LLAMA_TINY
    return cfg, make_model(cfg, synth.make_llama_weights(cfg, seed=seed, head_std=0.08), torch.float16)


def _prompts(cfg, rng, Vr, extras):
    PATCH, START, END = cfg.vocab - 3, cfg.vocab - 2, cfg.vocab - 1
    prompts, feats = [], []
    for extra in extras:
        prompts.append([1] + rng.integers(3, cfg.vocab - 3, 5 + extra).tolist() + [START] + [PATCH] * Vr + [END] + rng.integers(3, cfg.vocab - 3, 4).tolist())
        feats.append(torch.from_numpy(rng.standard_normal((Vr, 1024), dtype=np.float32)))
    return prompts, torch.stack(feats).half()


# ---- 1. the kernel against the rules -------------------------------------------------------------------------------------------------------------
def _kernel_case(V, B, rng, n):
    """Rows of mixed lengths over a small alphabet (n-grams repeat), a configuration that exercises every rule, logits with -inf and NaN entries."""
    alphabet = rng.choice(V, min(8, V), replace=False)
    pool = [0, 1, max(n - 1, 0), n, 63, 64, 65, 1000, 4095]
    lens = [pool[(b + n) % len(pool)] for b in range(B)]         # B >= 9 covers the whole pool
    lens[0] = 4095                                               # the longest record in every case
    if B >= 2:
        lens[1] = n
    ids = np.full((B, STRIDE), -7, dtype=np.int32)               # entries behind a row's length: never read (they would change the matches)
    for b in range(B):
        ids[b, :lens[b]] = rng.choice(alphabet, lens[b])
    plens = [int(rng.integers(0, L + 1)) if b % 2 else L for b, L in enumerate(lens)]
    eos = int(alphabet[0])
    words = [[int(t) for t in rng.choice(alphabet, int(rng.integers(1, 6)))] for _ in range(5)]
    for b in range(B):                               # words whose prefix IS the end of a row
        if lens[b] >= 3:
            words.append([int(t) for t in ids[b, lens[b] - 2:lens[b]]] + [int(rng.integers(0, V))])
    words.append([int(t) for t in rng.choice(alphabet, 16)])
    bans = LogitBans(no_repeat_ngram=n, bad_words=words[:40], suppress=[int(t) for t in rng.integers(0, V, 4)],
                     begin_suppress=[int(t) for t in rng.integers(0, V, 3)], min_length=66, min_new_tokens=3).check(V, eos)
    logits = torch.from_numpy(rng.standard_normal((B, V)).astype(np.float32) * 3)
    flat = logits.view(-1)
    k = max(1, flat.numel() // 50)
    flat[torch.from_numpy(rng.integers(0, flat.numel(), k))] = NEG
    flat[torch.from_numpy(rng.integers(0, flat.numel(), k))] = float("nan")
    return bans, eos, logits, ids, lens, plens


def _run_kernel(ctx, bans, eos, logits, ids, lens, plens):
    dev = logits.to(DEV).contiguous()
    ctx.ban_logits(dev, torch.from_numpy(ids).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV),
                   torch.tensor(plens, dtype=torch.int32, device=DEV), bans, eos)
    return dev.cpu()


@pytest.mark.parametrize("V,B", [(32003, 8), (515, 17), (50, 2), (1, 1)])
def test_kernel_equals_the_rules(ctx, V, B):
    rng = np.random.default_rng(V * 3 + B)
    banned_rows = 0
    for n in (1, 2, 3, 5):
        bans, eos, logits, ids, lens, plens = _kernel_case(V, B, rng, n)
        got = _run_kernel(ctx, bans, eos, logits, ids, lens, plens)
        for b in range(B):
            want = banned_ids(bans, ids[b, :lens[b]].tolist(), plens[b], eos, V)
            mask = torch.zeros(V, dtype=torch.bool)
            mask[sorted(want)] = True
            print(f"V={V} B={B} n={n} row {b}: L={lens[b]} prompt={plens[b]} banned={len(want)}")
            assert bool((got[b][mask] == NEG).all()), (n, b, "an id of the set is not -inf")
            assert torch.equal(bits(got[b][~mask]), bits(logits[b][~mask])), (n, b, "an entry outside the set changed")
            banned_rows += bool(want)
    assert banned_rows >= 2 * B                     # the comparison does not pass on empty sets


def test_kernel_rows_do_not_depend_on_the_batch(ctx):
    """The same inputs through one 64-row call and as 64 one-row calls give the same bytes."""
    V, B = 515, 64
    bans, eos, logits, ids, lens, plens = _kernel_case(V, B, np.random.default_rng(64), 3)
    whole = _run_kernel(ctx, bans, eos, logits, ids, lens, plens)
    for b in range(B):
        one = _run_kernel(ctx, bans, eos, logits[b:b + 1], ids[b:b + 1], lens[b:b + 1], plens[b:b + 1])
        assert torch.equal(bits(one[0]), bits(whole[b])), b


def test_kernel_neutral_configuration_leaves_the_buffer_alone(ctx):
    V, B = 515, 3
    _, eos, logits, ids, lens, plens = _kernel_case(V, B, np.random.default_rng(1), 2)
    for bans, e in ((LogitBans(), eos), (LogitBans(min_length=100, min_new_tokens=100), -1)):
        got = _run_kernel(ctx, bans, e, logits, ids, lens, plens)
        assert torch.equal(bits(got), bits(logits))


def test_kernel_refuses_limits_and_out_of_range_ids_with_the_value(ctx):
    V, B = 50, 1
    args = (torch.zeros(B, V, device=DEV), torch.zeros(B, 8, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV),
            torch.zeros(B, dtype=torch.int32, device=DEV))
    for bans, word in ((LogitBans(bad_words=[[1, 2]] * 257), "257 bad words"), (LogitBans(bad_words=[[1] * 17]), "17 ids"),
                       (LogitBans(suppress=[1] * 1000, begin_suppress=[2] * 25), "1025 listed ids"), (LogitBans(suppress=[50]), "id 50 outside"),
                       (LogitBans(bad_words=[[3, 77]]), "id 77 outside"), (LogitBans(begin_suppress=[-1]), "id -1 outside"),
                       (LogitBans(no_repeat_ngram=-2), "is -2")):
        with pytest.raises(ValueError, match=word):
            ctx.ban_logits(*args, bans, 2)           # unchecked records: the refusal is the library's
    assert float(args[0].abs().sum()) == 0.0


# ---- 2. the id record ----------------------------------------------------------------------------------------------------------------------------
def test_id_record_follows_every_call(ctx):
    """After prefill, 5 decode steps, pgv_kv_truncate, _append, pgv_kv_fork([2, 1, 3]) and a _slots_n refill, pgv_kv_ids_peek equals the host's
    bookkeeping of every slot: the ids handed to the prefills plus every token a step consumed, at their cache positions, and the prompt length."""
    cfg, m = _tiny()
    rng = np.random.default_rng(6)
    prompts, feats_t = _prompts(cfg, rng, 20, (2, 11, 0))
    bans = LogitBans(no_repeat_ngram=2).check(cfg.vocab)
    kv, _nxt, _ = m.prefill(prompts, feats_t, 128, capacity=6, bans=bans)
    try:
        rec = [list(p) for p in prompts]
        plen = [len(p) for p in prompts]

        def check(what):
            for s, r in enumerate(rec):
                assert m.kv_len(kv, s) == len(r), (what, s, m.kv_len(kv, s), len(r))
                got, got_plen = m.ids_peek(kv, s, len(r))
                assert got == r and got_plen == plen[s], (what, s, got_plen, plen[s])

        check("prefill")
        cur = m.greedy_last(kv, 3)                                   # the banned first token: consumed by the first step
        toks = m.decode_greedy(kv, cur, 5)
        for b in range(3):
            rec[b] += [int(cur[b])] + toks[b, :4].tolist()
        cur = toks[:, 4].contiguous()
        check("5 decode steps")
        m.kv_truncate(kv, 1, len(rec[1]) - 3)
        rec[1] = rec[1][:-3]
        check("truncate")
        more = [rng.integers(3, cfg.vocab - 3, k).tolist() for k in (4, 1, 9)]
        _kv, cur, _ = m.prefill(more, None, 0, append_to=kv)
        for b in range(3):
            rec[b] += more[b]
            plen[b] = len(rec[b])                                    # HF sees the whole conversation as the prompt
        check("append")
        m.fork(kv, [2, 1, 3])
        src = [0, 0, 1, 2, 2, 2]
        rec, plen, cur = [list(rec[i]) for i in src], [plen[i] for i in src], cur[torch.tensor(src, device=DEV)].contiguous()
        check("fork")
        fresh = [rng.integers(3, cfg.vocab - 3, k).tolist() for k in (7, 30)]
        nx, _ = m.prefill_slots(kv, [4, 1, 5], fresh, None, counts=[2, 1])
        for s, i in ((4, 0), (1, 0), (5, 1)):
            rec[s], plen[s] = list(fresh[i]), len(fresh[i])
        cur[torch.tensor([4, 1, 5], device=DEV)] = nx
        check("slots_n refill")
        toks = m.decode_greedy(kv, cur, 2)
        for s in range(6):
            rec[s] += [int(cur[s]), int(toks[s, 0])]
        check("steps after the refill")
    finally:
        m.set_bans(kv, None)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------------------
def _greedy_setup():
    """B = 3 ragged prompts; EOS = a token the unbanned greedy run emits within 6 steps; a two-id bad word and a suppressed id taken from the other rows
    of that run, so that every rule bites."""
    cfg, m = _tiny(seed=8)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(4), 20, (2, 17, 6))
    free = m.generate(prompts, video_spatio_temporal_features=feats_t, max_new_tokens=48, eos_token_id=None)
    new = new_ids_of(free, prompts, 48)
    eos = new[0][2]
    raw = LogitBans(no_repeat_ngram=2, min_new_tokens=6, bad_words=[[new[1][0], new[1][1]]], suppress=[new[2][0]])
    return cfg, m, prompts, feats_t, eos, raw


def _host_greedy(m, prompts, feats_t, raw, eos, n):
    """Step with plain pgv_llm_decode, apply HF's processors to the returned logits on the CPU, take the first-index arg-max; EOS is sticky."""
    B = len(prompts)
    kv, _nxt, logits = m.prefill(prompts, feats_t, 128, want_logits=True)
    ids, done, new = [list(p) for p in prompts], [False] * B, [[] for _ in range(B)]
    for _ in range(n):
        step = []
        for b in range(B):
            if done[b]:
                step.append(eos)
                continue
            x = hf_scores(raw, ids[b], len(prompts[b]), eos, logits[b].cpu())
            t = int(torch.argmax(x))
            step.append(t); ids[b].append(t); new[b].append(t)
            done[b] = t == eos
        if all(done):
            break
        _nxt, logits = m.decode_step(kv, torch.tensor(step, dtype=torch.int32, device=DEV), want_logits=True)
    return new


def test_greedy_with_bans_equals_host_loop(ctx):
    cfg, m, prompts, feats_t, eos, raw = _greedy_setup()
    n, B = 48, 3
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=eos)
    free = m.generate(prompts, **kw)
    out = m.generate(prompts, bans=raw, chunk=6, **kw)
    want = _host_greedy(m, prompts, feats_t, raw, eos, n)
    for b in range(B):
        k = len(want[b])
        row = out[b, len(prompts[b]):].tolist()
        print(f"row {b}: {k} new tokens, eos {eos}: {want[b]}")
        assert row[:k] == want[b] and all(t == eos for t in row[k:]), (b, row, want[b])
        assert out[b, :len(prompts[b])].tolist() == prompts[b]
        # the conditions that make the comparison mean something
        f = free[b, len(prompts[b]):].tolist()
        f = f[:f.index(eos) + 1] if eos in f else f
        assert f != want[b], (b, "the bans did not change the row")
        assert k >= 6, (b, k)                                                   # min_new_tokens
        seq = prompts[b] + want[b]
        for t in range(len(prompts[b]), len(seq)):                              # no generated token completes a bigram the sequence already holds
            earlier = set(zip(seq[:t - 1], seq[1:t]))
            assert (seq[t - 1], seq[t]) not in earlier, (b, t, "a bigram repeats")
        assert raw.suppress[0] not in want[b]


def test_sampled_with_bans_equals_stepwise_hf_chain(ctx):
    cfg, m = _tiny()
    prompts, feats_t = _prompts(cfg, np.random.default_rng(2), 20, (3, 40, 0))
    n, temp, top_k, top_p, pen, B = 24, 0.7, 50, 0.9, 1.1, 3
    gen = torch.Generator(device=DEV).manual_seed(11)
    kw = dict(video_spatio_temporal_features=feats_t, do_sample=True, temperature=temp, top_k=top_k, max_new_tokens=n, generator=gen, eos_token_id=None,
              top_p=top_p, repetition_penalty=pen)
    plain = m.generate(prompts, chunk=32, **kw)
    p_new = new_ids_of(plain, prompts, n)
    raw = LogitBans(no_repeat_ngram=2, bad_words=[[p_new[0][0], p_new[0][1]], [p_new[1][3]]], suppress=[p_new[2][0]], begin_suppress=[p_new[1][0]])
    gen.manual_seed(11)
    out = m.generate(prompts, chunk=7, bans=raw, **kw)
    assert not torch.equal(out, plain)
    gen.manual_seed(11)
    u = torch.rand(n, B, device=DEV, generator=gen).cpu()
    kv, _nxt, logits = m.prefill(prompts, feats_t, 128, want_logits=True)
    n_exact = 0
    for i in range(n):
        got = [int(out[b, len(prompts[b]) + i]) for b in range(B)]
        for b in range(B):
            seen = prompts[b] + out[b, len(prompts[b]):len(prompts[b]) + i].tolist()
            x = hf_scores(raw, seen, len(prompts[b]), -1, logits[b].cpu())
            assert x[got[b]] > NEG, (i, b, "a banned token was drawn")
            x2, y = warp_chain(x[None], torch.tensor([seen]), temp, top_k, top_p, pen)
            n_lo, n_hi, _ = band(x2, top_p)
            cdf = cdf_of(y)[0]
            want = int((cdf <= u[i, b].double()).sum().clamp_max(cfg.vocab - 1))
            if int(n_lo) == int(n_hi) and float((cdf - u[i, b].double()).abs().min()) > 1e-5:
                assert got[b] == want, (i, b, got[b], want)
                n_exact += 1
            else:
                assert float(torch.softmax(x2[0], -1)[got[b]]) > 0
        _nxt, logits = m.decode_step(kv, torch.tensor(got, dtype=torch.int32, device=DEV), want_logits=True)
    assert n_exact > 0.9 * n * B, n_exact


def test_logprobs_under_bans(ctx):
    """token_logprobs stay the raw log-softmax (HF's `logits`), transition_scores are the log-softmax of the processed scores (HF's `scores`); the
    two differ in at least one step.  Greedy without a penalty, and sampled."""
    cfg, m, prompts, feats_t, eos, raw = _greedy_setup()
    n, B = 16, 3
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=None)
    raw = LogitBans(no_repeat_ngram=2, bad_words=raw.bad_words, suppress=raw.suppress)
    ids = m.generate(prompts, bans=raw, **kw)
    a = m.generate(prompts, bans=raw, output_logprobs=True, chunk=5, **kw)
    assert torch.equal(a.sequences, ids)
    new = new_ids_of(ids, prompts, n)
    steps = replay_logits(m, prompts, feats_t, new)
    differ = 0
    for i in range(n):
        tok = torch.tensor([new[b][i] for b in range(B)])
        assert_within(a.token_logprobs[:, i], lsm_at(steps[i], tok), row_tol(steps[i]), f"greedy model step {i}")
        for b in range(B):
            x = hf_scores(raw, prompts[b] + new[b][:i], len(prompts[b]), -1, steps[i][b])[None]
            want = lsm_at(x, tok[b:b + 1])
            assert_within(a.transition_scores[b, i], want, row_tol(x), f"greedy pick step {i} seq {b}")
            differ += abs(float(a.transition_scores[b, i]) - float(a.token_logprobs[b, i])) > 2 * float(row_tol(x))
    print(f"greedy: {differ} of {n * B} steps with pick != model")
    assert differ >= 1
    # sampled
    temp, top_k, top_p, pen = 0.7, 50, 0.9, 1.1
    gen = torch.Generator(device=DEV).manual_seed(5)
    skw = dict(kw, do_sample=True, temperature=temp, top_k=top_k, top_p=top_p, repetition_penalty=pen, generator=gen)
    s = m.generate(prompts, bans=raw, output_logprobs=True, chunk=7, **skw)
    gen.manual_seed(5)
    assert torch.equal(m.generate(prompts, bans=raw, **skw), s.sequences)
    new = new_ids_of(s.sequences, prompts, n)
    steps = replay_logits(m, prompts, feats_t, new)
    differ = n_open = 0
    for i in range(n):
        tok = torch.tensor([new[b][i] for b in range(B)])
        assert_within(s.token_logprobs[:, i], lsm_at(steps[i], tok), row_tol(steps[i]), f"sampled model step {i}")
        for b in range(B):
            seen = prompts[b] + new[b][:i]
            x = hf_scores(raw, seen, len(prompts[b]), -1, steps[i][b])[None]
            x2, y = warp_chain(x, torch.tensor([seen]), temp, top_k, top_p, pen)
            n_lo, n_hi, _ = band(x2, top_p)
            if int(n_lo) != int(n_hi):
                n_open += 1
                continue
            assert_within(s.transition_scores[b, i], lsm_at(y, tok[b:b + 1]), row_tol(x2), f"sampled pick step {i} seq {b}")
            differ += abs(float(s.transition_scores[b, i]) - float(s.token_logprobs[b, i])) > 2 * float(row_tol(x2))
    assert differ >= 1 and n_open <= 0.1 * n * B, (differ, n_open)


def test_ids_do_not_depend_on_chunk_slot_or_width(ctx):
    from video_llava_amd.continuous import Task, generate_continuous
    cfg, m, prompts, feats_t, eos, raw = _greedy_setup()
    kw = dict(max_new_tokens=20, eos_token_id=eos, bans=raw)
    base = m.generate(prompts, video_spatio_temporal_features=feats_t, chunk=32, **kw)
    for chunk in (1, 7):
        assert torch.equal(m.generate(prompts, video_spatio_temporal_features=feats_t, chunk=chunk, **kw), base), chunk
    # the same task alone, at width 8 (among other tasks), and as a refill of generate_continuous
    rng = np.random.default_rng(9)
    more, more_f = _prompts(cfg, rng, 20, [int(x) for x in rng.integers(0, 30, 5)])
    all_p, all_f = prompts + more, torch.cat([feats_t, more_f])
    alone = {i: m.generate([all_p[i]], video_spatio_temporal_features=all_f[i:i + 1], **kw)[0, len(all_p[i]):].tolist() for i in range(8)}
    for i in range(3):
        assert alone[i] == base[i, len(prompts[i]):len(prompts[i]) + len(alone[i])].tolist()
    wide = m.generate(all_p, video_spatio_temporal_features=all_f, **kw)
    for i in range(8):
        assert wide[i, len(all_p[i]):len(all_p[i]) + len(alone[i])].tolist() == alone[i], i
    tasks = [Task(i, all_p[i], all_f[i].to(DEV), max_new_tokens=20) for i in range(8)]
    for W in (2, 3):
        got = dict(generate_continuous(m, iter(tasks), W, 20, refill_min=1, chunk=5, eos_token_id=eos, bans=raw))
        assert got == alone, W
    # sampled: samples_per_prompt = 3 equals the prompts repeated
    gen = torch.Generator(device=DEV).manual_seed(3)
    skw = dict(do_sample=True, temperature=0.8, max_new_tokens=12, eos_token_id=eos, bans=raw, generator=gen)
    forked = m.generate(prompts, video_spatio_temporal_features=feats_t, samples_per_prompt=3, **skw)
    gen.manual_seed(3)
    rep = [p for p in prompts for _ in range(3)]
    repeated = m.generate(rep, video_spatio_temporal_features=feats_t.repeat_interleave(3, 0), **skw)
    assert torch.equal(forked, repeated)


def test_off_means_off(ctx):
    cfg, m, prompts, feats_t, eos, raw = _greedy_setup()
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=16, eos_token_id=eos)
    plain = m.generate(prompts, output_logprobs=True, **kw)
    for neutral in (None, LogitBans(), {}, LogitBans(bad_words=[[eos]])):
        got = m.generate(prompts, output_logprobs=True, bans=neutral, **kw)
        assert torch.equal(got.sequences, plain.sequences)
        assert torch.equal(bits(got.token_logprobs), bits(plain.token_logprobs)) and torch.equal(bits(got.transition_scores), bits(plain.transition_scores))
    gen = torch.Generator(device=DEV).manual_seed(2)
    skw = dict(kw, do_sample=True, temperature=0.9, generator=gen)
    s_plain = m.generate(prompts, **skw)
    gen.manual_seed(2)
    assert torch.equal(m.generate(prompts, bans=LogitBans(), **skw), s_plain)
    # a call with bans, then one without: the cache's configuration was cleared
    banned = m.generate(prompts, bans=raw, **kw)
    assert not torch.equal(banned, plain.sequences)
    assert torch.equal(m.generate(prompts, **kw), plain.sequences)
    gen.manual_seed(2)
    assert torch.equal(m.generate(prompts, **skw), s_plain)


def test_beams_with_bans_raise(ctx):
    cfg, m = _tiny()
    ids = [1, 17, 230, 9, 44]
    with pytest.raises(ValueError, match="`bans` cannot be combined with `beams`=2"):
        m.generate([ids], max_new_tokens=4, eos_token_id=None, beams=2, bans=LogitBans(no_repeat_ngram=2))
    assert m.generate([ids], max_new_tokens=4, eos_token_id=None, beams=2, bans=LogitBans()).shape[0] == 1
    # ... and the library refuses a beam run on a cache that has bans set
    kv, _nxt, _ = m.prefill([ids], None, 64, capacity=2, bans=LogitBans(suppress=[5]).check(cfg.vocab))
    try:
        with pytest.raises(Exception, match="logit bans are set"):
            m.beam_begin(kv, 2, 4)
    finally:
        m.set_bans(kv, None)
