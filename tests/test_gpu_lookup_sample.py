"""GPU: prompt-lookup decoding for sampled runs -- generate(do_sample=True, lookup=D, lookup_sample=True).  Every row of a lookup step is picked with
the uniform the plain run draws for that token, so everything here is torch.equal against the plain sampled run from a generator seeded alike; no
tolerances.  What the inputs must exercise is computed from the PLAIN runs and the numpy drafting rule alone (`_plan`), before the code under test
runs; the seeds below were chosen so that it holds."""
import ctypes as C

import numpy as np
import pytest
import torch

from lookup_cases import peek, poison  # noqa: E402
from test_gpu_lookup import NEW, _feats, _new_tokens, _pick_eos, _prompts, ints, tiny  # noqa: E402,F401  (tiny: the module fixture, one model pair per module)
from video_llava_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NGRAM = 2

# per D: the chunk (lookup steps per call) of B = 1, 3, 8 -- B = 3 always runs chunks of 1 or 5, so that its slots enter chunks at unequal emit counts
CHUNKS = {1: (32, 1, 5), 3: (1, 5, 32), 7: (5, 1, 32)}
PICKS = [(0.2, 50), (0.7, 0), (1.0, 5)]
SEEDS = {1: 1000, 3: 3000, 7: 7000}          # base seed of the device generators per D (chosen with _plan; see the module docstring)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _max_seq(prompts, extra=0):
    return (max(len(p) for p in prompts) + NEW + extra + 63) // 64 * 64          # generate's own choice: the poisoned cache is the one it uses


def _chunk_starts_unequal(traces, chunk):
    """Does some chunk of `chunk` lookup steps start with live slots that have emitted different numbers of tokens?  traces[b]: emit count per step."""
    steps = max(len(t) for t in traces)
    for s in range(chunk, steps, chunk):
        live = [1 + sum(t[:s]) for t in traces if len(t) > s]
        if len(set(live)) > 1:
            return True
    return False


def _plan(m, vocab, D, base):
    """The cases of one D with their plain sampled answers, and what those answers exercise.  Runs plain generate() only (sampled and greedy)."""
    from video_llava_amd.lookup_reference import lookup_candidates, lookup_trace
    seen = {"accept": False, "reject": False, "eos_in_run": False, "budget_in_run": False, "not_greedy": False, "unequal_u_base": False}
    cases = []
    for iB, B in enumerate((1, 3, 8)):
        prompts = _prompts(vocab, range(10 * iB, 10 * iB + B))
        feats = _feats(B) if any(vocab - 3 in p for p in prompts) else None
        chunk = CHUNKS[D][iB]
        greedy = _new_tokens(m.generate(prompts, feats, max_new_tokens=NEW, eos_token_id=None), prompts, None)
        settings = [dict(temperature=0.2, top_k=50), dict(zip(("temperature", "top_k"), PICKS[1 + (iB + D) % 2]))]
        if (D, B) == (3, 3):
            settings += [dict(temperature=0.7, top_k=0, top_p=0.9), dict(temperature=1.0, top_k=50, filters={"min_p": 0.05})]
        for i_s, kw in enumerate(settings):
            seed = base + 100 * iB + 10 * i_s
            run = lambda eos: m.generate(prompts, feats, do_sample=True, max_new_tokens=NEW, eos_token_id=eos, chunk=chunk, generator=_gen(seed), **kw)
            plain = run(None)
            answers = _new_tokens(plain, prompts, None)
            picked = _pick_eos(prompts, answers, D, NGRAM)
            for eos in [None] + ([picked[0]] if picked else []):
                if eos is not None:
                    plain = run(eos)
                    answers = _new_tokens(plain, prompts, eos)
                traces = [lookup_trace(p + a[:1], a[1:], D, NGRAM, eos, NEW - 1) for p, a in zip(prompts, answers)]
                cases.append(dict(B=B, prompts=prompts, feats=feats, chunk=chunk, kw=kw, seed=seed, eos=eos, plain=plain, answers=answers, traces=traces))
                seen["not_greedy"] |= any(a[:len(g)] != g[:len(a)] for a, g in zip(answers, greedy))
                if B == 3:
                    seen["unequal_u_base"] |= _chunk_starts_unequal(traces, chunk)
                for b in range(B):
                    e, seq = 0, prompts[b] + answers[b][:1]
                    for c in traces[b]:
                        drafts = lookup_candidates(seq, D, NGRAM, eos)[:max(0, NEW - 1 - e - 1)]
                        rest = answers[b][1 + e:]
                        a = 0
                        while a < len(drafts) and a < len(rest) and drafts[a] == rest[a]:
                            a += 1
                        seen["accept"] |= a > 0
                        seen["reject"] |= a < len(drafts)
                        seq += answers[b][1 + e:1 + e + c]
                        e += c
                    if eos is not None and answers[b][-1] == eos and traces[b][-1] > 1:
                        seen["eos_in_run"] = True
                    if len(answers[b]) == NEW and traces[b][-1] > 1 and (eos is None or answers[b][-1] != eos):
                        seen["budget_in_run"] = True
    return cases, seen


@pytest.mark.parametrize("D", [1, 3, 7])
def test_generate_sampled_lookup_equals_sampled_generate(tiny, D):
    """B in {1, 3, 8}, ragged prompts with and without video rows, chunks of 1, 5 and 32 lookup steps, EOS off and on, three (temperature, top_k)
    pairs, a nucleus and a min_p filter: the ids are those of the sampled call without the two keywords from a generator seeded alike, and the
    device's per-step emit counts are lookup_trace of the PLAIN sampled answer, step for step."""
    models, vocab = tiny
    m = models[torch.float16]
    cases, seen = _plan(m, vocab, D, SEEDS[D])
    print(f"D={D} seed={SEEDS[D]} cases={len(cases)} {seen}")
    assert all(seen.values()), (D, seen)
    for c in cases:
        B, prompts, feats, eos, kw, answers, traces = c["B"], c["prompts"], c["feats"], c["eos"], c["kw"], c["answers"], c["traces"]
        tag = (B, D, eos, c["chunk"], kw)
        max_seq = _max_seq(prompts)
        poison(m, vocab, B, max_seq)
        tm = {}
        got = m.generate(prompts, feats, do_sample=True, max_new_tokens=NEW, eos_token_id=eos, chunk=c["chunk"], generator=_gen(c["seed"]), lookup=D,
                         lookup_ngram=NGRAM, lookup_sample=True, timings=tm, **kw)
        assert torch.equal(got, c["plain"]), tag
        assert tm["lookup_emitted"] == sum(len(a) - 1 for a in answers) and tm["lookup_steps"] == max(len(t) for t in traces), (tm, tag)
        # the device's own counts, from one decode_lookup_sample call on a fresh prefill (the uniforms generate() drew: one torch.rand(NEW, B))
        u = torch.rand(NEW, B, device=DEV, dtype=torch.float32, generator=_gen(c["seed"]))
        kv, _, _ = m.prefill(prompts, feats, max_seq, lookup=(D, NGRAM))
        try:
            if "filters" in kw:
                m.set_filters(kv, kw["filters"])
            nxt = m.sample_last(kv, u[0], kw["temperature"], kw["top_k"], top_p=kw.get("top_p", 1.0))
            toks, counts = m.decode_lookup_sample(kv, nxt, NEW - 1, -1 if eos is None else eos, [NEW - 1] * B, [1] * B, kw["temperature"], kw["top_k"], u)
        finally:
            m.set_filters(kv, None)
            m.set_warpers(kv, 1.0, 1.0)
            m.set_lookup(kv, 0)
        toks = toks.cpu()
        for b in range(B):
            assert int(nxt[b]) == answers[b][0]
            steps = counts[:, b].tolist()
            assert steps[:len(traces[b])] == traces[b] and not any(steps[len(traces[b]):]), (tag, b, steps, traces[b])
            assert toks[b, :sum(traces[b])].tolist() == answers[b][1:]
            assert m.kv_len(kv, b) == len(prompts[b]) + len(answers[b]) - 1


@pytest.mark.parametrize("temperature,top_k,top_p", [(0.2, 50, 1.0), (1.0, 5, 1.0), (0.7, 0, 0.9)])
def test_cache_after_a_sampled_lookup_run_is_the_plain_runs_cache(tiny, temperature, top_k, top_p):
    """After one decode_lookup_sample call the lengths and cache rows [0, len) of every layer are those of the plain sampled run, bit for bit, and 4 plain
    sampled steps from there give the same tokens on both caches (the seen-set and the current tokens took what a plain run gives them)."""
    models, vocab = tiny
    m = models[torch.float16]
    D, B = 3, 3
    prompts = _prompts(vocab, range(10, 10 + B))
    feats = _feats(B) if any(vocab - 3 in p for p in prompts) else None
    max_seq = _max_seq(prompts, 4)
    u = torch.rand(NEW + 4, B, device=DEV, dtype=torch.float32, generator=_gen(4242))
    poison(m, vocab, B, max_seq)
    kv, _, _ = m.prefill(prompts, feats, max_seq, lookup=(D, NGRAM))
    nxt = m.sample_last(kv, u[0], temperature, top_k, top_p=top_p)
    toks, counts = m.decode_lookup_sample(kv, nxt, NEW - 1, -1, [NEW - 1] * B, [1] * B, temperature, top_k, u[:NEW])
    m.set_lookup(kv, 0)
    assert counts.sum(axis=0).tolist() == [NEW - 1] * B
    lens = [m.kv_len(kv, b) for b in range(B)]
    rows = [peek(m, kv, b, 0, lens[b]).clone() for b in range(B)]
    look = toks[:, :NEW - 1].clone()
    tail = m.decode_sample(kv, look[:, -1].contiguous(), 4, -1, temperature, top_k, u[NEW:], top_p=top_p).clone()
    poison(m, vocab, B, max_seq)
    kv2, _, _ = m.prefill(prompts, feats, max_seq)
    nxt2 = m.sample_last(kv2, u[0], temperature, top_k, top_p=top_p)
    plain = m.decode_sample(kv2, nxt2, NEW - 1, -1, temperature, top_k, u[1:NEW], top_p=top_p).clone()
    assert torch.equal(nxt, nxt2) and torch.equal(look, plain)
    assert lens == [m.kv_len(kv2, b) for b in range(B)] == [len(p) + NEW - 1 for p in prompts]
    for b in range(B):
        assert torch.equal(rows[b], peek(m, kv2, b, 0, lens[b])), b
    assert torch.equal(tail, m.decode_sample(kv2, plain[:, -1].contiguous(), 4, -1, temperature, top_k, u[NEW:], top_p=top_p))
    m.set_warpers(kv2, 1.0, 1.0)


def test_sampled_lookup_refusals_leave_the_cache_unchanged(tiny):
    models, vocab = tiny
    m = models[torch.float16]
    rng = np.random.default_rng(5)
    prompts = [[1] + rng.integers(3, vocab - 3, n - 1).tolist() for n in (20, 28)]
    lib, h = m.ctx.lib, m.ctx.handle
    out = torch.full((2, 8), -5, dtype=torch.int32, device=DEV)
    cnt = torch.full((2, 2), -5, dtype=torch.int32, device=DEV)
    other = torch.tensor([5, 6], dtype=torch.int32, device=DEV)            # a refused call must not make these the current tokens
    u = torch.rand(16, 2, device=DEV, generator=_gen(1))
    kv, nxt, _ = m.prefill(prompts, None, 32)

    def look(budget, steps=2, ubase=(1, 1), T=0.7, d_u=u.data_ptr(), u_rows=16, kv_=None, first=other, out_=out, cnt_=cnt):
        hb = ints(ubase) if ubase is not None else None
        return lib.pgv_llm_decode_lookup_sample(h, m.handle, kv if kv_ is None else kv_, first.data_ptr(), steps, -1, ints(budget), hb, C.c_float(T), 50, d_u, u_rows,
                                                out_.data_ptr(), cnt_.data_ptr(), _lib.stream_ptr())

    assert look([1, 1]) == _lib.PGV_ESTATE and b"lookup is off" in lib.pgv_last_error()
    m.set_lookup(kv, 3)
    assert look([1, 1]) == _lib.PGV_ESTATE and b"id record" in lib.pgv_last_error()                     # prefilled before lookup was set
    kv2, nxt, _ = m.prefill(prompts, None, 32, lookup=(3, 2))
    assert kv2.value == kv.value
    before = [peek(m, kv, b, 0, 32) for b in (0, 1)]
    assert look([13, 4]) == _lib.PGV_EINVAL and b"cache holds" in lib.pgv_last_error()                  # 20 + 13 > 32
    assert look([1, 1], steps=0) == _lib.PGV_EINVAL and look([1, 1], steps=33) == _lib.PGV_EINVAL
    assert look([1, 1], T=0.0) == _lib.PGV_EINVAL and b"temperature" in lib.pgv_last_error()
    assert look([1, 1], T=-1.0) == _lib.PGV_EINVAL
    assert look([1, 1], d_u=None) == _lib.PGV_EINVAL and b"null" in lib.pgv_last_error()
    assert look([1, 1], ubase=None) == _lib.PGV_EINVAL and b"null" in lib.pgv_last_error()
    assert look([1, 1], ubase=(1, -1)) == _lib.PGV_EINVAL and b"uniform rows" in lib.pgv_last_error()
    assert look([4, 4], ubase=(12, 13)) == _lib.PGV_EINVAL and b"uniform rows" in lib.pgv_last_error()   # 13 + 4 > 16 rows
    assert look([1, 1], u_rows=33) == _lib.PGV_EINVAL and look([1, 1], u_rows=0) == _lib.PGV_EINVAL     # the cache's own copy holds max_seq rows
    m.set_warpers(kv, 1.0, 1.3)
    assert look([1, 1]) == _lib.PGV_ESTATE and b"repetition penalty" in lib.pgv_last_error()
    m.set_warpers(kv, 1.0, 1.0)
    m.set_logprobs(kv, True)
    assert look([1, 1]) == _lib.PGV_ESTATE and b"log-probabilities" in lib.pgv_last_error()
    m.set_logprobs(kv, False)
    from video_llava_amd.logit_bans import LogitBans
    m.set_bans(kv, LogitBans(suppress=[7]))
    assert look([1, 1]) == _lib.PGV_ESTATE and b"bans" in lib.pgv_last_error()
    m.set_bans(kv, None)
    torch.cuda.synchronize()
    assert (out == -5).all() and (cnt == -5).all() and [m.kv_len(kv, b) for b in (0, 1)] == [20, 28]
    assert all(torch.equal(a, peek(m, kv, b, 0, 32)) for b, a in enumerate(before))
    # the current tokens are still the prefill's: continuing from them (first = None) gives what handing them in gives on a fresh prefill
    a_t, a_c = m.decode_lookup_sample(kv, None, 4, -1, [4, 4], [1, 1], 0.7, 50, u)
    a_t = a_t.clone()
    kv2, nxt2, _ = m.prefill(prompts, None, 32, lookup=(3, 2))
    assert torch.equal(nxt, nxt2)
    b_t, b_c = m.decode_lookup_sample(kv, nxt2, 4, -1, [4, 4], [1, 1], 0.7, 50, u)
    assert torch.equal(a_t, b_t) and (a_c == b_c).all() and a_c.sum(axis=0).tolist() == [4, 4]
    # a beam run in flight
    kv2, nxt, _ = m.prefill(prompts, None, 32, lookup=(3, 2))
    m.beam_begin(kv, 1, 4, -1, 1.0, False)
    assert look([1, 1]) == _lib.PGV_ESTATE and b"beam run" in lib.pgv_last_error()
    m.prefill(prompts, None, 32)                                                                        # a prefill ends the beam run
    m.set_lookup(kv, 0)
    # more rows than a step takes: 5 sequences x (1 + 15) in a cache whose row scratch holds 64
    kv5, nxt5, _ = m.prefill([p[:6] for p in prompts + prompts + prompts[:1]], None, 32, lookup=(15, 2))
    out5, cnt5 = torch.full((5, 32), -5, dtype=torch.int32, device=DEV), torch.full((2, 5), -5, dtype=torch.int32, device=DEV)
    u5 = torch.rand(16, 5, device=DEV, generator=_gen(2))
    before5 = [peek(m, kv5, b, 0, 32) for b in range(5)]
    assert look([1] * 5, ubase=[1] * 5, d_u=u5.data_ptr(), kv_=kv5, first=nxt5, out_=out5, cnt_=cnt5) == _lib.PGV_EINVAL
    assert b"5 sequences x 16 rows" in lib.pgv_last_error()
    torch.cuda.synchronize()
    assert (out5 == -5).all() and (cnt5 == -5).all() and [m.kv_len(kv5, b) for b in range(5)] == [6] * 5
    assert all(torch.equal(a, peek(m, kv5, b, 0, 32)) for b, a in enumerate(before5))
    m.set_lookup(kv5, 0)
    # generate(): do_sample with lookup still needs the new keyword, and the new keyword needs both
    with pytest.raises(ValueError, match="`do_sample` cannot be combined with `lookup`=3"):
        m.generate(prompts, None, do_sample=True, max_new_tokens=4, eos_token_id=None, lookup=3)
    with pytest.raises(ValueError, match="lookup_sample"):
        m.generate(prompts, None, do_sample=False, max_new_tokens=4, eos_token_id=None, lookup=3, lookup_sample=True)
    with pytest.raises(ValueError, match="lookup_sample"):
        m.generate(prompts, None, do_sample=True, max_new_tokens=4, eos_token_id=None, lookup_sample=True)


def test_runner_and_infer_take_lookup_sample(ctx, tmp_path):
    """The QA runner with `--do_sample --lookup 3 --lookup_sample` writes the predictions of `--do_sample` alone from the same generator state, and
    video_chatgpt_infer(do_sample=True, lookup=3, lookup_sample=True) is video_chatgpt_infer(do_sample=True)."""
    import json
    from helpers import SynthTokenizer
    from oracle import synth
    from test_gpu_runners import _tiny_components
    from video_llava_amd.eval import run_inference_qa_activitynet as qa
    from video_llava_amd.inference import video_chatgpt_infer
    ccfg, lcfg, cw, lw, tower, model, ip, V = _tiny_components()
    vd = tmp_path / "v"; vd.mkdir()
    names = ["s1", "s2", "s3"]
    frames = {n: synth.make_frames(5 + i, ccfg.image, seed=60 + i) for i, n in enumerate(names)}
    for n in names:
        np.save(vd / f"v_{n}.npy", frames[n])
    qs = [{"video_name": n, "question": f"what happens {i}?", "question_id": f"{n}_q"} for i, n in enumerate(names)]
    (tmp_path / "q.json").write_text(json.dumps(qs)); (tmp_path / "a.json").write_text(json.dumps([{"answer": "a"}] * 3))
    tok = SynthTokenizer(lcfg.vocab)
    outs = {}
    for tag, extra in (("plain", ["--do_sample"]), ("lookup", ["--do_sample", "--lookup", "3", "--lookup_sample"])):
        args = qa.parse_args(["--video_dir", str(vd), "--gt_file_question", str(tmp_path / "q.json"), "--gt_file_answers", str(tmp_path / "a.json"),
                              "--output_dir", str(tmp_path / tag), "--output_name", "p", "--model-name", "x", "--projection_path", "y",
                              "--conv-mode", "default", "--batch", "3", "--max_new_tokens", "48"] + extra)
        torch.manual_seed(2024)                                # the runner's sampled path draws from the device's default generator
        outs[tag] = qa.run_inference(args, components=(model, tower, tok, ip, V))
    assert [o["pred"] for o in outs["lookup"]] == [o["pred"] for o in outs["plain"]] and all(len(o["pred"].split()) > 5 for o in outs["plain"])
    for i, (n, o) in enumerate(zip(names, outs["plain"])):
        infer = lambda **kw: video_chatgpt_infer(frames[n], o["question"], "default", model, tower, tok, ip, V, do_sample=True, max_new_tokens=48, **kw)
        torch.manual_seed(77 + i)
        want = infer()
        torch.manual_seed(77 + i)
        assert infer(lookup=3, lookup_sample=True) == want and len(want.split()) > 5, (n, want)
