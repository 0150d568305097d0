"""N sampled answers per task from ONE prefill inside a live decode group (pgv_llm_prefill_slots_n, model.prefill_slots(counts=), Task.samples,
--samples_per_prompt).  The contract is bitwise: the call leaves what pgv_llm_prefill_slots leaves for the prompts repeated, so everything here is
torch.equal / == against that twin or against the sample run alone through generate(); no tolerances."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import synth

from helpers import SynthTokenizer as _Tok, make_model as _model  # noqa: E402
from test_gpu_refill import _prompt  # noqa: E402
from video_llava_amd import _lib
from video_llava_amd.continuous import Task, generate_continuous, sample_seed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, MAX_SEQ, W = 20, 256, 8
SLOTS = [6, 0, 3, 7, 5, 1]
TOP_P, PEN, TEMP, TOP_K = 0.7, 1.2, 1.0, 50


@pytest.fixture(scope="module")
def tiny(ctx):
    cfg = synth.LLAMA_TINY
    return _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16), cfg.vocab


def _feats(rng, n):
    return torch.from_numpy(rng.standard_normal((n, V, 1024)).astype(np.float32) * 0.5).to(torch.float16).to(DEV)


def _sized(rng, vocab, total, video):
    """A prompt of exactly `total` tokens, the video run included."""
    if total == 1:
        return [1]
    p = _prompt(rng, vocab, total - 6 - (V + 2 if video else 0), V, video=video)
    assert len(p) == total
    return p


def _group(rng, vocab):
    """The live group every case starts from: 8 ragged prompts, then 5 greedy decode steps."""
    prompts = [_prompt(rng, vocab, int(rng.integers(4, 60)), V) for _ in range(W)]
    return prompts, _feats(rng, W)


def _open(m, vocab, prompts, feats):
    """Poison the cache with another group's rows, open the group, 5 decode steps, log-probability switch on.  -> (kv, current tokens)"""
    rng = np.random.default_rng(991)
    m.prefill([[1] + rng.integers(3, vocab - 3, 199).tolist() for _ in range(W)], None, MAX_SEQ)
    kv, nxt, _ = m.prefill(prompts, feats, MAX_SEQ)
    cur = m.decode_greedy(kv, nxt, 5)[:, -1].contiguous()
    m.set_logprobs(kv, True)
    return kv, cur


def _peek(m, kv, slot, row0, nrows):
    L = m.config.num_hidden_layers
    return torch.stack([torch.stack([m.kv_peek(kv, l, w, slot, row0, nrows) for w in (0, 1)]) for l in range(L)]).view(torch.int16)


def _after(m, kv, cur, slots, lens, nx, lg, u_steps):
    """What a refill left and what follows from it: first tokens, logits, lengths, lp_last, cache rows [0, len) of the listed slots, 12 sampled steps."""
    out = {"nx": nx.clone(), "lg": lg.clone(), "len": [m.kv_len(kv, s) for s in range(W)], "lp_last": m.logprobs_last(kv, W).clone(),
           "rows": [_peek(m, kv, s, 0, n) for s, n in zip(slots, lens)]}
    cur = cur.clone()
    cur[slots] = nx
    out["toks"] = m.decode_sample(kv, cur, 12, -1, TEMP, TOP_K, u_steps, top_p=TOP_P, repetition_penalty=PEN).clone()
    out["lp"] = m.logprobs_steps(kv, W, 12).clone()
    return out


@pytest.mark.parametrize("totals,video,counts", [((1, 63, 65), (False, True, True), [3, 1, 2]), ((64, 7, 130), (True, False, True), [2, 1, 3])],
                         ids=["1-63-65", "64-7-130"])
def test_refill_samples_bitwise_twin(tiny, totals, video, counts):
    """Copied runs of 1, 65, 64 and 130 rows: below, above, at and twice over one copy block of 64 rows (1024 pieces of 16 bytes per head)."""
    m, vocab = tiny
    rng = np.random.default_rng(sum(totals))
    prompts, feats = _group(rng, vocab)
    new = [_sized(rng, vocab, n, v) for n, v in zip(totals, video)]
    new_feats = _feats(rng, 3)
    src = [i for i, c in enumerate(counts) for _ in range(c)]
    lens = [totals[i] for i in src]
    g = torch.Generator(device=DEV).manual_seed(5)
    u = torch.rand(len(SLOTS), device=DEV, generator=g)
    u_steps = torch.rand(12, W, device=DEV, generator=g)
    others = [s for s in range(W) if s not in SLOTS]
    assert others == [2, 4]

    # A: one prefill per prompt
    kv, cur = _open(m, vocab, prompts, feats)
    before = [_peek(m, kv, s, 0, MAX_SEQ) for s in others] + [_peek(m, kv, s, n, 8) for s, n in zip(SLOTS, lens)]
    lp_before = m.logprobs_last(kv, W).clone()
    nx, lg = m.prefill_slots(kv, SLOTS, new, new_feats, want_logits=True, u=u, temperature=TEMP, top_k=TOP_K, top_p=TOP_P, repetition_penalty=PEN,
                             counts=counts)
    assert torch.equal(m.logprobs_last(kv, W)[:, others].view(torch.int32), lp_before[:, others].view(torch.int32))
    after = [_peek(m, kv, s, 0, MAX_SEQ) for s in others] + [_peek(m, kv, s, n, 8) for s, n in zip(SLOTS, lens)]
    for i, (x, y) in enumerate(zip(before, after)):
        assert torch.equal(x, y), ("touched", i)
    a = _after(m, kv, cur, SLOTS, lens, nx, lg, u_steps)
    assert nx.shape == (6,) and lg.shape == (6, vocab)

    # B: the same state from scratch, the prompts repeated through the plain call
    kv, cur_b = _open(m, vocab, prompts, feats)
    assert torch.equal(cur_b, cur)
    nx, lg = m.prefill_slots(kv, SLOTS, [new[i] for i in src], new_feats[src].contiguous(), want_logits=True, u=u, temperature=TEMP, top_k=TOP_K,
                             top_p=TOP_P, repetition_penalty=PEN)
    b = _after(m, kv, cur_b, SLOTS, lens, nx, lg, u_steps)

    assert a["len"] == b["len"] and [a["len"][s] for s in SLOTS] == lens
    assert torch.equal(a["nx"], b["nx"]), (a["nx"].tolist(), b["nx"].tolist())
    assert torch.equal(a["lg"], b["lg"]), (a["lg"] != b["lg"]).any(dim=1).nonzero().flatten().tolist()
    # (the unlisted slots have made no pick since the switch went on: their two values are whatever the cache held before, checked above)
    assert torch.equal(a["lp_last"][:, SLOTS].view(torch.int32), b["lp_last"][:, SLOTS].view(torch.int32))
    for j, (x, y) in enumerate(zip(a["rows"], b["rows"])):
        assert torch.equal(x, y), ("cache rows of slot", SLOTS[j])
    assert torch.equal(a["toks"], b["toks"]), (a["toks"] != b["toks"]).any(dim=1).nonzero().flatten().tolist()
    assert torch.equal(a["lp"].view(torch.int32), b["lp"].view(torch.int32))
    # the samples of one prompt are different answers: they diverge somewhere in the first token or the 12 steps
    seqs = {i: {tuple([int(a["nx"][j])] + a["toks"][SLOTS[j]].tolist()) for j in range(6) if src[j] == i} for i in set(src)}
    assert any(len(v) > 1 for i, v in seqs.items() if counts[i] > 1), "the samples never diverged"


def test_refill_samples_greedy_under_a_penalty(tiny):
    """u = None with penalty 1.3: every sample's seen-set is the prompt's ids alone, so all samples of a prompt pick the same penalised arg-max."""
    m, vocab = tiny
    rng = np.random.default_rng(77)
    prompts, feats = _group(rng, vocab)
    new = [_sized(rng, vocab, n, v) for n, v in zip((1, 63, 65), (False, True, True))]
    new_feats, counts = _feats(rng, 3), [3, 1, 2]
    src = [i for i, c in enumerate(counts) for _ in range(c)]
    res = []
    for twin in (False, True):
        kv, cur = _open(m, vocab, prompts, feats)
        if twin:
            nx, lg = m.prefill_slots(kv, SLOTS, [new[i] for i in src], new_feats[src].contiguous(), want_logits=True, repetition_penalty=1.3)
        else:
            nx, lg = m.prefill_slots(kv, SLOTS, new, new_feats, want_logits=True, repetition_penalty=1.3, counts=counts)
        lp = m.logprobs_last(kv, W).clone()
        cur[SLOTS] = nx
        toks = m.decode_greedy(kv, cur, 8, -1, repetition_penalty=1.3)
        res.append((nx.clone(), lg.clone(), lp, toks.clone(), m.logprobs_steps(kv, W, 8).clone(), [m.kv_len(kv, s) for s in range(W)]))
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][:, SLOTS].view(torch.int32), b[2][:, SLOTS].view(torch.int32))
    assert torch.equal(a[3], b[3]) and torch.equal(a[4].view(torch.int32), b[4].view(torch.int32)) and a[5] == b[5]
    assert len(set(a[0][:3].tolist())) == 1 and len(set(a[0][4:].tolist())) == 1


def test_refill_samples_refusals_leave_the_group_alone(tiny):
    m, vocab = tiny
    rng = np.random.default_rng(13)
    prompts, feats = _group(rng, vocab)
    good = _sized(rng, vocab, 12, False)
    kv, cur = _open(m, vocab, prompts, feats)
    ref = m.decode_step(kv, cur, want_logits=True)
    ref = (ref[0].clone(), ref[1].clone())
    kv, cur = _open(m, vocab, prompts, feats)
    lens = [m.kv_len(kv, s) for s in range(W)]
    bad = [
        ([1, 2], [good, good], [0, 2], "count 0 of sequence 0 is below 1"),
        (list(range(8)) + [8], [good, good], [4, 5], "9 samples"),                  # S over the live width of 8
        ([1, 3, 1], [good, good], [2, 1], "slot 1 listed twice"),
        ([1, 3, 8], [good, good], [2, 1], "slot 8 outside"),
        ([1, -1], [good], [2], "slot -1 outside"),
    ]
    for sl, ps, cn, msg in bad:
        with pytest.raises(ValueError, match=msg):
            m.prefill_slots(kv, sl, ps, None, counts=cn)
        assert [m.kv_len(kv, s) for s in range(W)] == lens
    n2, l2 = m.decode_step(kv, cur, want_logits=True)
    assert torch.equal(n2, ref[0]) and torch.equal(l2, ref[1])
    h = C.c_void_p()
    _lib.check(m.ctx.lib.pgv_kv_create(m.ctx.handle, m.handle, 4, 64, C.byref(h)))
    try:
        with pytest.raises(RuntimeError, match="pgv_llm_prefill_slots_n: no live group"):
            m.prefill_slots(h, [0, 1], [good], None, counts=[2])
    finally:
        m.ctx.lib.pgv_kv_destroy(h)


class _Counting:
    """model.prefill / prefill_slots with the prompts of every call counted; everything else is the model's."""

    def __init__(self, m):
        self._m, self.prompts, self.sequences = m, 0, 0

    def __getattr__(self, name):
        return getattr(self._m, name)

    def prefill(self, seqs, *a, **k):
        self.prompts += len(seqs)
        self.sequences += max(len(seqs), int(k.get("capacity") or 0))
        return self._m.prefill(seqs, *a, **k)

    def prefill_slots(self, kv, slots, seqs, *a, **k):
        self.prompts += len(seqs)
        self.sequences += len(slots)
        return self._m.prefill_slots(kv, slots, seqs, *a, **k)


@pytest.fixture(scope="module")
def sched_case(tiny):
    """10 tasks with 1-3 samples each and, computed once, every sample run alone through generate()."""
    m, vocab = tiny
    rng = np.random.default_rng(31)
    feats = _feats(rng, 10)
    tasks = []
    for i in range(10):
        video = i % 5 != 3
        tasks.append(Task(i, _prompt(rng, vocab, int(rng.integers(3, 50)), V, video=video), feats[i] if video else None,
                          max_new_tokens=int(rng.integers(3, 21)), seed=int(rng.integers(0, 2 ** 31)), samples=int(rng.integers(1, 4))))
    assert {t.samples for t in tasks} == {1, 2, 3}
    want = {}
    for t in tasks:
        for j in range(t.samples):
            g = torch.Generator(device=DEV).manual_seed(sample_seed(t.seed, j))
            out = m.generate([t.ids], video_spatio_temporal_features=t.feats[None] if t.feats is not None else None, do_sample=True, temperature=TEMP,
                             top_k=TOP_K, top_p=TOP_P, repetition_penalty=PEN, max_new_tokens=t.max_new_tokens, generator=g, output_logprobs=True)
            k = int(out.new_lengths[0])
            want[t.task_id, j] = (out.sequences[0, len(t.ids):len(t.ids) + k].tolist(), out.token_logprobs[0, :k].tolist(), out.transition_scores[0, :k].tolist())
    return tasks, want


@pytest.mark.parametrize("width", [3, 4, 8])
def test_scheduler_samples_equal_generate_alone(tiny, sched_case, width):
    m, _ = tiny
    tasks, want = sched_case
    cm, lps, tms = _Counting(m), {}, {}
    got = dict(generate_continuous(cm, iter(tasks), width, 32, do_sample=True, temperature=TEMP, top_k=TOP_K, top_p=TOP_P, repetition_penalty=PEN,
                                   refill_min=1, chunk=5, logprobs=lps, timings=tms, max_seq=MAX_SEQ))
    assert set(got) == {t.task_id for t in tasks}
    for t in tasks:
        new, lp, tm = got[t.task_id], lps[t.task_id], tms[t.task_id]
        if t.samples == 1:
            new, lp, tm = [new], [lp], [tm]
        assert len(new) == len(lp) == len(tm) == t.samples
        for j in range(t.samples):
            ids, model_lp, pick_lp = want[t.task_id, j]
            assert new[j] == ids, (width, t.task_id, j)
            assert lp[j]["token_logprobs"] == model_lp and lp[j]["transition_scores"] == pick_lp, (width, t.task_id, j)
    assert cm.prompts == len(tasks) and cm.sequences >= sum(t.samples for t in tasks)


def test_runner_samples_per_prompt(ctx, tmp_path):
    from test_gpu_runners import _tiny_components
    from video_llava_amd.eval import run_inference_qa_activitynet as qa
    from video_llava_amd.inference import best_sample
    ccfg, lcfg, cw, lw, tower, model, ip, Vt = _tiny_components()
    tok = _Tok(lcfg.vocab)
    vd = tmp_path / "v"; vd.mkdir()
    for i, n in enumerate(["a", "b", "c"]):
        np.save(vd / f"v_{n}.npy", synth.make_frames(5 + i, ccfg.image, seed=80 + i))
    order = ["a", "b", "c", "a", "missing", "b", "c"]
    qs = [{"video_name": n, "question": f"question {'x' * i} {i}?", "question_id": f"q{i}"} for i, n in enumerate(order)]
    (tmp_path / "q.json").write_text(json.dumps(qs)); (tmp_path / "a.json").write_text(json.dumps([{"answer": "x"}] * len(qs)))
    base = ["--video_dir", str(vd), "--gt_file_question", str(tmp_path / "q.json"), "--gt_file_answers", str(tmp_path / "a.json"),
            "--output_dir", str(tmp_path / "out"), "--model-name", "x", "--projection_path", "y", "--max_new_tokens", "24",
            "--schedule", "refill", "--do_sample", "--seed", "7"]
    comps = (model, tower, tok, ip, Vt)
    plain = qa.run_inference(qa.parse_args(base + ["--output_name", "p", "--batch", "4"]), components=comps)
    one = qa.run_inference(qa.parse_args(base + ["--output_name", "o", "--batch", "4", "--samples_per_prompt", "1"]), components=comps)
    assert one == plain and len(plain) == len(order) - 1
    outs = []
    for b in ("3", "8"):
        so = tmp_path / f"s{b}.jsonl"
        outs.append(qa.run_inference(qa.parse_args(base + ["--output_name", f"n{b}", "--batch", b, "--samples_per_prompt", "3", "--sample_pick", "best",
                                                           "--samples_out", str(so)]), components=comps))
        lines = [json.loads(x) for x in so.read_text().splitlines()]
        assert len(lines) == len(order) - 1 and all(len(x["samples"]) == 3 for x in lines)
        by_q = {f"q{x['task']}": x for x in lines}
        for rec in outs[-1]:
            x = by_q[rec["id"]]
            assert x["picked"] == best_sample(x["samples"])
            assert rec["pred"] == x["samples"][x["picked"]]["text"]
        # sample 0 draws from the task's own stream: it is the answer of the run without the flag
        for rec, p in zip(outs[-1], plain):
            x = by_q[rec["id"]]
            assert x["samples"][0]["text"] == p["pred"]
    assert outs[0] == outs[1]
    maj = qa.run_inference(qa.parse_args(base + ["--output_name", "m", "--batch", "8", "--samples_per_prompt", "3", "--sample_pick", "majority"]), components=comps)
    assert len(maj) == len(order) - 1
    for flags in (["--samples_per_prompt", "2", "--schedule", "group"], ["--samples_per_prompt", "0"]):
        with pytest.raises(SystemExit):
            qa.parse_args([a for a in base if a != "--do_sample"] + flags)
