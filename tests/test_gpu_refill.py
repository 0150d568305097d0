"""Continuous batching (pgv_llm_prefill_slots + video_llava_amd.continuous): refilling some slots of a live decode group leaves the other slots
bitwise untouched, and a refilled sequence's tokens and logits are bitwise those of the same prompt run alone."""
import json

import numpy as np
import pytest
import torch

from oracle import synth

from helpers import SynthTokenizer as _Tok, make_model as _model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _prompt(rng, vocab, n_head, V, video=True):
    head = [1] + rng.integers(3, vocab - 3, n_head).tolist()
    tail = rng.integers(3, vocab - 3, 5).tolist()
    return head + ([vocab - 2] + [vocab - 3] * V + [vocab - 1] if video else []) + tail


def _run_refill_case(m, vocab, V, W, seed, max_seq, head_range=(4, 60)):
    """prefill W prompts, 5 decode steps, refill 3 slots (0, one inside, the last) with prompts of other lengths (two with video, one text
    only), 7 decode steps -- every step's tokens and logits against single-sequence runs / the same group without the refill."""
    rng = np.random.default_rng(seed)
    prompts = [_prompt(rng, vocab, int(rng.integers(*head_range)), V) for _ in range(W)]
    feats = torch.from_numpy(rng.standard_normal((W, V, 1024)).astype(np.float32) * 0.5).to(torch.float16).to(DEV)
    slots = sorted({0, W // 2, W - 1}) if W > 1 else [0]
    new = [_prompt(rng, vocab, int(rng.integers(head_range[1], head_range[1] + 40)), V, video=(i != 1)) for i in range(len(slots))]
    new_feats = torch.from_numpy(rng.standard_normal((len(slots), V, 1024)).astype(np.float32) * 0.5).to(torch.float16).to(DEV)
    # the group without the refill: 12 steps
    kv, nxt, lg = m.prefill(prompts, feats, max_seq, want_logits=True)
    ref = [(nxt.clone(), lg.clone())]
    for _ in range(12):
        nxt, lg = m.decode_step(kv, nxt, want_logits=True)
        ref.append((nxt.clone(), lg.clone()))
    # the same group, refilled after step 5
    kv, nxt, lg = m.prefill(prompts, feats, max_seq, want_logits=True)
    for t in range(1, 6):
        nxt, lg = m.decode_step(kv, nxt, want_logits=True)
        assert torch.equal(lg, ref[t][1]) and torch.equal(nxt, ref[t][0]), t
    nx, lgr = m.prefill_slots(kv, slots, new, new_feats, want_logits=True)
    for i, s in enumerate(slots):
        assert m.kv_len(kv, s) == len(new[i])
    untouched = [b for b in range(W) if b not in slots]
    for b in untouched:
        assert m.kv_len(kv, b) == len(prompts[b]) + 5
    cur = nxt.clone()
    cur[slots] = nx
    got = [(nx.clone(), lgr.clone())]
    for t in range(6, 13):
        cur, lg = m.decode_step(kv, cur, want_logits=True)
        for b in untouched:
            assert torch.equal(lg[b], ref[t][1][b]) and int(cur[b]) == int(ref[t][0][b]), (W, b, t)
        got.append((cur[slots].clone(), lg[slots].clone()))
    for i, p in enumerate(new):
        f = new_feats[i:i + 1] if i != 1 else None
        kv1, n1, l1 = m.prefill([p], f, max_seq, want_logits=True)
        for t in range(8):
            assert torch.equal(l1[0], got[t][1][i]), (W, i, t)
            assert int(n1[0]) == int(got[t][0][i]), (W, i, t)
            if t < 7:
                n1, l1 = m.decode_step(kv1, n1, want_logits=True)


@pytest.mark.parametrize("W", [8, 17, 64])
def test_refill_bitwise_tiny(ctx, W):
    cfg = synth.LLAMA_TINY
    m = _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16)
    _run_refill_case(m, cfg.vocab, 20, W, 100 + W, 256)


def _seven_b(layers, weights, seed=11):
    from video_llava_amd import random_init as ri
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    vocab = 32003
    cfg = VideoChatGPTConfig(vocab_size=vocab, hidden_size=4096, intermediate_size=11008, num_hidden_layers=layers, num_attention_heads=32, eos_token_id=None)
    m = VideoChatGPTLlamaForCausalLM(cfg, VisionConfig(frame_size=224), torch.bfloat16, torch.device(DEV))
    ri.load_streaming(m, ri.iter_llama_tensors(vocab=vocab, hidden=4096, inter=11008, layers=layers, device=DEV, dtype=torch.bfloat16, seed=seed))
    vc = m.get_model().vision_config
    vc.vid_patch_token, vc.vid_start_token, vc.vid_end_token, vc.use_vid_start_end = vocab - 3, vocab - 2, vocab - 1, True
    if weights == "fp8":
        m.quantize_weights_fp8()
    return m, vocab


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_refill_bitwise_7b_shaped_two_layers(ctx, weights):
    """Width 16: the bf16 decode GEMVs stream the 12-bit copies; fp8: the e4m3 copies.  356 video rows."""
    m, vocab = _seven_b(2, weights)
    _run_refill_case(m, vocab, 356, 16, 7, 512, head_range=(30, 70))


def test_refill_bitwise_full_7b(ctx):
    """32 layers at width 33 (three MFMA column tiles, the 16-bit stream)."""
    m, vocab = _seven_b(32, "bf16")
    _run_refill_case(m, vocab, 356, 33, 8, 512, head_range=(30, 70))


def test_refill_state_errors_eos_and_idle_rewind(ctx):
    import ctypes as C
    from video_llava_amd import _lib
    cfg = synth.LLAMA_TINY
    m = _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16)
    vocab, V, W = cfg.vocab, 20, 6
    rng = np.random.default_rng(5)
    prompts = [_prompt(rng, vocab, 10 + 3 * b, V) for b in range(W)]
    feats = torch.from_numpy(rng.standard_normal((W, V, 1024)).astype(np.float32)).half().to(DEV)
    kv, nxt, _ = m.prefill(prompts, feats, 128)
    toks = m.decode_greedy(kv, nxt, 4)
    nxt = toks[:, -1].contiguous()
    lens = [m.kv_len(kv, b) for b in range(W)]
    # the next step of the untouched group: what every refused call below must leave intact
    kv_ref, n_ref, _ = m.prefill(prompts, feats, 128)
    t_ref = m.decode_greedy(kv_ref, n_ref, 4)
    step_ref = m.decode_step(kv_ref, t_ref[:, -1].contiguous(), want_logits=True)
    kv, nxt, _ = m.prefill(prompts, feats, 128)
    nxt = m.decode_greedy(kv, nxt, 4)[:, -1].contiguous()
    good = _prompt(rng, vocab, 7, V, video=False)
    bad = [
        ([W], [good], None),                                   # slot outside the live group
        ([-1], [good], None),
        ([1, 1], [good, good], None),                          # duplicate
        ([2], [[1] * 200], None),                              # longer than the cache (128)
        ([2], [[1, vocab + 5, 4]], None),                      # token id outside the vocabulary
        ([2], [[1, vocab - 2] + [vocab - 3] * V], feats[:1]),  # video run without its end token
    ]
    for sl, ps, f in bad:
        with pytest.raises((ValueError, RuntimeError)):
            m.prefill_slots(kv, sl, ps, f)
        assert [m.kv_len(kv, b) for b in range(W)] == lens
    n2, l2 = m.decode_step(kv, nxt, want_logits=True)
    assert torch.equal(l2, step_ref[1]) and torch.equal(n2, step_ref[0])
    # no live group: a fresh cache
    h = C.c_void_p()
    _lib.check(m.ctx.lib.pgv_kv_create(m.ctx.handle, m.handle, 4, 64, C.byref(h)))
    try:
        with pytest.raises(RuntimeError, match="no live group"):
            m.prefill_slots(h, [0], [good], None)
    finally:
        m.ctx.lib.pgv_kv_destroy(h)
    # EOS: slot 0 hits an "EOS" (its own third token), then is refilled: the done flag is cleared and it continues from the new prompt
    kv, nxt, _ = m.prefill(prompts, feats, 128)
    free = m.decode_greedy(kv, nxt, 6)
    eos = int(free[0, 2])
    kv, nxt, _ = m.prefill(prompts, feats, 128)
    t1 = m.decode_greedy(kv, nxt, 6, eos)
    assert t1[0, 2:].tolist() == [eos] * 4
    p0 = _prompt(rng, vocab, 13, V, video=False)
    nx, _ = m.prefill_slots(kv, [0], [p0], None)
    cur = t1[:, -1].contiguous()
    cur[0] = nx[0]
    t2 = m.decode_greedy(kv, cur, 6, eos)
    kv1, s1, _ = m.prefill([p0], None, 128)
    r1 = m.decode_greedy(kv1, s1, 6, eos)
    assert int(nx[0]) == int(s1[0]) and t2[0].tolist() == r1[0].tolist()
    # idle slot rewound every chunk: 20 chunks of 8 steps in a cache of 64 positions, slot 0 refilled each chunk, slot 1 idle
    kv, nxt, _ = m.prefill([[1, 5, 9, 13], [1, 7, 7]], None, 64)
    cur = nxt.clone()
    for c in range(20):
        p = [1] + rng.integers(3, vocab - 3, 20).tolist()
        nx, _ = m.prefill_slots(kv, [0], [p], None)
        cur[0] = nx[0]
        m.kv_truncate(kv, 1, 1)
        toks = m.decode_greedy(kv, cur, 8)
        cur = toks[:, -1].contiguous()
    kv1, s1, _ = m.prefill([p], None, 64)
    assert m.decode_greedy(kv1, s1, 8)[0].tolist() == toks[0].tolist()


def _tasks(rng, vocab, V, n, feats_dev, budgets, seeds=None, stops=None):
    from video_llava_amd.continuous import Task
    out = []
    for i in range(n):
        video = i % 5 != 3
        ids = _prompt(rng, vocab, int(rng.integers(3, 50)), V, video=video)
        out.append(Task(i, ids, feats_dev[i] if video else None, stop=stops[i] if stops else None, max_new_tokens=int(budgets[i]),
                        seed=None if seeds is None else int(seeds[i])))
    return out


def test_continuous_sampling_is_slot_and_width_independent(ctx):
    from video_llava_amd.continuous import generate_continuous
    cfg = synth.LLAMA_TINY
    m = _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16)
    V, n = 20, 70
    rng = np.random.default_rng(9)
    feats = torch.from_numpy(rng.standard_normal((n, V, 1024)).astype(np.float32)).half().to(DEV)
    budgets = rng.integers(2, 24, n)
    tasks = _tasks(rng, cfg.vocab, V, n, feats, budgets, seeds=rng.integers(0, 2 ** 31, n))
    want = {}
    for t in tasks:
        g = torch.Generator(device=DEV).manual_seed(t.seed)
        f = t.feats[None] if t.feats is not None else None
        out = m.generate([t.ids], video_spatio_temporal_features=f, do_sample=True, temperature=1.0, top_k=50, max_new_tokens=t.max_new_tokens,
                         generator=g)
        want[t.task_id] = out[0, len(t.ids):].tolist()
    for W, order in ((1, tasks[:12]), (8, tasks[::-1]), (64, tasks[5:] + tasks[:5])):
        got = dict(generate_continuous(m, order, W, 32, do_sample=True, temperature=1.0, top_k=50, refill_min=1))
        assert len(got) == len(order)
        for t in order:
            assert got[t.task_id] == want[t.task_id], (W, t.task_id)


def test_continuous_scheduler_matches_generate(ctx):
    from video_llava_amd.continuous import generate_continuous

    class StopTok(_Tok):
        def __init__(self, vocab, stop_ids):
            super().__init__(vocab)
            self.stop_ids = set(stop_ids)

        def batch_decode(self, ids, skip_special_tokens=True):
            return [" ".join("###" if int(t) in self.stop_ids else str(int(t)) for t in row) for row in ids]

    cfg = synth.LLAMA_TINY
    m = _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16)
    V, n = 20, 40
    rng = np.random.default_rng(21)
    feats = torch.from_numpy(rng.standard_normal((n, V, 1024)).astype(np.float32)).half().to(DEV)
    budgets = rng.integers(1, 51, n)
    stops = ["###" if i % 3 == 0 else None for i in range(n)]
    tasks = _tasks(rng, cfg.vocab, V, n, feats, budgets, stops=stops)
    # EOS / stop ids: tokens that some free-running answers emit early
    free = [m.generate([t.ids], video_spatio_temporal_features=t.feats[None] if t.feats is not None else None, max_new_tokens=30)[0, len(t.ids):].tolist()
            for t in tasks[:12]]
    import collections
    common = [tk for tk, _ in collections.Counter(tk for f in free for tk in f[1:]).most_common(3)]
    eos, stop_ids = common[0], set(common[1:])
    tok = StopTok(cfg.vocab, stop_ids)
    want = {}
    for t in tasks:
        f = t.feats[None] if t.feats is not None else None
        out = m.generate([t.ids], video_spatio_temporal_features=f, max_new_tokens=t.max_new_tokens, eos_token_id=eos,
                         stop_strings=[t.stop], tokenizer=tok)
        new = out[0, len(t.ids):].tolist()
        want[t.task_id] = new
    assert sum(len(want[t.task_id]) < t.max_new_tokens for t in tasks) >= 2                    # EOS / stop strings end answers early
    tm = {}
    got = dict(generate_continuous(m, iter(tasks), 8, 50, tokenizer=tok, eos_token_id=eos, timings=tm))
    assert set(got) == set(want)
    for i in want:
        assert got[i] == want[i], (i, got[i], want[i])
    assert all(tm[i]["steps"] >= 0 and tm[i]["group_size"] >= 1 for i in want)


def test_runner_refill_schedule_matches_group(ctx, tmp_path):
    from test_gpu_runners import _tiny_components
    from video_llava_amd.eval import run_inference_qa_activitynet as qa
    ccfg, lcfg, cw, lw, tower, model, ip, V = _tiny_components()
    tok = _Tok(lcfg.vocab)
    vd = tmp_path / "v"; vd.mkdir()
    for i, n in enumerate(["a", "b", "c"]):
        np.save(vd / f"v_{n}.npy", synth.make_frames(5 + i, ccfg.image, seed=80 + i))
    order = ["a", "b", "c", "a", "missing", "b", "c"]
    qs = [{"video_name": n, "question": f"question {'x' * i} {i}?", "question_id": f"q{i}"} for i, n in enumerate(order)]
    (tmp_path / "q.json").write_text(json.dumps(qs)); (tmp_path / "a.json").write_text(json.dumps([{"answer": "x"}] * len(qs)))
    base = ["--video_dir", str(vd), "--gt_file_question", str(tmp_path / "q.json"), "--gt_file_answers", str(tmp_path / "a.json"),
            "--output_dir", str(tmp_path / "out"), "--model-name", "x", "--projection_path", "y", "--max_new_tokens", "24"]
    comps = (model, tower, tok, ip, V)
    outs = {}
    for sched in ("group", "refill"):
        for b in ("2", "auto"):
            outs[sched, b] = qa.run_inference(qa.parse_args(base + ["--output_name", f"{sched}{b}", "--schedule", sched, "--batch", b]), components=comps)
            assert json.loads((tmp_path / "out" / f"{sched}{b}.json").read_text()) == outs[sched, b]
    assert outs["refill", "2"] == outs["group", "2"] == outs["refill", "auto"] == outs["group", "auto"]
    assert len(outs["group", "2"]) == len(order) - 1
    sampled = [qa.run_inference(qa.parse_args(base + ["--output_name", f"s{b}", "--schedule", "refill", "--do_sample", "--seed", "7", "--batch", b]),
                                components=comps) for b in ("1", "2", "64")]
    assert sampled[0] == sampled[1] == sampled[2] and len(sampled[0]) == len(order) - 1
