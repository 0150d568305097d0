"""pgv_kv_fork: one prefill, N sequences.  A forked slot is bit for bit the slot of the same prompt prefilled again -- cache rows, length, current
token, done flag, seen-set, logits row, latest log-probabilities -- so everything here is torch.equal against the group that ran the
repeat_interleave'd prompts; no tolerances.  Every fork runs in a cache that another group of the same shape has filled before (`_poison`): a
copy that did not happen cannot hide behind identical leftovers."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import synth

from helpers import SynthTokenizer as _Tok, make_model as _model  # noqa: E402
from test_gpu_refill import _prompt, _seven_b  # noqa: E402
from video_llava_amd import _lib
from video_llava_amd.generation import fork_sources

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V_TINY = 20


@pytest.fixture(scope="module")
def tiny(ctx):
    cfg = synth.LLAMA_TINY
    return _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16), cfg.vocab


def _feats(rng, n, V):
    return torch.from_numpy(rng.standard_normal((n, V, 1024)).astype(np.float32) * 0.5).to(torch.float16).to(DEV)


def _poison(m, vocab, W, max_seq, seed=991):
    """Fill all W slots of the (W, max_seq) cache with another group's rows, tokens and seen-sets."""
    rng = np.random.default_rng(seed)
    n = min(max_seq, 90)
    kv, _, _ = m.prefill([[1] + rng.integers(3, vocab - 3, n - 1).tolist() for _ in range(W)], None, max_seq)
    return kv


def _raw_fork(m, kv, counts):
    """pgv_kv_fork itself (model.fork validates the counts on the host first)."""
    P = len(counts)
    _lib.check(m.ctx.lib.pgv_kv_fork(m.ctx.handle, m.handle, kv, (C.c_int32 * P)(*counts), P, _lib.stream_ptr(m.device)), "pgv_kv_fork")


def _steps(m, kv, u, n_steps, temperature=1.0, top_k=50):
    """sample_last with u, then n_steps decode steps: [(tokens, logits or None)]."""
    nxt = m.sample_last(kv, u, temperature, top_k)
    out = [(nxt.clone(), None)]
    for _ in range(n_steps):
        nxt, lg = m.decode_step(kv, nxt, want_logits=True)
        out.append((nxt.clone(), lg.clone()))
    return out


def _run_fork_equals_repeated_prefill(m, vocab, V, counts, seed, max_seq, head_range):
    rng = np.random.default_rng(seed)
    P, W = len(counts), sum(counts)
    src = fork_sources(counts)
    prompts = [_prompt(rng, vocab, int(rng.integers(*head_range)), V, video=(p % 4 != 3)) for p in range(P)]
    feats = _feats(rng, P, V)
    u = torch.rand(W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))       # distinct per slot: the copies diverge
    _poison(m, vocab, W, max_seq)
    kv, _, _ = m.prefill(prompts, feats, max_seq, capacity=W)
    assert m.fork(kv, counts) == W
    got_len = [m.kv_len(kv, i) for i in range(W)]
    got = _steps(m, kv, u, 6)
    got_len2 = [m.kv_len(kv, i) for i in range(W)]
    kv, _, _ = m.prefill([prompts[s] for s in src], feats[src].contiguous(), max_seq)
    ref_len = [m.kv_len(kv, i) for i in range(W)]
    ref = _steps(m, kv, u, 6)
    assert got_len == ref_len == [len(prompts[s]) for s in src]
    assert got_len2 == [m.kv_len(kv, i) for i in range(W)] == [n + 6 for n in ref_len]
    for t, ((gn, gl), (rn, rl)) in enumerate(zip(got, ref)):
        assert torch.equal(gn, rn), (counts, t, (gn != rn).nonzero().flatten().tolist())
        if rl is not None:
            assert torch.equal(gl, rl), (counts, t, (gl != rl).any(dim=1).nonzero().flatten().tolist())
    if max(counts) > 1:
        first = got[0][0].tolist()
        assert any(len(set(first[b:b + c])) > 1 for b, c in zip(np.cumsum([0] + counts[:-1]).tolist(), counts) if c > 1), "the copies never diverged"


@pytest.mark.parametrize("counts", [[2], [2, 2, 2], [1, 3, 1], [17, 17], [64], [16] * 4], ids=lambda c: "-".join(map(str, c)))
def test_fork_equals_repeated_prefill(tiny, counts):
    """[2,2,2]: slot 1 is a source and another source's destination; [17,17]: 34 sequences cross the 16- and 32-sequence column tiles."""
    m, vocab = tiny
    _run_fork_equals_repeated_prefill(m, vocab, V_TINY, counts, 300 + sum(counts), 128, (4, 60))


def test_fork_equals_repeated_prefill_7b_shaped_two_layers(ctx):
    """32 heads, 356 video rows, width 16: the bf16 decode GEMVs stream the 12-bit weight copies."""
    m, vocab = _seven_b(2, "bf16")
    _run_fork_equals_repeated_prefill(m, vocab, 356, [8, 8], 17, 512, (30, 70))


def _peek_all(m, kv, slots, max_seq):
    L = m.config.num_hidden_layers
    return torch.stack([torch.stack([torch.stack([m.kv_peek(kv, l, w, s, 0, max_seq) for w in (0, 1)]) for l in range(L)]) for s in range(slots)]).view(torch.int16)


def test_fork_copies_exactly_rows_0_to_len(tiny):
    """Through pgv_kv_peek: after fork([2,2,2]) rows [0, len) of each new slot are the source's, rows [len, max_seq) of EVERY slot are byte for byte
    what an earlier, longer group left there.  Lengths 1 (a one-token text prompt), 33 and max_seq."""
    m, vocab = tiny
    V, max_seq = V_TINY, 64
    rng = np.random.default_rng(41)
    older = [[1] + rng.integers(3, vocab - 3, n - 1).tolist() for n in (64, 50, 64, 57, 64, 61)]
    m.prefill(older, None, max_seq)
    prompts = [[1], _prompt(rng, vocab, 5, V), _prompt(rng, vocab, 36, V)]
    assert [len(p) for p in prompts] == [1, 33, 64]
    kv, _, _ = m.prefill(prompts, _feats(rng, 3, V), max_seq, capacity=6)
    before = _peek_all(m, kv, 6, max_seq)                      # [slot, layer, K/V, head, row, 128]
    assert m.fork(kv, [2, 2, 2]) == 6
    after = _peek_all(m, kv, 6, max_seq)
    assert before[3:].abs().sum() > 0                          # the unlisted slots really hold the older group's rows
    for i, s in enumerate(fork_sources([2, 2, 2])):
        n = len(prompts[s])
        assert m.kv_len(kv, i) == n
        assert torch.equal(after[i, ..., :n, :], before[s, ..., :n, :]), (i, s)
        assert torch.equal(after[i, ..., n:, :], before[i, ..., n:, :]), (i, s)
    # the read-back itself: a window of rows equals the same rows of the full read; out-of-range windows are refused
    win = m.kv_peek(kv, 1, 1, 4, 7, 9).view(torch.int16)
    assert torch.equal(win, after[4, 1, 1, :, 7:16, :])
    for bad in ((2, 0, 0, 0, 1), (0, 2, 0, 0, 1), (0, 0, 6, 0, 1), (0, 0, 0, 60, 5), (0, 0, 0, -1, 2), (0, 0, 0, 0, 0)):
        with pytest.raises(ValueError):
            m.kv_peek(kv, *bad)


def test_fork_after_decode_steps_then_graph_chunks(tiny):
    """Rows written by the decode path, the single-step graph already captured at width P; then 9 greedy steps in one call at the new width: an
    8-step graph and a single-step graph, both rebuilt for it."""
    m, vocab = tiny
    V, max_seq, counts = V_TINY, 128, [2, 3, 1]
    rng = np.random.default_rng(51)
    src = fork_sources(counts)
    prompts = [_prompt(rng, vocab, int(rng.integers(4, 60)), V) for _ in counts]
    feats = _feats(rng, 3, V)
    _poison(m, vocab, 6, max_seq)
    kv, nxt, _ = m.prefill(prompts, feats, max_seq, capacity=6)
    for _ in range(5):
        nxt, _lg = m.decode_step(kv, nxt)
    assert m.fork(kv, counts) == 6
    got = m.decode_greedy(kv, nxt[src].contiguous(), 9)
    got_len = [m.kv_len(kv, i) for i in range(6)]
    kv, rn, _ = m.prefill([prompts[s] for s in src], feats[src].contiguous(), max_seq)
    for _ in range(5):
        rn, _lg = m.decode_step(kv, rn)
    assert torch.equal(rn, nxt[src])
    ref = m.decode_greedy(kv, rn, 9)
    assert torch.equal(got, ref)
    assert got_len == [m.kv_len(kv, i) for i in range(6)] == [len(prompts[s]) + 14 for s in src]


@pytest.mark.parametrize("chunk", [3, 64])
def test_generate_samples_per_prompt_equals_repeated_prompts(tiny, chunk):
    """top_p, repetition penalty and log-probabilities: the seen-set and the slot's latest log-probabilities travel with the fork -- the first
    token's values included."""
    m, vocab = tiny
    V, n, new = V_TINY, 3, 12
    rng = np.random.default_rng(61)
    prompts = [_prompt(rng, vocab, 9, V), _prompt(rng, vocab, 31, V)]
    feats = _feats(rng, 2, V)
    src = fork_sources([n, n])
    kw = dict(do_sample=True, temperature=0.9, top_p=0.8, repetition_penalty=1.3, output_logprobs=True, max_new_tokens=new, chunk=chunk)
    _poison(m, vocab, 2 * n, (max(len(p) for p in prompts) + new + 63) // 64 * 64)
    tm = {}
    got = m.generate(prompts, video_spatio_temporal_features=feats, generator=torch.Generator(device=DEV).manual_seed(7), samples_per_prompt=n,
                     timings=tm, **kw)
    ref = m.generate([prompts[s] for s in src], video_spatio_temporal_features=feats[src].contiguous(),
                     generator=torch.Generator(device=DEV).manual_seed(7), **kw)
    assert tm["samples_per_prompt"] == n and tm["batch"] == 2 * n
    assert got.sequences.shape[0] == 2 * n and torch.equal(got.sequences, ref.sequences)
    assert torch.equal(got.token_logprobs.view(torch.int32), ref.token_logprobs.view(torch.int32))
    assert torch.equal(got.transition_scores.view(torch.int32), ref.transition_scores.view(torch.int32))
    assert torch.equal(got.new_lengths, ref.new_lengths) and int(got.new_lengths.min()) >= 1
    assert (got.token_logprobs[:, 0] < 0).all()
    rows = [got.sequences[i].tolist() for i in range(2 * n)]
    assert len({tuple(r) for r in rows[:n]}) > 1 or len({tuple(r) for r in rows[n:]}) > 1, "the samples of a prompt never diverged"
    # without the keyword nothing changed: one sample per prompt is the call as it always was
    one = m.generate(prompts, video_spatio_temporal_features=feats, generator=torch.Generator(device=DEV).manual_seed(7), samples_per_prompt=1, **kw)
    plain = m.generate(prompts, video_spatio_temporal_features=feats, generator=torch.Generator(device=DEV).manual_seed(7), **kw)
    assert torch.equal(one.sequences, plain.sequences) and torch.equal(one.token_logprobs.view(torch.int32), plain.token_logprobs.view(torch.int32))


def test_refused_forks_leave_the_cache_unchanged(tiny):
    m, vocab = tiny
    V, max_seq = V_TINY, 128
    rng = np.random.default_rng(71)
    prompts = [_prompt(rng, vocab, 6 + 11 * b, V) for b in range(3)]
    feats = _feats(rng, 3, V)

    def run(refuse):
        kv, nxt, _ = m.prefill(prompts, feats, max_seq, capacity=6)
        out = []
        for t in range(4):
            if refuse and t == 2:
                for counts, what in (([2, 2], "2 counts"), ([1, 1, 1, 1], "4 counts"), ([2, 0, 1], "count 0"), ([1, -3, 1], "count -3"), ([3, 3, 1], "7")):
                    with pytest.raises(ValueError, match=what):
                        _raw_fork(m, kv, counts)
                    assert [m.kv_len(kv, b) for b in range(3)] == [len(p) + 2 for p in prompts]
                with pytest.raises(ValueError):
                    m.fork(kv, [1, 0, 1])                       # the host-side slot map refuses it first
                _raw_fork(m, kv, [1, 1, 1])                     # all ones: accepted, nothing to do
            nxt, lg = m.decode_step(kv, nxt, want_logits=True)
            out.append((nxt.clone(), lg.clone()))
        return out
    ref, got = run(False), run(True)
    for (rn, rl), (gn, gl) in zip(ref, got):
        assert torch.equal(rn, gn) and torch.equal(rl, gl)
    h = C.c_void_p()
    _lib.check(m.ctx.lib.pgv_kv_create(m.ctx.handle, m.handle, 4, 64, C.byref(h)))
    try:
        with pytest.raises(RuntimeError, match="no live group"):
            _raw_fork(m, h, [2])
    finally:
        m.ctx.lib.pgv_kv_destroy(h)


def test_video_chatgpt_infer_samples_and_best_sample(tiny):
    from video_llava_amd.inference import best_sample, build_prompt, video_chatgpt_infer_samples
    m, vocab = tiny
    V, n, new = V_TINY, 5, 10
    tok = _Tok(vocab)
    rng = np.random.default_rng(81)
    feats = _feats(rng, 1, V)[0]
    q, mode = "what happens 0?", "pg-video-llava"
    prompt, stop = build_prompt(q, mode, V, True)
    ids = torch.as_tensor(tok([prompt]).input_ids)
    n_in = ids.shape[1]
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)  # noqa: E731
    free = m.generate(ids, video_spatio_temporal_features=feats[None], do_sample=True, temperature=0.9, max_new_tokens=new, generator=gen(), samples_per_prompt=n)
    assert free.shape == (n, n_in + new)
    eos = collections.Counter(free[:, n_in + 1:].flatten().tolist()).most_common(1)[0][0]        # an "EOS" some answers hit early
    res = video_chatgpt_infer_samples(None, q, mode, m, None, tok, None, V, n, temperature=0.9, max_new_tokens=new, features=feats, generator=gen(),
                                      eos_token_id=eos)
    out = m.generate(ids, video_spatio_temporal_features=feats[None], do_sample=True, temperature=0.9, max_new_tokens=new, generator=gen(), eos_token_id=eos,
                     stop_strings=[stop], tokenizer=tok, samples_per_prompt=n, output_logprobs=True)
    assert len(res) == n and len({len(r["ids"]) for r in res}) > 1
    for j, r in enumerate(res):
        k = int(out.new_lengths[j])
        assert set(r) == {"text", "ids", "token_logprobs", "transition_scores", "logprob"}
        assert r["ids"] == out.sequences[j, n_in:n_in + k].tolist() and 1 <= k <= new
        assert r["text"] == tok.batch_decode([r["ids"]])[0].strip().rstrip(stop).strip()
        assert r["token_logprobs"] == out.token_logprobs[j, :k].tolist() and r["transition_scores"] == out.transition_scores[j, :k].tolist()
        assert r["logprob"] == float(out.sequence_logprob[j])
    best = best_sample(res)
    assert res[best]["logprob"] == max(r["logprob"] for r in res) and all(r["logprob"] < res[best]["logprob"] for r in res[:best])
