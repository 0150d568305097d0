"""Beam search on the device: the in-group cache gather (pgv_kv_gather), the beam pick on crafted logits (pgv_beam_pick_logits) and the whole
run (pgv_beam_begin / pgv_llm_decode_beam / generate(beams=K)) against the numpy rules of video_llava_amd/beam_reference.py -- which
tests/test_beam_cpu.py checks against HF's own generate(num_beams=K)."""
import itertools

import numpy as np
import pytest
import torch

from oracle import synth

from helpers import make_model as _model  # noqa: E402
from test_gpu_fork import _feats, _peek_all, _poison, _steps  # noqa: E402
from test_gpu_refill import _prompt, _seven_b  # noqa: E402
from video_llava_amd import _lib
from video_llava_amd import beam_reference as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V_TINY = 20
EOS = 2
# The end-to-end cases (P, K, N, length_penalty, early_stopping) and the (seed, lm_head scale) of the model each one runs on: chosen on the GPU so that
# every selection boundary of the case's reference run is >= 1e-2 wide (each test asserts it) and hypotheses end on EOS.
E2E_SHAPES = [(3, 3, 10, 1.0, False), (2, 4, 12, 2.0, True), (1, 8, 9, 0.0, "never"), (3, 2, 20, 1.0, "never")]
E2E_MODELS = [(2, 150.0)] * 4
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def tiny(ctx):
    cfg = synth.LLAMA_TINY
    return _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16), cfg.vocab


def beam_weights(seed, scale=25.0):
    """LLAMA_TINY with an lm_head scaled so that candidates lie far apart, and an EOS row that follows ten other tokens: EOS reaches the
    top K at several steps."""
    cfg = synth.LLAMA_TINY
    w = synth.make_llama_weights(cfg, seed=seed, head_std=0.08)
    w["lm_head.weight"] = w["lm_head.weight"] * np.float32(scale)
    w["lm_head.weight"][EOS] = np.float32(0.7) * w["lm_head.weight"][3:13].sum(0)
    return cfg, w


@pytest.fixture(scope="module")
def beam_models(ctx):
    """(seed, scale) -> (model, vocab), built once per module."""
    built = {}

    def get(key):
        if key not in built:
            cfg, w = beam_weights(*key)
            built[key] = (_model(cfg, w, torch.float16), cfg.vocab)
        return built[key]
    return get


# ---- 1. gather ----------------------------------------------------------------------------------------------------------------------------
def _group_state(m, vocab, P, K, suffix, max_seq, seed):
    """P ragged prompts in a poisoned cache, forked to K slots each, then `suffix` sampled steps with distinct uniforms: the copies diverge.
    -> (kv, prompt lengths, current tokens [P * K])."""
    rng = np.random.default_rng(seed)
    W = P * K
    prompts = [_prompt(rng, vocab, int(rng.integers(4, 30)), V_TINY, video=(p != 1)) for p in range(P)]
    feats = _feats(rng, P, V_TINY)
    _poison(m, vocab, W, max_seq)
    kv, _, _ = m.prefill(prompts, feats, max_seq, capacity=W)
    m.fork(kv, [K] * P)
    u = torch.rand(W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    cur = _steps(m, kv, u, suffix)[-1][0]
    return kv, [len(p) for p in prompts], cur


def _greedy(m, kv, cur, n):
    out = []
    for _ in range(n):
        cur, lg = m.decode_step(kv, cur, want_logits=True)
        out.append((cur.clone(), lg.clone()))
    return out


def _check_gather(m, vocab, P, K, suffix, src, max_seq=128, seed=77, steps=3):
    W = P * K
    full = [g * K + src[g * K + i] for g in range(P) for i in range(K)]
    kv, row0, cur = _group_state(m, vocab, P, K, suffix, max_seq, seed)
    before = _peek_all(m, kv, W, max_seq)
    lens = [m.kv_len(kv, i) for i in range(W)]
    assert lens == [row0[i // K] + suffix for i in range(W)]
    m.kv_gather(kv, K, src, row0)
    after = _peek_all(m, kv, W, max_seq)
    for i, s in enumerate(full):
        n = lens[i]
        assert torch.equal(after[i, ..., :n, :], before[s, ..., :n, :]), (src, i, s)
        assert torch.equal(after[i, ..., n:, :], before[i, ..., n:, :]), (src, i, "rows beyond the length changed")
    assert [m.kv_len(kv, i) for i in range(W)] == lens
    got = _greedy(m, kv, cur[full].contiguous(), steps)
    kv, _, cur2 = _group_state(m, vocab, P, K, suffix, max_seq, seed)              # the control run: the same state, never gathered
    assert torch.equal(cur, cur2)
    ref = _greedy(m, kv, cur2, steps)
    for t, ((gn, gl), (rn, rl)) in enumerate(zip(got, ref)):
        assert torch.equal(gn, rn[full]) and torch.equal(gl, rl[full]), (src, t)
    if suffix and K > 1:
        assert any(not torch.equal(before[g * K, ..., row0[g]:lens[g * K], :], before[g * K + 1, ..., row0[g]:lens[g * K], :]) for g in range(P)), "the beams never diverged"


MAPS3 = {"identity": [0, 1, 2] * 3, "broadcast": [1, 1, 1] * 3, "swap": [1, 0, 2] * 3, "cycle": [1, 2, 0] * 3, "mixed": [0, 1, 2, 2, 2, 0, 1, 0, 2]}


@pytest.mark.parametrize("suffix", [0, 1, 9])
def test_gather_maps_at_three_suffix_lengths(tiny, suffix):
    """P = 3 ragged prompts x K = 3; suffix 0 is right after the fork (nothing to move).  Through pgv_kv_peek: new slot i holds old slot src[i] on
    [0, len) in every layer and plane, rows >= len keep the poison; then 3 greedy steps are bit for bit those of slot src[i] in an ungathered run."""
    m, vocab = tiny
    for name, src in MAPS3.items():
        _check_gather(m, vocab, 3, 3, suffix, src, seed=70 + suffix)


@pytest.mark.parametrize("K", [1, 2, 8])
def test_gather_group_widths(tiny, K):
    m, vocab = tiny
    P = 2 if K == 8 else 3
    src = np.random.default_rng(K).integers(0, K, P * K).tolist()
    _check_gather(m, vocab, P, K, 4, src, seed=90 + K)


def test_gather_7b_shaped_two_layers(ctx):
    """32 heads, 356 video rows: the grid's (plane, head) rows at the real head count."""
    m, vocab = _seven_b(2, "bf16")
    rng = np.random.default_rng(5)
    P, K, max_seq, suffix = 2, 4, 512, 3
    prompts = [_prompt(rng, vocab, int(rng.integers(30, 70)), 356) for _ in range(P)]
    feats = _feats(rng, P, 356)
    kv, _, _ = m.prefill(prompts, feats, max_seq, capacity=P * K)
    m.fork(kv, [K] * P)
    u = torch.rand(P * K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    _steps(m, kv, u, suffix)
    src = [3, 3, 0, 1, 1, 2, 3, 0]
    full = [g * K + src[g * K + i] for g in range(P) for i in range(K)]
    before = _peek_all(m, kv, P * K, max_seq)
    m.kv_gather(kv, K, src, [len(p) for p in prompts])
    after = _peek_all(m, kv, P * K, max_seq)
    for i, s in enumerate(full):
        n = len(prompts[i // K]) + suffix
        assert torch.equal(after[i, ..., :n, :], before[s, ..., :n, :]) and torch.equal(after[i, ..., n:, :], before[i, ..., n:, :]), (i, s)


def test_refused_gathers_leave_the_cache_unchanged(tiny):
    """Host-checked bad arguments: the return code only, and the cache as it was."""
    m, vocab = tiny
    kv, row0, _cur = _group_state(m, vocab, 3, 3, 2, 128, 55)
    before = _peek_all(m, kv, 9, 128)
    ok = [0, 1, 2] * 3
    bad = [(4, ok, row0),                              # the width 9 is no multiple of 4
           (2, ok, row0 + row0[:1]),
           (9, ok, row0[:1]), (0, ok, row0),            # group width outside [1, 8]
           (3, [0, 3, 2] + ok[3:], row0), (3, [0, -1, 2] + ok[3:], row0),
           (3, ok, [0] + row0[1:]),                     # row0 outside [1, len]
           (3, ok, row0[:2] + [row0[2] + 3])]
    for K, src, r0 in bad:
        with pytest.raises(ValueError):
            m.kv_gather(kv, K, src, r0)
    assert torch.equal(_peek_all(m, kv, 9, 128), before)
    empty = m._get_kv(5, 192)                                  # a cache no prefill has filled: no live group
    with pytest.raises(RuntimeError, match="no live group"):
        m.kv_gather(empty, 1, [0] * 5, [1] * 5)


# ---- 2. the pick on crafted logits ---------------------------------------------------------------------------------------------------------
def _craft(rng, st, K, V, t, eos, mode):
    """Logits [K, V] whose log-softmax is EXACT in fp32 on the device and in the reference: one entry per row at the row maximum (exp 0 = 1), every
    other entry at least 60 below it (the sum of exponentials is 1.0 in fp32 and fp64, its logarithm 0), all values multiples of 0.25 -- so scores
    are exact sums and equal scores are exact ties.  mode: "ties" (equal values inside a row and, from step 1 on, across beams), "eos_top" (EOS is
    beam 0's best), "eos_all" (EOS is every beam's best, everything else far below: all top-K candidates end), "inf" (-inf entries)."""
    x = np.empty((K, V), dtype=np.float32)
    second0 = 0.0                                              # how far beam 0's second candidate lies below its best
    far = 5000.0 if mode == "eos_all" else 1000.0
    base = 2000.0 if mode == "eos_all" else 60.0
    for k in range(K):
        M = np.float32(0.25 * rng.integers(-40, 40))
        x[k] = M - np.float32(far)
        if mode == "inf":
            x[k, rng.random(V) < 0.3] = -np.inf
        cols = rng.permutation(np.arange(3, V))[:2 * K + 2]
        d = base + 0.25 * rng.integers(0, 160, cols.size)
        d[0] = 0.0
        if mode == "ties":
            d[2] = d[1]                                        # a tie inside the row
        if mode in ("eos_top", "eos_all") and (k == 0 or mode == "eos_all"):
            cols[0] = eos
        x[k, cols] = M - d.astype(np.float32)
        if mode == "ties" and k == 1 and t >= 1 and st.run[1] > -1e8:
            # a tie across beams: a candidate of beam 1 scores exactly what beam 0's second candidate does
            want = np.float32(st.run[0]) - np.float32(second0) - np.float32(st.run[1])
            if -900 < want <= -60:
                x[1, cols[3]] = M + want
        if k == 0:
            second0 = d[1]
    return x


PICK_MODES = ["ties", "eos_top", "ties", "eos_all", "inf", "ties"]          # step t runs PICK_MODES[t]; the last step is the budget's


def _run_pick_case(ctx, V, P, K, configs, seed):
    rng = np.random.default_rng(seed)
    N = len(PICK_MODES)
    for early, lp in configs:
        states = [br.BeamState(K) for _ in range(P)]
        d_state = torch.from_numpy(np.stack([s.to_words() for s in states]).view(np.int32)).to(DEV)
        saw_eos_finish = saw_eos_backup = False
        for t in range(N):
            logits = np.concatenate([_craft(rng, states[p], K, V, t, EOS, PICK_MODES[t]) for p in range(P)])
            tok, par = ctx.beam_pick_logits(torch.from_numpy(logits).to(DEV), d_state, K, t, N, EOS, lp, br.early_code(early))
            tok, par, words = tok.cpu().numpy().reshape(P, K), par.cpu().numpy().reshape(P, K), d_state.cpu().numpy().view(np.uint32)
            for p in range(P):
                res = br.beam_step(states[p], logits[p * K:(p + 1) * K], t, N, EOS, lp, early)
                where = (V, P, K, early, lp, t, p)
                assert tok[p].tolist() == res.tokens.tolist() and par[p].tolist() == res.parents.tolist(), where
                got, ref = br.BeamState.from_words(words[p], K), states[p]
                for name in ("fin_len", "fin_parent", "fin_tok", "fin_flag"):
                    assert getattr(got, name).tolist() == getattr(ref, name).tolist(), (where, name)
                assert (got.unsat, got.open) == (ref.unsat, ref.open), where
                for name in ("run", "fin_score"):
                    g, r = getattr(got, name).astype(np.float64), getattr(ref, name).astype(np.float64)
                    assert (np.abs(g - r) <= ULP * np.maximum(1.0, np.abs(r))).all(), (where, name, g, r)
                eos_rank = [j for j in range(2 * K) if res.top_index[j] % V == EOS]
                saw_eos_finish |= any(j < K for j in eos_rank)
                saw_eos_backup |= any(j >= K for j in eos_rank)
        assert saw_eos_finish, (V, P, K, early, lp)
        if K > 1:
            assert all(s.fin_flag.any() for s in states), (V, P, K, early, lp)
    return saw_eos_backup


ALL_CONFIGS = list(itertools.product((False, True, "never"), (0.0, 1.0, 2.0)))


@pytest.mark.parametrize("P,K", list(itertools.product((1, 3, 8), (1, 2, 3, 5, 8))), ids=lambda v: str(v))
def test_pick_on_crafted_logits_small_vocab(ctx, P, K):
    """V = 515, every early_stopping x length_penalty, six steps from the start state (step 0: the -1e9 beams) to the budget: parents, tokens, flags
    and the finished bookkeeping are exactly the numpy rules, scores within 2^-23 max(1, |score|)."""
    _run_pick_case(ctx, 515, P, K, ALL_CONFIGS, 1000 + 10 * P + K)


@pytest.mark.parametrize("P,K", [(1, 1), (3, 3), (8, 8), (1, 5), (3, 2)], ids=lambda v: str(v))
def test_pick_on_crafted_logits_real_vocab(ctx, P, K):
    _run_pick_case(ctx, 32003, P, K, [(False, 1.0), (True, 2.0), ("never", 0.0)], 2000 + 10 * P + K)


def test_pick_eos_among_the_backups_does_not_finish(ctx):
    """EOS at a rank in [K, 2K): the candidate is pushed out of the running beams but is no finished hypothesis."""
    K, V, N = 3, 515, 4
    st = br.BeamState(K)
    st.run[:] = [0.0, -1.0, -2.0]
    x = np.full((K, V), -1000.0, dtype=np.float32)
    for k in range(K):
        x[k, 10 + k] = 0.0                                     # ranks 0, 1, 2
    x[0, 20], x[0, EOS], x[0, 21] = -60.0, -61.0, -62.0        # ranks 3, 4 (EOS), 5
    ref = br.BeamState.from_words(st.to_words(), K)
    d_state = torch.from_numpy(st.to_words().view(np.int32)[None]).to(DEV)
    tok, par = ctx.beam_pick_logits(torch.from_numpy(x).to(DEV), d_state, K, 1, N, EOS, 1.0, 0)
    res = br.beam_step(ref, x, 1, N, EOS, 1.0, False)
    assert res.top_index.tolist()[4] == EOS and tok.tolist() == res.tokens.tolist() == [10, 11, 12]
    got = br.BeamState.from_words(d_state.cpu().numpy().view(np.uint32)[0], K)
    assert not got.fin_flag.any() and not ref.fin_flag.any() and par.tolist() == res.parents.tolist() == [0, 1, 2]
    assert got.run.tolist() == ref.run.tolist() == [0.0, -1.0, -2.0]


def test_pick_refusals(ctx):
    """Host-checked bad arguments: the return code only."""
    for kw in (dict(beams=9), dict(t=5), dict(t=-1), dict(max_new_tokens=0), dict(eos_id=515), dict(early_stopping=3), dict(length_penalty=float("inf"))):
        a = dict(beams=2, t=0, max_new_tokens=5, eos_id=EOS, length_penalty=1.0, early_stopping=0)
        a.update(kw)
        lg = torch.zeros(a["beams"], 515, device=DEV)
        st = torch.zeros(1, _lib.beam_state_words(a["beams"]), dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError):
            ctx.beam_pick_logits(lg, st, **a)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------------
def _prompts(vocab, P, seed=9):
    rng = np.random.default_rng(seed)
    prompts = [_prompt(rng, vocab, int(rng.integers(4, 30)), V_TINY, video=(p != 1)) for p in range(P)]
    return prompts, _feats(rng, P, V_TINY)


def reference_beams(m, prompts, feats, K, N, lp, early, max_seq=128):
    """The numpy rules driven step by step with pgv_llm_decode logits and pgv_kv_gather -> [BeamRun per prompt]."""
    P, W = len(prompts), len(prompts) * K
    kv, _, lg = m.prefill(prompts, feats, max_seq, want_logits=True, capacity=W)
    m.fork(kv, [K] * P)
    runs = [br.BeamRun(K, N, EOS, lp, early) for _ in range(P)]
    lg = lg.cpu().numpy()
    logits = np.repeat(lg, K, axis=0)
    row0 = [len(p) for p in prompts]
    while True:
        tok, par = zip(*[runs[p].step(logits[p * K:(p + 1) * K]) for p in range(P)])
        if runs[0].t >= N or not any(r.state.open for r in runs):
            return runs
        m.kv_gather(kv, K, np.concatenate(par).tolist(), row0)
        _, lg = m.decode_step(kv, torch.from_numpy(np.concatenate(tok).astype(np.int32)).to(DEV), want_logits=True)
        logits = lg.cpu().numpy()


def device_beams(m, prompts, feats, K, N, lp, early, chunk, max_seq=128, eos=EOS):
    P = len(prompts)
    kv, _, _ = m.prefill(prompts, feats, max_seq, capacity=P * K)
    m.beam_begin(kv, K, N, eos, lp, early)
    done = 1
    while done < N and any(m.beam_open(kv, P)):
        n = min(chunk, N - done)
        m.decode_beam(kv, n)
        done += n
    return [[m.beam_result(kv, p, r) for r in range(K)] for p in range(P)], done


@pytest.mark.parametrize("case", range(len(E2E_SHAPES)), ids=lambda i: "-".join(map(str, E2E_SHAPES[i])))
def test_abi_run_equals_the_rules_step_by_step(beam_models, case):
    """All K hypotheses of every prompt: sequences exact, flags equal, scores within steps x 2^-23 max(1, |score|) (fp32 accumulation of that many
    terms; the device takes ln sum exp from its row-statistics kernel).  The reference run's selection boundaries are all >= 1e-2 wide."""
    (P, K, N, lp, early), (m, vocab) = E2E_SHAPES[case], beam_models(E2E_MODELS[case])
    prompts, feats = _prompts(vocab, P)
    runs = reference_beams(m, prompts, feats, K, N, lp, early)
    margin = min(r.margin for r in runs)
    print(f"P {P} K {K} N {N} lp {lp} early {early}: smallest selection margin {margin:.4g}, steps {runs[0].t}")
    assert margin >= 1e-2, margin
    got, _ = device_beams(m, prompts, feats, K, N, lp, early, 4)
    for p in range(P):
        for r, ((toks, score, fin), (rt, rs, rf)) in enumerate(zip(got[p], runs[p].results())):
            assert toks == rt and fin == rf, (p, r, toks, rt)
            assert abs(score - rs) <= max(1, len(rt)) * ULP * max(1.0, abs(rs)), (p, r, score, rs)
    assert any(t and t[-1] == EOS for p in range(P) for t, _s, _f in got[p]), "no hypothesis ended on EOS"


def test_generate_beams_equals_the_rules_whatever_the_chunk(beam_models):
    m, vocab = beam_models(E2E_MODELS[0])
    P, K, N = E2E_SHAPES[0][:3]
    prompts, feats = _prompts(vocab, P)
    runs = reference_beams(m, prompts, feats, K, N, 1.0, False)
    assert min(r.margin for r in runs) >= 1e-2
    outs = [m.generate(prompts, feats, max_new_tokens=N, eos_token_id=EOS, beams=K, chunk=c, output_beam_scores=True) for c in (1, 8, 32)]
    for o in outs[1:]:
        assert torch.equal(o.sequences, outs[0].sequences) and torch.equal(o.sequences_scores, outs[0].sequences_scores) and torch.equal(o.new_lengths, outs[0].new_lengths)
    plain = m.generate(prompts, feats, max_new_tokens=N, eos_token_id=EOS, beams=K)
    assert torch.equal(plain, outs[0].sequences)
    for p in range(P):
        toks, score, _fin = runs[p].results()[0]
        n = int(outs[0].new_lengths[p])
        assert outs[0].sequences[p, :len(prompts[p]) + n].tolist() == prompts[p] + toks
        assert abs(float(outs[0].sequences_scores[p]) - score) <= len(toks) * ULP * max(1.0, abs(score))
    # a prompt alone and inside the batch of 3: bit for bit
    for p in (0, 2):
        alone = m.generate([prompts[p]], feats[p:p + 1] if p != 1 else None, max_new_tokens=N, eos_token_id=EOS, beams=K, output_beam_scores=True)
        n = int(alone.new_lengths[0])
        assert n == int(outs[0].new_lengths[p]) and torch.equal(alone.sequences[0], outs[0].sequences[p, :len(prompts[p]) + n])
        assert torch.equal(alone.sequences_scores[0], outs[0].sequences_scores[p])


def test_abi_run_at_one_beam_is_greedy_decoding(beam_models):
    m, vocab = beam_models(E2E_MODELS[0])
    prompts, feats = _prompts(vocab, 3)
    N = 9
    kv, nxt, _ = m.prefill(prompts, feats, 128)
    want = torch.cat([nxt[:, None], m.decode_greedy(kv, nxt, N - 1)], dim=1).cpu().tolist()
    got, done = device_beams(m, prompts, feats, 1, N, 1.0, False, 32, eos=-1)       # no EOS: the one hypothesis is the budget's
    assert done == N
    for p in range(3):
        assert got[p][0][0] == want[p] and got[p][0][2], (p, got[p][0], want[p])


def test_beam_calls_refuse_without_a_run(beam_models):
    m, vocab = beam_models(E2E_MODELS[0])
    prompts, feats = _prompts(vocab, 2)
    kv, nxt, _ = m.prefill(prompts, feats, 128, capacity=8)
    with pytest.raises(RuntimeError, match="no beam run"):
        m.decode_beam(kv, 1)
    with pytest.raises(ValueError):
        m.beam_begin(kv, 5, 4, EOS)                            # 2 prompts x 5 beams in a cache of 8
    with pytest.raises(ValueError):
        m.beam_begin(kv, 2, 0, EOS)
    m.beam_begin(kv, 2, 3, EOS)
    m.decode_beam(kv, 2)
    with pytest.raises(ValueError, match="exceed max_new_tokens"):
        m.decode_beam(kv, 1)
    m.decode_step(kv, nxt.repeat_interleave(2).contiguous())   # any other stepping call ends the run
    with pytest.raises(RuntimeError, match="no beam run"):
        m.beam_open(kv, 2)


def test_video_chatgpt_infer_beams(beam_models):
    """The one-question wrapper: the best hypothesis of generate(beams=K) for the built prompt, cut and cleaned like the reference's answers."""
    from helpers import SynthTokenizer
    from video_llava_amd.inference import build_prompt, video_chatgpt_infer_beams
    from video_llava_amd.model.utils import first_stop_length
    m, vocab = beam_models(E2E_MODELS[0])
    tok = SynthTokenizer(vocab)
    feats = _feats(np.random.default_rng(81), 1, V_TINY)[0]
    q, mode, K, N = "what happens 0?", "pg-video-llava", 3, 8
    prompt, stop = build_prompt(q, mode, V_TINY, True)
    ids = torch.as_tensor(tok([prompt]).input_ids)
    n_in = ids.shape[1]
    out = m.generate(ids, video_spatio_temporal_features=feats[None], max_new_tokens=N, eos_token_id=EOS, beams=K, length_penalty=0.5, output_beam_scores=True)
    res = video_chatgpt_infer_beams(None, q, mode, m, None, tok, None, V_TINY, K, length_penalty=0.5, max_new_tokens=N, features=feats, eos_token_id=EOS)
    new = out.sequences[0, n_in:n_in + int(out.new_lengths[0])].tolist()
    cut = first_stop_length(new, tok, [stop]) if stop else None
    assert set(res) == {"text", "ids", "score"} and res["ids"] == (new if cut is None else new[:cut]) and 1 <= len(new) <= N
    assert res["score"] == float(out.sequences_scores[0])
    greedy = video_chatgpt_infer_beams(None, q, mode, m, None, tok, None, V_TINY, 1, max_new_tokens=N, features=feats, eos_token_id=EOS)
    assert greedy["score"] is None and len(greedy["ids"]) >= 1


def test_qa_runner_with_beams_equals_the_one_question_wrapper(ctx, tmp_path):
    """--beams 3 through the QA runner's group schedule (one tower pass, one prefill of the group, 3 x 3 decode slots): every prediction is what
    video_chatgpt_infer_beams gives for that clip alone."""
    import json
    from helpers import SynthTokenizer
    from test_gpu_runners import _tiny_components
    from video_llava_amd.eval import run_inference_qa_activitynet as qa
    from video_llava_amd.inference import video_chatgpt_infer_beams
    ccfg, lcfg, cw, lw, tower, model, ip, V = _tiny_components()
    vd = tmp_path / "v"
    vd.mkdir()
    names = ["b1", "b2", "b3"]
    frames = {n: synth.make_frames(5 + i, ccfg.image, seed=70 + i) for i, n in enumerate(names)}
    for n in names:
        np.save(vd / f"v_{n}.npy", frames[n])
    qs = [{"video_name": n, "question": f"what happens {i}?", "question_id": f"{n}_q"} for i, n in enumerate(names)]
    (tmp_path / "q.json").write_text(json.dumps(qs))
    (tmp_path / "a.json").write_text(json.dumps([{"answer": "a"}] * 3))
    tok = SynthTokenizer(lcfg.vocab)
    args = qa.parse_args(["--video_dir", str(vd), "--gt_file_question", str(tmp_path / "q.json"), "--gt_file_answers", str(tmp_path / "a.json"),
                          "--output_dir", str(tmp_path / "out"), "--output_name", "p", "--model-name", "x", "--projection_path", "y",
                          "--conv-mode", "pg-video-llava", "--batch", "3", "--max_new_tokens", "8", "--beams", "3", "--length_penalty", "0.5"])
    out = qa.run_inference(args, components=(model, tower, tok, ip, V))
    assert [o["id"] for o in out] == ["b1_q", "b2_q", "b3_q"]
    greedy = []
    for o, n in zip(out, names):
        ref = video_chatgpt_infer_beams(frames[n], o["question"], "pg-video-llava", model, tower, tok, ip, V, 3, length_penalty=0.5, max_new_tokens=8)
        assert o["pred"] == ref["text"] and len(ref["ids"]) == 8, (n, o["pred"], ref)
        greedy.append(video_chatgpt_infer_beams(frames[n], o["question"], "pg-video-llava", model, tower, tok, ip, V, 1, max_new_tokens=8)["text"])
    print("beam answers", [o["pred"] for o in out], "greedy answers", greedy)
