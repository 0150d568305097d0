"""GPU: constrained decoding by a token automaton on the device (csrc/logit_allow.hip), from the kernel (pgv_allow_logits) and the per-slot state
record (pgv_kv_allow_peek) up to model.generate(allowed=) / generate_continuous(allowed=).

Yardstick: video_llava_amd.allowed.allowed_ids / apply_allowed -- the rule in Python, itself held to the installed HF processor and to HF's
generate(prefix_allowed_tokens_fn=) by tests/test_allowed_cpu.py -- applied on the CPU to the stepped device logits (replay_logits).  A mask is a set
of indices: every comparison of sets, states and greedy tokens is exact.  Float comparisons: log-probabilities against values recomputed on the host
from the same device logits with the bound of tests/test_gpu_gen_logprobs.py (row_tol: 5e-5 + 2^-21 * max |finite score| of the row); sampled
tokens wherever the uniform lies farther than 1e-5 from a step of the host's fp64 CDF; guided rows (fp64 rule on the host against the fp32 kernel)
wherever the top-1 / top-2 gap among the allowed tokens exceeds 1e-3, as tests/test_gpu_guidance.py does.
"""
import types

import numpy as np
import pytest
import torch

from oracle import synth
from test_gpu_gen_logprobs import assert_within, bits, lsm_at, new_ids_of, replay_logits, row_tol
from test_gpu_warpers import band, cdf_of
from test_gpu_warpers import hf_chain as warp_chain
from video_llava_amd.allowed import DEAD, Allowed, TokenAutomaton, allowed_ids, apply_allowed, check_allowed, state_allowed_ids

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = float("-inf")


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


def _automata(cfg, seed=0, eos=2):
    """Over 40 distinct ordinary tokens: a trie of 4 choices with shared prefixes, a trie with nested prefixes (inner accepting states), `one or more
    digits` (a cycle that accepts) and a cycle that never accepts (the budget ends the answer)."""
    t = [int(x) for x in np.random.default_rng(seed).choice(np.arange(3, cfg.vocab - 3), 40, replace=False) if int(x) != eos]
    digits = t[12:22]
    return types.SimpleNamespace(
        trie=TokenAutomaton.from_sequences([[t[0], t[1], t[2]], [t[0], t[1], t[3]], [t[0], t[4]], [t[5], t[6]]]),
        nest=TokenAutomaton.from_sequences([[t[7]], [t[7], t[8]], [t[7], t[8], t[9]], [t[10], t[11], t[22], t[23], t[24]]]),
        cyc=TokenAutomaton.from_edges(2, [(s, d, 1) for s in (0, 1) for d in digits], [1]),
        loop=TokenAutomaton.from_edges(2, [(s, d, 1) for s in (0, 1) for d in digits], []), digits=digits)


# ---- 1. the kernel against the rule ----------------------------------------------------------------------------------------------------------------
def _kernel_case(V, rng):
    """An automaton with a state of 1 edge (0), a wide one (1: more than one stride of the 1024-thread workgroup where the vocabulary has room), an
    accepting inner state (2), an accepting terminal state (3) and a terminal state that does not accept (4); rows also sit in DEAD and in a state
    index outside the automaton, which is DEAD.  Logits carry -inf and NaN entries."""
    wide = int(min(V, 3000 if V > 3000 else max(1, (3 * V) // 4)))
    edges = [(0, int(rng.integers(0, V)), 1)]
    edges += [(1, int(tk), int(rng.integers(0, 5))) for tk in rng.choice(V, wide, replace=False)]
    edges += [(2, int(tk), 3 + i) for i, tk in enumerate(rng.choice(V, min(2, V), replace=False))]
    a = TokenAutomaton.from_edges(5, edges, [2, 3])
    kinds = [0, 1, 2, 3, 4, DEAD, a.n_states + 3]
    return a, kinds, wide


def _logits(B, V, rng):
    logits = torch.from_numpy(rng.standard_normal((B, V)).astype(np.float32) * 3)
    flat = logits.view(-1)
    k = max(1, flat.numel() // 20)
    flat[torch.from_numpy(rng.integers(0, flat.numel(), k))] = NEG
    flat[torch.from_numpy(rng.integers(0, flat.numel(), k))] = float("nan")
    return logits


def _run_kernel(ctx, a, eos, logits, states):
    dev = logits.to(DEV).contiguous()
    ctx.allow_logits(dev, torch.tensor(states, dtype=torch.int32, device=DEV), a, eos)
    return dev.cpu()


@pytest.mark.parametrize("V,B", [(32003, 8), (515, 17), (50, 2), (2, 1)])
def test_kernel_equals_the_rule(ctx, V, B):
    rng = np.random.default_rng(V * 3 + B)
    a, kinds, wide = _kernel_case(V, rng)
    assert wide > 1024 or V < 32003
    sizes = set()
    for shift in range(len(kinds)):                     # every row position meets every kind of state
        eos = int(rng.integers(0, V))
        states = [kinds[(b + shift) % len(kinds)] for b in range(B)]
        logits = _logits(B, V, rng)
        got = _run_kernel(ctx, a, eos, logits, states)
        for b in range(B):
            want = state_allowed_ids(a, states[b] if 0 <= states[b] < a.n_states else DEAD, eos)
            mask = torch.zeros(V, dtype=torch.bool)
            mask[sorted(want)] = True
            sizes.add(len(want))
            assert torch.equal(bits(got[b][mask]), bits(logits[b][mask])), (shift, b, states[b], "an entry inside the set changed")
            assert bool((got[b][~mask] == NEG).all()), (shift, b, states[b], "an entry outside the set is not -inf")
    print(f"V={V} B={B}: allowed-set sizes {sorted(sizes)}")
    assert 1 in sizes and max(sizes) >= min(V, wide)    # {eos} alone and the wide state were both compared


@pytest.mark.parametrize("V,B", [(32003, 8), (40003, 3), (515, 17), (50, 2)])
def test_kernel_copy_branch_equals_the_rule(ctx, V, B):
    """The launch a pick on a cache makes is out of place (the raw row in, the pick's copy out): pgv_allow_logits_copy, bit for bit against the rule
    at LLaMA's vocabulary (all 32 register slots of a thread, the clamped last load) and beyond 32 x 1024 entries (the tail loop).  The source
    stays as it is."""
    rng = np.random.default_rng(V * 5 + B)
    a, kinds, wide = _kernel_case(V, rng)
    for shift in range(len(kinds)):
        eos = int(rng.integers(0, V)) if shift else V - 1          # once the very last entry of the row
        states = [kinds[(b + shift) % len(kinds)] for b in range(B)]
        logits = _logits(B, V, rng)
        src = logits.to(DEV).contiguous()
        out = torch.full_like(src, 123.0)
        ctx.allow_logits(src, torch.tensor(states, dtype=torch.int32, device=DEV), a, eos, out=out)
        assert torch.equal(bits(src), bits(logits)), (shift, "the source row changed")
        got = out.cpu()
        for b in range(B):
            want = state_allowed_ids(a, states[b] if 0 <= states[b] < a.n_states else DEAD, eos)
            mask = torch.zeros(V, dtype=torch.bool)
            mask[sorted(want)] = True
            assert torch.equal(bits(got[b][mask]), bits(logits[b][mask])), (shift, b, states[b], "an entry inside the set is not the source's")
            assert bool((got[b][~mask] == NEG).all()), (shift, b, states[b], "an entry outside the set is not -inf")
        # the same bytes as the in-place form
        assert torch.equal(bits(got), bits(_run_kernel(ctx, a, eos, logits, states))), shift
    big = torch.zeros(B * V + 1, dtype=torch.float32, device=DEV)          # source and destination one float apart in one allocation: refused
    with pytest.raises(ValueError, match="overlap"):
        ctx.allow_logits(big[:B * V].view(B, V), torch.tensor(states, dtype=torch.int32, device=DEV), a, eos, out=big[1:].view(B, V))
    assert float(big.abs().sum()) == 0.0


def test_kernel_rows_do_not_depend_on_the_batch(ctx):
    """The same inputs through one 64-row call and as 64 one-row calls give the same bytes."""
    V, B = 515, 64
    rng = np.random.default_rng(64)
    a, kinds, _ = _kernel_case(V, rng)
    states = [kinds[b % len(kinds)] for b in range(B)]
    logits = _logits(B, V, rng)
    whole = _run_kernel(ctx, a, 7, logits, states)
    for b in range(B):
        one = _run_kernel(ctx, a, 7, logits[b:b + 1], states[b:b + 1])
        assert torch.equal(bits(one[0]), bits(whole[b])), b


def test_kernel_refuses_a_malformed_automaton_with_the_value(ctx):
    V = 50
    good = TokenAutomaton.from_sequences([[5, 6], [7]])
    raw = lambda **kw: types.SimpleNamespace(**dict(dict(row_ptr=good.row_ptr, edge_token=good.edge_token, edge_next=good.edge_next, accept=good.accept,        # noqa: E731
                                                        n_states=good.n_states, n_edges=good.n_edges), **kw))
    logits, states = torch.zeros(1, V, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for a, eos, word in ((good, -1, "eos_id -1 outside"), (good, V, "eos_id 50 outside"),
                         (raw(edge_token=np.array([5, 77, 6], dtype=np.int32)), 2, "edge token 77 of state 0 outside"),
                         (raw(edge_token=np.array([7, 5, 6], dtype=np.int32)), 2, "not sorted and distinct"),
                         (raw(edge_next=np.array([1, 9, 2], dtype=np.int32)), 2, "edge target 9 of state 0 outside the 4 states"),
                         (raw(row_ptr=np.array([0, 2, 1, 3, 3], dtype=np.int32)), 2, "row_ptr of state 1"),
                         (raw(n_states=(1 << 20) + 1), 2, "1048577 states outside")):
        with pytest.raises(ValueError, match=word):
            ctx.allow_logits(logits, states, a, eos)
    assert float(logits.abs().sum()) == 0.0


# ---- 2. the state record ---------------------------------------------------------------------------------------------------------------------------
def test_state_record_follows_every_call(ctx):
    """A constrained greedy run of B = 3 ragged prompts stepped through the kv calls, each prompt with its own automaton: after every step
    pgv_kv_allow_peek equals the numpy walk of the tokens the steps consumed; a re-pick stores nothing; after pgv_kv_truncate the run continues
    from the state behind the kept ids; pgv_kv_fork destinations carry the source's states and root."""
    cfg, m = _tiny()
    eos = 2
    A = _automata(cfg)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(6), 20, (2, 11, 0))
    al = check_allowed([A.nest, A.loop, A.cyc], 3, cfg.vocab, eos)
    auto, roots = al.automaton, list(al.roots)
    kv, _nxt, _ = m.prefill(prompts, feats_t, 128, capacity=6, allowed=al, eos_id=eos)
    try:
        P = [len(p) for p in prompts]
        gen = [[] for _ in prompts]                    # the tokens the steps consumed, per slot

        def check(what):
            for s, g in enumerate(gen):
                assert m.kv_len(kv, s) == P[s] + len(g), (what, s)
                got, root = m.allow_peek(kv, s, P[s] + len(g))
                want = [auto.walk(roots[s], g[:i + 1]) for i in range(len(g))]
                assert root == roots[s] and got[P[s]:] == want, (what, s, root, roots[s], got[P[s]:], want)

        def allowed_now(s):
            return allowed_ids(auto, roots[s], gen[s], eos)

        before = [m.allow_peek(kv, s, 128) for s in range(3)]
        cur = m.greedy_last(kv, 3)                      # the first pick, on the prefill's logits: reads the root
        again = m.greedy_last(kv, 3)                    # a re-pick
        assert torch.equal(cur, again) and [m.allow_peek(kv, s, 128) for s in range(3)] == before, "a pick that advances nothing stored a state"
        for b in range(3):
            assert int(cur[b]) in allowed_now(b), (b, int(cur[b]))
        for step in range(6):                           # one step per call: peek after each
            toks = m.decode_greedy(kv, cur, 1)
            for b in range(3):
                gen[b].append(int(cur[b]))
                assert int(toks[b, 0]) in allowed_now(b), (step, b, int(toks[b, 0]), sorted(allowed_now(b)))
            cur = toks[:, 0].contiguous()
            check(f"step {step}")
        assert auto.walk(roots[0], gen[0]) == DEAD and auto.walk(roots[1], gen[1]) == roots[1] + 1      # slot 0 answered and ended (DEAD behind EOS), slot 1 still cycles
        # truncate slot 1 to a shorter answer and continue on another branch: the state behind the kept ids is where the walk goes on
        gen[1] = gen[1][:2]
        m.kv_truncate(kv, 1, P[1] + 2)
        other = next(d for d in A.digits if d != gen[1][-1])
        cur = cur.clone()
        cur[1] = other
        toks = m.decode_greedy(kv, cur, 2)
        for b in range(3):
            gen[b] += [int(cur[b]), int(toks[b, 0])]
        cur = toks[:, 1].contiguous()
        check("truncate + 2 steps")
        assert gen[1][2] == other and auto.walk(roots[1], gen[1]) == al.roots[1] + 1
        # fork: the destinations carry the source's states and root
        m.fork(kv, [2, 1, 3])
        src = [0, 0, 1, 2, 2, 2]
        P, gen, roots = [P[i] for i in src], [list(gen[i]) for i in src], [roots[i] for i in src]
        cur = cur[torch.tensor(src, device=DEV)].contiguous()
        check("fork")
        toks = m.decode_greedy(kv, cur, 2)
        for s in range(6):
            gen[s] += [int(cur[s]), int(toks[s, 0])]
            assert int(toks[s, 1]) in allowed_now(s), s
        check("2 steps after the fork")
    finally:
        m.set_allowed(kv, None)


def _big():
    """One decoder layer of the tiny width under a vocabulary beyond 32 x 1024: the pick's copy of a row then uses every register slot of
    logit_allow_kernel's threads and its tail loop, and a state can be wider than one stride of the workgroup."""
    from helpers import make_model
    cfg = synth.LlamaCfg(vocab=40003, hidden=512, inter=768, layers=1, heads=4)
    return cfg, make_model(cfg, synth.make_llama_weights(cfg, seed=5, head_std=0.08), torch.float16)


def _wide_automaton(cfg, n=2500, seed=1):
    """Three states with the same n sorted edges each; edge j of state s leads to state (j + s) % 3, so the walk tells WHICH edge a lookup found.
    n = 2500 is 2 x 1024 + 452: the first level of the lookup gives every thread a run of 3 edges, 833 full runs and a last one of 1 edge.  No state
    accepts: the budget ends an answer."""
    toks = np.sort(np.random.default_rng(seed).choice(np.arange(3, cfg.vocab - 3), n, replace=False)).astype(np.int32)
    assert toks[-1] > 32768 and n % 3 != 0
    j = np.arange(n, dtype=np.int32)
    a = TokenAutomaton(np.arange(4, dtype=np.int32) * n, np.tile(toks, 3), np.concatenate([(j + s_) % 3 for s_ in range(3)]), np.zeros(3, dtype=np.uint8))
    return a, toks


def test_wide_state_lookup_on_a_large_vocabulary(ctx):
    """States of 2500 edges (the two-level lookup) on a vocabulary of 40003, stepped through the kv calls with the consumed tokens forced: the
    first, the middle and the last edge of a run, the last edge of a full run, the last edge of the state (a run of one), a token that lies between
    two edges (no edge: DEAD, and DEAD stays).  After every step pgv_kv_allow_peek equals the numpy walk and the token the step picked is allowed.
    Then generate(allowed=) on the same model equals the rule replayed on the stepped logits, token for token, and its `pick` log-probability is
    the log-softmax over the survivors: the production launch of the copy branch at this size.  Last, pgv_llm_prefill_append: the next answer
    starts at the root again."""
    cfg, m = _big()
    eos = 2
    auto, toks = _wide_automaton(cfg)
    n = len(toks)
    gap = next(int(toks[k]) + 1 for k in range(1, n - 1) if toks[k + 1] - toks[k] > 1)          # inside the range of a run, on no edge
    assert gap not in set(toks.tolist())
    rng = np.random.default_rng(12)
    prompts = [[1] + rng.integers(3, cfg.vocab - 3, k).tolist() for k in (5, 9, 7)]
    roots = [0, 1, 2]
    script = [[0, 2, 3, n - 1, n - 2, 1], [n - 2, n - 4, n - 1, 0, 5, n - 3], [n // 2, n - 1, 2, None, 0, 0]]       # edge indices; None: `gap`
    kv, _nxt, _ = m.prefill(prompts, None, 64, allowed=Allowed(auto, roots), eos_id=eos)
    try:
        P = [len(p) for p in prompts]
        gen = [[] for _ in prompts]

        def check(what):
            for s_, g in enumerate(gen):
                got, root = m.allow_peek(kv, s_, P[s_] + len(g))
                want = [auto.walk(roots[s_], g[:i + 1]) for i in range(len(g))]
                assert root == roots[s_] and got[P[s_]:] == want, (what, s_, got[P[s_]:], want)

        first = m.greedy_last(kv, 3)
        for b in range(3):
            assert int(first[b]) in allowed_ids(auto, roots[b], [], eos), b
        for step in range(6):
            forced = [gap if script[b][step] is None else int(toks[script[b][step]]) for b in range(3)]
            out = m.decode_greedy(kv, torch.tensor(forced, dtype=torch.int32, device=DEV), 1)
            for b in range(3):
                gen[b].append(forced[b])
                assert int(out[b, 0]) in allowed_ids(auto, roots[b], gen[b], eos), (step, b, int(out[b, 0]))
            check(f"step {step}")
        assert auto.walk(roots[2], gen[2]) == DEAD and all(auto.walk(roots[b], gen[b]) >= 0 for b in (0, 1))
        # an appended turn: the prompt length moves behind it and the next answer starts at the root again, the DEAD slot included
        more = [rng.integers(3, cfg.vocab - 3, k).tolist() for k in (4, 1, 6)]
        _kv, _n, _ = m.prefill(more, None, 0, append_to=kv)
        P = [P[b] + len(gen[b]) + len(more[b]) for b in range(3)]
        gen = [[] for _ in prompts]
        cur = m.greedy_last(kv, 3)
        for b in range(3):
            assert m.kv_len(kv, b) == P[b] and int(cur[b]) in set(toks.tolist()), (b, int(cur[b]))
        out = m.decode_greedy(kv, cur, 1)
        for b in range(3):
            gen[b].append(int(cur[b]))
            assert int(out[b, 0]) in allowed_ids(auto, roots[b], gen[b], eos), b
        check("append + 1 step")
    finally:
        m.set_allowed(kv, None)
    # generate(): token-exact against the rule on the replayed logits, and the pick's log-probability over the survivors
    N = 8
    al = Allowed(auto, roots)
    kw = dict(max_new_tokens=N, eos_token_id=eos, allowed=al)
    res = m.generate(prompts, output_logprobs=True, chunk=3, **kw)
    assert torch.equal(m.generate(prompts, **kw), res.sequences)
    exact, total = _verify(m, prompts, None, res.sequences, al, N, eos)
    assert exact == total == 3 * N
    new = _new(res.sequences, prompts, N, eos)
    steps = replay_logits(m, prompts, None, new)
    for i in range(N):
        for b in range(3):
            x = apply_allowed(auto, roots[b], steps[i][b], new[b][:i], eos)[None]
            assert int(torch.isfinite(x).sum()) == n
            assert_within(res.transition_scores[b, i], lsm_at(x, torch.tensor([new[b][i]])), row_tol(x), f"pick step {i} seq {b}")


# ---- 3. generate(allowed=) against the rule -------------------------------------------------------------------------------------------------------
def _is_path(al, b, new, eos, n):
    """The answer is a path of its automaton that ends in an accepting state (then EOS), or is cut by the budget."""
    body = new[:new.index(eos)] if eos in new else new
    state = al.automaton.walk(al.roots[b], body)
    return state != DEAD and (bool(al.automaton.accept[state]) if eos in new else len(new) == n)


def _new(out, prompts, n, eos):
    """The new ids of every row, padded with EOS to n: generate() cuts its result where the longest answer ends."""
    return [row + [eos] * (n - len(row)) for row in new_ids_of(out, prompts, n)]


def _verify(m, prompts, feats_t, out, al, n, eos, sampled=None, bans=None):
    """Replay the rule on the stepped device logits.  Greedy: the first-index arg-max of the masked fp32 row, exactly.  sampled = (temperature,
    top_k, top_p, u [n, B]): the inverse-CDF pick of the masked row under HF's warpers, wherever the host can tell.  -> (steps checked exactly, live steps)."""
    B = len(prompts)
    new = _new(out, prompts, n, eos)
    steps = replay_logits(m, prompts, feats_t, new)
    live, exact, total = [True] * B, 0, 0
    for i in range(n):
        for b in range(B):
            if not live[b]:
                assert new[b][i] == eos, (i, b, "a finished row went on")
                continue
            g = new[b][:i]
            ok = allowed_ids(al.automaton, al.roots[b], g, eos)
            x = apply_allowed(al.automaton, al.roots[b], steps[i][b], g, eos)
            if bans is not None:
                from bans_hf import hf_scores
                x = hf_scores(bans, prompts[b] + g, len(prompts[b]), eos, x)           # the union of both -inf sets
            assert new[b][i] in ok and float(x[new[b][i]]) > NEG, (i, b, new[b][i], sorted(ok)[:12])
            total += 1
            if sampled is None:
                assert new[b][i] == int(torch.argmax(x)), (i, b, new[b][i], int(torch.argmax(x)))
                exact += 1
            else:
                temp, top_k, top_p, u = sampled
                x2, y = warp_chain(x[None], torch.tensor([prompts[b] + g]), temp, top_k, top_p, 1.0)
                n_lo, n_hi, _ = band(x2, top_p)
                cdf = cdf_of(y)[0]
                want = int((cdf <= u[i, b].double()).sum().clamp_max(x.numel() - 1))
                if int(n_lo) == int(n_hi) and float((cdf - u[i, b].double()).abs().min()) > 1e-5:
                    assert new[b][i] == want, (i, b, new[b][i], want)
                    exact += 1
            live[b] = new[b][i] != eos
    for b in range(B):
        assert _is_path(al, b, new[b], eos, n), (b, new[b])
        assert out[b, :len(prompts[b])].tolist() == prompts[b]
    return exact, total


@pytest.mark.parametrize("B", [1, 3, 8])
def test_greedy_run_equals_the_rule(ctx, B):
    """One automaton for all prompts and one per prompt; chunks 1 / 5 / 32 give the same ids; a cycle that never accepts runs up to max_new_tokens."""
    cfg, m = _tiny(seed=8)
    eos, n = 2, 12
    A = _automata(cfg)
    rng = np.random.default_rng(40 + B)
    prompts, feats_t = _prompts(cfg, rng, 20, [int(x) for x in rng.integers(0, 30, B)])
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=eos)
    free = _new(m.generate(prompts, **kw), prompts, n, eos)
    per_prompt = [(A.trie, A.cyc, A.nest, A.loop)[b % 4] for b in range(B)]
    for allowed in (A.nest, A.loop, per_prompt):
        al = check_allowed(allowed, B, cfg.vocab, eos)
        out = m.generate(prompts, allowed=allowed, chunk=32, **kw)
        for chunk in (1, 5):
            assert torch.equal(m.generate(prompts, allowed=allowed, chunk=chunk, **kw), out), chunk
        exact, total = _verify(m, prompts, feats_t, out, al, n, eos)
        new = _new(out, prompts, n, eos)
        assert exact == total and all(new[b] != free[b] for b in range(B)), "the constraint did not change the answers"
        if allowed is A.loop:
            assert all(eos not in row and len(row) == n for row in new)       # cut by the budget


def test_sampled_run_equals_the_rule(ctx):
    """Sampled, with the call's own uniforms: the same generator state draws torch.rand(n, B).  Also samples_per_prompt = 3: the prompts repeated,
    every sample from its prompt's root."""
    cfg, m = _tiny()
    eos, n, temp, top_k, top_p = 2, 12, 0.9, 50, 0.9
    A = _automata(cfg)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(2), 20, (3, 40, 0))
    gen = torch.Generator(device=DEV).manual_seed(11)
    kw = dict(video_spatio_temporal_features=feats_t, do_sample=True, temperature=temp, top_k=top_k, top_p=top_p, max_new_tokens=n, generator=gen,
              eos_token_id=eos)
    exact = total = 0
    for allowed, samples in (([A.cyc, A.nest, A.cyc], 1), (A.cyc, 1), ([A.cyc, A.trie, A.nest], 3)):
        al = check_allowed(allowed, 3, cfg.vocab, eos)
        extra = {"samples_per_prompt": samples} if samples > 1 else {}
        gen.manual_seed(11)
        out = m.generate(prompts, allowed=allowed, chunk=32, **extra, **kw)
        gen.manual_seed(11)
        assert torch.equal(m.generate(prompts, allowed=allowed, chunk=5, **extra, **kw), out)
        gen.manual_seed(11)
        u = torch.rand(n, 3 * samples, device=DEV, generator=gen).cpu()
        rep = [p for p in prompts for _ in range(samples)]
        wide = Allowed(al.automaton, [r for r in al.roots for _ in range(samples)])          # roots follow fork_sources
        assert out.shape[0] == 3 * samples
        e, t = _verify(m, rep, feats_t.repeat_interleave(samples, 0), out, wide, n, eos, sampled=(temp, top_k, top_p, u))
        exact, total = exact + e, total + t
        if samples > 1:
            new = _new(out, rep, n, eos)
            assert len({tuple(r) for r in new[:3]}) > 1 or len({tuple(r) for r in new[6:]}) > 1, "the samples of a prompt are all the same"
    print(f"sampled: {exact} of {total} live draws farther than 1e-5 from a CDF step")
    assert exact >= 0.9 * total, (exact, total)


def test_together_with_bans_is_the_union(ctx):
    """no_repeat_ngram = 2 on the cyclic automaton: every pick is allowed by the automaton AND survives the ban; greedy and sampled."""
    from video_llava_amd.logit_bans import LogitBans
    cfg, m = _tiny(seed=8)
    eos, n = 2, 12
    A = _automata(cfg)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(4), 20, (2, 17, 6))
    raw = LogitBans(no_repeat_ngram=2, min_new_tokens=4)
    al = check_allowed(A.cyc, 3, cfg.vocab, eos)
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=eos)
    only = m.generate(prompts, allowed=A.cyc, **kw)
    out = m.generate(prompts, allowed=A.cyc, bans=raw, chunk=5, **kw)
    assert not torch.equal(out, only), "the bans did not change the constrained answers"
    exact, total = _verify(m, prompts, feats_t, out, al, n, eos, bans=raw.check(cfg.vocab, eos))
    assert exact == total
    for b, row in enumerate(_new(out, prompts, n, eos)):
        body = row[:row.index(eos)] if eos in row else row
        assert len(body) >= 4 and len(set(zip(body, body[1:]))) == len(body) - 1, (b, row)          # min_new_tokens; no bigram of the answer repeats
    gen = torch.Generator(device=DEV).manual_seed(5)
    skw = dict(kw, do_sample=True, temperature=0.9, top_k=50, top_p=0.9, generator=gen)      # (band() decides a nucleus boundary: top_p < 1)
    s = m.generate(prompts, allowed=A.cyc, bans=raw, **skw)
    gen.manual_seed(5)
    u = torch.rand(n, 3, device=DEV, generator=gen).cpu()
    exact, total = _verify(m, prompts, feats_t, s, al, n, eos, sampled=(0.9, 50, 0.9, u), bans=raw.check(cfg.vocab, eos))
    assert exact >= 0.9 * total, (exact, total)


def test_together_with_guidance(ctx):
    """The mask is applied to the GUIDED row with the conditional slot's state: every token is allowed, and it is the arg-max of the fp64 guided
    scores among the allowed tokens wherever their top-1 / top-2 gap exceeds 1e-3."""
    from test_gpu_guidance import _model, _negatives, _replay
    from test_gpu_guidance import _prompts as g_prompts
    from video_llava_amd.guidance import Guidance, guided_scores
    cfg, m = _model(4.0)
    eos, n, B, scale = 2, 10, 3, 1.5
    A = _automata(cfg)
    prompts, feats_t = g_prompts(cfg, 2, (3, 40, 0))
    neg_arg, negs = _negatives(cfg, prompts, "no_video")
    allowed = [A.cyc, A.nest, A.loop]
    al = check_allowed(allowed, B, cfg.vocab, eos)
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=eos, guidance=Guidance(scale, neg_arg))
    out = m.generate(prompts, allowed=allowed, chunk=4, **kw)
    assert torch.equal(m.generate(prompts, allowed=allowed, chunk=32, **kw), out)
    new = _new(out, prompts, n, eos)
    close = total = 0
    live = [True] * B
    for i, (cond, uncond) in enumerate(_replay(m, cfg, prompts, negs, feats_t, new, n)):
        ref = guided_scores(cond.numpy(), uncond.numpy(), scale)
        for b in range(B):
            if not live[b]:
                assert new[b][i] == eos
                continue
            ok = sorted(allowed_ids(al.automaton, al.roots[b], new[b][:i], eos))
            assert new[b][i] in ok, (i, b, new[b][i], ok)
            x = apply_allowed(al.automaton, al.roots[b], ref[b], new[b][:i], eos)
            top = np.sort(x[ok])[-2:]
            total += 1
            if len(ok) == 1 or top[1] - top[0] > 1e-3:
                assert new[b][i] == int(np.argmax(x)), (i, b, new[b][i], int(np.argmax(x)))
            else:
                close += 1
            live[b] = new[b][i] != eos
    print(f"guided: {close} of {total} live steps with an fp64 top-1 / top-2 gap below 1e-3 among the allowed tokens")
    assert close <= 0.1 * total and all(_is_path(al, b, new[b], eos, n) for b in range(B)), (close, total, new)


def test_logprobs_under_an_automaton(ctx):
    """token_logprobs stay the raw log-softmax, transition_scores are the log-softmax over the survivors; the ids are those of the call without the
    keyword."""
    cfg, m = _tiny(seed=8)
    eos, n, B = 2, 12, 3
    A = _automata(cfg)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(4), 20, (2, 17, 6))
    allowed = [A.cyc, A.nest, A.loop]
    al = check_allowed(allowed, B, cfg.vocab, eos)
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=eos, allowed=allowed)
    ids = m.generate(prompts, **kw)
    a = m.generate(prompts, output_logprobs=True, chunk=5, **kw)
    assert torch.equal(a.sequences, ids)
    new = _new(ids, prompts, n, eos)
    steps = replay_logits(m, prompts, feats_t, new)
    differ = 0
    for b in range(B):
        k = int(a.new_lengths[b])
        assert 1 <= k <= n
        for i in range(k):
            tok = torch.tensor([new[b][i]])
            raw = steps[i][b][None]
            assert_within(a.token_logprobs[b, i], lsm_at(raw, tok), row_tol(raw), f"model step {i} seq {b}")
            x = apply_allowed(al.automaton, al.roots[b], steps[i][b], new[b][:i], eos)[None]
            assert_within(a.transition_scores[b, i], lsm_at(x, tok), row_tol(x), f"pick step {i} seq {b}")
            differ += abs(float(a.transition_scores[b, i]) - float(a.token_logprobs[b, i])) > 2 * float(row_tol(x))
    assert differ >= 1


# ---- 4. the refill runner -------------------------------------------------------------------------------------------------------------------------
def test_generate_continuous_equals_every_task_alone(ctx):
    """6 tasks over 2 slots, ONE automaton: every answer equals the same task run alone, greedy and sampled-free (the refilled slots start at root 0)."""
    from video_llava_amd.continuous import Task, generate_continuous
    cfg, m = _tiny(seed=8)
    eos, n = 2, 10
    A = _automata(cfg)
    rng = np.random.default_rng(9)
    prompts, feats_t = _prompts(cfg, rng, 20, [int(x) for x in rng.integers(0, 30, 6)])
    lengths = set()
    for allowed in (A.nest, A.cyc):
        al = check_allowed(allowed, 1, cfg.vocab, eos)
        alone = {}
        for i, p in enumerate(prompts):
            row = m.generate([p], video_spatio_temporal_features=feats_t[i:i + 1], max_new_tokens=n, eos_token_id=eos, allowed=allowed)[0, len(p):].tolist()
            assert _is_path(al, 0, row, eos, n), (i, row)
            alone[i] = row
            lengths.add(len(row))
        tasks = [Task(i, prompts[i], feats_t[i].to(DEV), max_new_tokens=n) for i in range(6)]
        got = dict(generate_continuous(m, iter(tasks), 2, n, refill_min=1, chunk=3, eos_token_id=eos, allowed=allowed))
        assert got == alone, (got, alone)
    assert len(lengths) > 1                             # answers of different lengths: slots were refilled at different times


# ---- 5. off is off ----------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(ctx):
    from video_llava_amd.logit_bans import LogitBans
    cfg, m = _tiny(seed=8)
    eos = 2
    A = _automata(cfg)
    prompts, feats_t = _prompts(cfg, np.random.default_rng(4), 20, (2, 17, 6))
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=16, eos_token_id=eos)
    raw = LogitBans(no_repeat_ngram=2, min_new_tokens=6)
    plain = m.generate(prompts, output_logprobs=True, **kw)
    banned = m.generate(prompts, bans=raw, **kw)            # bans only, before the new code path has run on this cache
    got = m.generate(prompts, output_logprobs=True, allowed=None, **kw)
    assert torch.equal(got.sequences, plain.sequences)
    assert torch.equal(bits(got.token_logprobs), bits(plain.token_logprobs)) and torch.equal(bits(got.transition_scores), bits(plain.transition_scores))
    gen = torch.Generator(device=DEV).manual_seed(2)
    skw = dict(kw, do_sample=True, temperature=0.9, generator=gen)
    s_plain = m.generate(prompts, **skw)
    gen.manual_seed(2)
    assert torch.equal(m.generate(prompts, allowed=None, **skw), s_plain)
    # a constrained call, alone and together with the bans; then calls without the keyword: the cache's automaton was cleared
    constrained = m.generate(prompts, allowed=A.cyc, **kw)
    assert not torch.equal(constrained, plain.sequences)
    m.generate(prompts, allowed=A.cyc, bans=raw, **kw)
    assert torch.equal(m.generate(prompts, **kw), plain.sequences)
    gen.manual_seed(2)
    assert torch.equal(m.generate(prompts, **skw), s_plain)
    assert torch.equal(m.generate(prompts, bans=raw, **kw), banned), "bans-only output changed after the automaton had been used on the cache"
    # ... and through the kv calls: a run after set_allowed(None)
    kv, nxt, _ = m.prefill(prompts, feats_t, 128)
    base = m.decode_greedy(kv, nxt, 8, eos)
    kv, _n, _ = m.prefill(prompts, feats_t, 128, allowed=check_allowed(A.cyc, 3, cfg.vocab, eos), eos_id=eos)
    m.set_allowed(kv, None)
    kv, nxt2, _ = m.prefill(prompts, feats_t, 128)
    assert torch.equal(nxt2, nxt) and torch.equal(m.decode_greedy(kv, nxt2, 8, eos), base)


def test_library_refusals(ctx):
    cfg, m = _tiny()
    A = _automata(cfg)
    ids = [1, 17, 230, 9, 44]
    with pytest.raises(ValueError, match="`allowed` cannot be combined with `beams`=2"):
        m.generate([ids], max_new_tokens=4, eos_token_id=2, beams=2, allowed=A.trie)
    with pytest.raises(ValueError, match="`allowed` cannot be combined with `lookup`=3"):
        m.generate([ids], max_new_tokens=4, eos_token_id=2, lookup=3, allowed=A.trie)
    kv, _nxt, _ = m.prefill([ids], None, 64, capacity=2, allowed=check_allowed(A.trie, 1, cfg.vocab, 2), eos_id=2)
    try:
        with pytest.raises(Exception, match="a token automaton is set"):
            m.beam_begin(kv, 2, 4)
        with pytest.raises(Exception, match="a token automaton is set"):
            m.set_lookup(kv, 3, 2)
        with pytest.raises(Exception, match="eos_id -1 outside"):
            m.set_allowed(kv, A.trie, [0], -1)
        with pytest.raises(Exception, match="root 99 of sequence 0 outside"):
            m.set_allowed(kv, A.trie, [99], 2)
    finally:
        m.set_allowed(kv, None)
    m.set_lookup(kv, 3, 2)
    try:
        with pytest.raises(Exception, match="pgv_kv_set_lookup is on"):
            m.set_allowed(kv, A.trie, [0], 2)
    finally:
        m.set_lookup(kv, 0)


# ---- 6. one cache through every feature ----------------------------------------------------------------------------------------------------------
def test_one_cache_object_through_every_feature(ctx):
    """ONE cache object (2 prompts, max_seq 128, capacity 4) runs, a first token and 10 decode steps each (on a used cache one 8-step graph and two 1-step graphs) and every feature switched off again behind its run: plain
    greedy; bans; plain greedy; an automaton; automaton + bans; sampled with fixed uniforms; greedy with log-probabilities; guidance with 1 pair (the
    2 slots are a prompt and its negative); lookup D = 3, n = 2; beam K = 2; plain greedy.  Every run's tokens -- and log-probabilities, beam scores
    and lookup counts where there are any -- equal bit for bit the same run on a freshly created cache, and the three plain runs equal each other:
    the decode graphs' key and the per-kind eager-first flags separate every configuration (a stale graph would replay another run's launches)."""
    from video_llava_amd.logit_bans import LogitBans
    cfg, m = _tiny(seed=8)
    eos, n, W = 2, 10, 2
    A = _automata(cfg)
    p0 = [1] + np.random.default_rng(21).integers(3, cfg.vocab - 3, 14).tolist()
    prompts = [p0, p0[-4:]]                                  # the second prompt is the first one's negative: its last tokens without the context
    bans = LogitBans(no_repeat_ngram=2, min_new_tokens=4).check(cfg.vocab, eos)
    al = check_allowed(A.cyc, W, cfg.vocab, eos)
    u = torch.rand(n + 1, W, generator=torch.Generator().manual_seed(7))
    seen = []                                                # the cache handle of every run

    def prefill(**kw):
        kv, nxt, _ = m.prefill(prompts, None, 128, capacity=4, **kw)
        seen.append(kv.value)
        return kv, nxt

    def greedy(kv, nxt, repick):
        if repick:
            nxt = m.greedy_last(kv, W)                       # the prefill's arg-max knows no processor (generate_loop.first_pick)
        return [nxt.cpu(), m.decode_greedy(kv, nxt, n, eos).cpu()]

    def plain():
        return greedy(*prefill(), False)

    def banned():
        kv, nxt = prefill(bans=bans, eos_id=eos)
        try:
            return greedy(kv, nxt, True)
        finally:
            m.set_bans(kv, None)

    def constrained(with_bans):
        kv, nxt = prefill(allowed=al, eos_id=eos, **({"bans": bans} if with_bans else {}))
        try:
            return greedy(kv, nxt, True)
        finally:
            m.set_allowed(kv, None)
            m.set_bans(kv, None)

    def sampled():
        kv, _nxt = prefill()
        first = m.sample_last(kv, u[0], 0.9, 50, top_p=0.9)
        out = [first.cpu(), m.decode_sample(kv, first, n, eos, 0.9, 50, u[1:], top_p=0.9).cpu()]
        m.set_warpers(kv)
        return out

    def logprobs():
        kv, nxt = prefill(logprobs=True)
        try:
            out = [bits(m.logprobs_last(kv, W).cpu())] + greedy(kv, nxt, False)
            return out + [bits(m.logprobs_steps(kv, W, n).cpu())]
        finally:
            m.set_logprobs(kv, False)

    def guided():
        kv, nxt = prefill()
        m.set_guidance(kv, 1.5, 1)
        try:
            return greedy(kv, nxt, True)
        finally:
            m.set_guidance(kv, 1.0, 0)

    def lookup():
        kv, nxt = prefill(lookup=(3, 2))
        try:
            toks, counts = m.decode_lookup(kv, nxt, n, eos, [n] * W)
            return [nxt.cpu(), toks.cpu(), torch.from_numpy(counts)]
        finally:
            m.set_lookup(kv, 0)

    def beam():
        kv, _nxt = prefill()
        m.beam_begin(kv, 2, n + 1, eos)                      # the first pick, then n steps: the budget ends the run
        m.decode_beam(kv, n)
        out = []
        for p in range(W):
            toks, score, fin = m.beam_result(kv, p, 0)
            out += [torch.tensor(toks), bits(torch.tensor([score])), torch.tensor([fin])]
        return out

    runs = [("plain", plain), ("bans", banned), ("plain again", plain), ("automaton", lambda: constrained(False)), ("automaton + bans", lambda: constrained(True)),
            ("sampled", sampled), ("logprobs", logprobs), ("guidance", guided), ("lookup", lookup), ("beam", beam), ("plain last", plain)]

    def fresh_cache():
        for kv in m._kv.values():
            m.ctx.lib.pgv_kv_destroy(kv)
        m._kv.clear()

    want = []
    for _name, run in runs:
        fresh_cache()
        want.append(run())
    fresh_cache()
    seen.clear()
    got = [run() for _name, run in runs]
    assert len(set(seen)) == 1 and len(seen) == len(runs), "the runs did not share one cache object"
    for (name, _run), g, w in zip(runs, got, want):
        assert len(g) == len(w) and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(g, w)), (name, g, w)
    for i in (2, 10):
        assert all(torch.equal(a, b) for a, b in zip(got[0], got[i])), runs[i][0]
    tokens = {name: torch.cat([g[0][:, None], g[1]], 1) for (name, _r), g in zip(runs, got) if name in ("plain", "bans", "automaton", "sampled", "guidance")}
    print({k: not torch.equal(tokens["plain"], v) for k, v in tokens.items()}, "<- which features changed the plain answers")
    assert not torch.equal(tokens["plain"], tokens["automaton"]), "the automaton left the answers as they were: the run pins nothing"
