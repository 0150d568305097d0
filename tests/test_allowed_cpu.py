"""Constrained decoding, host side: the rule of video_llava_amd/allowed.py (allowed_ids -- what the GPU tests hold the kernel to) against the
installed HF PrefixConstrainedLogitsProcessor and HF's own generate(prefix_allowed_tokens_fn=) on tiny CPU llamas; the automaton's constructors,
the host checks of generate(allowed=), the refusal of HF's callback argument, the chunk loop over a scripted backend, the callers' flags and the
decode-graph key.  No GPU."""
import itertools
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from allowed_hf import hf_allowed, hf_scores, prefix_fn
from test_generate_loop_cpu import LoopLM, _gen, _ids, _new
from test_guidance_cpu import hf_models                     # noqa: F401  (the tiny llamas: vocabulary 41, seeds 0 - 7)
from test_runner_core_cpu import EOS as SEOS, V as VROWS
from video_llava_amd import generation as G
from video_llava_amd.allowed import (DEAD, MAX_EDGES, MAX_STATES, Allowed, TokenAutomaton, allowed_ids, apply_allowed, check_allowed,
                                     state_allowed_ids)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, EOS, PAD, MAX_NEW, PROMPT = 41, 2, 40, 7, 5
NEG = float("-inf")
DIGITS = list(range(20, 30))


def trie4():
    """Four choices with shared prefixes."""
    return TokenAutomaton.from_sequences([[5, 6, 7], [5, 6, 8], [5, 9], [11, 12]])


def nested():
    """A choice that is a prefix of another, twice over: inner accepting states."""
    return TokenAutomaton.from_sequences([[14], [14, 15], [14, 15, 16], [17, 18]])


def cyclic():
    """One or more `digits`: state 1 loops on itself and accepts."""
    return TokenAutomaton.from_edges(2, [(s, t, 1) for s in (0, 1) for t in DIGITS], [1])


AUTOMATA = {"trie4": trie4, "nested": nested, "cyclic": cyclic}


# ---- 1. the rule against HF's processor class ----------------------------------------------------------------------------------------------------
def test_rule_equals_hf_processor_class():
    """Random finite scores through PrefixConstrainedLogitsProcessor(fn, 1), fn closing over the automaton: exactly the -inf set of allowed_ids, the
    entries inside the set bit for bit.  Walks: the root, shared prefixes, an inner accepting state, a terminal state, a dead walk, a cycle."""
    rng = np.random.default_rng(0)
    walks = {"trie4": [[], [5], [5, 6], [5, 6, 7], [5, 9], [11], [5, 7], [30], [5, 6, 7, 5], [EOS]],
             "nested": [[], [14], [14, 15], [14, 15, 16], [17], [17, 18], [14, 16], [14, 15, 16, 14]],
             "cyclic": [[], [20], [29, 20, 25], DIGITS * 3, [20, 5], [5], [20, EOS]]}
    seen_kinds = set()
    for name, V in itertools.product(AUTOMATA, (VOCAB, 1000)):
        a = AUTOMATA[name]()
        for gen in walks[name]:
            want = allowed_ids(a, 0, gen, EOS)
            state = a.walk(0, gen)
            assert want == state_allowed_ids(a, state, EOS)
            assert hf_allowed(a, 0, gen, EOS, V) == want, (name, gen)
            scores = torch.from_numpy(rng.standard_normal(V).astype(np.float32) * 4)
            hf = hf_scores(a, 0, gen, EOS, scores)
            ours = apply_allowed(a, 0, scores, gen, EOS)
            assert torch.equal(ours.view(torch.int32), hf.view(torch.int32)), (name, gen)
            assert np.array_equal(apply_allowed(a, 0, scores.numpy(), gen, EOS).view(np.int32), hf.numpy().view(np.int32))
            kind = "dead" if state == DEAD else "terminal" if not a.edges(state) else "inner accept" if a.accept[state] else "open"
            seen_kinds.add(kind)
            assert (want == {EOS}) == (kind in ("dead", "terminal")), (name, gen, want)
            assert (EOS in want) == (kind != "open")
    assert seen_kinds == {"dead", "terminal", "inner accept", "open"}
    # entries inside the set keep their bits, NaN and -inf included; everything outside is -inf, a NaN too (HF's `scores + mask` would leave that NaN)
    x = np.array([0.5, np.nan, NEG, 1.5, np.nan, 2.5], dtype=np.float32)
    a = TokenAutomaton.from_sequences([[1], [2], [3]])
    y = apply_allowed(a, 0, x, [], 0)
    assert np.isnan(y[1]) and y[2] == NEG and y[3] == np.float32(1.5) and y[0] == NEG and y[4] == NEG and y[5] == NEG
    assert x[0] == np.float32(0.5)                                  # a copy


# ---- 2. the rule against HF's generate -----------------------------------------------------------------------------------------------------------
def _last_logits(model, ids):
    with torch.no_grad():
        return model(torch.tensor([ids])).logits[0, -1].double().numpy()


def replay(model, prompt, pen, automaton=None, root=0):
    """The rule and this project's pick rules -- HF's repetition penalty over prompt + answer, then the mask, first-index arg-max, EOS ends the answer
    -- driven with the HF model's own logits.  -> (tokens, the smallest top-1 / top-2 gap among the allowed tokens)."""
    seq, new, gap = list(prompt), [], float("inf")
    for _ in range(MAX_NEW):
        x = _last_logits(model, seq)
        if pen != 1.0:
            seen = sorted(set(seq))
            x[seen] = np.where(x[seen] < 0, x[seen] * pen, x[seen] / pen)
        if automaton is not None:
            ok = sorted(allowed_ids(automaton, root, new, EOS))
            x = apply_allowed(automaton, root, x, new, EOS)
            top = np.sort(x[ok])[-2:]
        else:
            top = np.sort(x)[-2:]
        if len(top) == 2:
            gap = min(gap, float(top[1] - top[0]))
        t = int(np.argmax(x))
        new.append(t)
        seq.append(t)
        if t == EOS:
            break
    return new, gap


def test_rule_equals_hf_generate(hf_models):        # noqa: F811
    """{trie of 4 choices, nested-prefix trie, cyclic, per-prompt roots in a batch of 2} x {penalty 1.0, 1.3} x seeds 0 - 7 = 64 cases: HF's greedy
    generate(prefix_allowed_tokens_fn=fn) returns, token for token, what the numpy replay of the rule gives; every decision has a top-1 / top-2 gap
    >= 1e-3 among the allowed tokens; at least half of the constrained answers differ from the unconstrained ones; every answer is a path of its
    automaton that ends in an accepting state or is cut by the budget."""
    differ = rows = 0
    smallest = float("inf")
    cases = list(itertools.product(("trie4", "nested", "cyclic", "per_prompt"), (1.0, 1.3), range(8)))
    for kind, pen, seed in cases:
        m = hf_models[seed]
        rng = np.random.default_rng(100 + seed)
        B = 2 if kind == "per_prompt" else 1
        prompts = [[1] + [int(v) for v in rng.integers(3, VOCAB - 1, PROMPT - 1)] for _ in range(B)]
        if kind == "per_prompt":
            automaton, roots = TokenAutomaton.union([trie4(), cyclic()])
            assert roots == [0, trie4().n_states]
        else:
            automaton, roots = AUTOMATA[kind](), [0]
        with torch.no_grad():
            hf = m.generate(torch.tensor(prompts), prefix_allowed_tokens_fn=prefix_fn(automaton, roots, PROMPT, EOS), max_new_tokens=MAX_NEW,
                            do_sample=False, repetition_penalty=pen, pad_token_id=PAD, eos_token_id=EOS)
        for b in range(B):
            row = hf[b, PROMPT:].tolist()
            new, gap = replay(m, prompts[b], pen, automaton, roots[b])
            assert row[:len(new)] == new and all(t == PAD for t in row[len(new):]), (kind, pen, seed, b, row, new)
            assert gap >= 1e-3, (kind, pen, seed, b, gap)
            smallest = min(smallest, gap)
            body = new[:-1] if new[-1] == EOS else new
            state = automaton.walk(roots[b], body)
            assert state != DEAD and (bool(automaton.accept[state]) if new[-1] == EOS else len(new) == MAX_NEW), (kind, pen, seed, b, new)
            free, _ = replay(m, prompts[b], pen)
            differ += free != new
            rows += 1
    print(f"{differ} of {rows} constrained answers differ from the unconstrained one; smallest top-1 / top-2 gap {smallest:.3g}")
    assert len(cases) == 64 and differ >= rows // 2, (differ, rows)


# ---- 3. constructors -----------------------------------------------------------------------------------------------------------------------------
def test_from_sequences_builds_a_trie():
    a = TokenAutomaton.from_sequences([[5, 6], [5, 7, 8], [5], [9], [5, 6], (5, 7, 8)])          # a prefix of another; duplicates merge
    assert a.n_states == 6 and a.n_edges == 5 and a.row_ptr.tolist() == [0, 2, 4, 4, 5, 5, 5]
    assert a.edges(0) == [(5, 1), (9, 5)] and a.edges(1) == [(6, 2), (7, 3)] and a.accept.tolist() == [0, 1, 1, 0, 1, 1]
    assert a.row_ptr.dtype == a.edge_token.dtype == a.edge_next.dtype == np.int32 and a.accept.dtype == np.uint8
    assert a == TokenAutomaton.from_sequences([[5, 6], [5, 7, 8], [5], [9]]) and a != trie4()       # states are numbered in order of first use
    assert allowed_ids(a, 0, [], 2) == {5, 9} and allowed_ids(a, 0, [5], 2) == {2, 6, 7} and allowed_ids(a, 0, [5, 7], 2) == {8}
    assert allowed_ids(a, 0, [5, 6], 2) == {2} and allowed_ids(a, 0, [4], 2) == {2} and allowed_ids(a, 0, [4, 5], 2) == {2}      # DEAD stays DEAD
    assert a.walk(0, [5, 7, 8]) == 4 and a.walk(0, [5, 8]) == DEAD and a.step(DEAD, 5) == DEAD
    for bad, msg in (([[5], []], "an empty sequence"), ([], "no sequence given"), ([[5, -1]], "non-negative token ids"), ([[5, 1.5]], "non-negative token ids")):
        with pytest.raises(ValueError, match=msg):
            TokenAutomaton.from_sequences(bad)


def test_from_edges_takes_cycles_and_refuses_a_second_edge_on_a_token():
    c = cyclic()
    assert c.n_states == 2 and c.n_edges == 20 and c.accept.tolist() == [0, 1]
    assert allowed_ids(c, 0, [], EOS) == set(DIGITS) and allowed_ids(c, 0, DIGITS * 5, EOS) == set(DIGITS) | {EOS} and allowed_ids(c, 0, [20, 3], EOS) == {EOS}
    assert c == TokenAutomaton.from_edges(2, reversed([(s, t, 1) for s in (0, 1) for t in DIGITS]), [False, True])      # any order; one flag per state
    with pytest.raises(ValueError, match="state 0 has two edges on token 7"):
        TokenAutomaton.from_edges(2, [(0, 7, 1), (0, 7, 0)], [1])
    for edges, acc, msg in (([(0, 7, 2)], [1], "edge .* is not"), ([(2, 7, 0)], [1], "edge .* is not"), ([(0, -7, 1)], [1], "edge .* is not"),
                            ([(0, 7, 1)], [2], "accepting state 2 outside")):
        with pytest.raises(ValueError, match=msg):
            TokenAutomaton.from_edges(2, edges, acc)
    with pytest.raises(ValueError, match="`n_states` has to be a positive integer"):
        TokenAutomaton.from_edges(0, [], [])
    with pytest.raises(ValueError, match="sorted and distinct"):
        TokenAutomaton([0, 2], [7, 7], [0, 0], [1])
    with pytest.raises(ValueError, match="outside the 1 states"):
        TokenAutomaton([0, 1], [7], [1], [1])


class WordTok:
    """A tokenizer of whole words over a fixed list; a leading space makes a piece of its own id, as sentencepiece's does."""
    words = {"yes": 10, "no": 11, "maybe": 12, " yes": 20, " no": 21, "not": 13, "sure": 14}

    def __call__(self, text, add_special_tokens=True):
        ids, rest = ([1] if add_special_tokens else []), text
        while rest:
            w = max((w for w in self.words if rest.startswith(w)), key=len, default=None)
            if w is None:
                assert rest[0] == " ", rest
                rest = rest[1:]
                continue
            ids.append(self.words[w])
            rest = rest[len(w):]
        return types.SimpleNamespace(input_ids=ids)


def test_from_texts_asks_the_tokenizer_without_special_tokens():
    tok = WordTok()
    assert TokenAutomaton.from_texts(tok, ["yes", "no"]) == TokenAutomaton.from_sequences([[10], [11]])
    assert TokenAutomaton.from_texts(tok, ["yes", "no"], prefix=" ") == TokenAutomaton.from_sequences([[20], [21]])          # the leading-space pieces
    assert TokenAutomaton.from_texts(tok, ["not sure", "no"]) == TokenAutomaton.from_sequences([[13, 14], [11]])
    assert "leading-space" in TokenAutomaton.from_texts.__doc__ and "caller's job" in TokenAutomaton.from_texts.__doc__
    with pytest.raises(ValueError, match="an empty sequence"):
        TokenAutomaton.from_texts(tok, ["yes", ""])


def test_union_lays_automata_side_by_side():
    a, c = trie4(), cyclic()
    u, roots = TokenAutomaton.union([a, c, a, trie4()])
    assert roots == [0, a.n_states, 0, 0] and u.n_states == a.n_states + 2 and u.n_edges == a.n_edges + c.n_edges      # equal automata are laid down once
    for gen in ([], [5], [5, 6, 7], [20], [20, 21], [5, 20]):
        assert allowed_ids(u, roots[0], gen, EOS) == allowed_ids(a, 0, gen, EOS)
        assert allowed_ids(u, roots[1], gen, EOS) == allowed_ids(c, 0, gen, EOS)
    with pytest.raises(ValueError, match="no automaton given"):
        TokenAutomaton.union([])
    with pytest.raises(ValueError, match="is not a TokenAutomaton"):
        TokenAutomaton.union([a, [[5]]])


# ---- 4. the checks of a call ---------------------------------------------------------------------------------------------------------------------
def test_check_allowed():
    a, c = trie4(), cyclic()
    assert check_allowed(None, 3, VOCAB, EOS) is None and check_allowed(None, 3, VOCAB, None, beams=4, lookup=3) is None        # None asks nothing
    one = check_allowed(a, 3, VOCAB, EOS)
    assert one.automaton is a and one.roots == [0, 0, 0]
    per = check_allowed([a, c, a], 3, VOCAB, EOS)
    assert per.roots == [0, a.n_states, 0] and check_allowed(per, 3, VOCAB, EOS) is per
    for args, msg in (((a, 1, 12, EOS), r"vocabulary size is 12, but `allowed` has edges on the tokens \[12\]"),
                      ((a, 1, VOCAB, None), "`allowed` needs an EOS token"), ((a, 1, VOCAB, -1), "`allowed` needs an EOS token"),
                      ((a, 1, VOCAB, VOCAB), "eos_token_id 41 outside the vocabulary"),
                      (([a, c], 3, VOCAB, EOS), "`allowed` lists 2 automata for 3 prompts"),
                      ((per, 2, VOCAB, EOS), "carries 3 roots for 2 prompts"),
                      ((Allowed(a, [0, 99]), 2, VOCAB, EOS), "roots .* outside the 8 states"),
                      (("yes,no", 1, VOCAB, EOS), "has to be a TokenAutomaton, a list with one per prompt or None")):
        with pytest.raises(ValueError, match=msg):
            check_allowed(*args)
    with pytest.raises(ValueError, match=r"`allowed` cannot be combined with `beams`=2 \(the beam pick applies no logits processor"):
        check_allowed(a, 1, VOCAB, EOS, beams=2)
    with pytest.raises(ValueError, match=r"`allowed` cannot be combined with `lookup`=3 \(the drafts are verified against the unconstrained pick\)"):
        check_allowed(a, 1, VOCAB, EOS, lookup=3)
    # the limits of include/pgv.h
    assert (MAX_STATES, MAX_EDGES) == (1 << 20, 1 << 22)
    header = open(os.path.join(ROOT, "include", "pgv.h")).read()
    assert "#define PGV_ALLOW_MAX_STATES (1 << 20)" in header and "#define PGV_ALLOW_MAX_EDGES (1 << 22)" in header
    chain = TokenAutomaton(np.arange(MAX_STATES + 2, dtype=np.int32).clip(max=MAX_STATES), np.zeros(MAX_STATES, dtype=np.int32),
                           np.arange(1, MAX_STATES + 1, dtype=np.int32), np.zeros(MAX_STATES + 1, dtype=np.uint8))
    with pytest.raises(ValueError, match=f"has {MAX_STATES + 1} states, the limit is {MAX_STATES}"):
        check_allowed(chain, 1, VOCAB, EOS)
    E = MAX_EDGES + 1
    wide = TokenAutomaton(np.array([0, E], dtype=np.int32), np.arange(E, dtype=np.int32), np.zeros(E, dtype=np.int32), np.ones(1, dtype=np.uint8))
    with pytest.raises(ValueError, match=f"has {E} edges, the limit is {MAX_EDGES}"):
        check_allowed(wide, 1, 1 << 23, EOS)


ONE = [[1, 2, 3]]


def test_generate_refusals_and_their_wording():
    a = TokenAutomaton.from_sequences([[5, 6]])
    for kw, msg in ((dict(allowed=a, beams=2), "`allowed` cannot be combined with `beams`=2"), (dict(allowed=a, lookup=3), "`allowed` cannot be combined with `lookup`=3"),
                    (dict(allowed=a, eos_token_id=None), "`allowed` needs an EOS token"), (dict(allowed=[a, a]), "lists 2 automata for 1 prompts"),
                    (dict(allowed=TokenAutomaton.from_sequences([[300]])), "vocabulary size is 256")):
        with pytest.raises(ValueError, match=msg):
            G.plan_generate(LoopLM(), ONE, max_new_tokens=4, **kw)
    # a call that is faulty twice keeps the error it has always had
    for kw, msg in ((dict(top_p=1.5), "`top_p` has to be a float"), (dict(beams=9), "`beams`=9 has to be an integer"), (dict(lookup=99), "`lookup`=99 has to be an integer")):
        with pytest.raises(ValueError, match=msg):
            G.plan_generate(LoopLM(), ONE, max_new_tokens=4, allowed=[a, a], **kw)
    p = G.plan_generate(LoopLM(), ONE, max_new_tokens=4, allowed=a)
    assert p.allowed.automaton is a and p.allowed.roots == [0] and p.settings.allowed is p.allowed
    assert p.settings.prefill_kwargs() == {"allowed": p.allowed, "eos_id": SEOS}


def test_hf_callback_argument_is_refused_with_a_hint():
    fn = lambda batch_id, ids: [5]          # noqa: E731
    assert "prefix_allowed_tokens_fn" in G.REFUSED
    with pytest.raises(ValueError, match=r"argument `prefix_allowed_tokens_fn`=.* is not implemented by this package .*own keyword `allowed` \(allowed.TokenAutomaton"):
        G.check_generate_kwargs({"prefix_allowed_tokens_fn": fn})
    with pytest.raises(ValueError, match="`prefix_allowed_tokens_fn`"):
        LoopLM().generate(ONE, max_new_tokens=4, prefix_allowed_tokens_fn=fn)
    with pytest.raises(ValueError, match="generation_config field `prefix_allowed_tokens_fn`"):
        G.check_generate_kwargs({}, {"prefix_allowed_tokens_fn": fn})
    G.check_generate_kwargs({"prefix_allowed_tokens_fn": None})           # HF's neutral default passes
    out, _ = _gen(LoopLM(), [_ids("q {hi$}")], max_new_tokens=5, prefix_allowed_tokens_fn=None)
    assert _new(out, [_ids("q {hi$}")])[0][:2] == [ord("h"), ord("i")]


# ---- 5. the chunk loop over the scripted backend ------------------------------------------------------------------------------------------------
class AllowLM(LoopLM):
    """LoopLM with the automaton switch: `sets` records it, `roots` what the switch was handed, `repicks` the greedy re-picks of the first token."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.roots, self.repicks = None, 0

    def set_allowed(self, kv, automaton=None, roots=None, eos_id=-1):
        self.sets.append(("allowed", automaton is not None))
        if automaton is not None:
            self.roots, self.eos = list(roots), eos_id

    def prefill(self, seqs, feats, max_seq, want_logits=False, want_all_logits=False, append_to=None, logprobs=None, capacity=None, bans=None, eos_id=-1,
                lookup=None, allowed=None):
        out = super().prefill(seqs, feats, max_seq, want_logits, want_all_logits, append_to, logprobs, capacity, bans, eos_id, lookup)
        if allowed is not None:             # the real prefill sets what it is given before the prompt runs
            self.set_allowed(out[0], allowed.automaton, allowed.roots, eos_id)
        return out

    def greedy_last(self, kv, width, repetition_penalty=1.0):
        self.repicks += 1
        return super().greedy_last(kv, width, repetition_penalty)


def test_the_loop_switches_the_automaton_on_for_the_call_only():
    prompts = [_ids("tell me {abcabc abcab$}"), _ids("q {hi$}"), _ids("a much longer question {}")]
    a, c = TokenAutomaton.from_sequences([[ord("h"), ord("i")]]), TokenAutomaton.from_sequences([[ord("a")], [ord("b")]])
    for mode in ({}, {"do_sample": True, "temperature": 0.2}):
        plain, tm0 = _gen(LoopLM(), prompts, max_new_tokens=17, chunk=5, **mode)
        for allowed, roots in ((a, [0, 0, 0]), ([a, c, a], [0, a.n_states, 0])):
            m = AllowLM()
            out, tm = _gen(m, prompts, max_new_tokens=17, chunk=5, allowed=allowed, **mode)
            # the scripted backend knows no constraint: the answers are the script's, the switch went on with the prefill and off at the end
            assert torch.equal(out, plain) and tm["steps"] == tm0["steps"]
            assert m.calls == [("prefill", 3)] and m.sets == [("allowed", True), ("allowed", False)] and m.roots == roots and m.eos == SEOS
            assert m.repicks == (0 if mode else 1)          # greedy: the first token is re-picked over the processed logits, as under bans
    # samples_per_prompt: the roots are per PROMPT -- the fork carries them to the samples (pgv_kv_fork copies a slot's root)
    m = AllowLM()
    _gen(m, prompts[:2], max_new_tokens=5, allowed=[a, c], do_sample=True, temperature=0.2, samples_per_prompt=3)
    assert m.roots == [0, a.n_states] and m.sets == [("allowed", True), ("allowed", False)]
    # with bans and log-probabilities: one scope for all three
    m = AllowLM()
    _gen(m, prompts, max_new_tokens=5, allowed=a, bans={"suppress": [5]}, output_logprobs=True)
    assert sorted(m.sets[:3]) == [("allowed", True), ("bans", True), ("logprobs", True)] and sorted(m.sets[3:]) == [("allowed", False), ("bans", False), ("logprobs", False)]
    # kv_reuse_key falls back to the full prefill
    m = AllowLM()
    for _ in range(2):
        m.generate([list(prompts[1])], video_spatio_temporal_features=torch.full((1, VROWS, 8), 65.0), max_new_tokens=5, allowed=a, kv_reuse_key="clip")
    assert m.calls == [("prefill", 1), ("prefill", 1)]
    # the switch is cleared when a step fails
    m = AllowLM(fail=("decode_greedy",))
    with pytest.raises(RuntimeError, match="injected"):
        _gen(m, prompts, max_new_tokens=17, allowed=a)
    assert m.sets == [("allowed", True), ("allowed", False)]


def test_none_is_the_call_without_the_keyword():
    prompts = [_ids("tell me {abcabc abcab$}"), _ids("q {hi$}")]
    assert G.plan_generate(LoopLM(), prompts, max_new_tokens=9, allowed=None) == G.plan_generate(LoopLM(), prompts, max_new_tokens=9)
    for mode in ({}, {"do_sample": True, "temperature": 0.2}):
        x, y = AllowLM(), AllowLM()
        out_x, tm_x = _gen(x, prompts, max_new_tokens=9, allowed=None, **mode)
        out_y, tm_y = _gen(y, prompts, max_new_tokens=9, **mode)
        assert torch.equal(out_x, out_y) and x.calls == y.calls and x.sets == y.sets == [] and x.repicks == y.repicks == 0 and tm_x["steps"] == tm_y["steps"]
    p = G.plan_generate(LoopLM(), prompts, max_new_tokens=9)
    assert p.allowed is None and p.settings.allowed is None and p.settings == G.CacheSettings(eos_id=SEOS) and "allowed" not in p.settings.prefill_kwargs()


def test_generate_continuous_takes_one_automaton():
    import inspect
    from video_llava_amd import continuous, inference
    from video_llava_amd.model.video_chatgpt import VideoChatGPTLlamaForCausalLM as M
    assert inspect.signature(continuous.generate_continuous).parameters["allowed"].default is None
    assert inspect.signature(M.generate).parameters["allowed"].default is None and callable(M.set_allowed) and callable(M.allow_peek)
    assert inspect.signature(M.prefill).parameters["allowed"].default is None
    for fn in (inference.video_chatgpt_infer, inference.video_chatgpt_infer_logprobs):
        assert inspect.signature(fn).parameters["allowed"].default is None
    a = TokenAutomaton.from_sequences([[5]])
    with pytest.raises(ValueError, match="ONE TokenAutomaton shared by every task"):
        next(continuous.generate_continuous(LoopLM(), iter([]), 2, 4, allowed=[a, a]))
    with pytest.raises(ValueError, match=r"generate_continuous\(\): `allowed` needs an EOS token"):
        next(continuous.generate_continuous(LoopLM(), iter([]), 2, 4, allowed=a, eos_token_id=None))


# ---- 6. the callers' flags -----------------------------------------------------------------------------------------------------------------------
def test_runner_and_chat_flags(tmp_path):
    from video_llava_amd.chat import allowed_from_choices, answer_choices_from_flags, parse_args
    from video_llava_amd.eval import _sharded
    assert answer_choices_from_flags(None, None) is None and answer_choices_from_flags(None, None, lookup=3, beams=4) is None
    assert answer_choices_from_flags("yes,no", None) == ["yes", "no"] and answer_choices_from_flags(" yes , no ,,", None) == ["yes", "no"]
    f = tmp_path / "answers.txt"
    f.write_text("yes\nno\n\nnot sure\n")
    assert answer_choices_from_flags(None, str(f)) == ["yes", "no", "not sure"]
    for args, kw, msg in ((("yes,no", str(f)), {}, "pass one of them"), ((" , ", None), {}, "no answer given"),
                          (("yes,no", None), dict(beams=2), r"--answer_choices cannot be combined with --beams 2 \(the beam pick"),
                          (("yes,no", None), dict(lookup=3), r"--answer_choices cannot be combined with --lookup 3 \(the drafts")):
        with pytest.raises(ValueError, match=msg):
            answer_choices_from_flags(*args, **kw)
    with pytest.raises(OSError):
        answer_choices_from_flags(None, str(tmp_path / "missing.txt"))
    tok = WordTok()
    assert allowed_from_choices(tok, None) is None and allowed_from_choices(tok, []) is None
    assert allowed_from_choices(tok, ["yes", "no", "not sure"]) == TokenAutomaton.from_sequences([[10], [11], [13, 14]])
    base = ["--model-name", "m", "--projection_path", "p"]
    a = parse_args(base + ["--answer_choices", "yes,no"])
    assert a.answer_choices == "yes,no" and a.answer_choice_list == ["yes", "no"] and parse_args(base).answer_choice_list is None
    assert parse_args(base + ["--answer_choices_file", str(f)]).answer_choice_list == ["yes", "no", "not sure"]
    for bad in (["--answer_choices", "yes,no", "--lookup", "3"], ["--answer_choices", ","], ["--answer_choices_file", str(tmp_path / "missing.txt")]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    ns = types.SimpleNamespace(answer_choices="yes,no", answer_choices_file=None, lookup=0, beams=1)
    assert _sharded.answer_choices_from_args(ns) == ["yes", "no"]
    assert _sharded.allowed_from_args(ns, tok) == {"allowed": TokenAutomaton.from_sequences([[10], [11]])}
    assert _sharded.allowed_from_args(types.SimpleNamespace(), tok) == {} and _sharded.answer_choices_from_args(types.SimpleNamespace()) is None
    ns.beams = 2
    with pytest.raises(ValueError, match="--beams 2"):
        _sharded.answer_choices_from_args(ns)
    import argparse
    parser = _sharded.add_runtime_arguments(argparse.ArgumentParser())
    ns, _ = parser.parse_known_args(["--answer_choices", "A,B,C,D"])
    assert _sharded.answer_choices_from_args(ns) == ["A", "B", "C", "D"] and parser.parse_known_args([])[0].answer_choices is None
    with pytest.raises(SystemExit):
        parser.parse_known_args(["--answer_choices", "yes,no", "--beams", "2"])


# ---- 7. the decode-graph key ---------------------------------------------------------------------------------------------------------------------
def test_decode_graph_key_carries_the_automaton_generation(tmp_path):
    """Two keys that differ only in the automaton's generation counter compare unequal (the allow kernel's launch and the automaton's addresses are
    baked in); generation 0 -- the feature off -- is the key as it has always been, the bans' counter untouched."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    prog = r"""#include <cstdio>
#include "pick_params.h"
int main() {
    const PickParams p{0.7f, 50, 0.9f, 1.2f, false};
    const int F = AM_INC_POS | AM_RECORD | AM_SAMPLE;
    const DecodeGraphKey off = decode_graph_key(2, 7, F, 3, false, p), a = decode_graph_key(2, 7, F, 3, false, p, 0, 0, 0, 0, 0, 1.f, 1),
                         b = decode_graph_key(2, 7, F, 3, false, p, 0, 0, 0, 0, 0, 1.f, 2), bans = decode_graph_key(2, 7, F, 3, false, p, 0, 1);
    int bad = 0;
    bad |= !(off.allowed == 0 && a.allowed == 1 && b.allowed == 2 && DecodeGraphKey{}.allowed == 0 && bans.allowed == 0 && a.bans == 0);
    bad |= (off == a) || (a == b) || (a == bans) || !(a == decode_graph_key(2, 7, F, 3, false, p, 0, 0, 0, 0, 0, 1.f, 1));
    bad |= !(off == decode_graph_key(2, 7, F, 3, false, p, 0, 0, 0, 0, 0, 1.f, 0));
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
"""
    src = tmp_path / "key.cpp"
    src.write_text(prog)
    exe = tmp_path / "key"
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "video_llava_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout
