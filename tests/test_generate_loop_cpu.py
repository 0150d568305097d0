"""generate()'s host driver on the CPU: the call plan (generation.plan_generate), the cache-settings scope (generation.CacheSettings) and the
chunk loop (generate_loop) over a scripted backend -- test_runner_core_cpu.ScriptedLM widened to every step method a call can reach.  The
error texts and the `steps` figures below were recorded from the commit before the loop moved out of the model class.  No GPU."""
import numpy as np
import pytest
import torch

from test_runner_core_cpu import EOS, FILLER, V, CharTok, ScriptedLM, _KV
from video_llava_amd import generation as G
from video_llava_amd.continuous import Task, generate_continuous
from video_llava_amd.generation import fork_sources

D = 3               # drafts per lookup step in every lookup case


def _flip(t, u):
    """The scripted `sampled` token: the script's letter, its case flipped when the uniform is below 0.5 -- so a wrong row of uniforms shows."""
    return int(t) ^ 0x20 if u is not None and float(u) < 0.5 and chr(int(t)).isalpha() else int(t)


class LoopLM(ScriptedLM):
    """ScriptedLM with every step method of the model class, each with the real parameter list; `sets` records the set_* calls as
    (switch, on) and `fail` names the step methods that raise."""

    def __init__(self, max_pos=512, fail=()):
        super().__init__(max_pos)
        self.sets, self.fail = [], set(fail)

    def _hit(self, name):
        if name in self.fail:
            raise RuntimeError(f"injected: {name}")

    def set_logprobs(self, kv, on=True):
        self.sets.append(("logprobs", bool(on)))

    def set_bans(self, kv, bans=None, eos_id=-1):
        self.sets.append(("bans", bans is not None))

    def set_filters(self, kv, filters=None):
        self.sets.append(("filters", filters is not None))

    def set_lookup(self, kv, D, n=2):           # noqa: N803
        self.sets.append(("lookup", D > 0))
        kv.D = int(D)

    def prefill(self, seqs, feats, max_seq, want_logits=False, want_all_logits=False, append_to=None, logprobs=None, capacity=None, bans=None,
                eos_id=-1, lookup=None):
        self.calls.append(("prefill", len(seqs)))
        kv = _KV(max(len(seqs), int(capacity or 0)), max_seq)
        kv.D = 0
        if logprobs is not None:                # the real prefill sets what it is given before the prompt runs
            self.set_logprobs(kv, logprobs)
        if bans is not None:
            self.set_bans(kv, bans, eos_id)
        if lookup is not None:
            self.set_lookup(kv, *lookup)
        return kv, torch.tensor([self._start(kv, s, p, feats[s]) for s, p in enumerate(seqs)], dtype=torch.int32), None

    def fork(self, kv, counts):
        self._hit("fork")
        src = fork_sources(counts)
        kv.script, kv.g, kv.done, kv.len = ([x[i] for i in src] for x in (kv.script, kv.g, kv.done, kv.len))
        return len(src)

    def _first(self, kv, u=None):
        return torch.tensor([_flip(sc[0] if sc else ord(FILLER), None if u is None else u[s]) for s, sc in enumerate(kv.script)], dtype=torch.int32)

    def greedy_last(self, kv, width, repetition_penalty=1.0):
        return self._first(kv)

    def sample_last(self, kv, u, temperature, top_k=50, top_p=1.0, repetition_penalty=1.0):
        assert u.shape == (len(kv.g),)
        return self._first(kv, u)

    def decode_greedy(self, kv, first, n, eos_id=-1, repetition_penalty=1.0):
        self._hit("decode_greedy")
        return super().decode_greedy(kv, first, n, eos_id)

    def decode_sample(self, kv, first, n, eos_id, temperature, top_k, u, top_p=1.0, repetition_penalty=1.0):
        assert u.shape == (n, len(kv.g))
        out = super().decode_greedy(kv, first, n, eos_id)
        return torch.tensor([[_flip(out[s, i], u[i, s]) for i in range(n)] for s in range(len(kv.g))], dtype=torch.int32)

    @staticmethod
    def _lp(kv, s, t):
        """Token t of slot s: a value of its own, so a shifted or wrongly cut row shows."""
        return -(0.25 * (t + 1) + 0.01 * len(kv.script[s]))

    def logprobs_last(self, kv, width):
        row = torch.tensor([self._lp(kv, s, kv.g[s] - 1) for s in range(width)], dtype=torch.float32)
        return torch.stack([row, 2 * row])

    def logprobs_steps(self, kv, width, n):
        rows = torch.tensor([[self._lp(kv, s, kv.g[s] - n + i) for i in range(n)] for s in range(width)], dtype=torch.float32)
        return torch.stack([rows, 2 * rows])

    def decode_lookup(self, kv, first, steps, eos_id, budget, u_base=None, u=None):
        """Every step a sequence emits a run of 1 + (position mod (1 + D)) tokens of its script: the drafts the script `accepts`."""
        self._hit("decode_lookup")
        B = len(budget)
        toks, counts = torch.zeros(B, steps * (1 + kv.D), dtype=torch.int32), np.zeros((steps, B), dtype=np.int32)
        for s in range(B):
            e = 0
            for i in range(steps):
                for _ in range(0 if kv.done[s] else min(1 + kv.g[s] % (1 + kv.D), budget[s] - e)):
                    t = self._emit(kv, s, eos_id)
                    toks[s, e] = t if u is None else _flip(t, u[u_base[s] + e, s])
                    e, kv.len[s] = e + 1, kv.len[s] + 1
                    counts[i, s] += 1
                    if kv.done[s]:
                        break
        return toks, counts

    def decode_lookup_sample(self, kv, first, steps, eos_id, budget, u_base, temperature, top_k, u):
        assert u.dim() == 2 and u.shape[1] == len(budget) == len(u_base)
        return self.decode_lookup(kv, first, steps, eos_id, budget, u_base, u)


def _ids(text):
    return CharTok()._encode(text)


PROMPTS = [_ids("tell me {abcabc abcab$}"), _ids("q {hi$}"), _ids("a much longer question {}")]       # EOS at token 13 / 3 / never
MODES = {"greedy": {}, "sampled": {"do_sample": True, "temperature": 0.2}, "lookup": {"lookup": D},
         "lookup_sample": {"do_sample": True, "temperature": 0.2, "lookup": D, "lookup_sample": True}}
BANS, FILTERS = {"suppress": [5]}, {"min_p": 0.1}


def _gen(m, prompts, **kw):
    """-> (what generate returned, its timings); sampled runs draw from one seed."""
    tm = {}
    if kw.get("do_sample"):
        kw["generator"] = torch.Generator().manual_seed(5)
    out = m.generate([list(p) for p in prompts], video_spatio_temporal_features=torch.full((len(prompts), V, 8), 65.0), timings=tm, **kw)
    return out, tm


def _run(mode, prompts, **kw):
    return _gen(LoopLM(), prompts, **MODES[mode], **kw)


def _new(out, prompts):
    """The new ids of every row of a generate() result, pads included."""
    seq = out if torch.is_tensor(out) else out.sequences
    return [seq[b, len(p):].tolist() for b, p in enumerate(prompts)]


# ---- 1. error order: the first ValueError of a call with several faults ------------------------------------------------------------------------
never = lambda ids, scores: False       # noqa: E731
ONE, TWO = [[1, 2, 3]], [[1, 2, 3], [1, 2, 3, 4]]
FAULTY = [       # (prompts, keywords with two or more faults, the ValueError the commit before raised)
    (ONE, dict(beams=2, do_sample=True, top_p=1.5), "`top_p` has to be a float > 0 and <= 1, but is 1.5"),
    (ONE, dict(lookup=3, samples_per_prompt=2, bans=BANS),
     "generate(): `samples_per_prompt`=2 needs do_sample=True (HF: \"Greedy methods without beam search do not support `num_return_sequences` "
     "different than 1\")"),
    (ONE, dict(stop_strings=["a", "b"], do_sample=True, temperature=0),
     "`temperature` (=0.0) has to be a strictly positive float; use do_sample=False for greedy decoding"),
    (ONE, dict(num_beams=2, beams=99),
     "generate(): argument `num_beams`=2 is not implemented by this package (it would change the result of HF's generate()); implemented: "
     "temperature, top_k, top_p, repetition_penalty; beam search: this package's own keyword `beams`"),
    (ONE, dict(output_beam_scores=True, samples_per_prompt=0),
     "generate(): `output_beam_scores` needs `beams` > 1 (a greedy answer's log-probabilities: `output_logprobs=True`)"),
    (ONE, dict(beams=2, bans=BANS, filters={"min_p": 2}),
     "generate(): `bans` cannot be combined with `beams`=2 (the beam pick applies no logits processor; each beam's sequence would have to be "
     "rebuilt from the parent history)"),
    (ONE, dict(lookup=3, do_sample=True, filters={"typical_p": 0}),
     "generate(): `do_sample` cannot be combined with `lookup`=3 (a sampled token has no draft to verify; speculative sampling is not "
     "implemented -- `lookup_sample`=True verifies against the run's own uniforms)"),
    (ONE, dict(lookup=99, max_new_tokens=10 ** 6), "generate(): `lookup`=99 has to be an integer in [0, 15]"),
    (TWO, dict(max_new_tokens=10 ** 6, stopping_criteria=[never]), "prompt + max_new_tokens = 1000004 exceeds max_position_embeddings 4096"),
    (TWO, dict(stopping_criteria=[never], do_sample=True, temperature=0),
     "stopping_criteria are evaluated on one sequence (the reference passes them with batch size 1 only)"),
    (ONE, dict(repetition_penalty=0, beams=0), "`penalty` has to be a strictly positive float, but is 0.0"),
    (ONE, dict(samples_per_prompt=2, do_sample=True, kv_reuse_key="k", lookup_sample=True),
     "generate(): `samples_per_prompt`=2 cannot be combined with `kv_reuse_key` (the kept cache would hold 2 different answers)"),
    (ONE, dict(beams=2, stop_strings=["x"], kv_reuse_key="k"),
     "generate(): `stop_strings` cannot be combined with `beams`=2 (they cut one running sequence, not a set of hypotheses)"),
    (ONE, dict(bans={"nope": 1}, lookup=3, output_logprobs=True),
     "`bans` has no field `nope`; fields: bad_words, begin_suppress, min_length, min_new_tokens, no_repeat_ngram, suppress"),
    (ONE, dict(output_logprobs=True, return_dict_in_generate=True, top_p=0),
     "generate(): argument `return_dict_in_generate`=True is not implemented by this package (generate() returns the ids only; "
     "`output_logprobs=True` adds the per-token log-probabilities, HF's compute_transition_scores)"),
    (ONE, dict(lookup_sample=True, filters={"bogus": 1}), "generate(): `lookup_sample` needs `do_sample` (the greedy form is `lookup` alone)"),
]


@pytest.mark.parametrize("case", range(len(FAULTY)))
def test_a_call_with_several_faults_raises_the_same_first_error(case):
    prompts, kw, want = FAULTY[case]
    m = LoopLM(4096)
    with pytest.raises(ValueError) as e:
        m.generate(prompts, **kw)
    assert str(e.value) == want
    assert m.calls == [] and m.sets == []           # refused on the host, before any device work


# ---- 2. chunk independence ------------------------------------------------------------------------------------------------------------------------
# timings["steps"] of the scripted runs below at the commit before, the same for chunk 1, 3 and 32: (B, max_new_tokens) -> steps, in every mode
STEPS = {(1, 1): 1, (1, 2): 2, (1, 17): 13, (3, 1): 1, (3, 2): 2, (3, 17): 17}
ANSWERS = ["abcabc abcab", "hi", FILLER * 17]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_result_does_not_depend_on_the_chunk(mode, B):
    prompts, plain = PROMPTS[:B], mode in ("greedy", "sampled")
    for new in (1, 2, 17):
        runs = [_run(mode, prompts, max_new_tokens=new, chunk=c, **({"output_logprobs": True} if plain else {})) for c in (1, 3, 32)]
        (ref, _), ids = runs[0], _new(runs[0][0], prompts)
        for out, tm in runs:
            assert _new(out, prompts) == ids and tm["steps"] == STEPS[B, new] and tm["batch"] == B
            assert ("lookup_steps" in tm) == (not plain)
            if plain:
                assert out.new_lengths.tolist() == ref.new_lengths.tolist()
                assert torch.equal(out.token_logprobs, ref.token_logprobs) and torch.equal(out.transition_scores, ref.transition_scores)
        if plain:
            # the values are those of the kept tokens, cut with the ids: token t of a sequence carries LoopLM._lp(t)
            assert ref.new_lengths.tolist() == [min(new, len(a) + 1) for a in ANSWERS[:B]]
            for b, n in enumerate(ref.new_lengths.tolist()):
                want = [-(0.25 * (t + 1) + 0.01 * (len(ANSWERS[b]) + 1 if b < 2 else 0)) for t in range(n)]
                assert np.allclose(ref.token_logprobs[b, :n].numpy(), want, atol=1e-6) and not ref.token_logprobs[b, n:].any()
            assert torch.equal(_run(mode, prompts, max_new_tokens=new)[0], ref.sequences)                  # the keyword changes no id
        # lookup steps give the tokens of the plain run, greedy and sampled (the case flips show that each token drew from its own uniform)
        assert _new(_run(mode.replace("lookup_sample", "sampled").replace("lookup", "greedy"), prompts, max_new_tokens=new)[0], prompts) == ids
        if mode.startswith("greedy") or mode == "lookup":
            assert [CharTok().batch_decode([r])[0] for r in ids] == [a[:new] for a in ANSWERS[:B]]


# ---- 3. cuts inside a chunk -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("cut", ["stop", "eos", "criterion"])
def test_a_cut_inside_a_chunk_gives_the_ids_of_the_per_token_run(cut, mode):
    prompt, kept = {"stop": (_ids("colour {red ### blue$}"), 7), "eos": (_ids("w {abcde$fgh}"), 6), "criterion": (_ids("count {abcdefghijklmnop}"), 5)}[cut]
    kw = {"stop": {"stop_strings": ["###"], "tokenizer": CharTok()}, "eos": {},
          "criterion": {"stopping_criteria": [lambda ids, scores: ids.shape[1] - len(prompt) >= kept]}}[cut]
    plain = mode in ("greedy", "sampled")
    if plain:
        kw["output_logprobs"] = True
    (ref, _), (out, tm) = (_run(mode, [prompt], max_new_tokens=30, chunk=c, **kw) for c in (1, 32))
    assert _new(out, [prompt]) == _new(ref, [prompt]) and len(_new(out, [prompt])[0]) == kept
    assert tm["steps"] >= kept
    if plain:
        assert out.new_lengths.tolist() == [kept] and out.token_logprobs.shape == (1, kept)
        assert torch.equal(out.token_logprobs, ref.token_logprobs) and torch.equal(out.transition_scores, ref.transition_scores)


# ---- 4. the cache settings of a call are cleared however it ends --------------------------------------------------------------------------------------
class RaisingTok(CharTok):
    def batch_decode(self, ids, skip_special_tokens=True):
        raise RuntimeError("injected: tokenizer")


def raising(ids, scores):
    raise RuntimeError("injected: criterion")


def _scoped(sets, on):
    """`sets` switches exactly the settings `on` on, then each of them off once, and touches nothing else."""
    k = len(on)
    assert sorted(sets[:k]) == sorted((name, True) for name in on), sets
    assert sorted(sets[k:]) == sorted((name, False) for name in on), sets


SAMPLED = {"do_sample": True, "temperature": 0.2}
ENDS = [        # (what raises after the prefill went through, the call with every switch on that combines, the switches that are on)
    ("fork", dict(SAMPLED, samples_per_prompt=2, output_logprobs=True, bans=BANS, filters=FILTERS), {"logprobs", "bans", "filters"}),
    ("criterion", dict(SAMPLED, stopping_criteria=[raising], output_logprobs=True, bans=BANS, filters=FILTERS), {"logprobs", "bans", "filters"}),
    ("criterion", dict(SAMPLED, stopping_criteria=[raising], lookup=D, lookup_sample=True, filters=FILTERS), {"lookup", "filters"}),
    ("tokenizer", dict(stop_strings=["###"], tokenizer=RaisingTok(), output_logprobs=True, bans=BANS, filters=FILTERS), {"logprobs", "bans"}),
    ("tokenizer", dict(stop_strings=["###"], tokenizer=RaisingTok(), lookup=D), {"lookup"}),
    ("decode_greedy", dict(output_logprobs=True, bans=BANS, filters=FILTERS), {"logprobs", "bans"}),        # filters are inert without do_sample
    ("decode_lookup", dict(lookup=D), {"lookup"}),
    (None, dict(SAMPLED, output_logprobs=True, bans=BANS, filters=FILTERS), {"logprobs", "bans", "filters"}),
    (None, dict(SAMPLED, lookup=D, lookup_sample=True, filters=FILTERS), {"lookup", "filters"}),
    (None, {}, set()),
]


@pytest.mark.parametrize("case", range(len(ENDS)))
def test_settings_are_cleared_however_the_call_ends(case):
    what, kw, on = ENDS[case]
    m = LoopLM(fail=[what])
    if what is None:
        _gen(m, PROMPTS[:1], max_new_tokens=8, **kw)
    else:
        with pytest.raises(RuntimeError, match=f"injected: {what}"):
            _gen(m, PROMPTS[:1], max_new_tokens=8, **kw)
    assert m.calls == [("prefill", 1)]
    _scoped(m.sets, on)


@pytest.mark.parametrize("closed_early", [True, False])
def test_settings_are_cleared_when_the_continuous_generator_is_closed(closed_early):
    m = LoopLM()
    tasks = [Task(i, list(p), torch.full((V, 8), 65.0)) for i, p in enumerate(PROMPTS)]
    gen = generate_continuous(m, tasks, 2, 8, do_sample=True, temperature=0.2, tokenizer=CharTok(), logprobs={}, bans=BANS, filters=FILTERS)
    first = next(gen)
    assert first[1] is not None and m.sets[-1][1] is True
    if closed_early:
        gen.close()
    else:
        assert len(list(gen)) == 2
    _scoped(m.sets, {"logprobs", "bans", "filters"})
    m = LoopLM()
    assert len(list(generate_continuous(m, tasks, 2, 8, tokenizer=CharTok(), filters=FILTERS))) == 3 and m.sets == []     # greedy: nothing is on


# ---- 5. a neutral call passes none of the newer keywords ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, SAMPLED], ids=["greedy", "sampled"])
def test_a_plain_call_runs_on_the_narrow_step_methods(kw):
    out, tm = _gen(ScriptedLM(512), PROMPTS, max_new_tokens=17, **kw)      # a TypeError here: a keyword leaked into a step method
    assert [CharTok().batch_decode([r])[0] for r in _new(out, PROMPTS)] == ANSWERS and tm["steps"] == 17


# ---- 6. given(): the callers' keyword funnel ------------------------------------------------------------------------------------------------------------
def test_given_keeps_what_is_not_neutral():
    import inspect
    from video_llava_amd.inference import video_chatgpt_infer, video_chatgpt_infer_logprobs
    for fn in (video_chatgpt_infer, video_chatgpt_infer_logprobs):
        prm = inspect.signature(fn).parameters
        defaults = {k: prm[k].default for k in ("bans", "filters", "lookup", "lookup_ngram", "lookup_sample")}
        assert G.given(**defaults) == {}
    assert G.given(beams=1, samples_per_prompt=1, output_logprobs=False, top_p=None, lookup=0, lookup_ngram=3) == {}
    for k, v in dict(bans={}, filters={}, lookup=3, lookup_sample=True, beams=2, samples_per_prompt=4, output_logprobs=True, top_p=0.9,
                     bans_=BANS).items():
        k = k.rstrip("_")
        assert G.given(**{k: v}) == {k: v}
    # `lookup_ngram` travels with `lookup`, as it always has: kept, its default included, exactly when `lookup` is
    assert G.given(lookup=3, lookup_ngram=2, bans=None) == {"lookup": 3, "lookup_ngram": 2}
    assert G.given(lookup=0, lookup_ngram=2, filters=FILTERS, lookup_sample=False) == {"filters": FILTERS}


def test_plan_views_are_empty_when_neutral():
    cfg = ScriptedLM(512)
    p = G.plan_generate(cfg, [[1, 2, 3]], max_new_tokens=4)
    assert p.warp == {} and p.pen == {} and p.settings.prefill_kwargs() == {} and p.settings == G.CacheSettings(eos_id=EOS)
    p = G.plan_generate(cfg, [[1, 2, 3]], max_new_tokens=4, do_sample=True, top_p=0.9, output_logprobs=True, bans=BANS, filters=FILTERS)
    assert p.warp == {"top_p": 0.9, "repetition_penalty": 1.0} and p.pen == {}
    assert p.settings.prefill_kwargs() == {"logprobs": True, "bans": p.bans, "eos_id": EOS} and p.settings.filters == p.filters
    p = G.plan_generate(cfg, [[1, 2, 3]], max_new_tokens=4, repetition_penalty=1.5, filters=FILTERS, stopping_criteria=[never], chunk=32)
    assert p.pen == {"repetition_penalty": 1.5} and p.warp == {"top_p": 1.0, "repetition_penalty": 1.5}
    assert p.settings == G.CacheSettings(eos_id=EOS) and not p.filters.neutral and p.chunk == 16          # greedy: the filters are inert; criteria cap the chunk
    p = G.plan_generate(cfg, [[1, 2, 3]], max_new_tokens=4, lookup=D, kv_reuse_key="clip")
    assert p.settings == G.CacheSettings(eos_id=EOS, lookup=(D, 2)) and p.max_seq == 512                     # one cache for the whole conversation
