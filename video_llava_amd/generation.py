"""Which sampling parameters a `generate()` call runs with, and which HF `generate()` arguments it refuses.

The reference calls HF's `model.generate(...)` (video_chatgpt/inference.py:105-112, chat.py:148-154).  HF merges the checkpoint's
`generation_config.json` into every call: an argument given in the call wins, else the file's value, else HF's own default
(GenerationMixin._prepare_generation_config: `generation_config = copy(self.generation_config); generation_config.update(**kwargs)`).
This module is that precedence for the four parameters the device pick implements, plus the list of arguments that would change HF's
result and have no counterpart here -- those raise instead of being ignored.  Pure host code: importable without a GPU.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

from .guidance import check_guidance
from .allowed import check_allowed
from .logit_bans import LogitBans, check_bans
from .sample_filters import check_filters

GENERATION_CONFIG_NAME = "generation_config.json"

# HF's GenerationConfig defaults (generation/configuration_utils.py) of the parameters the pick implements
HF_DEFAULTS = {"temperature": 1.0, "top_k": 50, "top_p": 1.0, "repetition_penalty": 1.0}
# keyword of generate() -> the value at which it asks nothing, where that is not None / 0 / False (given)
NEUTRAL = {"beams": 1, "samples_per_prompt": 1}


def given(**kw) -> Dict[str, Any]:
    """The keywords of a generate() call that ask something: an entry at its neutral value (None, 0, False; NEUTRAL) is dropped, so a caller
    hands on only what it was given and the call stays the call it has always been.  `lookup_ngram` only qualifies `lookup`: it is kept, its
    default included, exactly when `lookup` is."""
    def asks(k, v):
        return not (v is None or (isinstance(v, (bool, int, float)) and v == NEUTRAL.get(k, 0)))
    return {k: v for k, v in kw.items() if (asks("lookup", kw.get("lookup")) if k == "lookup_ngram" else asks(k, v))}


def _positive(v) -> bool:
    return v is not None and v > 0


# argument -> True when the value asks HF for something this package does not compute (HF's neutral default passes)
REFUSED = {
    "num_beams": lambda v: v is not None and v > 1,
    "num_beam_groups": lambda v: v is not None and v > 1,
    "num_return_sequences": lambda v: v is not None and v > 1,
    "min_p": lambda v: v is not None,
    "typical_p": lambda v: v is not None and v < 1.0,
    "penalty_alpha": lambda v: v is not None and v != 0,
    "no_repeat_ngram_size": _positive,
    "encoder_no_repeat_ngram_size": _positive,
    "bad_words_ids": lambda v: v is not None,
    "min_length": _positive,
    "min_new_tokens": _positive,
    "epsilon_cutoff": _positive,
    "eta_cutoff": _positive,
    "encoder_repetition_penalty": lambda v: v is not None and v != 1.0,
    "prefix_allowed_tokens_fn": lambda v: v is not None,
}


# the refused HF arguments that `generate(bans=...)` covers under this package's own names (logit_bans.LogitBans): named in the refusal
BANS_HINT = {"no_repeat_ngram_size": "no_repeat_ngram", "bad_words_ids": "bad_words", "min_length": "min_length", "min_new_tokens": "min_new_tokens"}


# the refused HF arguments that `generate(filters=...)` covers (sample_filters.SampleFilters, HF's own field names): named in the refusal
FILTERS_HINT = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


class GenerationDefaults:
    """The fields of a checkpoint's generation_config.json, as attributes (`model.generation_config`).  An absent field reads as None."""

    def __init__(self, **fields):
        self._fields = dict(fields)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return self._fields.get(name)

    def to_dict(self) -> Dict[str, Any]:
        return dict(self._fields)

    def __repr__(self):
        return f"GenerationDefaults({self._fields})"


def load_generation_config(path: str) -> Optional[GenerationDefaults]:
    """`path`/generation_config.json -> GenerationDefaults; None when the checkpoint directory has no such file."""
    f = os.path.join(path, GENERATION_CONFIG_NAME)
    if not os.path.isfile(f):
        return None
    with open(f) as fh:
        return GenerationDefaults(**json.load(fh))


def _config_get(generation_config, name):
    if generation_config is None:
        return None
    if isinstance(generation_config, dict):
        return generation_config.get(name)
    return getattr(generation_config, name, None)


def check_generate_kwargs(kwargs: Dict[str, Any], generation_config=None, who: str = "generate()", filters_given: bool = False) -> None:
    """Raise ValueError naming the first argument -- of the call, else of the model's generation config -- that changes what HF's generate()
    returns and that this package does not implement.  Everything else in `kwargs` is inert here (use_cache, pad_token_id, an all-ones
    attention_mask, output_scores=False, ...) and stays ignored.  filters_given: the call passes `filters=`, which takes over the four
    FILTERS_HINT fields of the generation config (sample_filters.resolve_filters); as arguments of the call they stay refused."""
    for name, asks in REFUSED.items():
        if name in kwargs:
            v, where = kwargs[name], "argument"
        elif filters_given and name in FILTERS_HINT:
            continue
        else:
            v, where = _config_get(generation_config, name), "generation_config field"
        if asks(v):
            hint = {"num_return_sequences": "; several sampled answers per prompt: this package's own keyword `samples_per_prompt`",
                    "num_beams": "; beam search: this package's own keyword `beams`",
                    **{hf: f"; HF's -inf processors: this package's own keyword `bans` (logit_bans.LogitBans({field}=...))"
                       for hf, field in BANS_HINT.items()},
                    "prefix_allowed_tokens_fn": "; a callback cannot run on the device -- constrained decoding: this package's own keyword `allowed` "
                                                "(allowed.TokenAutomaton.from_sequences / from_texts / from_edges)",
                    **{hf: f"; HF's sampling warpers behind top_p: this package's own keyword `filters` (sample_filters.SampleFilters({hf}=...))"
                       for hf in FILTERS_HINT}}.get(name, "")
            raise ValueError(f"{who}: {where} `{name}`={v!r} is not implemented by this package (it would change the result of HF's generate()); "
                             f"implemented: temperature, top_k, top_p, repetition_penalty{hint}")
    for name in ("output_scores", "output_attentions", "output_hidden_states", "return_dict_in_generate"):
        if kwargs.get(name):
            raise ValueError(f"{who}: argument `{name}`={kwargs[name]!r} is not implemented by this package (generate() returns the ids only; "
                             f"`output_logprobs=True` adds the per-token log-probabilities, HF's compute_transition_scores)")
    mask = kwargs.get("attention_mask")
    if mask is not None:
        import torch
        if not bool(torch.as_tensor(mask).to(torch.bool).all()):
            raise ValueError(f"{who}: argument `attention_mask` with padding is not implemented; pass a list of prompts for a ragged batch")


MAX_GROUP = 64          # sequences one decode group holds (pgv_kv_create's batch limit)


def fork_sources(counts: Sequence[int]) -> list:
    """The slot map of pgv_kv_fork / model.fork(kv, counts): new slot i is a copy of old slot fork_sources(counts)[i] -- prompt p repeated
    counts[p] times, in order (HF's _expand_inputs_for_generation: repeat_interleave).  fork_sources([2, 1, 3]) == [0, 0, 1, 2, 2, 2]."""
    src = []
    for p, c in enumerate(counts):
        if int(c) != c or c < 1:
            raise ValueError(f"fork_sources: count {c!r} of sequence {p} is not an integer >= 1")
        src += [p] * int(c)
    return src


def check_samples_per_prompt(n, batch: int, do_sample: bool, has_criteria: bool, has_reuse_key: bool, who: str = "generate()") -> int:
    """Validate generate(samples_per_prompt=n) on the host, before any device work; returns n as an int."""
    if isinstance(n, bool) or int(n) != n or n < 1:
        raise ValueError(f"{who}: `samples_per_prompt`={n!r} has to be an integer >= 1")
    n = int(n)
    if n == 1:
        return n
    if not do_sample:
        raise ValueError(f"{who}: `samples_per_prompt`={n} needs do_sample=True (HF: \"Greedy methods without beam search do not support "
                         f"`num_return_sequences` different than 1\")")
    if batch * n > MAX_GROUP:
        raise ValueError(f"{who}: {batch} prompts x `samples_per_prompt`={n} = {batch * n} sequences exceed the {MAX_GROUP} of one decode group")
    if has_criteria:
        raise ValueError(f"{who}: `samples_per_prompt`={n} cannot be combined with `stopping_criteria` (they are evaluated on one sequence); "
                         f"use `stop_strings`")
    if has_reuse_key:
        raise ValueError(f"{who}: `samples_per_prompt`={n} cannot be combined with `kv_reuse_key` (the kept cache would hold {n} different answers)")
    return n


MAX_LOOKUP, MAX_LOOKUP_NGRAM = 15, 4           # drafts per step / ngram size (pgv_kv_set_lookup)


def check_lookup(lookup, lookup_ngram=2, batch: int = 1, do_sample: bool = False, beams=1, samples_per_prompt=1, repetition_penalty: float = 1.0,
                 has_bans: bool = False, output_logprobs: bool = False, who: str = "generate()", lookup_sample: bool = False) -> Tuple[int, int]:
    """Validate generate(lookup=D, lookup_ngram=n, lookup_sample=) on the host, before any device work; returns (D, n).  D == 0 (or None) is the
    call without the keyword and combines with everything.  Lookup steps verify drafts against the plain pick -- the arg-max, or with
    `lookup_sample` the sampled pick from the uniform the plain run uses for that token -- so whatever else changes the pick is refused.
    `lookup_sample` needs do_sample and a D >= 1; without it do_sample is refused as before."""
    if lookup_sample and not do_sample:
        raise ValueError(f"{who}: `lookup_sample` needs `do_sample` (the greedy form is `lookup` alone)")
    if lookup is None or (not isinstance(lookup, bool) and lookup == 0):
        if lookup_sample:
            raise ValueError(f"{who}: `lookup_sample` needs `lookup` >= 1 drafts per step")
        return 0, 0
    if isinstance(lookup, bool) or int(lookup) != lookup or lookup < 0 or lookup > MAX_LOOKUP:
        raise ValueError(f"{who}: `lookup`={lookup!r} has to be an integer in [0, {MAX_LOOKUP}]")
    if isinstance(lookup_ngram, bool) or int(lookup_ngram) != lookup_ngram or lookup_ngram < 1 or lookup_ngram > MAX_LOOKUP_NGRAM:
        raise ValueError(f"{who}: `lookup_ngram`={lookup_ngram!r} has to be an integer in [1, {MAX_LOOKUP_NGRAM}]")
    D, n = int(lookup), int(lookup_ngram)
    verified = "the plain pick without it" if lookup_sample else "the plain arg-max"
    refused = [("do_sample", bool(do_sample) and not lookup_sample,
                "a sampled token has no draft to verify; speculative sampling is not implemented -- `lookup_sample`=True verifies against the run's own uniforms"),
               ("beams", beams is not None and beams != 1, "a beam step already runs K rows per prompt"),
               ("samples_per_prompt", samples_per_prompt is not None and samples_per_prompt != 1,
                "the samples share no uniforms with a plain run" if lookup_sample else "it needs do_sample"),
               ("repetition_penalty", float(repetition_penalty) != 1.0, f"the drafts are verified against {verified}"),
               ("bans", bool(has_bans), f"the drafts are verified against {verified}"),
               ("output_logprobs", bool(output_logprobs), "lookup steps record no log-probabilities")]
    for name, bad, why in refused:
        if bad:
            raise ValueError(f"{who}: `{name}` cannot be combined with `lookup`={D} ({why})")
    if batch * (1 + D) > MAX_GROUP:
        raise ValueError(f"{who}: {batch} prompts x (1 + `lookup`={D}) = {batch * (1 + D)} rows exceed the {MAX_GROUP} of one decode step")
    return D, n


MAX_BEAMS = 8           # beams per prompt (pgv_beam_config.beams)
HF_BEAM_DEFAULTS = {"length_penalty": 1.0, "early_stopping": False}


def check_beams(beams, batch: int, do_sample: bool = False, samples_per_prompt=1, repetition_penalty: float = 1.0, output_logprobs: bool = False,
                has_criteria: bool = False, has_stop_strings: bool = False, has_reuse_key: bool = False, length_penalty=None, early_stopping=None,
                generation_config=None, who: str = "generate()") -> Tuple[int, float, object]:
    """Validate generate(beams=K, ...) on the host, before any device work.  Returns (K, length_penalty, early_stopping): the latter two from the
    call if given, else from the generation config, else HF's defaults (1.0, False).  K == 1 is greedy decoding and combines with everything."""
    if isinstance(beams, bool) or int(beams) != beams or beams < 1 or beams > MAX_BEAMS:
        raise ValueError(f"{who}: `beams`={beams!r} has to be an integer in [1, {MAX_BEAMS}]")
    K = int(beams)
    if K == 1:              # greedy decoding: the two beam parameters stay inert, as in a call without `beams`
        return K, 1.0, False
    lp = length_penalty if length_penalty is not None else _config_get(generation_config, "length_penalty")
    lp = float(HF_BEAM_DEFAULTS["length_penalty"] if lp is None else lp)
    es = early_stopping if early_stopping is not None else _config_get(generation_config, "early_stopping")
    es = HF_BEAM_DEFAULTS["early_stopping"] if es is None else es
    if not (isinstance(es, bool) or es == "never"):
        raise ValueError(f"{who}: `early_stopping`={es!r} has to be False, True or \"never\"")
    if lp != lp or lp in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: `length_penalty`={lp!r} has to be a finite float")
    refused = [("do_sample", bool(do_sample), "beam search picks by score; HF's beam sampling is not implemented"),
               ("samples_per_prompt", samples_per_prompt is not None and samples_per_prompt != 1, "the K beams of a prompt are its group of slots"),
               ("repetition_penalty", float(repetition_penalty) != 1.0, "the beam pick applies no logits processor"),
               ("output_logprobs", bool(output_logprobs), "a hypothesis' score is returned with `output_beam_scores=True`"),
               ("stopping_criteria", bool(has_criteria), "they are evaluated on one running sequence"),
               ("stop_strings", bool(has_stop_strings), "they cut one running sequence, not a set of hypotheses"),
               ("kv_reuse_key", bool(has_reuse_key), f"the kept cache would hold {K} different beams")]
    for name, bad, why in refused:
        if bad:
            raise ValueError(f"{who}: `{name}` cannot be combined with `beams`={K} ({why})")
    if batch * K > MAX_GROUP:
        raise ValueError(f"{who}: {batch} prompts x `beams`={K} = {batch * K} sequences exceed the {MAX_GROUP} of one decode group")
    return K, lp, es


@dataclass
class GenerateBeamsOutput:
    """What `generate(..., beams=K, output_beam_scores=True)` returns.  sequences: exactly what generate(beams=K) returns without the keyword -- the
    best hypothesis of every prompt, prompt echoed, shorter rows padded.  sequences_scores: fp32 [B] on the host, HF's `sequences_scores` (the sum of
    the hypothesis' token log-probabilities over length ** length_penalty).  new_lengths: int64 [B], the new tokens of every row."""
    sequences: Any
    sequences_scores: Any
    new_lengths: Any = None


def resolve_sampling(temperature=None, top_k=None, top_p=None, repetition_penalty=None, generation_config=None) -> Tuple[float, int, float, float]:
    """(temperature, top_k, top_p, repetition_penalty) of a call: each from the call if given (not None), else from the model's
    generation config, else HF's default -- HF's own precedence.  top_p / repetition_penalty are validated with HF's wording."""
    given = {"temperature": temperature, "top_k": top_k, "top_p": top_p, "repetition_penalty": repetition_penalty}
    out = {}
    for name, v in given.items():
        if v is None:
            v = _config_get(generation_config, name)
        if v is None:
            v = HF_DEFAULTS[name]
        out[name] = v
    t, k, p, r = float(out["temperature"]), int(out["top_k"]), float(out["top_p"]), float(out["repetition_penalty"])
    if not 0.0 < p <= 1.0:
        raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {p}")
    if not r > 0.0:
        raise ValueError(f"`penalty` has to be a strictly positive float, but is {r}")
    return t, k, p, r


@dataclass
class GenerateLogprobsOutput:
    """What `generate(..., output_logprobs=True)` returns.  sequences: exactly what generate() returns without the keyword.  token_logprobs /
    transition_scores: fp32 [B, n_new] on the host, entry i belongs to new token i of the sequence -- the `model` / `pick` values of pgv.h
    (pgv_kv_set_logprobs): HF's compute_transition_scores(sequences, logits / scores, normalize_logits=True).  Both are cut exactly where the ids
    are cut (EOS, stop strings, stopping criteria, budget) and are 0 beyond a sequence's end.  sequence_logprob: fp64 [B], the sums of
    token_logprobs.  new_lengths: int64 [B], the new tokens each sequence kept (`sequences` pads shorter rows to the longest)."""
    sequences: Any
    token_logprobs: Any
    transition_scores: Any
    sequence_logprob: Any
    new_lengths: Any = None

    @classmethod
    def assemble(cls, sequences, n_kept: Sequence[int], model_rows: Sequence, pick_rows: Sequence) -> "GenerateLogprobsOutput":
        """n_kept[b]: new tokens sequence b kept; model_rows[b] / pick_rows[b]: the values of every token the device emitted for it, in
        generation order (at least n_kept[b] of them; the surplus past a cut is dropped)."""
        import numpy as np
        import torch
        B, width = len(n_kept), max([int(n) for n in n_kept], default=0)
        out = np.zeros((2, B, width), dtype=np.float32)
        for b, n in enumerate(n_kept):
            for k, rows in enumerate((model_rows, pick_rows)):
                row = np.asarray(rows[b], dtype=np.float32).reshape(-1)
                if row.size < n:
                    raise ValueError(f"sequence {b} kept {n} tokens but has {row.size} log-probabilities")
                out[k, b, :n] = row[:n]
        return cls(sequences, torch.from_numpy(out[0]), torch.from_numpy(out[1]), torch.from_numpy(out[0].astype(np.float64).sum(axis=1)),
                   torch.tensor([int(n) for n in n_kept], dtype=torch.long))


def step_kwargs(top_p: float, repetition_penalty: float) -> Tuple[dict, dict]:
    """(warp, pen): what the sampled / the greedy step methods of the model take as keywords -- passed on only when they differ from the neutral
    values the methods default to, so a plain call keeps the argument lists it has always had."""
    warp = {} if (top_p == 1.0 and repetition_penalty == 1.0) else {"top_p": top_p, "repetition_penalty": repetition_penalty}
    return warp, ({} if repetition_penalty == 1.0 else {"repetition_penalty": repetition_penalty})


@dataclass(frozen=True)
class CacheSettings:
    """What a KV cache is switched to for the length of ONE call, and the one scope that does it: `apply` (or the prefill, for what it takes)
    switches on what is on, `clear` switches off exactly that.  logprobs: True records log-probabilities (False: `apply` turns the switch off, None
    leaves it).  bans: a checked LogitBans with the `eos_id` its length rules ban; filters: a checked SampleFilters; lookup: (D, n); guidance:
    (scale, pairs), switched on behind the prefill of prompts + negatives (no prefill takes it: its own first token is not a covered pick); allowed:
    a checked allowed.Allowed (automaton, one root per prompt), which also uses `eos_id`.  None: off."""
    logprobs: Optional[bool] = None
    bans: Any = None
    eos_id: int = -1
    filters: Any = None
    lookup: Optional[Tuple[int, int]] = None
    guidance: Optional[Tuple[float, int]] = None
    allowed: Any = None

    def prefill_kwargs(self) -> dict:
        """The keywords of model.prefill that are on: it sets them before the prompt runs, so that the first pick and the id record see them."""
        kw = {"logprobs": True} if self.logprobs else {}
        if self.bans is not None:
            kw.update(bans=self.bans, eos_id=self.eos_id)
        if self.lookup is not None:
            kw.update(lookup=self.lookup)
        if self.allowed is not None:
            kw.update(allowed=self.allowed, eos_id=self.eos_id)
        return kw

    def apply(self, model, kv, prefilled: bool = False):
        """prefilled: `kv` comes from model.prefill(**prefill_kwargs()), which applied those; the filters, which no prefill takes, are left."""
        if not prefilled:
            if self.logprobs is not None:
                model.set_logprobs(kv, self.logprobs)
            if self.bans is not None:
                model.set_bans(kv, self.bans, self.eos_id)
            if self.lookup is not None:
                model.set_lookup(kv, *self.lookup)
            if self.allowed is not None:
                model.set_allowed(kv, self.allowed.automaton, self.allowed.roots, self.eos_id)
        if self.filters is not None:
            model.set_filters(kv, self.filters)
        if self.guidance is not None:
            model.set_guidance(kv, *self.guidance)

    def clear(self, model, kv):
        if self.logprobs:
            model.set_logprobs(kv, False)
        if self.bans is not None:
            model.set_bans(kv, None)
        if self.filters is not None:
            model.set_filters(kv, None)
        if self.lookup is not None:
            model.set_lookup(kv, 0)
        if self.guidance is not None:
            model.set_guidance(kv, 1.0, 0)
        if self.allowed is not None:
            model.set_allowed(kv, None)


@dataclass(frozen=True)
class GenerationPlan:
    """Everything one generate() call derives on the host before it touches the device (plan_generate).  bans / filters: the checked records,
    `bans_on` / `filters_on`: whether they change a pick of this call; lookup: (D, n), (0, 0) off; stops: one stop string per prompt or None;
    chunk: already capped under stopping criteria; max_seq: the cache positions to allocate."""
    do_sample: bool
    temperature: float
    top_k: int
    top_p: float
    repetition_penalty: float
    max_new_tokens: int
    eos_id: int
    chunk: int
    max_seq: int
    beams: int
    length_penalty: float
    early_stopping: Any
    output_beam_scores: bool
    samples_per_prompt: int
    output_logprobs: bool
    bans: LogitBans
    bans_on: bool
    filters: Any
    filters_on: bool
    lookup: Tuple[int, int]
    lookup_sample: bool
    criteria: tuple = ()
    stops: Optional[list] = None
    guidance: Any = None            # the checked guidance.Guidance of a guided call (None: off) and its negatives, one id list per prompt
    negatives: Optional[tuple] = None
    allowed: Any = None             # the checked allowed.Allowed of a constrained call (None: off)

    @property
    def warp(self) -> dict:
        return step_kwargs(self.top_p, self.repetition_penalty)[0]

    @property
    def pen(self) -> dict:
        return step_kwargs(self.top_p, self.repetition_penalty)[1]

    @property
    def settings(self) -> CacheSettings:
        return CacheSettings(True if self.output_logprobs else None, self.bans if self.bans_on else None, self.eos_id,
                             self.filters if self.filters_on else None, self.lookup if self.lookup[0] else None,
                             (self.guidance.scale, len(self.negatives)) if self.guidance is not None else None, self.allowed)


def plan_generate(model, seqs, do_sample=False, temperature=None, max_new_tokens=1024, stopping_criteria=None, eos_token_id="config", chunk=32,
                  top_k=None, stop_strings=None, tokenizer=None, kv_reuse_key=None, top_p=None, repetition_penalty=None, output_logprobs=False,
                  samples_per_prompt=1, beams=1, length_penalty=None, early_stopping=None, output_beam_scores=False, bans=None, filters=None,
                  lookup=0, lookup_ngram=2, lookup_sample=False, unused=None, guidance=None, allowed=None) -> GenerationPlan:
    """The plan of generate(seqs, ...) -- its keywords under their own names, `unused` what fell into **_unused -- or the first ValueError of the
    call: every check in the order generate() has always made them, on the host.  Of `model` only generation_config, config and (under `bans`,
    `allowed` or `guidance`) vocab_size are read."""
    gc, B = model.generation_config, len(seqs)       # `model.config` is read where it is needed: a call refused before that needs none
    check_generate_kwargs(unused or {}, gc, filters_given=filters is not None)
    temperature, top_k, top_p, rep_pen = resolve_sampling(temperature, top_k, top_p, repetition_penalty, gc)
    reuse, sample = kv_reuse_key is not None, bool(do_sample)
    K, length_penalty, early_stopping = check_beams(beams, B, sample, samples_per_prompt, rep_pen, bool(output_logprobs), bool(stopping_criteria),
                                                    stop_strings is not None and any(stop_strings), reuse, length_penalty, early_stopping, gc)
    if output_beam_scores and K == 1:
        raise ValueError("generate(): `output_beam_scores` needs `beams` > 1 (a greedy answer's log-probabilities: `output_logprobs=True`)")
    n_samples = check_samples_per_prompt(samples_per_prompt, B, sample, bool(stopping_criteria), reuse)
    eos = model.config.eos_token_id if eos_token_id == "config" else eos_token_id
    eos_i = -1 if eos is None else int(eos)
    ban = LogitBans() if bans is None else check_bans(bans, model.vocab_size, eos_i, K)       # None: the call as it has always been
    ban_on = not ban.effective_neutral(eos_i)
    look = check_lookup(lookup, lookup_ngram, B, sample, K, n_samples, rep_pen, ban_on, bool(output_logprobs), lookup_sample=bool(lookup_sample))
    filt = check_filters(filters, gc, K)
    allow = None if allowed is None else check_allowed(allowed, B, model.vocab_size, eos_i if eos_i >= 0 else None, K, look[0])      # None: the call as it has always been
    max_seq = max(len(s) for s in seqs) + max_new_tokens
    if max_seq > model.config.max_position_embeddings:
        raise ValueError(f"prompt + max_new_tokens = {max_seq} exceeds max_position_embeddings {model.config.max_position_embeddings}")
    max_seq = (max_seq + 63) // 64 * 64
    criteria, stops = [], None
    if K == 1:              # a beam search takes none of these (check_beams)
        if reuse and B == 1:
            max_seq = min(int(model.config.max_position_embeddings), 4096)      # one cache for the whole conversation: later turns grow into it
        criteria = list(stopping_criteria) if stopping_criteria else []
        if criteria and B != 1:
            raise ValueError("stopping_criteria are evaluated on one sequence (the reference passes them with batch size 1 only)")
        if sample and not float(temperature) > 0.0:
            raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float; use do_sample=False for greedy decoding")
        if criteria:
            chunk = min(chunk, 16)                         # at most 15 surplus steps past a stop string
        stops = list(stop_strings) if stop_strings is not None else None
        if stops is not None:
            if len(stops) != B or tokenizer is None:
                raise ValueError("stop_strings needs one entry per sequence and the tokenizer that decodes them")
            stops = stops if any(stops) else None
    # guidance: after every other check, so that the first error of a faulty call stays what it has always been
    guide = check_guidance(guidance, seqs, None if guidance is None else model.vocab_size, K, look[0], n_samples, reuse, bool(output_logprobs))
    negatives = None
    if guide is not None:
        negatives = tuple(tuple(n) for n in guide.negatives(seqs))
        longest = max(len(n) for n in negatives) + max_new_tokens
        if longest > model.config.max_position_embeddings:
            raise ValueError(f"`guidance` negative + max_new_tokens = {longest} exceeds max_position_embeddings {model.config.max_position_embeddings}")
        max_seq = max(max_seq, (longest + 63) // 64 * 64)
    return GenerationPlan(sample, temperature, top_k, top_p, rep_pen, max_new_tokens, eos_i, chunk, max_seq, K, length_penalty, early_stopping,
                          bool(output_beam_scores), n_samples, bool(output_logprobs), ban, ban_on, filt, sample and not filt.neutral, look,
                          bool(lookup_sample), tuple(criteria), stops, guide, negatives, allow)
