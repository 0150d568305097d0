"""Logit bans: HF's logits processors that set scores to -inf, as this package's `generate(bans=...)` runs them on the device.

HF's generate() arguments `no_repeat_ngram_size`, `bad_words_ids`, `min_length`, `min_new_tokens`, `suppress_tokens` and `begin_suppress_tokens`
become NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
SuppressTokensLogitsProcessor and SuppressTokensAtBeginLogitsProcessor (transformers/generation/logits_process.py).  HF's chain is repetition
penalty, n-gram, bad words, min length, min new tokens, suppress, begin-suppress, and then the warpers.  Every one of the bans writes -inf or nothing,
and -inf * p and -inf / p are -inf for p > 0: their order among themselves and against the penalty does not change the result, so the device applies
them in one kernel between the lm_head and the pick (csrc/logit_ban.hip; include/pgv.h: pgv_kv_set_bans states the same rules).

This module is the host side: the record of what a call asks for (LogitBans), its validation with HF's wording, and the rules in plain Python for
one sequence at one step (banned_ids) -- what the kernel is held to, and what the tests hold against the installed HF.  Pure host code: importable
without a GPU.
"""
from __future__ import annotations

import numbers
from dataclasses import dataclass, fields, replace
from typing import Any, Sequence, Set, Tuple

MAX_IDS, MAX_WORDS, MAX_WORD_LEN = 1024, 256, 16          # PGV_BAN_MAX_IDS / _WORDS / _WORD_LEN of include/pgv.h

# HF generate() argument -> field of LogitBans (the HF names themselves stay refused: generation.REFUSED)
HF_ARGUMENTS = {"no_repeat_ngram_size": "no_repeat_ngram", "bad_words_ids": "bad_words", "min_length": "min_length", "min_new_tokens": "min_new_tokens",
                "suppress_tokens": "suppress", "begin_suppress_tokens": "begin_suppress"}


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)          # numpy integers included


@dataclass(frozen=True)
class LogitBans:
    """What `generate(bans=...)` asks for.  no_repeat_ngram: HF's no_repeat_ngram_size (0: off).  bad_words: HF's bad_words_ids, a list of id
    lists.  suppress / begin_suppress: HF's suppress_tokens / begin_suppress_tokens.  min_length / min_new_tokens: HF's (0: off)."""
    no_repeat_ngram: int = 0
    bad_words: Sequence[Sequence[int]] = ()
    suppress: Sequence[int] = ()
    begin_suppress: Sequence[int] = ()
    min_length: int = 0
    min_new_tokens: int = 0

    @classmethod
    def coerce(cls, bans: Any) -> "LogitBans":
        """None -> the neutral record; a dict -> LogitBans(**dict); a LogitBans stays."""
        if bans is None:
            return cls()
        if isinstance(bans, cls):
            return bans
        if isinstance(bans, dict):
            known = {f.name for f in fields(cls)}
            for k in bans:
                if k not in known:
                    hint = f" (HF's `{k}` is `{HF_ARGUMENTS[k]}` here)" if k in HF_ARGUMENTS else ""
                    raise ValueError(f"`bans` has no field `{k}`{hint}; fields: {', '.join(sorted(known))}")
            return cls(**bans)
        raise ValueError(f"`bans` has to be a LogitBans, a dict of its fields or None, but is {bans!r}")

    @property
    def neutral(self) -> bool:
        """True when nothing is asked: the call is the call without `bans`."""
        return (self.no_repeat_ngram == 0 and len(self.bad_words) == 0 and len(self.suppress) == 0 and len(self.begin_suppress) == 0
                and self.min_length == 0 and self.min_new_tokens == 0)

    def check(self, vocab: int, eos: int = -1) -> "LogitBans":
        """Validate with HF's wording where HF has one, apply HF's EOS filter to the bad words (NoBadWordsLogitsProcessor.__init__ drops a word
        equal to [eos]) and return the record the device takes: plain ints, lists as tuples.  `eos` < 0 / None: no EOS."""
        eos = -1 if eos is None else int(eos)
        n = self.no_repeat_ngram
        # 0 is this package's `off` (HF builds no processor for None / 0); anything else goes through HF's constructor check
        if not _is_int(n) or n < 0:
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {n}")
        for name in ("min_length", "min_new_tokens"):
            v = getattr(self, name)
            if not _is_int(v) or v < 0:
                word = "non-negative" if name == "min_length" else "positive"
                raise ValueError(f"`{name}` has to be a {word} integer, but is {v}")
        words = self.bad_words
        if words is None or (not isinstance(words, (list, tuple))):
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {words}.")
        if any(not isinstance(w, (list, tuple)) for w in words):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {words}.")
        if any(len(w) == 0 or any((not _is_int(t) or t < 0) for t in w) for w in words):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {words}.")
        words = tuple(tuple(int(t) for t in w) for w in words)
        if eos >= 0:
            words = tuple(w for w in words if w != (eos,))
        lists = {}
        for name in ("suppress", "begin_suppress"):
            v = getattr(self, name)
            if not isinstance(v, (list, tuple)) or any((not _is_int(t) or t < 0) for t in v):
                raise ValueError(f"`{name}` has to be a list of non-negative integers, but is {v}")
            lists[name] = tuple(int(t) for t in v)
        invalid = [t for w in words for t in w if t >= vocab]
        if invalid:           # SequenceBiasLogitsProcessor._prepare_bias_variables
            raise ValueError(f"The model vocabulary size is {vocab}, but the following tokens were being biased: {invalid}")
        for name, v in lists.items():
            bad = [t for t in v if t >= vocab]
            if bad:
                raise ValueError(f"The model vocabulary size is {vocab}, but `{name}` lists the tokens {bad}")
        if len(words) > MAX_WORDS:
            raise ValueError(f"`bad_words`: {len(words)} words exceed the limit of {MAX_WORDS}")
        long = [len(w) for w in words if len(w) > MAX_WORD_LEN]
        if long:
            raise ValueError(f"`bad_words`: a word of {long[0]} ids exceeds the limit of {MAX_WORD_LEN}")
        total = sum(len(w) for w in words) + len(lists["suppress"]) + len(lists["begin_suppress"])
        if total > MAX_IDS:
            raise ValueError(f"`bans` lists {total} ids in total, the limit is {MAX_IDS}")
        return replace(self, no_repeat_ngram=int(n), bad_words=words, suppress=lists["suppress"], begin_suppress=lists["begin_suppress"],
                       min_length=int(self.min_length), min_new_tokens=int(self.min_new_tokens))

    def effective_neutral(self, eos: int = -1) -> bool:
        """`neutral`, or only length rules in a run without EOS (which makes both empty)."""
        eos = -1 if eos is None else int(eos)
        return self.neutral or (eos < 0 and replace(self, min_length=0, min_new_tokens=0).neutral)


def check_bans(bans: Any, vocab: int, eos, beams: int = 1, who: str = "generate()") -> LogitBans:
    """Validate generate(bans=...) on the host, before any device work; returns the checked record (neutral for None)."""
    b = LogitBans.coerce(bans).check(vocab, eos)
    if beams is not None and beams > 1 and not b.effective_neutral(eos):
        raise ValueError(f"{who}: `bans` cannot be combined with `beams`={int(beams)} (the beam pick applies no logits processor; each beam's "
                         f"sequence would have to be rebuilt from the parent history)")
    return b


def banned_ids(bans: LogitBans, input_ids: Sequence[int], prompt_len: int, eos: int, vocab: int) -> Set[int]:
    """The ids whose scores HF's processors set to -inf for ONE sequence at ONE step: `input_ids` is everything the model has seen (prompt as
    handed to generate(), placeholder ids included, plus the tokens generated so far), `prompt_len` the length it was prefilled with."""
    ids = [int(t) for t in input_ids]
    L = len(ids)
    eos = -1 if eos is None else int(eos)
    out: Set[int] = set()
    n = int(bans.no_repeat_ngram)
    if n > 0 and L >= n:
        # NoRepeatNGramLogitsProcessor: every earlier n-gram that starts with the last n - 1 ids bans its last id (the suffix has no successor yet)
        suffix = ids[L - n + 1:L]
        for j in range(0, L - n + 1):
            if ids[j:j + n - 1] == suffix:
                out.add(ids[j + n - 1])
    for w in bans.bad_words:
        w = [int(t) for t in w]
        m = len(w)
        if m == 1:
            out.add(w[0])
        elif 1 < m <= L and ids[L - m + 1:L] == w[:-1]:
            out.add(w[-1])
    out.update(int(t) for t in bans.suppress)
    if L == prompt_len:
        out.update(int(t) for t in bans.begin_suppress)
    if eos >= 0 and (L < bans.min_length or L - prompt_len < bans.min_new_tokens):
        out.add(eos)
    return {t for t in out if 0 <= t < vocab}


def apply_bans(bans: LogitBans, scores, input_ids: Sequence[int], prompt_len: int, eos: int):
    """`scores` (a 1-D numpy array or torch tensor over the vocabulary) with -inf at banned_ids: a copy."""
    out = scores.copy() if hasattr(scores, "copy") else scores.clone()
    idx = sorted(banned_ids(bans, input_ids, prompt_len, eos, int(out.shape[-1])))
    if idx:
        out[idx] = float("-inf")
    return out
