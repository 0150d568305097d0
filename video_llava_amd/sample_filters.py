"""Sample filters: HF's four remaining sampling warpers, as this package's `generate(filters=...)` runs them inside the device pick.

HF's generate() arguments `min_p`, `typical_p`, `epsilon_cutoff` and `eta_cutoff` become MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper
and EtaLogitsWarper (transformers/generation/logits_process.py).  In HF's sampled chain they form one tail behind top-p:

    repetition penalty -> temperature -> top-k -> top-p -> min_p -> typical_p -> epsilon_cutoff -> eta_cutoff -> softmax -> multinomial

Each stage recomputes the softmax over what the stage before left and keeps the largest CURRENT survivor (HF's min_tokens_to_keep = 1).  The typical
stage keeps a band in the logit, not a threshold: it routinely removes the row's largest logit, and "the top" of the two stages behind it is the
largest logit that is still there.  include/pgv.h (pgv_kv_set_filters) states the same rules; csrc/sampling.hip runs them.

This module is the host side: the record of what a call asks for (SampleFilters), its validation with HF's wording, the precedence over a
checkpoint's generation config, and the rules in fp64 numpy for one row (filter_chain) -- what the kernel is held to, and what the tests hold against
the installed HF.  Pure host code: importable without a GPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Any, Optional

# field of SampleFilters == HF's generate() argument and generation_config field (the HF arguments themselves stay refused: generation.REFUSED)
HF_ARGUMENTS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
NEUTRAL = {"min_p": None, "typical_p": 1.0, "epsilon_cutoff": 0.0, "eta_cutoff": 0.0}


def _number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) or (hasattr(v, "dtype") and getattr(v, "ndim", 1) == 0)


@dataclass(frozen=True)
class SampleFilters:
    """What `generate(filters=...)` asks for, under HF's names.  min_p: None or 0 is off.  typical_p: 1 is off.  epsilon_cutoff / eta_cutoff: 0 is
    off."""
    min_p: Optional[float] = None
    typical_p: float = 1.0
    epsilon_cutoff: float = 0.0
    eta_cutoff: float = 0.0

    @classmethod
    def coerce(cls, filters: Any) -> "SampleFilters":
        """None -> the neutral record; a dict -> SampleFilters(**dict); a SampleFilters stays."""
        if filters is None:
            return cls()
        if isinstance(filters, cls):
            return filters
        if isinstance(filters, dict):
            known = {f.name for f in fields(cls)}
            for k in filters:
                if k not in known:
                    raise ValueError(f"`filters` has no field `{k}`; fields: {', '.join(sorted(known))}")
            return cls(**filters)
        raise ValueError(f"`filters` has to be a SampleFilters, a dict of its fields or None, but is {filters!r}")

    @property
    def neutral(self) -> bool:
        """True when nothing is asked: the call is the call without `filters`."""
        return ((self.min_p is None or self.min_p == 0) and self.typical_p is not None and self.typical_p == 1 and self.epsilon_cutoff == 0
                and self.eta_cutoff == 0)

    def check(self) -> "SampleFilters":
        """Validate with HF's wording (the constructors of the four warper classes) and return the record the device takes: plain floats.  The
        neutral values are this package's: HF's generate() builds no warper for them, and its constructors refuse typical_p = 1 and a cutoff of 0."""
        m = self.min_p
        if m is not None and not (_number(m) and 0 <= m <= 1.0):
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {m}")
        t = self.typical_p
        if not (_number(t) and 0 < t <= 1):
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {t}")
        for name in ("epsilon_cutoff", "eta_cutoff"):
            v = getattr(self, name)
            if not (_number(v) and 0 <= v < 1):
                raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
        return SampleFilters(None if m is None else float(m), float(t), float(self.epsilon_cutoff), float(self.eta_cutoff))


def resolve_filters(filters: Any = None, generation_config=None) -> SampleFilters:
    """The checked record of a call.  `filters` None: neutral, whatever the generation config holds (its four fields are then refused by
    generation.check_generate_kwargs, as they have always been).  Otherwise each field comes from the call if given -- a key of a dict, or a field
    of a record that differs from its neutral default -- else from the model's generation config under HF's name, else it is neutral: the
    precedence of generation.resolve_sampling."""
    if filters is None:
        return SampleFilters()
    given = dict(filters) if isinstance(filters, dict) else None
    rec = SampleFilters.coerce(filters)
    out = {}
    for name in HF_ARGUMENTS:
        v = getattr(rec, name)
        is_given = (name in given) if given is not None else (v != NEUTRAL[name])
        if not is_given and generation_config is not None:
            c = generation_config.get(name) if isinstance(generation_config, dict) else getattr(generation_config, name, None)
            if c is not None:
                v = c
        out[name] = NEUTRAL[name] if v is None else v
    return SampleFilters(**out).check()


def check_filters(filters: Any, generation_config=None, beams: int = 1, who: str = "generate()") -> SampleFilters:
    """Validate generate(filters=...) on the host, before any device work; returns the checked record (neutral for None)."""
    f = resolve_filters(filters, generation_config)
    if beams is not None and beams > 1 and not f.neutral:
        raise ValueError(f"{who}: `filters` cannot be combined with `beams`={int(beams)} (beam search picks by score; the sampling warpers apply to "
                         f"sampled picks only)")
    return f


def filter_chain(scores_row, filters: SampleFilters, rel: float = 0.0, dH: float = 0.0, dmass: float = 0.0):
    """The kept mask (numpy bool [V]) of ONE row after HF's min_p -> typical_p -> epsilon_cutoff -> eta_cutoff, in fp64.  `scores_row`: the scores
    after repetition penalty / temperature / top-k / top-p, -inf (or NaN) where removed.  The three perturbations move every decision boundary a
    little, for callers that have to know which rows a rounding error can change: `rel` scales the probability thresholds by (1 + rel), `dH` is
    added to the entropies, `dmass` to the typical mass."""
    import numpy as np
    y = np.asarray(scores_row, dtype=np.float64).reshape(-1)
    keep = np.isfinite(y)

    def softmax(keep):
        e = np.zeros_like(y)
        e[keep] = np.exp(y[keep] - y[keep].max())
        return e / e.sum()

    def entropy(p):
        q = p[p > 0]
        return float(-(q * np.log(q)).sum()) + dH

    def top(keep):
        return keep & (y == y[keep].max())

    if filters.min_p is not None and filters.min_p > 0 and keep.any():
        p = softmax(keep)
        keep = (keep & (p >= filters.min_p * (1.0 + rel) * p.max())) | top(keep)
    if filters.typical_p < 1 and keep.any():
        p = softmax(keep)
        H = entropy(p)
        idx = np.flatnonzero(keep)
        with np.errstate(divide="ignore"):
            d = np.abs(-np.log(p[idx]) - H)
        order = np.argsort(d, kind="stable")
        cum = np.cumsum(p[idx][order])
        last = min(int((cum < filters.typical_p + dmass).sum()), idx.size - 1)
        band = np.zeros_like(keep)
        band[idx[d <= d[order][last]]] = True
        keep = band
    if filters.epsilon_cutoff > 0 and keep.any():
        p = softmax(keep)
        keep = (keep & (p >= filters.epsilon_cutoff * (1.0 + rel))) | top(keep)
    if filters.eta_cutoff > 0 and keep.any():
        p = softmax(keep)
        eta = min(filters.eta_cutoff, math.sqrt(filters.eta_cutoff) * math.exp(-entropy(p)))
        keep = (keep & (p >= eta * (1.0 + rel))) | top(keep)
    return keep
