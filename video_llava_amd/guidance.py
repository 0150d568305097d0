"""Classifier-free guidance: HF's UnbatchedClassifierFreeGuidanceLogitsProcessor, as this package's `generate(guidance=...)` runs it on the device.

HF's generate(guidance_scale=s, negative_prompt_ids=...) runs the model a second time on a negative prompt and hands the rest of its chain

    guided = s * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond)

(transformers/generation/logits_process.py; the first processor GenerationMixin._get_logits_processor builds, so the repetition penalty, the bans
and the warpers all see the guided scores).  Here the unconditional stream is B more rows of the same decode group: the negatives are prefilled
with the prompts as one ragged batch of 2B rows, every token step runs both, and a kernel between the lm_head and the pick mixes each pair
(csrc/guidance.hip; include/pgv.h: pgv_kv_set_guidance states the same rule).  For a video LLM the natural negative is the same question WITHOUT
the video: contrast decoding against the language prior.

This module is the host side: the record of what a call asks for (Guidance), its validation, the negatives of a batch, and the rule in fp64
numpy (guided_scores) -- what the kernel is held to, and what the tests hold against the installed HF.  Pure host code: importable without a GPU.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

MAX_PAIRS = 32              # a decode group holds 64 sequences: 32 prompts and their 32 twins

# HF generate() argument -> field of Guidance (the HF names themselves are not arguments of this package's generate())
HF_ARGUMENTS = {"guidance_scale": "scale", "negative_prompt_ids": "negative"}


@dataclass(frozen=True)
class Guidance:
    """What `generate(guidance=...)` asks for.  scale: HF's guidance_scale (1: off; > 1 pushes towards the prompt, 0 picks from the negative alone).
    negative: None or "last_token" -- HF's default, each prompt's last id on its own -- or one id list per prompt (HF's negative_prompt_ids, ragged).
    negative_feats: pooled video features [B, V, C] for negatives that carry a video placeholder run; None: the call's own features."""
    scale: float = 1.0
    negative: Any = None
    negative_feats: Any = None

    @classmethod
    def coerce(cls, guidance: Any) -> "Guidance":
        """None -> the neutral record; a number -> Guidance(scale); a dict -> Guidance(**dict); a Guidance stays."""
        if guidance is None:
            return cls()
        if isinstance(guidance, cls):
            return guidance
        if isinstance(guidance, numbers.Real) and not isinstance(guidance, bool):
            return cls(float(guidance))
        if isinstance(guidance, dict):
            known = ("scale", "negative", "negative_feats")
            for k in guidance:
                if k not in known:
                    hint = f" (HF's `{k}` is `{HF_ARGUMENTS[k]}` here)" if k in HF_ARGUMENTS else ""
                    raise ValueError(f"`guidance` has no field `{k}`{hint}; fields: {', '.join(known)}")
            return cls(**guidance)
        raise ValueError(f"`guidance` has to be a Guidance, a scale, a dict of its fields or None, but is {guidance!r}")

    @property
    def neutral(self) -> bool:
        """True when nothing is asked: the call is the call without `guidance` (HF builds the processor only for a scale other than 1)."""
        return isinstance(self.scale, numbers.Real) and not isinstance(self.scale, bool) and float(self.scale) == 1.0

    def negatives(self, seqs: Sequence[Sequence[int]]) -> List[List[int]]:
        """The negative prompt of every sequence: its last id ("last_token" / None), or the ids given."""
        if self.negative is None or (isinstance(self.negative, str) and self.negative == "last_token"):
            return [[int(s[-1])] for s in seqs]
        return [[int(t) for t in n] for n in self.negative]


def check_guidance(guidance, seqs: Sequence[Sequence[int]], vocab: Optional[int] = None, beams=1, lookup=0, samples_per_prompt=1,
                   has_reuse_key: bool = False, output_logprobs: bool = False, who: str = "generate()") -> Optional[Guidance]:
    """Validate generate(guidance=...) on the host, before any device work; returns the record, or None for a neutral one (None, scale 1), which
    is the call without the keyword and combines with everything.  Everything that is a pick on a row combines with guidance (sampling,
    temperature, top_k, top_p, filters, repetition_penalty, bans, stop strings, stopping criteria); what moves, multiplies or re-reads slots does not."""
    g = Guidance.coerce(guidance)
    s = g.scale
    if not isinstance(s, numbers.Real) or isinstance(s, bool) or not math.isfinite(float(s)):
        raise ValueError(f"{who}: `guidance` scale has to be a finite float, but is {s!r}")
    if float(s) == 1.0:
        return None
    B, scale = len(seqs), float(s)
    neg = g.negative
    if not (neg is None or (isinstance(neg, str) and neg == "last_token")):
        if isinstance(neg, str) or not isinstance(neg, (list, tuple)) or len(neg) != B:
            raise ValueError(f"{who}: `guidance` negative has to be None, \"last_token\" or one id list per prompt ({B}), but is {neg!r}")
        for b, n in enumerate(neg):
            if not isinstance(n, (list, tuple)) or len(n) < 1:
                raise ValueError(f"{who}: `guidance` negative {b} has to be a non-empty id list, but is {n!r}")
            for t in n:
                if not isinstance(t, numbers.Integral) or isinstance(t, bool) or t < 0 or (vocab is not None and t >= vocab):
                    raise ValueError(f"{who}: `guidance` negative {b} holds {t!r}: not a token id" + (f" below the vocabulary size {vocab}" if vocab is not None else ""))
    refused = [("beams", beams is not None and beams != 1, "a beam step already runs K rows per prompt and applies no logits processor"),
               ("lookup", lookup is not None and lookup != 0, "the drafts are verified against the unguided pick"),
               ("samples_per_prompt", samples_per_prompt is not None and samples_per_prompt != 1, "a fork would separate the twins from their prompts"),
               ("kv_reuse_key", bool(has_reuse_key), "the kept cache would hold the negative prompt's rows as well"),
               ("output_logprobs", bool(output_logprobs), "a guided pick records no log-probabilities")]
    for name, bad, why in refused:
        if bad:
            raise ValueError(f"{who}: `{name}` cannot be combined with `guidance` scale {scale:g} ({why})")
    if B > MAX_PAIRS:
        raise ValueError(f"{who}: {B} prompts under `guidance` need {2 * B} sequences, beyond the {2 * MAX_PAIRS} of one decode group")
    return Guidance(scale, neg, g.negative_feats)


def stack_features(feats, negative_feats, negatives: Sequence[Sequence[int]], patch_token: Optional[int]):
    """The features of the 2B rows of a guided prefill, [2B, V, C]: rows [0, B) the call's, row B + b those of negative b -- `negative_feats[b]` (None:
    the call's own) when it carries a video placeholder run, zeros for a text-only negative (the splice never reads them).  None stays None."""
    import torch
    if feats is None:
        return None
    B = len(negatives)
    f = feats.unsqueeze(0) if feats.dim() == 2 else feats
    if f.shape[0] != B:
        raise ValueError(f"{f.shape[0]} video feature sets for {B} prompts")
    nf = f if negative_feats is None else (negative_feats.unsqueeze(0) if negative_feats.dim() == 2 else negative_feats)
    if tuple(nf.shape) != tuple(f.shape):
        raise ValueError(f"`guidance` negative_feats of shape {tuple(nf.shape)} for features of shape {tuple(f.shape)}")
    has_video = torch.tensor([patch_token is not None and patch_token in n for n in negatives], dtype=torch.bool, device=f.device)
    neg = torch.where(has_video[:, None, None], nf.to(device=f.device, dtype=f.dtype), torch.zeros_like(f))
    return torch.cat([f, neg], dim=0)


def guided_scores(cond, uncond, scale: float):
    """The rule in fp64 numpy: cond / uncond [..., V] logits -> scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond).  -inf entries
    follow IEEE arithmetic, as HF's tensors do: -inf in cond gives -inf for scale > 0 and NaN for scale 0."""
    import numpy as np

    def log_softmax(x):
        x = np.asarray(x, dtype=np.float64)
        m = np.max(x, axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (x - m) - np.log(np.sum(np.exp(x - m), axis=-1, keepdims=True))

    lc, lu = log_softmax(cond), log_softmax(uncond)
    with np.errstate(invalid="ignore"):
        return float(scale) * (lc - lu) + lu
