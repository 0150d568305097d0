"""Prompt-lookup drafting as pure host functions (numpy only): the rule of HF's `PromptLookupCandidateGenerator.get_candidates`
(transformers/generation/candidate_generator.py; `generate(prompt_lookup_num_tokens=D, max_matching_ngram_size=n)`) and the step-by-step trace a
greedy answer takes under it.  This is the reference a drafting kernel has to reproduce; nothing on the product path imports it."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np


def lookup_candidates(ids: Sequence[int], D: int, n: int, eos: Optional[int] = None) -> List[int]:
    """The draft tokens for the sequence `ids` (prompt + answer so far, length L): for ngram size min(n, L - 1) down to 1, the LEFTMOST window equal
    to the last ngram whose continuation [idx + ngram, min(idx + ngram + D, L)) is not empty; that continuation, cut before its first `eos`.
    The search stops at the first such window even when the cut leaves nothing (HF does the same).  No match: []."""
    a = np.asarray(ids, dtype=np.int64).reshape(-1)
    L = int(a.size)
    if D < 1 or n < 1:
        raise ValueError("lookup_candidates: D and n must be positive")
    for g in range(min(n, L - 1), 0, -1):
        win = np.lib.stride_tricks.sliding_window_view(a, g)            # [L - g + 1, g]
        for idx in np.nonzero((win == a[L - g:]).all(axis=1))[0].tolist():
            start, end = idx + g, min(idx + g + D, L)
            if start < end:
                out = a[start:end].tolist()
                if eos is not None and eos in out:
                    out = out[:out.index(eos)]
                return out
    return []


def lookup_trace(prompt: Sequence[int], answer: Sequence[int], D: int, n: int, eos: Optional[int], budget: int) -> List[int]:
    """Emit count of every lookup step that reproduces the greedy `answer` after `prompt`.

    `prompt`: every id the model has consumed or is about to consume -- the prompt plus the first picked token as its last entry; `answer`: the
    plain greedy tokens that follow it (at least `budget` of them unless an `eos` ends it earlier).  A step drafts `lookup_candidates` of the
    sequence so far, at most budget - emitted - 1 of them; the model's tokens behind the current token and behind every draft are answer[e], answer[e + 1],
    ...; the step emits the token behind the current one and one more per leading draft that equals the token in front of it, stops behind an
    `eos` and at the budget.  The counts sum to the length of `answer` cut behind its first `eos` or at `budget`."""
    seq = [int(t) for t in prompt]
    ans = [int(t) for t in answer]
    counts: List[int] = []
    e = 0
    while e < budget:
        drafts = lookup_candidates(seq, D, n, eos)[:max(0, budget - e - 1)]
        a = 0
        while a < len(drafts) and e + a < len(ans) and drafts[a] == ans[e + a]:
            a += 1
        emit = ans[e:e + a + 1]
        if len(emit) != a + 1:
            raise ValueError("lookup_trace: the answer is shorter than the budget and holds no eos")
        if eos is not None and eos in emit:
            emit = emit[:emit.index(eos) + 1]
        counts.append(len(emit))
        seq += emit
        e += len(emit)
        if eos is not None and emit[-1] == eos:
            break
    return counts
