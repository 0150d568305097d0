"""Teacher-forced scoring, host side: HF's label shift and the bookkeeping around the per-row numbers pgv_llm_score returns.

The reference computes one number from `forward(labels=...)` (video_chatgpt/model/video_chatgpt.py:228-239): logits and labels shifted by one,
flattened, `CrossEntropyLoss()` -- the mean of -log P(labels[p] | ids[:p]) over every position whose label is not -100.  `forward(labels=)` stays
refused here (it belongs to the training path); `VideoChatGPTLlamaForCausalLM.score()` gives the same number and its per-token terms.

Pure host code: importable without a GPU, like generation.py.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence

import numpy as np
import torch

IGNORE_INDEX = -100         # CrossEntropyLoss's default ignore_index, what the reference's labels carry on unscored positions


def id_rows(x) -> List[List[int]]:
    """A [B, S] / [S] tensor or a ragged list of id sequences -> list of int lists."""
    if torch.is_tensor(x):
        x = x.cpu()
        return [row.tolist() for row in (x[None] if x.dim() == 1 else x)]
    return [[int(t) for t in (row.tolist() if hasattr(row, "tolist") else row)] for row in x]


def shift_labels(seqs, labels) -> np.ndarray:
    """HF's shift (:234-235) on a ragged batch -> flat int32 targets [sum of lengths], one per row of the concatenated batch: row p of a
    sequence is scored iff p + 1 < len and labels[p + 1] != -100, and its target is labels[p + 1]; every other row gets -1."""
    seqs, labels = id_rows(seqs), id_rows(labels)
    if len(seqs) != len(labels):
        raise ValueError(f"{len(labels)} label rows for {len(seqs)} sequences")
    out = []
    for b, (s, l) in enumerate(zip(seqs, labels)):
        if len(s) != len(l):
            raise ValueError(f"sequence {b}: {len(l)} labels for {len(s)} tokens")
        t = np.full(len(s), -1, dtype=np.int32)
        if len(s) > 1:
            nxt = np.asarray(l[1:], dtype=np.int64)
            if ((nxt < 0) & (nxt != IGNORE_INDEX)).any():
                raise ValueError(f"sequence {b}: negative labels other than {IGNORE_INDEX}")
            t[:-1] = np.where(nxt == IGNORE_INDEX, -1, nxt)
        out.append(t)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int32)


def continuation_labels(prompt_ids: Sequence[int], full_ids: Sequence[int]) -> List[int]:
    """Labels that score only what follows the prompt: -100 on the first len(prompt_ids) positions, the ids themselves behind them.  Raises
    if `prompt_ids` is not a prefix of `full_ids` (a tokenizer that merges across the boundary would silently score the wrong span)."""
    prompt_ids, full_ids = [int(t) for t in prompt_ids], [int(t) for t in full_ids]
    n = len(prompt_ids)
    if len(full_ids) < n or full_ids[:n] != prompt_ids:
        raise ValueError("continuation_labels: the prompt's ids are not a prefix of the full sequence's ids (the tokenizer merged across the boundary)")
    return [IGNORE_INDEX] * n + full_ids[n:]


@dataclasses.dataclass
class ScoreOutput:
    """What score() returns.  Per sequence b, aligned with its labels: token_logprobs[b][p] = log P(labels[p] | ids[:p]) (fp32; 0 where unscored),
    scored[b][p] = position p was scored, argmax[b][p] = the model's greedy token for position p (-1 where unscored).  sequence_logprob [B] =
    fp64 sums of the fp32 per-token values, counts [B] = scored positions, loss = -sum / count over the whole batch: CrossEntropyLoss's mean as
    the reference computes it (video_chatgpt/model/video_chatgpt.py:231-239; nan when nothing is scored, as torch).  All tensors are on the host.
    `kv`: the cache handle the call filled (a live group, as after prefill())."""
    token_logprobs: List[torch.Tensor]
    scored: List[torch.Tensor]
    argmax: List[torch.Tensor]
    sequence_logprob: torch.Tensor
    counts: torch.Tensor
    loss: float
    kv: Optional[object] = None

    @classmethod
    def from_rows(cls, lens: Sequence[int], targets: np.ndarray, logprob: np.ndarray, argmax: np.ndarray, kv=None) -> "ScoreOutput":
        """From per-ROW arrays [sum of lens] (row p predicts position p + 1): the flat targets of shift_labels and the library's results."""
        targets, logprob, argmax = np.asarray(targets), np.asarray(logprob, dtype=np.float32), np.asarray(argmax, dtype=np.int32)
        if not (targets.shape == logprob.shape == argmax.shape == (int(sum(lens)),)):
            raise ValueError("from_rows: arrays must hold one entry per row of the concatenated batch")
        lp, sc, am, sums, counts = [], [], [], [], []
        off = 0
        for n in lens:
            t = torch.zeros(n, dtype=torch.float32)
            m = torch.zeros(n, dtype=torch.bool)
            a = torch.full((n,), -1, dtype=torch.int32)
            on = targets[off:off + n - 1] >= 0 if n > 1 else np.zeros(0, dtype=bool)
            if n > 1:
                m[1:] = torch.from_numpy(on)
                t[1:] = torch.from_numpy(np.where(on, logprob[off:off + n - 1], np.float32(0)).astype(np.float32))
                a[1:] = torch.from_numpy(np.where(on, argmax[off:off + n - 1], -1).astype(np.int32))
            lp.append(t); sc.append(m); am.append(a)
            sums.append(float(t[m].double().sum()))
            counts.append(int(m.sum()))
            off += n
        total = int(sum(counts))
        loss = -float(np.sum(np.asarray(sums, dtype=np.float64))) / total if total else float("nan")
        return cls(lp, sc, am, torch.tensor(sums, dtype=torch.float64), torch.tensor(counts, dtype=torch.int64), loss, kv)
