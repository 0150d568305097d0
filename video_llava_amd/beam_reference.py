"""The beam-search rules of this package, restated in numpy (host only, no GPU, no torch).

These are steps b-g of HF's `GenerationMixin._beam_search` (transformers 5) for one prompt, with the one thing HF leaves open -- the order of
equal scores inside torch.topk -- fixed: higher score first, then the lower index.  include/pgv.h (pgv_beam_begin) states the same rules for the
device kernel (csrc/beam.hip), tests/test_beam_cpu.py checks this file against HF itself, the GPU tests check the kernel against this file.
All arithmetic is fp32, as on the device; only ln sum exp, which the device takes from its row-statistics kernel, is computed in fp64 and rounded.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

NEG = np.float32(-1.0e9)
F32 = np.float32


def early_code(early_stopping) -> int:
    """False / True / "never" (HF's three values; 0 / 1 / 2 pass through) -> the code of pgv_beam_config."""
    if isinstance(early_stopping, str):
        if early_stopping != "never":
            raise ValueError(f"`early_stopping`={early_stopping!r} has to be False, True or \"never\"")
        return 2
    if isinstance(early_stopping, (bool, np.bool_)):
        return 1 if early_stopping else 0
    if early_stopping in (0, 1, 2):
        return int(early_stopping)
    raise ValueError(f"`early_stopping`={early_stopping!r} has to be False, True or \"never\"")


def state_words(K: int) -> int:
    """PGV_BEAM_STATE_WORDS(K)."""
    return 6 * K + 2


@dataclass
class BeamState:
    """The state of one prompt (the state words of pgv.h, field by field)."""
    K: int
    run: np.ndarray = None            # [K] f32 running scores
    fin_score: np.ndarray = None      # [K] f32, best first
    fin_len: np.ndarray = None        # [K] tokens of the hypothesis (0: none)
    fin_parent: np.ndarray = None     # [K] the beam its last token continued
    fin_tok: np.ndarray = None        # [K] its last token
    fin_flag: np.ndarray = None       # [K]
    unsat: bool = True
    open: bool = True

    def __post_init__(self):
        K = self.K
        if self.run is None:
            self.run = np.full(K, NEG, dtype=F32)
            self.run[0] = 0
            self.fin_score = np.full(K, NEG, dtype=F32)
            self.fin_len = np.zeros(K, dtype=np.int32)
            self.fin_parent = np.zeros(K, dtype=np.int32)
            self.fin_tok = np.zeros(K, dtype=np.int32)
            self.fin_flag = np.zeros(K, dtype=np.int32)

    def to_words(self) -> np.ndarray:
        K = self.K
        w = np.zeros(state_words(K), dtype=np.uint32)
        w[0:K] = self.run.astype(F32).view(np.uint32)
        w[K:2 * K] = self.fin_score.astype(F32).view(np.uint32)
        w[2 * K:3 * K] = self.fin_len.astype(np.int32).view(np.uint32)
        w[3 * K:4 * K] = self.fin_parent.astype(np.int32).view(np.uint32)
        w[4 * K:5 * K] = self.fin_tok.astype(np.int32).view(np.uint32)
        w[5 * K:6 * K] = self.fin_flag.astype(np.int32).view(np.uint32)
        w[6 * K] = 1 if self.unsat else 0
        w[6 * K + 1] = 1 if self.open else 0
        return w

    @classmethod
    def from_words(cls, w: np.ndarray, K: int) -> "BeamState":
        w = np.ascontiguousarray(w).view(np.uint32).reshape(-1)
        return cls(K, w[0:K].view(F32).copy(), w[K:2 * K].view(F32).copy(), w[2 * K:3 * K].view(np.int32).copy(), w[3 * K:4 * K].view(np.int32).copy(),
                   w[4 * K:5 * K].view(np.int32).copy(), w[5 * K:6 * K].view(np.int32).copy(), bool(w[6 * K]), bool(w[6 * K + 1]))


def denom(length: int, length_penalty: float) -> np.float32:
    """length ** length_penalty as HF divides by it: a Python float, rounded to fp32 by the division."""
    return F32(float(length) ** float(length_penalty))


def log_probs(logits: np.ndarray) -> np.ndarray:
    """Step b without the running scores: (x - max) - ln sum exp(x - max) per row, fp32."""
    x = np.asarray(logits, dtype=F32)
    finite = np.where(np.isnan(x), -np.inf, x)
    m = finite.max(axis=1, keepdims=True).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - m).astype(F32)
        ls = np.log(np.exp(d.astype(np.float64)).sum(axis=1, keepdims=True)).astype(F32)
        return ((d - ls).astype(F32))


def _gaps(scores: np.ndarray, first: int) -> float:
    """The smallest gap between neighbours among the `first` best of `scores`, entries pushed down by NEG left out (they are never chosen while a
    real score is there, and fp32 cannot tell them apart)."""
    s = np.asarray(scores, dtype=np.float64)
    s = np.sort(s[np.isfinite(s) & (s > float(NEG) / 2)])[::-1][:first]
    return float(np.min(-np.diff(s))) if s.size >= 2 else float("inf")


def top_order(scores: np.ndarray, n: int) -> np.ndarray:
    """Indices of the n first entries in the order (score down, index up); a NaN ranks as -inf."""
    s = np.asarray(scores, dtype=F32)
    s = np.where(np.isnan(s), F32(-np.inf), s)
    # a stable sort of -s keeps equal scores in index order
    with np.errstate(invalid="ignore"):
        return np.argsort(-s.astype(np.float64), kind="stable")[:n]


@dataclass
class StepResult:
    tokens: np.ndarray                # [K] the new running beams' tokens
    parents: np.ndarray               # [K] the beams they continue
    top_scores: np.ndarray            # [2K] step c
    top_index: np.ndarray             # [2K] flat indices
    margin: float                     # the smallest gap at a selection boundary of this step (inf: none applies)


def beam_step(state: BeamState, logits: np.ndarray, t: int, max_new: int, eos_id: int, length_penalty: float, early_stopping) -> StepResult:
    """One pick (steps b-g) for one prompt: logits [K, V] of its K running beams, t = tokens generated so far.  Updates `state` in place."""
    K = state.K
    early = early_code(early_stopping)
    x = np.asarray(logits, dtype=F32)
    V = x.shape[1]
    assert x.shape[0] == K and V >= 2 * K
    with np.errstate(invalid="ignore"):
        acc = (log_probs(x) + state.run.astype(F32)[:, None]).astype(F32).reshape(-1)
    acc = np.where(np.isnan(acc), F32(-np.inf), acc)
    idx = top_order(acc, 2 * K)
    top = acc[idx]
    parent, token = (idx // V).astype(np.int32), (idx % V).astype(np.int32)
    hit = ((token == eos_id) & (eos_id >= 0)) | (t + 1 >= max_new)
    r = (top + np.where(hit, NEG, F32(0))).astype(F32)
    keep = top_order(r, K)
    # the selection boundaries of this step: the order of the top 2K and the first candidate left out; the order of the first K + 1 running scores
    rest = np.delete(acc, idx)
    margin = _gaps(np.concatenate([top, rest.max(keepdims=True)]) if rest.size else top, 2 * K + 1)
    margin = min(margin, _gaps(r, K + 1))
    new_run = r[keep].astype(F32)
    res = StepResult(token[keep].copy(), parent[keep].copy(), top.copy(), idx.copy(), margin)
    state.run = new_run
    if not state.open:
        return res
    all_fin = bool(state.fin_flag.all())
    did = hit & (np.arange(2 * K) < K)
    s = (top / denom(t + 1, length_penalty)).astype(F32)
    if all_fin and early == 1:
        s = (s + NEG).astype(F32)
    if not state.unsat:
        s = (s + NEG).astype(F32)
    s = (s + np.where(did, F32(0), NEG)).astype(F32)
    # (+ 0 where a flag does not apply: HF adds flag * -1e9, and x + 0 == x)
    ms = np.concatenate([state.fin_score.astype(F32), s])
    mlen = np.concatenate([state.fin_len, np.full(2 * K, t + 1, dtype=np.int32)])
    mpar = np.concatenate([state.fin_parent, parent])
    mtok = np.concatenate([state.fin_tok, token])
    mflag = np.concatenate([state.fin_flag, did.astype(np.int32)])
    sel = top_order(ms, K)
    margin = min(margin, _gaps(ms, K + 1))           # ... the order of the first K + 1 finished scores
    state.fin_score, state.fin_len, state.fin_parent, state.fin_tok, state.fin_flag = ms[sel].astype(F32), mlen[sel].astype(np.int32), mpar[sel].astype(np.int32), \
        mtok[sel].astype(np.int32), mflag[sel].astype(np.int32)
    hyp_len = max_new if (early == 2 and length_penalty > 0) else t + 1
    best = F32(new_run[0] / denom(hyp_len, length_penalty))
    worst = np.where(state.fin_flag != 0, state.fin_score.min(), NEG)
    if state.fin_flag.all():
        margin = min(margin, abs(float(best) - float(state.fin_score.min())))       # ... and the heuristic's comparison
    res.margin = margin
    state.unsat = bool(state.unsat and (best > worst).any())
    all_fin2 = bool(state.fin_flag.all())
    state.open = bool(state.unsat and not (all_fin2 and early == 1) and not hit.all())
    return res


def trace(hist_tok: Sequence[np.ndarray], hist_par: Sequence[np.ndarray], n: int, parent: int, last: int) -> List[int]:
    """The n tokens of a finished entry: its last token, then back through the parents of picks n - 2 .. 0 (hist_*[u]: [K] of pick u)."""
    if n <= 0:
        return []
    out = [0] * n
    out[n - 1] = int(last)
    s = int(parent)
    for u in range(n - 2, -1, -1):
        out[u] = int(hist_tok[u][s])
        s = int(hist_par[u][s])
    return out


@dataclass
class BeamRun:
    """The rules driven step by step for ONE prompt: feed the logits of the K running beams, get the tokens to run next and the map that reorders
    the caller's per-beam state (new beam i continues old beam parents[i])."""
    K: int
    max_new: int
    eos_id: int = -1
    length_penalty: float = 1.0
    early_stopping: object = False
    state: BeamState = None
    t: int = 0
    hist_tok: list = field(default_factory=list)
    hist_par: list = field(default_factory=list)
    margin: float = float("inf")

    def __post_init__(self):
        if self.state is None:
            self.state = BeamState(self.K)

    def step(self, logits: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        res = beam_step(self.state, logits, self.t, self.max_new, self.eos_id, self.length_penalty, self.early_stopping)
        self.hist_tok.append(res.tokens)
        self.hist_par.append(res.parents)
        self.margin = min(self.margin, res.margin)
        self.t += 1
        return res.tokens, res.parents

    @property
    def open(self) -> bool:
        return self.state.open and self.t < self.max_new

    def results(self) -> List[Tuple[List[int], float, bool]]:
        """(tokens, score, finished) of the K finished entries, best first."""
        st = self.state
        return [(trace(self.hist_tok, self.hist_par, int(st.fin_len[i]), int(st.fin_parent[i]), int(st.fin_tok[i])), float(st.fin_score[i]), bool(st.fin_flag[i]))
                for i in range(self.K)]
