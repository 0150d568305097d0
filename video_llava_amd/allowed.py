"""Constrained decoding: HF's PrefixConstrainedLogitsProcessor, as this package's `generate(allowed=...)` runs it on the device.

HF's generate(prefix_allowed_tokens_fn=fn) calls a Python function per sequence per step on the host and sets every score outside the returned list
to -inf (transformers/generation/logits_process.py).  A callback cannot run on the device.  Here the constraint is compiled ONCE into a
deterministic token automaton -- states, per state a list of edges (token, next state) with distinct tokens, and a per-state accept flag -- which the
device follows inside the captured decode graphs (csrc/logit_allow.hip; include/pgv.h: pgv_kv_set_allowed states the same rule).  HF's chain is
repetition penalty, the bans, prefix-constrained, then the warpers; the bans and this processor write -inf or nothing, so, as logit_bans.py argues,
their order among themselves and against the penalty does not change the result: one place between the lm_head and the pick is right.

This module is the host side: the automaton and its constructors (TokenAutomaton), the validation of a call (check_allowed) and the rule in plain
Python for one sequence at one step (allowed_ids) -- what the kernel is held to, and what the tests hold against the installed HF.  Pure host code:
importable without a GPU.
"""
from __future__ import annotations

import numbers
from typing import Any, Iterable, List, Optional, Sequence, Set, Tuple

import numpy as np

MAX_STATES, MAX_EDGES = 1 << 20, 1 << 22          # PGV_ALLOW_MAX_STATES / _EDGES of include/pgv.h
DEAD = -1                                         # the state behind a token that has no edge; it has no edge itself


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)          # numpy integers included


class TokenAutomaton:
    """A deterministic automaton over token ids, stored as CSR: the edges of state s are entries row_ptr[s] .. row_ptr[s + 1] of edge_token (sorted
    within a state, distinct) and edge_next; accept[s] says that an answer may end in s.  State 0 is the root unless a call says otherwise (union).
    Build one with from_sequences / from_texts (a closed set of answers), from_edges (the general form, cycles allowed) or union."""

    def __init__(self, row_ptr, edge_token, edge_next, accept):
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        self.edge_token = np.ascontiguousarray(edge_token, dtype=np.int32)
        self.edge_next = np.ascontiguousarray(edge_next, dtype=np.int32)
        self.accept = np.ascontiguousarray(accept, dtype=np.uint8)
        S, E = self.n_states, self.n_edges
        if S < 1 or self.row_ptr.shape != (S + 1,) or self.edge_next.shape != (E,) or self.row_ptr[0] != 0 or self.row_ptr[-1] != E:
            raise ValueError("TokenAutomaton: row_ptr has to run from 0 to the number of edges over at least one state")
        if np.any(np.diff(self.row_ptr) < 0):
            raise ValueError("TokenAutomaton: row_ptr has to rise")
        if E and (self.edge_next.min() < 0 or self.edge_next.max() >= S):
            raise ValueError(f"TokenAutomaton: an edge leads outside the {S} states")
        if E and self.edge_token.min() < 0:
            raise ValueError("TokenAutomaton: a negative edge token")
        inner = np.ones(E, dtype=bool)
        inner[self.row_ptr[:-1][self.row_ptr[:-1] < E]] = False            # the first edge of a state has no predecessor to exceed
        if E and np.any((np.diff(self.edge_token, prepend=-1) <= 0) & inner):
            raise ValueError("TokenAutomaton: the edge tokens of a state have to be sorted and distinct")

    @property
    def n_states(self) -> int:
        return int(self.accept.shape[0])

    @property
    def n_edges(self) -> int:
        return int(self.edge_token.shape[0])

    def edges(self, state: int) -> List[Tuple[int, int]]:
        """[(token, next state)] of `state`, by token."""
        a, b = int(self.row_ptr[state]), int(self.row_ptr[state + 1])
        return list(zip(self.edge_token[a:b].tolist(), self.edge_next[a:b].tolist()))

    def step(self, state: int, token: int) -> int:
        """The state behind `token` in `state`: DEAD when it has no such edge, and DEAD stays DEAD."""
        if state < 0:
            return DEAD
        a, b = int(self.row_ptr[state]), int(self.row_ptr[state + 1])
        i = a + int(np.searchsorted(self.edge_token[a:b], int(token)))
        return int(self.edge_next[i]) if i < b and int(self.edge_token[i]) == int(token) else DEAD

    def walk(self, root: int, ids: Iterable[int]) -> int:
        state = int(root)
        for t in ids:
            state = self.step(state, int(t))
        return state

    def __eq__(self, other):
        return isinstance(other, TokenAutomaton) and all(np.array_equal(getattr(self, f), getattr(other, f))
                                                         for f in ("row_ptr", "edge_token", "edge_next", "accept"))

    __hash__ = None

    def __repr__(self):
        return f"TokenAutomaton({self.n_states} states, {self.n_edges} edges, {int(self.accept.sum())} accepting)"

    # ---- constructors --------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_edges(cls, n_states: int, edges: Iterable[Tuple[int, int, int]], accept: Iterable[int]) -> "TokenAutomaton":
        """The general form: `edges` is (state, token, next state) triples, `accept` the accepting states' indices (or one True / False per state).  Cycles are
        allowed ("one or more digits"); a state with two edges on the same token is refused -- the automaton is deterministic."""
        if not _is_int(n_states) or n_states < 1:
            raise ValueError(f"from_edges: `n_states` has to be a positive integer, but is {n_states!r}")
        S = int(n_states)
        per: List[dict] = [dict() for _ in range(S)]
        for e in edges:
            s, t, nx = e
            if not (_is_int(s) and _is_int(t) and _is_int(nx)) or not (0 <= s < S and 0 <= nx < S) or t < 0:
                raise ValueError(f"from_edges: edge {tuple(e)!r} is not (state, token, next state) with both states in [0, {S}) and a token >= 0")
            if int(t) in per[int(s)]:
                raise ValueError(f"from_edges: state {int(s)} has two edges on token {int(t)}")
            per[int(s)][int(t)] = int(nx)
        acc = list(accept)
        flags = np.zeros(S, dtype=np.uint8)
        if len(acc) == S and all(isinstance(a, (bool, np.bool_)) for a in acc):       # one True / False per state
            flags[:] = [1 if a else 0 for a in acc]
        else:
            for a in acc:
                if not _is_int(a) or not 0 <= a < S:
                    raise ValueError(f"from_edges: accepting state {a!r} outside [0, {S})")
                flags[int(a)] = 1
        return cls._from_dicts(per, flags)

    @classmethod
    def _from_dicts(cls, per: Sequence[dict], flags) -> "TokenAutomaton":
        row_ptr, tok, nxt = [0], [], []
        for d in per:
            for t in sorted(d):
                tok.append(t)
                nxt.append(d[t])
            row_ptr.append(len(tok))
        return cls(row_ptr, tok, nxt, flags)

    @classmethod
    def from_sequences(cls, sequences: Iterable[Sequence[int]]) -> "TokenAutomaton":
        """A trie of the id lists: the answer has to be one of them.  A sequence that is a prefix of another makes an inner accepting state;
        duplicates merge; an empty sequence is refused (the answer would be allowed to be nothing)."""
        per: List[dict] = [dict()]
        flags = [0]
        n = 0
        for seq in sequences:
            seq = list(seq)
            if len(seq) == 0:
                raise ValueError("from_sequences: an empty sequence (an answer of no tokens) cannot be a choice")
            if any((not _is_int(t) or t < 0) for t in seq):
                raise ValueError(f"from_sequences: {seq!r} is not a list of non-negative token ids")
            s = 0
            for t in seq:
                t = int(t)
                if t not in per[s]:
                    per[s][t] = len(per)
                    per.append(dict())
                    flags.append(0)
                s = per[s][t]
            flags[s] = 1
            n += 1
        if n == 0:
            raise ValueError("from_sequences: no sequence given")
        return cls._from_dicts(per, np.asarray(flags, dtype=np.uint8))

    @classmethod
    def from_texts(cls, tokenizer, texts: Iterable[str], prefix: str = "") -> "TokenAutomaton":
        """from_sequences of tokenizer(prefix + t, add_special_tokens=False).input_ids for every text.  The ids must be the ones the MODEL would
        produce for the answer behind its prompt: under sentencepiece a word at the start of an answer usually carries the leading-space piece,
        which `tokenizer("yes")` and `tokenizer(" yes")` may or may not give -- getting that tokenisation right (with `prefix`, or by passing id
        lists to from_sequences) is the caller's job, exactly as for HF's bad_words_ids."""
        texts = list(texts)
        return cls.from_sequences([tokenizer(prefix + t, add_special_tokens=False).input_ids for t in texts])

    @staticmethod
    def union(automata: Sequence["TokenAutomaton"]) -> Tuple["TokenAutomaton", List[int]]:
        """Several automata side by side in one: (automaton, roots) with roots[i] the state automaton i's state 0 became -- so every sequence of a
        batch can have its own start state (per-question multiple choice).  Equal automata are laid down once."""
        automata = list(automata)
        if not automata:
            raise ValueError("union: no automaton given")
        kept: List[TokenAutomaton] = []
        base: List[int] = []
        roots: List[int] = []
        total = 0
        for a in automata:
            if not isinstance(a, TokenAutomaton):
                raise ValueError(f"union: {a!r} is not a TokenAutomaton")
            for k, b in enumerate(kept):
                if a is b or a == b:
                    roots.append(base[k])
                    break
            else:
                kept.append(a)
                base.append(total)
                roots.append(total)
                total += a.n_states
        row_ptr, e = [np.zeros(1, dtype=np.int32)], 0
        for a in kept:
            row_ptr.append(a.row_ptr[1:] + e)
            e += a.n_edges
        return (TokenAutomaton(np.concatenate(row_ptr), np.concatenate([a.edge_token for a in kept]),
                               np.concatenate([a.edge_next + o for a, o in zip(kept, base)]), np.concatenate([a.accept for a in kept])), roots)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def allowed_ids(automaton: TokenAutomaton, root: int, generated_ids: Sequence[int], eos: int) -> Set[int]:
    """The ids that may come next for ONE sequence at ONE step.  `generated_ids`: everything behind the prompt length the slot was prefilled with.
    Walk them from `root` (a token without an edge leads to DEAD, DEAD stays DEAD); allowed are the tokens of the reached state's edges, plus `eos`
    if the state accepts.  A DEAD state, or one without edges that does not accept, allows {eos} alone: the answer ends, where HF raises a
    ValueError for an empty list."""
    state = automaton.walk(root, generated_ids)
    return state_allowed_ids(automaton, state, eos)


def state_allowed_ids(automaton: TokenAutomaton, state: int, eos: int) -> Set[int]:
    """allowed_ids for a sequence whose walk has reached `state`."""
    if state < 0:
        return {int(eos)}
    out = {t for t, _ in automaton.edges(state)}
    if automaton.accept[state] or not out:
        out.add(int(eos))
    return out


def apply_allowed(automaton: TokenAutomaton, root: int, scores, generated_ids: Sequence[int], eos: int):
    """`scores` (a 1-D numpy array or torch tensor over the vocabulary) with -inf everywhere outside allowed_ids: a copy.  Entries inside the set
    keep their bits, NaN and -inf included."""
    out = scores.copy() if hasattr(scores, "copy") else scores.clone()
    keep = sorted(t for t in allowed_ids(automaton, root, generated_ids, eos) if 0 <= t < int(out.shape[-1]))
    kept = out[keep].copy() if hasattr(out, "copy") else out[keep].clone()
    out[...] = float("-inf")
    out[keep] = kept
    return out


# ---- the call ------------------------------------------------------------------------------------------------------------------------------
class Allowed:
    """What a checked generate(allowed=...) holds: one automaton and the root of every prompt."""

    def __init__(self, automaton: TokenAutomaton, roots: Sequence[int]):
        self.automaton, self.roots = automaton, [int(r) for r in roots]

    def __repr__(self):
        return f"Allowed({self.automaton!r}, roots={self.roots})"


def check_allowed(allowed: Any, batch: int, vocab: int, eos, beams: int = 1, lookup: int = 0, who: str = "generate()") -> Optional[Allowed]:
    """Validate generate(allowed=...) on the host, before any device work.  `allowed`: one TokenAutomaton for all prompts (root 0), a list with one
    per prompt (laid side by side by union), an Allowed, or None -- which makes the call the call without the keyword (returns None)."""
    if allowed is None:
        return None
    if isinstance(allowed, Allowed):
        out = allowed
        if len(out.roots) != batch:
            raise ValueError(f"{who}: `allowed` carries {len(out.roots)} roots for {batch} prompts")
    elif isinstance(allowed, TokenAutomaton):
        out = Allowed(allowed, [0] * batch)
    elif isinstance(allowed, (list, tuple)):
        if len(allowed) != batch:
            raise ValueError(f"{who}: `allowed` lists {len(allowed)} automata for {batch} prompts (one for all, or one per prompt)")
        out = Allowed(*TokenAutomaton.union(allowed))
    else:
        raise ValueError(f"{who}: `allowed` has to be a TokenAutomaton, a list with one per prompt or None, but is {allowed!r}")
    a = out.automaton
    if eos is None or int(eos) < 0:
        raise ValueError(f"{who}: `allowed` needs an EOS token (the rule ends an answer with it); eos_token_id is {eos!r}")
    if int(eos) >= vocab:
        raise ValueError(f"{who}: eos_token_id {int(eos)} outside the vocabulary of {vocab}")
    if a.n_states > MAX_STATES:
        raise ValueError(f"{who}: `allowed` has {a.n_states} states, the limit is {MAX_STATES}")
    if a.n_edges > MAX_EDGES:
        raise ValueError(f"{who}: `allowed` has {a.n_edges} edges, the limit is {MAX_EDGES}")
    if a.n_edges and int(a.edge_token.max()) >= vocab:
        bad = sorted(set(a.edge_token[a.edge_token >= vocab].tolist()))[:8]
        raise ValueError(f"{who}: the model vocabulary size is {vocab}, but `allowed` has edges on the tokens {bad}")
    if any(not 0 <= r < a.n_states for r in out.roots):
        raise ValueError(f"{who}: `allowed` roots {out.roots} outside the {a.n_states} states")
    if beams is not None and beams > 1:
        raise ValueError(f"{who}: `allowed` cannot be combined with `beams`={int(beams)} (the beam pick applies no logits processor; each beam's "
                         f"state would have to be rebuilt from the parent history)")
    if lookup:
        raise ValueError(f"{who}: `allowed` cannot be combined with `lookup`={int(lookup)} (the drafts are verified against the unconstrained pick)")
    return out
