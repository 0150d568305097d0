"""The host loop of `model.generate`, as a function of (model, plan, ...) over the model's public step methods only, each handed a keyword only
when the plan (generation.GenerationPlan) makes it non-neutral.  The cache's per-call switches live in ONE scope (`open_cache`), the two ways
of stepping (`PlainStep`, `LookupStep`) feed ONE `Answers.absorb`.  Tokens never leave the device inside a chunk."""
from __future__ import annotations

import time
from contextlib import contextmanager

import numpy as np
import torch

from .generation import GenerateBeamsOutput, GenerateLogprobsOutput, fork_sources
from .guidance import stack_features
from .model.utils import AnswerState


def echo_and_pad(seqs, new, eos_id: int, device) -> torch.Tensor:
    """LongTensor [B, longest] on `device`: every prompt echoed with its new ids behind it, shorter rows padded with EOS (0 without one)."""
    out = torch.full((len(seqs), max(len(s) + len(n) for s, n in zip(seqs, new))), eos_id if eos_id >= 0 else 0, dtype=torch.long)
    for b, (s, n) in enumerate(zip(seqs, new)):
        row = list(s) + list(n)
        out[b, :len(row)] = torch.tensor(row, dtype=torch.long)
    return out.to(device)


def fill_timings(timings, t0: float, t1: float, steps: int, batch: int, **more):
    """generate(timings=): prefill_s up to the first token's absorption, decode_s from there to now (host clock)."""
    if timings is not None:
        timings.update(prefill_s=t1 - t0, decode_s=time.perf_counter() - t1, steps=steps, batch=batch, **more)


@contextmanager
def open_cache(model, plan, seqs, feats, kv_reuse_key):
    """The filled cache of the call -> (kv, the prefill's first tokens, B, seqs, stops, reused), by one of four routes: the cache kept under
    `kv_reuse_key` truncated to the common prefix plus an append of the new tokens; one prefill at capacity B * n forked n ways (from there on
    the call IS the call on the prompts repeated n times each); under guidance one ragged prefill of the B prompts and their B negatives (slot
    B + b is the unconditional twin of b; B stays the number of answers); or a plain prefill.  It is the scope of the cache's settings: on from the
    prefill, off again however the call ends -- a refused fork, a criterion, the tokenizer or an interrupt included."""
    B, n, stops, on = len(seqs), plan.samples_per_prompt, plan.stops, plan.settings
    reused = 0
    if kv_reuse_key is not None and B == 1 and plan.repetition_penalty == 1.0 and not plan.bans_on and not plan.lookup[0] and plan.allowed is None:
        # under a repetition penalty the slot's seen-set has to be exactly prompt + answer: the surplus steps a kept cache carries past a stop
        # string would stay in it, so such a turn runs the full prefill; under bans or lookup the slot's id record, under `allowed` its state record, for
        # the same reason
        reused = model._reusable_prefix(kv_reuse_key, seqs[0], plan.max_new_tokens)
    if reused:
        kv = model._reuse[1]
        if reused < len(model._reuse[3]):
            model.kv_truncate(kv, 0, reused)
        _kv, nxt, _ = model.prefill([seqs[0][reused:]], None, 0, append_to=kv, **on.prefill_kwargs())
    elif plan.guidance is not None:
        negs = [list(x) for x in plan.negatives]
        both = stack_features(feats, plan.guidance.negative_feats, negs, getattr(model.model.vision_config, "vid_patch_token", None))
        kv, nxt, _ = model.prefill(list(seqs) + negs, both, plan.max_seq, **on.prefill_kwargs())
    else:
        kv, nxt, _ = model.prefill(seqs, feats, plan.max_seq, **({"capacity": B * n} if n > 1 else {}), **on.prefill_kwargs())
    try:
        on.apply(model, kv, prefilled=True)
        if n > 1:
            B = model.fork(kv, [n] * B)             # the prefill's own greedy first tokens are replaced by the draw, per slot
            seqs = [seqs[i] for i in fork_sources([n] * len(seqs))]
            stops = stops and [stops[i // n] for i in range(B)]
        yield kv, nxt, B, seqs, stops, reused
    finally:
        on.clear(model, kv)


def first_pick(model, plan, kv, nxt, B: int, generator):
    """-> (the call's uniforms [max_new_tokens, B] or None, first tokens [B] on the device, the log-probability blocks so far).  A sampled call
    draws; greedy under a penalty, bans, an automaton (`allowed`) or guidance re-picks over the processed logits (the prefill's argmax knows none of them; first index on
    ties).  Under guidance the group is 2B wide: the uniforms are the B columns of the call padded to that width (the twins' columns are never
    read), and the tokens come back 2B long, rows [B, 2B) repeating rows [0, B)."""
    u, lp_parts = None, []              # lp_parts: [2, B, steps] blocks in generation order (first token, then every chunk)
    W = 2 * B if plan.guidance is not None else B
    if plan.max_new_tokens >= 1:
        if plan.do_sample:
            u = torch.rand(plan.max_new_tokens, B, device=model.device_, dtype=torch.float32, generator=generator)
            if W != B:
                u = torch.nn.functional.pad(u, (0, W - B))
            nxt = model.sample_last(kv, u[0], plan.temperature, plan.top_k, **plan.warp)
        elif plan.repetition_penalty != 1.0 or plan.bans_on or plan.allowed is not None or W != B:
            nxt = model.greedy_last(kv, W, **plan.pen)
        if plan.output_logprobs:
            lp_parts.append(model.logprobs_last(kv, B)[:, :, None])
    return u, nxt, lp_parts


class Answers:
    """The answers of a call while its chunks come in: one AnswerState per sequence, the stopping criteria (B == 1) and `raw` -- every token the
    device emitted for sequence 0, stop cuts ignored (what its cache holds, shifted by one: the `kv_reuse_key` record)."""

    def __init__(self, plan, seqs, stops, tokenizer):
        self.states = [AnswerState(plan.max_new_tokens, plan.eos_id, stops[b] if stops is not None else None, tokenizer) for b in range(len(seqs))]
        self.criteria, self.prompt_t, self.raw = plan.criteria, torch.tensor(seqs[0], dtype=torch.long), []

    def criterion_fires(self) -> bool:
        """HF: a stopping criterion is asked after every appended token (B == 1)."""
        cur = torch.cat([self.prompt_t, torch.tensor(self.states[0].new, dtype=torch.long)])[None]
        return any(c(cur, None) for c in self.criteria)

    def absorb(self, h, runs):
        """h [B, cols]: a chunk's tokens on the host, the first runs[b] columns of row b those of sequence b.  -> (stop: every answer is complete
        or a criterion fired, taken: how far into the chunk the longest live answer went).  Under criteria token by token, the criteria asked
        after each; otherwise per SEQUENCE, not per step (a chunk of 64 steps x 8 sequences cost ~0.6 ms of Python between two decode launches,
        with the GPU idle): AnswerState.take absorbs a live sequence's whole run at once."""
        self.raw.extend(h[0, :int(runs[0])].tolist())
        stop, taken = False, 0
        for b, st in enumerate(self.states):
            if st.done or not runs[b]:
                continue
            if self.criteria:
                for i in range(int(runs[b])):
                    taken = i + 1
                    if st.take(h[b, i:i + 1]) or self.criterion_fires():
                        stop = True
                        break
            else:
                st.take(h[b, :int(runs[b])])
                taken = max(taken, st.taken)
        return stop or all(st.done for st in self.states), taken


class PlainStep:
    """A chunk of n decode steps (decode_sample / decode_greedy): every sequence emits n tokens; the log-probabilities are collected here."""

    def __init__(self, model, plan, kv, B: int, u, lp_parts):
        self.model, self.plan, self.kv, self.B, self.u, self.lp_parts = model, plan, kv, B, u, lp_parts
        self.limit, self.n, self.timings = plan.max_new_tokens, 0, {}

    def __call__(self, nxt, n_gen: int, answers):
        """-> (host tokens [B, n], runs [B], the first tokens of the next chunk)."""
        m, p, kv = self.model, self.plan, self.kv
        n = self.n = min(p.chunk, p.max_new_tokens - n_gen)
        if p.do_sample:
            toks = m.decode_sample(kv, nxt, n, p.eos_id, p.temperature, p.top_k, self.u[n_gen:n_gen + n], **p.warp)
        else:
            toks = m.decode_greedy(kv, nxt, n, p.eos_id, **p.pen)
        if p.output_logprobs:
            self.lp_parts.append(m.logprobs_steps(kv, self.B, n))
        if p.guidance is not None:          # the group is 2B wide; the twins' rows repeat the answers' and stay on the device
            return toks[:self.B].cpu().numpy(), np.full(self.B, n), toks[:, n - 1].contiguous()
        return toks.cpu().numpy(), np.full(self.B, n), toks[:, n - 1].contiguous()

    def steps(self, n_gen: int, stop: bool, taken: int, answers) -> int:
        """generate's `steps`: the chunk in full, or up to the last token taken when it ended the call."""
        return n_gen + (taken if stop else self.n)


class LookupStep:
    """A chunk of lookup steps (decode_lookup / decode_lookup_sample): every sequence emits a run of its own length; a sequence the host has
    finished gets no budget, and the budgets end the call (no `limit`).  The cache keeps the current tokens between chunks, so only the first
    chunk hands them in.  `timings`: the passes that emitted something and what they emitted."""

    def __init__(self, model, plan, kv, u):
        self.model, self.plan, self.kv, self.u = model, plan, kv, u
        self.limit, self.timings = float("inf"), {"lookup_steps": 0, "lookup_emitted": 0}

    def __call__(self, nxt, n_gen: int, answers):
        """-> (host tokens [B, steps * (1 + D)] packed from column 0, runs [B], None)."""
        m, p, states = self.model, self.plan, answers.states
        left = [0 if st.done else p.max_new_tokens - len(st.new) for st in states]
        first, steps = nxt if n_gen == 1 else None, min(p.chunk, max(left))
        if p.do_sample:         # the whole table of uniforms, and per sequence the row its next token draws from
            toks, counts = m.decode_lookup_sample(self.kv, first, steps, p.eos_id, left, [len(st.new) for st in states], p.temperature, p.top_k, self.u)
        else:
            toks, counts = m.decode_lookup(self.kv, first, steps, p.eos_id, left)
        h, runs = toks.cpu().numpy(), counts.sum(axis=0)
        self.timings["lookup_steps"] += int((counts.sum(axis=1) > 0).sum())       # steps behind the last token of the chunk emitted nothing
        self.timings["lookup_emitted"] += int(runs.sum())
        return h, runs, None

    def steps(self, n_gen: int, stop: bool, taken: int, answers) -> int:
        """generate's `steps` under lookup: the longest answer so far."""
        return max(2, max(len(st.new) for st in answers.states))


def generate_chunks(model, plan, seqs, feats, generator, tokenizer, timings, kv_reuse_key):
    """generate() without beams: what it returns, for the plan of the call (generation.plan_generate) and its parsed prompts."""
    t0 = time.perf_counter()
    with open_cache(model, plan, seqs, feats, kv_reuse_key) as (kv, nxt, B, seqs, stops, reused):
        u, nxt, lp_parts = first_pick(model, plan, kv, nxt, B, generator)
        answers = Answers(plan, seqs, stops, tokenizer)
        step = LookupStep(model, plan, kv, u) if plan.lookup[0] else PlainStep(model, plan, kv, B, u, lp_parts)
        n_gen, t1 = 0, t0
        if plan.max_new_tokens >= 1:
            stop, _ = answers.absorb(nxt[:B].cpu().numpy()[:, None], np.ones(B, dtype=np.int64))
            t1, n_gen = time.perf_counter(), 1
            while not stop and n_gen < step.limit:
                h, runs, nxt = step(nxt, n_gen, answers)
                stop, taken = answers.absorb(h, runs)
                n_gen = step.steps(n_gen, stop, taken, answers)
        new = [st.new for st in answers.states]
        fill_timings(timings, t0, t1, n_gen, B, reused_tokens=reused, samples_per_prompt=plan.samples_per_prompt, **step.timings)
        if kv_reuse_key is not None and B == 1:
            # the cache holds the prompt and every emitted token that was fed back (all but the last one)
            model._reuse = (kv_reuse_key, kv, plan.max_seq, list(seqs[0]) + answers.raw[:-1])
            assert model.kv_len(kv, 0) == len(model._reuse[3]), (model.kv_len(kv, 0), len(model._reuse[3]))
        out = echo_and_pad(seqs, new, plan.eos_id, model.device_)
        if not plan.output_logprobs:
            return out
        # a sequence's kept ids are a prefix of what the device emitted for it: the same cut applies to the values
        lp = torch.cat(lp_parts, dim=2).cpu().numpy() if lp_parts else np.zeros((2, B, 0), dtype=np.float32)
        return GenerateLogprobsOutput.assemble(out, [len(n_) for n_ in new], lp[0], lp[1])


def generate_beams(model, plan, seqs, feats, timings):
    """generate(beams=K > 1): one prefill of the B prompts in a cache of B * K slots, pgv_beam_begin, then chunks of beam steps until no prompt
    is open or the budget is spent.  The host reads one flag per prompt between chunks and the best hypothesis at the end."""
    t0 = t1 = time.perf_counter()
    B, K, budget = len(seqs), plan.beams, int(plan.max_new_tokens)
    new, n_gen = [([], 0.0)] * B, 0
    if budget >= 1:
        kv, _nxt, _ = model.prefill(seqs, feats, plan.max_seq, capacity=B * K)
        model.beam_begin(kv, K, budget, plan.eos_id, plan.length_penalty, plan.early_stopping)
        n_gen = 1
        still = model.beam_open(kv, B)          # synchronises: the prefill and the first pick are done
        t1 = time.perf_counter()
        while n_gen < budget and any(still):
            n = min(max(1, int(plan.chunk)), budget - n_gen)
            model.decode_beam(kv, n)
            n_gen += n
            still = model.beam_open(kv, B)
        new = [model.beam_result(kv, b, 0)[:2] for b in range(B)]
    fill_timings(timings, t0, t1, n_gen, B * K, reused_tokens=0, samples_per_prompt=1, beams=K)
    out = echo_and_pad(seqs, [n_[0] for n_ in new], plan.eos_id, model.device_)
    if plan.output_beam_scores:
        return GenerateBeamsOutput(out, torch.tensor([n_[1] for n_ in new], dtype=torch.float32), torch.tensor([len(n_[0]) for n_ in new], dtype=torch.long))
    return out
