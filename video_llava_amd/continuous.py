"""Continuous batching: answer a stream of tasks through a fixed group of decode slots, refilling the slots whose answer has finished with
queued tasks (pgv_llm_prefill_slots) instead of holding them until the longest answer of a static group is done.

`model.generate` on a static group keeps stepping until its LONGEST answer ends: with the runners' max_new_tokens = 1024 and answers of
5-60 tokens, one answer that runs to the cap keeps every other slot of its group decoding discarded tokens for ~1000 steps.  Here a slot
whose task ended (EOS, stop string or its token budget) is refilled at the next chunk boundary, while the other slots keep their cache and
state.  Every kernel on the path treats a sequence independently of the others (batch invariance is bitwise), so a task's ids are exactly
those of `model.generate([ids], ...)` on its own -- greedy, or sampled with the task's own seeded uniform stream.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Any, Callable, Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

from .model.utils import AnswerState

DEFAULT_CHUNK = 16          # decode steps between two host checks (EOS / stop strings / budgets) and refills
SAMPLE_SEED_STRIDE = 2 ** 20        # seeds of one task's samples lie this far apart: runs that seed their tasks base, base + 1, ... do not collide below 2^20 tasks


def sample_seed(base: int, j: int) -> int:
    """Seed of sample j of a task whose seed is `base`; sample 0 draws from the task's own stream."""
    return int(base) + int(j) * SAMPLE_SEED_STRIDE


@dataclass
class Task:
    """One prompt to answer.  feats: pooled video features [V, C] (None: text only).  stop: stop string (needs the tokenizer).
    max_new_tokens: this task's token budget (None: the call's).  seed: seed of the task's uniform stream (do_sample).
    samples: sampled answers wanted from ONE prefill of the prompt (do_sample; sample j draws from the stream seeded sample_seed(seed, j))."""
    task_id: Any
    ids: List[int]
    feats: Optional[torch.Tensor] = None
    stop: Optional[str] = None
    max_new_tokens: Optional[int] = None
    seed: Optional[int] = None
    samples: int = 1


def task_uniforms(n: int, seed: int, device) -> torch.Tensor:
    """The task's uniform stream: the [n, 1] draw `model.generate(do_sample=True, generator=Generator(device).manual_seed(seed))` makes for a
    single prompt with max_new_tokens = n; value t picks new token t."""
    g = torch.Generator(device=device).manual_seed(int(seed))
    return torch.rand(n, 1, device=device, dtype=torch.float32, generator=g)[:, 0]


class _Slot:
    """A decode slot's task: its answer state and what the scheduler keeps about it (uniform stream, timing counters)."""
    __slots__ = ("task", "answer", "u", "prefill_s", "decode_s", "steps", "group_size", "lp", "arrival", "j")

    def __init__(self, task: Task, answer: AnswerState, u: Optional[torch.Tensor], prefill_s: float, group_size: int, arrival: int = 0, j: int = 0):
        self.task, self.answer, self.u, self.group_size = task, answer, u, group_size
        self.arrival, self.j = arrival, j       # the task's arrival index and which of its samples this is
        self.prefill_s, self.decode_s, self.steps = prefill_s, 0.0, 0
        self.lp: List[np.ndarray] = []      # logprobs: [2, steps] blocks (model | pick) of every token the device emitted for the task, in order


def split_refused(parts: List[list], call: Callable[[list], Any]) -> Iterator[Tuple[list, Any, Optional[Exception]]]:
    """`call(part)` for every part, in order.  A call that raises was refused as a whole (one bad item, or too much at once): its part is split
    in halves and tried again, until the bad item is alone.  Yields (part, result, None) for a call that went through and (part of one item,
    None, exception) for an item refused on its own."""
    parts = list(parts)
    while parts:
        part = parts.pop(0)
        if not part:
            continue
        try:
            result = call(part)
        except Exception as e:                                     # noqa: BLE001
            if len(part) > 1:
                parts[:0] = [part[:len(part) // 2], part[len(part) // 2:]]
            else:
                yield part, None, e
            continue
        yield part, result, None


def _default_on_error(task_id, exc):
    print(f"Error processing task {task_id!r}: {exc}")


def generate_continuous(model, tasks: Iterable[Task], width: int, max_new_tokens: int, *, do_sample: bool = False, temperature: float = 0.2,
                        top_k: int = 50, tokenizer=None, chunk: int = DEFAULT_CHUNK, refill_min: Optional[int] = None, max_seq: Optional[int] = None,
                        prompt_slack: int = 128, eos_token_id="config", seed: int = 0,
                        on_error: Callable[[Any, Exception], None] = _default_on_error,
                        timings: Optional[dict] = None, top_p: float = 1.0, repetition_penalty: float = 1.0,
                        logprobs: Optional[dict] = None, bans=None, filters=None, allowed=None) -> Iterator[Tuple[Any, Optional[List[int]]]]:
    """Yield (task_id, new_ids) as each task finishes; new_ids is None for a task that failed (`on_error(task_id, exc)` is told why) -- a failed
    task costs only itself.

    width: decode slots (<= 64).  The group opens with `model.prefill` over the first `width` tasks; every `chunk` decode steps the host applies
    EOS, the stop-string cut and the budgets (model.utils.AnswerState, the bookkeeping `generate` keeps per sequence), then refills the freed slots
    with ONE `prefill_slots` call once at least `refill_min` slots are free (default: width // 8, at least 1) -- or sooner when waiting would
    stall: no task left decoding, or the queue holds fewer tasks than that.  Slots without a task are rewound to one position every chunk
    (pgv_kv_truncate) so that they neither outgrow the cache nor read a long one.
    do_sample: task t draws from its own stream `task_uniforms(budget, task.seed, device)` (seed None: `seed` + the task's arrival index), so a
    sampled answer equals generate(do_sample=True, generator=<that seeded generator>) whatever its slot and the group width.
    top_p, repetition_penalty: HF's nucleus filter (sampling only) and repetition penalty (both modes) for every task of the call, as in
    `generate`; a task's seen-set is its own prompt and answer -- a refilled slot starts clean (pgv_llm_prefill_slots).
    max_seq: cache positions per slot (default: longest prompt of the first group + `prompt_slack` + max_new_tokens + chunk, rounded to 64);
    a later task that does not fit fails alone.
    Task.samples = n > 1 (needs do_sample; n <= width): the prompt is prefilled ONCE and answered n times -- the opening group forks the prompt's
    slot (model.fork), a refill hands the task n free slots in one prefill_slots(counts=) call -- sample j drawing from
    task_uniforms(budget, sample_seed(base, j)), base = the task's seed as above.  Each sample decodes, ends and frees its slot on its own; the task
    yields once, with its last sample: (task_id, [new_ids_0, ..., new_ids_(n-1)]), and timings / logprobs hold lists of n dicts for it.  Admission is
    strictly first in, first out: the head task waits until n slots are free (all are once nothing is live), nothing overtakes it.  The opening
    group takes tasks while their samples fit `width`; when a task is left waiting the group still opens `width` slots wide (the last prompt's fork
    run is padded with slots that start idle), so that the waiting task fits later.
    timings (a dict): timings[task_id] = {prefill_s, decode_s, steps, group_size} of each finished task (host clock; the prefill call that
    started it and the decode chunks it was live in).
    logprobs (a dict): logprobs[task_id] = {"token_logprobs": [...], "transition_scores": [...]} of each finished task, one entry per new id --
    what `generate(output_logprobs=True)` returns for the task on its own, bit for bit, whatever its slot and the group width (the values are
    recorded on the device at pick time: pgv_kv_set_logprobs).
    bans (logit_bans.LogitBans, a dict of its fields, or None): HF's -inf processors, one configuration for every task of the call, as in
    `generate`; a task's sequence is its own prompt and answer -- a refilled slot's id record starts from its prompt (pgv_kv_set_bans).
    filters (sample_filters.SampleFilters, a dict of its fields, or None): HF's min_p / typical_p / epsilon_cutoff / eta_cutoff warpers behind top_p,
    one record for every sampled pick of the call -- the opening draw, every refill's first-token draw and every decode step (pgv_kv_set_filters);
    fields not given come from the model's generation config, as in `generate`.  Inert with do_sample=False.
    allowed (allowed.TokenAutomaton or None): constrained decoding as in `generate`, ONE automaton shared by every task of the call -- every slot,
    the refilled ones included, starts its answer at state 0 (pgv_kv_set_allowed).  An automaton per task is not implemented: a list is refused."""
    if not 1 <= width <= 64:
        raise ValueError(f"width {width} outside [1, 64]")
    if do_sample and not float(temperature) > 0.0:
        raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float; use do_sample=False for greedy decoding")
    from .generation import CacheSettings, check_samples_per_prompt, fork_sources, resolve_sampling, step_kwargs
    _, _, top_p, rep_pen = resolve_sampling(temperature if do_sample else 1.0, top_k, top_p, repetition_penalty)      # validates, HF's wording
    warp, pen = step_kwargs(top_p, rep_pen)     # empty when neutral: the model calls below then keep the argument lists they have always had
    chunk = max(1, int(chunk))
    k_min = max(1, int(refill_min) if refill_min is not None else width // 8)
    eos = model.config.eos_token_id if eos_token_id == "config" else eos_token_id
    eos_i = -1 if eos is None else int(eos)
    from .logit_bans import LogitBans, check_bans
    ban = LogitBans() if bans is None else check_bans(bans, model.vocab_size, eos_i, who="generate_continuous()")      # on the host, before any device work
    ban_on = not ban.effective_neutral(eos_i)
    from .sample_filters import check_filters
    filt = check_filters(filters, getattr(model, "generation_config", None), who="generate_continuous()")
    from .allowed import TokenAutomaton, check_allowed
    if allowed is not None and not isinstance(allowed, TokenAutomaton):
        raise ValueError(f"generate_continuous(): `allowed` has to be ONE TokenAutomaton shared by every task or None, but is {allowed!r} (an automaton per "
                         f"task is not implemented in the refill runner)")
    allow = check_allowed(allowed, 1, model.vocab_size, eos_i if eos_i >= 0 else None, who="generate_continuous()")      # roots: 0 for every slot
    want_lp = logprobs is not None
    # on for this call only: cleared in the finally below, also when the generator is closed early
    on = CacheSettings(True if want_lp else None, ban if ban_on else None, eos_i, filt if do_sample and not filt.neutral else None, allowed=allow)
    dev = model.device_

    source = iter(tasks)
    pending: List[Tuple[int, Task]] = []
    arrivals = [0]
    exhausted = [False]

    def pull(n: int):
        while len(pending) < n and not exhausted[0]:
            try:
                t = next(source)
            except StopIteration:
                exhausted[0] = True
                break
            pending.append((arrivals[0], t))
            arrivals[0] += 1

    def budget_of(t: Task) -> int:
        return int(t.max_new_tokens) if t.max_new_tokens is not None else int(max_new_tokens)

    def samples_of(t: Task) -> int:
        n = getattr(t, "samples", 1)            # anything but an integer >= 1 counts as one slot until check() refuses the task
        return n if isinstance(n, int) and not isinstance(n, bool) and n >= 1 else 1

    def check(t: Task, limit: int, slots_limit: int):
        """Host-side checks of one task (the ones the library would refuse a whole call for): a bad task fails alone."""
        n = check_samples_per_prompt(getattr(t, "samples", 1), 1, do_sample, False, False, who=f"task {t.task_id!r}")
        if n > slots_limit:
            raise ValueError(f"task {t.task_id!r}: `samples`={n} exceeds the {slots_limit} slots of the decode group")
        if len(t.ids) < 1:
            raise ValueError("empty prompt")
        if budget_of(t) < 1:
            raise ValueError(f"max_new_tokens {budget_of(t)} < 1")
        if len(t.ids) + budget_of(t) + chunk > limit:
            raise ValueError(f"prompt of {len(t.ids)} tokens + {budget_of(t)} new tokens does not fit the group's {limit} cache positions")
        if t.stop and tokenizer is None:
            raise ValueError("a stop string needs the tokenizer")
        vp = model._video_positions([t.ids], t.feats.shape[-2])[0] if t.feats is not None else -1
        a = np.asarray(t.ids)
        vocab = model.vocab_size
        keep = np.ones(len(a), dtype=bool)
        if vp >= 0:
            keep[vp + 1:vp + 1 + t.feats.shape[-2]] = False
        if ((a[keep] < 0) | (a[keep] >= vocab)).any():
            raise ValueError(f"token id outside the vocabulary ({vocab})")

    def feats_for(group: List[Task]) -> Optional[torch.Tensor]:
        shapes = {tuple(t.feats.shape) for t in group if t.feats is not None}
        if not shapes:
            return None
        if len(shapes) > 1:
            raise ValueError(f"video feature shapes differ inside one prefill call: {sorted(shapes)}")
        ref = next(t.feats for t in group if t.feats is not None)
        return torch.stack([(t.feats if t.feats is not None else torch.zeros_like(ref)).to(dev) for t in group])

    def uniforms(arrival: int, t: Task, j: int = 0) -> Optional[torch.Tensor]:
        if not do_sample:
            return None
        return task_uniforms(budget_of(t), sample_seed(t.seed if t.seed is not None else seed + arrival, j), dev)

    boxes: dict = {}            # arrival index of a live task with samples > 1 -> what its finished samples left, until the last one ends

    def admit(arrival: int, t: Task):
        n = samples_of(t)
        if n > 1:
            boxes[arrival] = {"left": n, "ids": [None] * n, "tm": [None] * n, "lp": [None] * n}

    # ---- open the group ------------------------------------------------------------------------------------------
    pull(width)
    first: List[Tuple[int, Task]] = []
    if max_seq is None:
        if not pending:
            return
        longest = max(len(t.ids) for _, t in pending)
        max_seq = longest + prompt_slack + int(max_new_tokens) + chunk
        max_seq = min((max_seq + 63) // 64 * 64, int(getattr(model.config, "max_position_embeddings", 4096)), 4096)
    taken = 0                                   # slots the first group's samples take
    while pending and taken < width:
        a, t = pending[0]
        try:
            check(t, max_seq, width)
        except Exception as e:                                     # noqa: BLE001 -- one bad task fails alone
            pending.pop(0)
            on_error(t.task_id, e)
            yield t.task_id, None
            pull(width)
            continue
        if taken + samples_of(t) > width:
            break                                                  # first in, first out: the head waits for its slots, nothing overtakes it
        pending.pop(0)
        first.append((a, t))
        taken += samples_of(t)
        pull(width)
    if not first:
        return
    # the group is as wide as its samples; a head task left waiting needs up to `width` slots later, so then the group opens at full width and the
    # last prompt's run is padded with slots that start idle
    W = width if pending else taken
    counts = [samples_of(t) for _, t in first]
    counts[-1] += W - taken
    forked = W != len(first)
    t0 = time.perf_counter()
    kv, nxt, _ = model.prefill([t.ids for _, t in first], feats_for([t for _, t in first]), max_seq, **({"capacity": W} if forked else {}),
                               **on.prefill_kwargs())
    try:
        on.apply(model, kv, prefilled=True)
        slots: List[Optional[_Slot]] = [None] * W
        # slot s holds sample j of first[i]; j beyond the task's samples: an idle padding slot
        owner = [(i, s - sum(counts[:i])) for s, i in enumerate(fork_sources(counts))]
        us = [uniforms(*first[i], j) if j < samples_of(first[i][1]) else None for i, j in owner]
        if forked:
            model.fork(kv, counts)
            nxt = nxt[torch.as_tensor(fork_sources(counts), device=nxt.device)]
        if do_sample:
            idle = torch.full((), 0.5, dtype=torch.float32, device=dev)
            nxt = model.sample_last(kv, torch.stack([u[0] if u is not None else idle for u in us]), temperature, top_k, **warp)
        elif rep_pen != 1.0 or ban_on or allow is not None:
            nxt = model.greedy_last(kv, W, **pen)                  # greedy over the penalised / banned logits (as generate does)
        cur = nxt.clone()
        first_lp = model.logprobs_last(kv, W).cpu().numpy() if want_lp else None
        first_tok = nxt.cpu().numpy()
        dt = time.perf_counter() - t0
        for a, t in first:
            admit(a, t)
        for s, (i, j) in enumerate(owner):
            a, t = first[i]
            if j >= samples_of(t):
                continue
            slots[s] = _Slot(t, AnswerState(budget_of(t), eos_i, t.stop, tokenizer), us[s], dt, W, a, j)
            if want_lp:
                slots[s].lp.append(first_lp[:, s:s + 1])

        def finish(s: int):
            """Slot s ended its answer: frees the slot; returns what the task yields, or None while other samples of the task are still live."""
            sl = slots[s]
            slots[s] = None
            tm = {"prefill_s": sl.prefill_s, "decode_s": sl.decode_s, "steps": sl.steps, "group_size": sl.group_size}
            lpd = None
            if want_lp:
                # the kept ids are a prefix of what the device emitted for the task: the same cut applies to the values
                lp = np.concatenate(sl.lp, axis=1)[:, :len(sl.answer.new)]
                lpd = {"token_logprobs": lp[0].tolist(), "transition_scores": lp[1].tolist()}
            box = boxes.get(sl.arrival)
            out = sl.answer.new
            if box is not None:
                box["ids"][sl.j], box["tm"][sl.j], box["lp"][sl.j] = sl.answer.new, tm, lpd
                box["left"] -= 1
                if box["left"]:
                    return None
                del boxes[sl.arrival]
                out, tm, lpd = box["ids"], box["tm"], box["lp"]
            if timings is not None:
                timings[sl.task.task_id] = tm
            if want_lp:
                logprobs[sl.task.task_id] = lpd
            return sl.task.task_id, out

        for s in range(W):
            if slots[s] is not None and slots[s].answer.take(first_tok[s:s + 1]):
                done = finish(s)
                if done is not None:
                    yield done

        # ---- decode / refill loop --------------------------------------------------------------------------------------
        head_ok = [-1]                      # arrival index of the queue's head once it has passed check()
        while True:
            free = [s for s in range(W) if slots[s] is None]
            live = W - len(free)
            pull(len(free) + width)
            while pending and pending[0][0] != head_ok[0]:          # the head of the queue is a task that can run: a bad one fails alone, now
                a, t = pending[0]
                try:
                    check(t, max_seq, W)
                    head_ok[0] = a
                except Exception as e:                             # noqa: BLE001
                    pending.pop(0)
                    on_error(t.task_id, e)
                    yield t.task_id, None
                    pull(1)
            queued = sum(samples_of(t) for _, t in pending)
            if free and pending and (len(free) >= k_min or live == 0 or (exhausted[0] and queued <= len(free))) and len(free) >= samples_of(pending[0][1]):
                group: List[Tuple[List[int], int, Task]] = []       # (the task's slots, arrival index, task), first in first out
                avail = list(free)
                while pending and avail:
                    a, t = pending[0]
                    if a != head_ok[0]:
                        try:
                            check(t, max_seq, W)
                        except Exception as e:                     # noqa: BLE001
                            pending.pop(0)
                            on_error(t.task_id, e)
                            yield t.task_id, None
                            pull(1)
                            continue
                    n = samples_of(t)
                    if n > len(avail):
                        head_ok[0] = a
                        break                                      # it waits for its slots; nothing overtakes it
                    pending.pop(0)
                    group.append((avail[:n], a, t))
                    del avail[:n]
                    if not pending:
                        pull(1)

                def prefill_part(part):
                    t0 = time.perf_counter()
                    u_part = [[uniforms(a, t, j) for j in range(len(ss))] for ss, a, t in part]
                    u0 = torch.stack([u[0] for us_ in u_part for u in us_]) if do_sample else None
                    flat = [s for ss, _, _ in part for s in ss]
                    many = {"counts": [len(ss) for ss, _, _ in part]} if len(flat) != len(part) else {}
                    nx, _ = model.prefill_slots(kv, flat, [t.ids for _, _, t in part], feats_for([t for _, _, t in part]),
                                                u=u0, temperature=temperature, top_k=top_k, **(warp if do_sample else pen), **many)
                    cur[flat] = nx
                    lp_part = model.logprobs_last(kv, W).cpu().numpy() if want_lp else None
                    return u_part, nx.cpu().numpy(), lp_part, time.perf_counter() - t0

                ok: List[Tuple[int, np.ndarray]] = []
                for part, res, e in split_refused([group], prefill_part):
                    if e is not None:                                  # the bad task, isolated
                        on_error(part[0][2].task_id, e)
                        yield part[0][2].task_id, None
                        continue
                    u_part, firsts, lp_part, dt = res
                    size = sum(len(ss) for ss, _, _ in part)
                    i = 0
                    for k, (ss, a, t) in enumerate(part):
                        admit(a, t)
                        for j, s in enumerate(ss):
                            slots[s] = _Slot(t, AnswerState(budget_of(t), eos_i, t.stop, tokenizer), u_part[k][j], dt, size, a, j)
                            if want_lp:
                                slots[s].lp.append(lp_part[:, s:s + 1])
                            ok.append((s, firsts[i:i + 1]))
                            i += 1
                for s, f in ok:
                    if slots[s].answer.take(f):
                        done = finish(s)
                        if done is not None:
                            yield done
                continue                                                # re-evaluate: refilled slots may have finished at their first token
            if live == 0:
                if not pending and exhausted[0]:
                    break
                continue
            # one chunk of decode steps for the whole group; slots without a task are rewound first
            for s in free:
                if model.kv_len(kv, s) > 1:
                    model.kv_truncate(kv, s, 1)
            n = min(chunk, max(sl.answer.budget - len(sl.answer.new) for sl in slots if sl is not None))
            t0 = time.perf_counter()
            if do_sample:
                u = torch.full((n, W), 0.5, dtype=torch.float32, device=dev)
                for s in range(W):
                    sl = slots[s]
                    if sl is not None:
                        seg = sl.u[len(sl.answer.new):len(sl.answer.new) + n]
                        u[:seg.numel(), s] = seg
                toks = model.decode_sample(kv, cur, n, eos_i, temperature, top_k, u, **warp)
            else:
                toks = model.decode_greedy(kv, cur, n, eos_i, **pen)
            cur = toks[:, n - 1].contiguous()
            lp_chunk = model.logprobs_steps(kv, W, n).cpu().numpy() if want_lp else None
            host = toks.cpu().numpy()
            dt = time.perf_counter() - t0
            for s in range(W):
                sl = slots[s]
                if sl is None:
                    continue
                sl.decode_s += dt
                sl.steps += n
                if want_lp:
                    sl.lp.append(lp_chunk[:, s])
                if sl.answer.take(host[s]):
                    done = finish(s)
                    if done is not None:
                        yield done
    finally:
        on.clear(model, kv)
