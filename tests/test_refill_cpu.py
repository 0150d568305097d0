"""Bookkeeping of the continuous-batching scheduler (video_llava_amd.continuous.generate_continuous) against a fake CPU backend: answers, slot
reuse, the refill threshold, failure isolation and the rewinding of idle slots -- no GPU needed."""
import torch

from video_llava_amd.continuous import Task, generate_continuous

VOCAB, EOS, POISON = 64, 2, 60


def _tok(prompt, g):
    return (sum(prompt) * 31 + g * 7 + len(prompt)) % (VOCAB - 8) + 2      # ids in [2, 58): EOS (2) shows up now and then


def _answer(prompt, budget, eos=EOS):
    out = []
    while len(out) < budget:
        t = _tok(prompt, len(out))
        out.append(t)
        if t == eos:
            break
    return out


class _Cfg:
    eos_token_id = EOS
    max_position_embeddings = 4096


class _KV:
    def __init__(self, W, max_seq):
        self.max_seq = max_seq
        self.prompt = [None] * W
        self.g = [0] * W            # tokens emitted so far (the next pick is _tok(prompt, g))
        self.len = [0] * W


class FakeModel:
    """The surface generate_continuous drives (prefill / prefill_slots / decode_greedy / kv_len / kv_truncate), with tokens that depend only
    on the slot's prompt and step -- like the real kernels, nothing crosses slots."""
    config = _Cfg()
    device_ = torch.device("cpu")
    vocab_size = VOCAB

    def __init__(self):
        self.refills = []           # slot lists of the prefill_slots calls
        self.truncates = 0

    def _video_positions(self, seqs, V):
        return [-1] * len(seqs)

    def _start(self, kv, s, p):
        kv.prompt[s], kv.g[s], kv.len[s] = list(p), 1, len(p)
        return _tok(p, 0)

    def prefill(self, seqs, feats, max_seq):
        kv = _KV(len(seqs), max_seq)
        return kv, torch.tensor([self._start(kv, s, p) for s, p in enumerate(seqs)], dtype=torch.int32), None

    def prefill_slots(self, kv, slots, seqs, feats, want_logits=False, u=None, temperature=1.0, top_k=50):
        if any(POISON in p for p in seqs):
            raise ValueError("refused: poison token")
        assert len(set(slots)) == len(slots) and all(0 <= s < len(kv.g) for s in slots)
        self.refills.append(list(slots))
        return torch.tensor([self._start(kv, s, p) for s, p in zip(slots, seqs)], dtype=torch.int32), None

    def decode_greedy(self, kv, first, n, eos_id=-1):
        out = torch.zeros(len(kv.g), n, dtype=torch.int32)
        for s in range(len(kv.g)):
            assert kv.len[s] + n <= kv.max_seq, f"slot {s} would grow to {kv.len[s] + n} of {kv.max_seq}"
            done = False
            for i in range(n):
                t = _tok(kv.prompt[s], kv.g[s])
                if done:
                    t = eos_id
                elif t == eos_id:
                    done = True
                out[s, i] = t
                kv.g[s] += 1
            kv.len[s] += n
        return out

    def kv_len(self, kv, s):
        return kv.len[s]

    def kv_truncate(self, kv, s, length):
        self.truncates += 1
        kv.len[s] = length


def _tasks(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        plen = int(torch.randint(3, 12, (1,), generator=g))
        ids = [1] + torch.randint(3, 50, (plen,), generator=g).tolist()
        out.append(Task(i, ids, max_new_tokens=int(torch.randint(1, 40, (1,), generator=g))))
    return out


def test_every_task_gets_its_own_answer_and_slots_are_reused():
    m = FakeModel()
    tasks = _tasks(50)
    got = dict(generate_continuous(m, iter(tasks), 8, 40, chunk=4, refill_min=1))
    assert set(got) == {t.task_id for t in tasks}
    for t in tasks:
        assert got[t.task_id] == _answer(t.ids, t.max_new_tokens), t.task_id
    assert sum(len(r) for r in m.refills) == len(tasks) - 8        # every task after the first group went into a freed slot
    assert {s for r in m.refills for s in r} == set(range(8))


def test_refill_threshold_batches_freed_slots():
    m = FakeModel()
    tasks = _tasks(60, seed=1)
    got = dict(generate_continuous(m, tasks, 8, 40, chunk=4, refill_min=4))
    assert all(got[t.task_id] == _answer(t.ids, t.max_new_tokens) for t in tasks)
    remaining = len(tasks) - 8
    for r in m.refills:
        # at least 4 slots per call, unless the queue ran short (the tail)
        assert len(r) >= 4 or len(r) == remaining, m.refills
        remaining -= len(r)
    assert remaining == 0


def test_a_failing_task_costs_only_itself():
    m = FakeModel()
    tasks = _tasks(30, seed=2)
    tasks[3].ids = tasks[3].ids + [VOCAB + 1]              # first group: refused by the host-side check
    tasks[17].ids = tasks[17].ids + [POISON]               # a refill: the library refuses the call, the scheduler isolates the task
    errors = []
    got = dict(generate_continuous(m, tasks, 6, 40, chunk=4, refill_min=3, on_error=lambda tid, e: errors.append(tid)))
    assert got[3] is None and got[17] is None and sorted(errors) == [3, 17]
    for t in tasks:
        if t.task_id not in (3, 17):
            assert got[t.task_id] == _answer(t.ids, t.max_new_tokens), t.task_id


def test_idle_slots_are_rewound_and_never_outgrow_the_cache():
    """Two tasks with long budgets and many short ones at width 4: at the tail two slots stay idle for many chunks; the fake backend asserts that
    no slot grows past the cache."""
    m = FakeModel()
    tasks = _tasks(12, seed=3)
    tasks[0].max_new_tokens = tasks[1].max_new_tokens = 300
    got = dict(generate_continuous(m, tasks, 4, 300, chunk=8, eos_token_id=None))
    for t in tasks:
        assert got[t.task_id] == _answer(t.ids, t.max_new_tokens, eos=-1)
    assert m.truncates > 0
