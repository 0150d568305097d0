"""Task.samples in the continuous-batching scheduler against a fake CPU backend that accepts `counts` / `capacity`: first in first out admission,
n slots per task, the seeds of the samples, what is yielded and what fails alone; and the sample maps of csrc/prefill_plan.h compiled on their
own.  No GPU."""
import os
import shutil
import subprocess

import pytest
import torch

from video_llava_amd import continuous
from video_llava_amd.continuous import SAMPLE_SEED_STRIDE, Task, generate_continuous, sample_seed, task_uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, EOS, POISON = 64, 2, 60
CPU = torch.device("cpu")


def _tok(prompt, g, u=None):
    """Token g of a slot: a function of its prompt, the step and the uniform it drew -- nothing crosses slots."""
    k = 0 if u is None else int(float(u) * 1000003)
    return (sum(prompt) * 31 + g * 7 + len(prompt) + k * 13) % (VOCAB - 8) + 2


def _answer(prompt, budget, u=None, eos=EOS):
    out = []
    while len(out) < budget:
        t = _tok(prompt, len(out), None if u is None else u[len(out)])
        out.append(t)
        if t == eos:
            break
    return out


def _sample_answer(t, j, base=None):
    return _answer(t.ids, t.max_new_tokens, task_uniforms(t.max_new_tokens, sample_seed(t.seed if base is None else base, j), CPU))


class _Cfg:
    eos_token_id = EOS
    max_position_embeddings = 4096


class _KV:
    def __init__(self, W, max_seq):
        self.max_seq, self.prompt, self.g, self.len, self.live = max_seq, [None] * W, [0] * W, [0] * W, 0


class FakeModel:
    """The surface generate_continuous drives, `counts` / `capacity` / fork included.  `log`: ("prefill" | "fork" | "prefill_slots", prompts,
    counts or None, slots or None) of every call that went through."""
    config = _Cfg()
    device_ = CPU
    vocab_size = VOCAB

    def __init__(self):
        self.log = []

    def _video_positions(self, seqs, V):
        return [-1] * len(seqs)

    def prefill(self, seqs, feats, max_seq, capacity=None):
        kv = _KV(max(len(seqs), int(capacity or 0)), max_seq)
        for s, p in enumerate(seqs):
            kv.prompt[s], kv.len[s], kv.g[s] = list(p), len(p), 1
        kv.live = len(seqs)
        self.log.append(("prefill", [list(p) for p in seqs], None, None))
        return kv, torch.tensor([_tok(p, 0) for p in seqs], dtype=torch.int32), None

    def fork(self, kv, counts):
        assert len(counts) == kv.live and all(c >= 1 for c in counts) and sum(counts) <= len(kv.g)
        src = [i for i, c in enumerate(counts) for _ in range(c)]
        kv.prompt, kv.len = [kv.prompt[i] for i in src], [kv.len[i] for i in src]
        kv.g, kv.live = [1] * len(src), len(src)
        self.log.append(("fork", None, list(counts), None))
        return len(src)

    def sample_last(self, kv, u, temperature, top_k=50):
        assert u.numel() == kv.live
        kv.g = [1] * kv.live
        return torch.tensor([_tok(kv.prompt[s], 0, u[s]) for s in range(kv.live)], dtype=torch.int32)

    def prefill_slots(self, kv, slots, seqs, feats, want_logits=False, u=None, temperature=1.0, top_k=50, counts=None):
        if any(POISON in p for p in seqs):
            raise ValueError("refused: poison token")
        counts = [1] * len(seqs) if counts is None else list(counts)
        assert len(counts) == len(seqs) and sum(counts) == len(slots) and (u is None or u.numel() == len(slots))
        assert len(set(slots)) == len(slots) and all(0 <= s < kv.live for s in slots)
        self.log.append(("prefill_slots", [list(p) for p in seqs], counts, list(slots)))
        out, j = [], 0
        for p, c in zip(seqs, counts):
            for _ in range(c):
                s = slots[j]
                kv.prompt[s], kv.g[s], kv.len[s] = list(p), 1, len(p)
                out.append(_tok(p, 0, None if u is None else u[j]))
                j += 1
        return torch.tensor(out, dtype=torch.int32), None

    def _decode(self, kv, n, eos_id, u):
        out = torch.zeros(kv.live, n, dtype=torch.int32)
        for s in range(kv.live):
            assert kv.len[s] + n <= kv.max_seq
            done = False
            for i in range(n):
                t = _tok(kv.prompt[s], kv.g[s], None if u is None else u[i, s])
                if done:
                    t = eos_id
                elif t == eos_id:
                    done = True
                out[s, i] = t
                kv.g[s] += 1
            kv.len[s] += n
        return out

    def decode_greedy(self, kv, first, n, eos_id=-1):
        return self._decode(kv, n, eos_id, None)

    def decode_sample(self, kv, first, n, eos_id, temperature, top_k, u):
        assert u.shape == (n, kv.live)
        return self._decode(kv, n, eos_id, u)

    def kv_len(self, kv, s):
        return kv.len[s]

    def kv_truncate(self, kv, s, length):
        kv.len[s] = length


class StrictModel(FakeModel):
    """The argument lists the model methods had before Task.samples: a call that passes `counts` or `capacity` is a TypeError."""

    def prefill(self, seqs, feats, max_seq):
        return FakeModel.prefill(self, seqs, feats, max_seq)

    def prefill_slots(self, kv, slots, seqs, feats, want_logits=False, u=None, temperature=1.0, top_k=50):
        return FakeModel.prefill_slots(self, kv, slots, seqs, feats, want_logits, u, temperature, top_k)

    def fork(self, kv, counts):
        raise AssertionError("no task asked for more than one sample")


def _tasks(samples, seed=0, budget=(3, 30)):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(samples):
        ids = [1] + torch.randint(3, 50, (int(torch.randint(3, 12, (1,), generator=g)),), generator=g).tolist()
        out.append(Task(i, ids, max_new_tokens=int(torch.randint(*budget, (1,), generator=g)), seed=1000 + 17 * i, samples=n))
    return out


def _started(m):
    """Prompts in the order the backend saw them start."""
    return [tuple(p) for kind, ps, _, _ in m.log if kind != "fork" for p in ps]


def test_sample_seed_keeps_sample_zero_on_the_task_stream():
    assert SAMPLE_SEED_STRIDE == 2 ** 20 and continuous.SAMPLE_SEED_STRIDE == 1048576
    assert sample_seed(12345, 0) == 12345 and sample_seed(7, 3) == 7 + 3 * 2 ** 20
    assert Task(0, [1]).samples == 1 and Task(0, [1], None, None, None, None, 4).samples == 4      # the new field is the last one


def test_every_sample_draws_from_its_own_stream_and_a_task_yields_once():
    m = FakeModel()
    tasks = _tasks([1, 3, 2, 1, 4, 2, 1, 3, 1, 2, 5, 1], seed=3)
    tms = {}
    got = list(generate_continuous(m, iter(tasks), 8, 30, do_sample=True, chunk=4, refill_min=1, timings=tms))
    assert sorted(tid for tid, _ in got) == [t.task_id for t in tasks]              # one yield per task
    got = dict(got)
    for t in tasks:
        want = [_sample_answer(t, j) for j in range(t.samples)]
        assert got[t.task_id] == (want if t.samples > 1 else want[0]), t.task_id
        assert (isinstance(tms[t.task_id], list) and len(tms[t.task_id]) == t.samples) if t.samples > 1 else isinstance(tms[t.task_id], dict)
    assert len(_started(m)) == len(tasks)                                           # every prompt ran once, whatever its samples
    # a task without a seed: base = the call's seed + its arrival index
    t = Task("x", [1, 9, 9], max_new_tokens=6, samples=2)
    got = dict(generate_continuous(FakeModel(), [Task("w", [1, 4], max_new_tokens=2), t], 4, 8, do_sample=True, seed=40))
    assert got["x"] == [_sample_answer(t, j, base=41) for j in range(2)]


def test_admission_is_first_in_first_out_and_the_head_waits_for_all_its_slots():
    m = FakeModel()
    tasks = _tasks([2, 3, 1, 1, 4, 1, 2], seed=5, budget=(6, 30))
    got = dict(generate_continuous(m, tasks, 4, 30, do_sample=True, chunk=3, refill_min=1, eos_token_id=None))
    assert all(got[t.task_id] == ([_answer(t.ids, t.max_new_tokens, task_uniforms(t.max_new_tokens, sample_seed(t.seed, j), CPU), eos=-1)
                                   for j in range(t.samples)] if t.samples > 1 else
                                  _answer(t.ids, t.max_new_tokens, task_uniforms(t.max_new_tokens, t.seed, CPU), eos=-1)) for t in tasks)
    assert _started(m) == [tuple(t.ids) for t in tasks]                             # nothing overtakes a waiting head
    # the opening group: task 0 alone (task 1 needs 3 of the 2 slots left), at full width so that task 1 fits later
    assert m.log[0][0] == "prefill" and len(m.log[0][1]) == 1 and m.log[1] == ("fork", None, [4], None)
    by_prompt = {tuple(p): (c, sl) for kind, ps, cn, sl in m.log if kind == "prefill_slots"
                 for p, c, sl in zip(ps, cn, [sl[sum(cn[:i]):sum(cn[:i + 1])] for i in range(len(cn))])}
    for t in tasks[1:]:
        c, sl = by_prompt[tuple(t.ids)]
        assert c == t.samples and len(sl) == t.samples, t.task_id                   # all its slots in one call
    assert max(len(sl) for kind, _, _, sl in m.log if kind == "prefill_slots") == 4 # task 4 waited for the whole group


def test_too_many_samples_and_greedy_samples_fail_alone():
    errors = {}
    tasks = _tasks([1, 5, 2, 1, 9, 1], seed=7)
    got = dict(generate_continuous(FakeModel(), tasks, 4, 30, do_sample=True, chunk=4, refill_min=1, on_error=lambda tid, e: errors.update({tid: str(e)})))
    assert got[1] is None and got[4] is None and sorted(errors) == [1, 4]
    assert "`samples`=5 exceeds the 4 slots" in errors[1] and "`samples`=9" in errors[4]
    for t in tasks:
        if t.task_id not in (1, 4):
            want = [_sample_answer(t, j) for j in range(t.samples)]
            assert got[t.task_id] == (want if t.samples > 1 else want[0])
    errors.clear()
    tasks = _tasks([1, 2, 1], seed=8)
    got = dict(generate_continuous(FakeModel(), tasks, 4, 30, chunk=4, on_error=lambda tid, e: errors.update({tid: str(e)})))
    assert got[1] is None and list(errors) == [1] and "`samples_per_prompt`=2 needs do_sample=True" in errors[1]
    assert got[0] == _answer(tasks[0].ids, tasks[0].max_new_tokens) and got[2] == _answer(tasks[2].ids, tasks[2].max_new_tokens)
    errors.clear()
    got = dict(generate_continuous(FakeModel(), [Task(0, [1, 5], max_new_tokens=3, samples=0), Task(1, [1, 6], max_new_tokens=3, samples=True)], 2, 8,
                                   do_sample=True, on_error=lambda tid, e: errors.update({tid: str(e)})))
    assert got == {0: None, 1: None} and all("integer >= 1" in v for v in errors.values())


def test_a_refused_task_with_samples_costs_only_itself():
    m = FakeModel()
    tasks = _tasks([2, 1, 2, 3, 2, 1, 2, 2, 1, 3], seed=9)
    tasks[6].ids = tasks[6].ids + [POISON]                  # a refill: the backend refuses the call, the scheduler isolates the task
    errors = []
    got = dict(generate_continuous(m, tasks, 6, 30, do_sample=True, chunk=4, refill_min=3, on_error=lambda tid, e: errors.append(tid)))
    assert got[6] is None and errors == [6] and len(got) == len(tasks)
    for t in tasks:
        if t.task_id != 6:
            want = [_sample_answer(t, j) for j in range(t.samples)]
            assert got[t.task_id] == (want if t.samples > 1 else want[0]), t.task_id


@pytest.mark.parametrize("do_sample", [False, True])
def test_single_sample_runs_never_pass_the_new_keywords(do_sample):
    m = StrictModel()
    tasks = _tasks([1] * 30, seed=11)
    got = dict(generate_continuous(m, iter(tasks), 8, 30, do_sample=do_sample, chunk=4, refill_min=2))
    for t in tasks:
        assert got[t.task_id] == (_sample_answer(t, 0) if do_sample else _answer(t.ids, t.max_new_tokens)), t.task_id
    assert all(cn == [1] * len(ps) for kind, ps, cn, _ in m.log if kind == "prefill_slots") and m.log[0][0] == "prefill" and len(m.log[0][1]) == 8


def test_prefill_plan_sample_maps_and_refusals(tmp_path):
    """csrc/prefill_plan.h compiled on its own: counts [3, 1, 2] over slots [6, 0, 3, 7, 5, 1] -- the sample -> sequence map, every sample's last
    row, length and slot, the rows of a sequence going to the FIRST slot of its run -- and the refusals of a count below 1, more samples than the
    group is wide, a slot listed twice or outside the group."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    csrc = os.path.join(ROOT, "video_llava_amd", "csrc")
    prog = r"""#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "prefill_plan.h"
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad = 1; } } while (0)
typedef std::initializer_list<int> L;
static bool sec(const std::vector<int>& meta, size_t off, size_t end, L want) {
    if (end - off != want.size() || end > meta.size()) return false;
    size_t i = off;
    for (int v : want) if (meta[i++] != v) return false;
    return true;
}
static const int lens[3] = {1, 3, 2}, ids[6] = {5, 6, 7, 8, 9, 10};
static std::vector<int> meta;
static PrefillPlan plan;
static char err[256];
static PrefillRows rows(const int* slots, const int* counts, int active) {
    PrefillRows r;
    r.who = "who"; r.ids = ids; r.seq_lens = lens; r.B = 3; r.vocab = 20; r.max_seq = 16; r.hidden = 4; r.slots = slots; r.counts = counts; r.active = active;
    return r;
}
static bool refused(const PrefillRows& r, const char* msg) {
    err[0] = 0;
    const bool hit = prefill_plan_build(r, meta, plan, err, sizeof(err)) == PLAN_EINVAL && !strncmp(err, "who: ", 5) && strstr(err, msg);
    if (!hit) printf("got \"%s\", want \"%s\"\n", err, msg);
    return hit;
}
int main() {
    const int slots[6] = {6, 0, 3, 7, 5, 1}, counts[3] = {3, 1, 2};
    {
        const PrefillLayout lo(6, 3, 0, 6);
        EXPECT(lo.samp_seq == lo.stgts && lo.samp_last == lo.samp_seq + 6 && lo.samp_lens == lo.samp_last + 6 && lo.samp_slots == lo.samp_lens + 6 && lo.total == lo.samp_slots + 6);
        EXPECT(PrefillLayout(6, 3, 0).total == lo.total - 24 && PrefillLayout(6, 3, 0).samp_slots == PrefillLayout(6, 3, 0).total);
    }
    {
        err[0] = 0;
        EXPECT(prefill_plan_build(rows(slots, counts, 8), meta, plan, err, sizeof(err)) == PLAN_OK && !err[0]);
        const PrefillLayout& lo = plan.lo;
        EXPECT(plan.M == 6 && plan.S == 6 && plan.max_len == 3 && meta.size() == lo.total);
        EXPECT(sec(meta, lo.samp_seq, lo.samp_last, {0, 0, 0, 1, 2, 2}));
        EXPECT(sec(meta, lo.samp_last, lo.samp_lens, {0, 0, 0, 3, 5, 5}));
        EXPECT(sec(meta, lo.samp_lens, lo.samp_slots, {1, 1, 1, 3, 2, 2}));
        EXPECT(sec(meta, lo.samp_slots, lo.total, {6, 0, 3, 7, 5, 1}));
        EXPECT(sec(meta, lo.slots, lo.raw_ids, {6, 7, 5}) && sec(meta, lo.row_b, lo.row_pos, {6, 7, 7, 7, 5, 5}));        // the first slot of every run
        EXPECT(sec(meta, lo.cu, lo.last, {0, 1, 4, 6}) && sec(meta, lo.last, lo.lens, {0, 3, 5}) && sec(meta, lo.lens, lo.offs, {1, 3, 2}));
        EXPECT(plan.attn_flops == 2.0 * (1 + 9 + 4) * 4);                                                                // the sequences' rows once
        EXPECT(prefill_plan_build(rows(slots, counts, 6), meta, plan, err, sizeof(err)) == PLAN_EINVAL);                // slots 6 and 7 lie outside a group of 6
    }
    {   // without counts nothing changes: one slot per sequence, no sample sections
        err[0] = 0;
        EXPECT(prefill_plan_build(rows(slots, nullptr, 8), meta, plan, err, sizeof(err)) == PLAN_OK && plan.S == 0 && plan.lo.samp_seq == plan.lo.total);
        EXPECT(sec(meta, plan.lo.slots, plan.lo.raw_ids, {6, 0, 3}));
    }
    {
        const int zero[3] = {3, 0, 2}, neg[3] = {-1, 1, 1}, wide[3] = {3, 1, 5}, fits[3] = {3, 1, 4};
        const int eight[8] = {6, 0, 3, 7, 5, 1, 2, 4}, twice[6] = {6, 0, 3, 7, 0, 1}, out[6] = {6, 0, 3, 7, 8, 1}, below[6] = {6, 0, -1, 7, 5, 1};
        EXPECT(refused(rows(slots, zero, 8), "count 0 of sequence 1 is below 1"));
        EXPECT(refused(rows(slots, neg, 8), "count -1 of sequence 0 is below 1"));
        EXPECT(refused(rows(eight, wide, 8), "9 samples up to sequence 2 for a live group of 8"));
        err[0] = 0;
        EXPECT(prefill_plan_build(rows(eight, fits, 8), meta, plan, err, sizeof(err)) == PLAN_OK && plan.S == 8);
        EXPECT(refused(rows(twice, counts, 8), "slot 0 listed twice"));
        EXPECT(refused(rows(out, counts, 8), "slot 8 outside the 8 of the live group"));
        EXPECT(refused(rows(below, counts, 8), "slot -1 outside the 8 of the live group"));
        EXPECT(refused(rows(nullptr, counts, 8), "sample counts without a slot list"));
    }
    if (!bad) printf("OK\n");
    return bad;
}
"""
    cpp, exe = tmp_path / "plan_n.cpp", tmp_path / "plan_n"
    cpp.write_text(prog)
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", csrc, str(cpp), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and r.stdout == "OK\n", (r.returncode, r.stdout, r.stderr[-2000:])


def test_runner_flags_and_the_majority_vote():
    from video_llava_amd.eval import run_inference_qa_activitynet as qa
    from video_llava_amd.inference import best_sample, majority_sample
    base = ["--video_dir", "v", "--gt_file_question", "q", "--gt_file_answers", "a", "--output_dir", "o", "--output_name", "n", "--model-name", "x",
            "--projection_path", "y"]
    a = qa.parse_args(base)
    assert a.samples_per_prompt == 1 and a.sample_pick == "best" and a.samples_out is None
    a = qa.parse_args(base + ["--schedule", "refill", "--do_sample", "--samples_per_prompt", "4", "--sample_pick", "majority", "--samples_out", "s.jsonl"])
    assert a.samples_per_prompt == 4 and a.sample_pick == "majority" and a.samples_out == "s.jsonl"
    for bad in (["--samples_per_prompt", "2"], ["--samples_per_prompt", "2", "--schedule", "refill"], ["--samples_per_prompt", "2", "--do_sample"],
                ["--samples_per_prompt", "0"], ["--schedule", "refill", "--do_sample", "--samples_per_prompt", "5", "--batch", "4"],
                ["--schedule", "refill", "--do_sample", "--samples_per_prompt", "2", "--sample_pick", "first"]):
        with pytest.raises(SystemExit):
            qa.parse_args(base + bad)
    s = [{"text": "a", "logprob": -1.0}, {"text": "b", "logprob": -0.1}, {"text": "a", "logprob": -3.0}, {"text": "c", "logprob": -0.2}]
    assert majority_sample(s) == 0 and best_sample(s) == 1                          # the most frequent string, its first sample
    s = [{"text": "a", "logprob": -2.0}, {"text": "b", "logprob": -0.5}, {"text": "b", "logprob": -2.5}, {"text": "a", "logprob": -0.5}]
    assert majority_sample(s) == 0                                                  # 2 : 2 -> the sums -2.5 against -3.0
    s = [{"text": "b", "logprob": -1.0}, {"text": "a", "logprob": -1.0}]
    assert majority_sample(s) == 0                                                  # a full tie goes to the first
    with pytest.raises(ValueError):
        majority_sample([])
