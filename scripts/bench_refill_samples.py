"""What Task.samples saves in the continuous-batching runner: n sampled answers per task from ONE prefill against the task queued n times, at
PG-Video-LLaVA-7B shapes with random bf16 weights (the setup of scripts/refill_bench.py: ~600-token prompts with a 356-row video run, EOS off,
budgets 5..64, 64 slots).

For n in --samples (default 2,4,8), over --answers / n prompts:
  (a) `queued`:  every prompt queued n times, copy j seeded sample_seed(base, j)      -- n prefills per prompt
  (b) `samples`: every prompt once with Task.samples = n                               -- one prefill, pgv_llm_prefill_slots_n / pgv_kv_fork
alternated --rounds times; asserts that every answer's ids are identical between the two and prints one JSON line with the median answers/s of
both, their spread and the prompts each prefilled.

--parent ROOT: also the n = 1 workload (every task one sample) on this tree and on the tree at ROOT (a checkout of the parent commit with its
library built), alternated round by round between two worker processes that each hold their own model; the ids must be identical too.

    python scripts/bench_refill_samples.py [--answers 256] [--samples 2,4,8] [--rounds 7] [--parent ../parent-checkout]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def _tasks(n_prompts: int, device, **extra):
    """refill_bench's `short` tasks with fixed seeds; extra: further Task fields."""
    from refill_bench import make_tasks
    from video_llava_amd.continuous import Task
    return [Task(t.task_id, t.ids, t.feats, max_new_tokens=t.max_new_tokens, seed=7000003 + 31 * i, **extra)
            for i, t in enumerate(make_tasks(n_prompts, "short", 1024, 1, device))]


class _Counting:
    """The model with the prompts of every prefill / prefill_slots call counted."""

    def __init__(self, m):
        self._m, self.prompts = m, 0

    def __getattr__(self, name):
        return getattr(self._m, name)

    def prefill(self, seqs, *a, **k):
        self.prompts += len(seqs)
        return self._m.prefill(seqs, *a, **k)

    def prefill_slots(self, kv, slots, seqs, *a, **k):
        self.prompts += len(seqs)
        return self._m.prefill_slots(kv, slots, seqs, *a, **k)


def _timed(m, tasks, width):
    import torch
    from video_llava_amd.continuous import generate_continuous
    cm = _Counting(m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = dict(generate_continuous(cm, iter(tasks), width, 1024, do_sample=True, temperature=0.2, top_k=50))
    torch.cuda.synchronize()
    return got, time.perf_counter() - t0, cm.prompts


def _median_spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def worker(a):
    """--worker: build the model of the tree this file's package was imported from, then one timed n = 1 run per line on stdin."""
    import torch
    import video_llava_amd                      # from --root, before refill_bench puts its own tree on the path
    from refill_bench import build_model
    print(f"[bench_refill_samples] worker of {os.path.dirname(video_llava_amd.__file__)}", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    tasks = _tasks(a.answers, dev)
    _timed(m, tasks[:a.width + 4], a.width)
    print("ready", flush=True)
    for _ in sys.stdin:
        got, dt, prompts = _timed(m, tasks, a.width)
        digest = hashlib.sha256(json.dumps([got[t.task_id] for t in tasks]).encode()).hexdigest()
        print(json.dumps({"s": dt, "prompts": prompts, "ids_sha256": digest}), flush=True)


def n1_against_parent(a):
    """Two workers, this tree and the parent's, one timed run each per round, this tree first in even rounds and second in odd ones."""
    roots = {"this": os.path.dirname(HERE), "parent": os.path.abspath(a.parent)}
    procs = {}
    for name, root in roots.items():
        env = dict(os.environ, PYTHONPATH=root)
        procs[name] = subprocess.Popen([sys.executable, os.path.join(HERE, "bench_refill_samples.py"), "--worker", "--root", root, "--answers", str(a.answers),
                                        "--width", str(a.width), "--layers", str(a.layers)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
    try:
        for name, p in procs.items():
            line = p.stdout.readline().strip()
            if line != "ready":
                raise RuntimeError(f"worker {name} did not start: {line!r}")
        runs = {"this": [], "parent": []}
        for r in range(a.rounds):
            for name in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
                procs[name].stdin.write("go\n")
                procs[name].stdin.flush()
                runs[name].append(json.loads(procs[name].stdout.readline()))
                print(f"[bench_refill_samples] n=1 {name} round {r}: {runs[name][-1]['s']:.2f} s", file=sys.stderr, flush=True)
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=120)
    digests = {x["ids_sha256"] for v in runs.values() for x in v}
    assert len(digests) == 1, "the n = 1 ids differ between this tree and the parent"
    out = {name: _median_spread([a.answers / x["s"] for x in v]) for name, v in runs.items()}
    out["ratio_this_over_parent"] = round(out["this"]["median"] / out["parent"]["median"], 4)
    out["identical_ids"] = True
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--answers", type=int, default=256, help="answers per run (prompts = answers / n)")
    ap.add_argument("--samples", default="2,4,8")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--parent", default=None, metavar="ROOT", help="a checkout of the parent commit (library built) for the n = 1 comparison")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    sys.path[:0] = [a.root, HERE]
    if a.worker:
        return worker(a)
    res = {"width": a.width, "answers": a.answers, "layers": a.layers, "rounds": a.rounds}
    ns = [int(x) for x in a.samples.split(",") if x]
    if a.parent:                                # first: the workers start from a process that has not touched the device
        res["n1"] = n1_against_parent(a)
    if ns:
        import torch
        from refill_bench import build_model
        from video_llava_amd.continuous import Task, sample_seed
        dev = torch.device("cuda", 0)
        m = build_model(a.layers, dev)
        for n in ns:
            base = _tasks(max(1, a.answers // n), dev)
            queued = [Task((t.task_id, j), t.ids, t.feats, max_new_tokens=t.max_new_tokens, seed=sample_seed(t.seed, j)) for t in base for j in range(n)]
            sampled = [Task(t.task_id, t.ids, t.feats, max_new_tokens=t.max_new_tokens, seed=t.seed, samples=n) for t in base]
            _timed(m, sampled[:a.width // n + 2], a.width)                       # warm-up: graphs, workspace
            rate = {"queued": [], "samples": []}
            prompts = {}
            for r in range(a.rounds):
                for name in (("queued", "samples") if r % 2 == 0 else ("samples", "queued")):
                    got, dt, prompts[name] = _timed(m, queued if name == "queued" else sampled, a.width)
                    ids = [got[t.task_id, j] for t in base for j in range(n)] if name == "queued" else [x for t in base for x in got[t.task_id]]
                    if r == 0 and name == "queued":
                        ref = ids
                    assert ids == ref, f"n = {n}: the ids of `{name}` differ from the first queued run"
                    rate[name].append(len(ids) / dt)
                    print(f"[bench_refill_samples] n={n} {name} round {r}: {dt:.2f} s", file=sys.stderr, flush=True)
            res[f"n{n}"] = {"prompts": len(base), "answers": len(base) * n, "identical_ids": True, "prompts_prefilled": prompts,
                            "queued_answers_per_s": _median_spread(rate["queued"]), "samples_answers_per_s": _median_spread(rate["samples"]),
                            "speedup": round(statistics.median(rate["samples"]) / statistics.median(rate["queued"]), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
