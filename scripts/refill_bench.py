"""Static groups against continuous batching (slot refill) on ragged answer lengths, at PG-Video-LLaVA-7B shapes with random weights.

Every task is a ~600-token prompt with a 356-row video run and its own token budget (EOS off, so the budget is the answer length):
  short: budgets drawn from 5..64;   tail: the same, but ~5 % of the tasks run to max_new_tokens = 1024.
`static`: groups of --width tasks through model.generate, each group decoding until its longest answer ends (what the runners' default
--schedule group does).  `refill`: the same tasks through video_llava_amd.continuous.generate_continuous with --width slots.  Checks that every
task's ids are identical between the two and prints one JSON line: answers/s of both schedules per distribution (short runs twice, alternated).

    python scripts/refill_bench.py [--tasks 256] [--width 64] [--refill-min K] [--dists short,tail]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VOCAB, V_ROWS = 32003, 356


def build_model(layers: int, device):
    from video_llava_amd import random_init as ri
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    cfg = VideoChatGPTConfig(vocab_size=VOCAB, hidden_size=4096, intermediate_size=11008, num_hidden_layers=layers, num_attention_heads=32,
                             eos_token_id=None)
    m = VideoChatGPTLlamaForCausalLM(cfg, VisionConfig(frame_size=224), torch.bfloat16, device)
    ri.load_streaming(m, ri.iter_llama_tensors(vocab=VOCAB, hidden=4096, inter=11008, layers=layers, device=str(device), dtype=torch.bfloat16, seed=11))
    vc = m.get_model().vision_config
    vc.vid_patch_token, vc.vid_start_token, vc.vid_end_token, vc.use_vid_start_end = VOCAB - 3, VOCAB - 2, VOCAB - 1, True
    return m


def make_tasks(n: int, dist: str, max_new: int, seed: int, device):
    from video_llava_amd.continuous import Task
    rng = np.random.default_rng(seed)
    budgets = rng.integers(5, 65, n)
    if dist == "tail":
        budgets[rng.random(n) < 0.05] = max_new
    tasks = []
    for i in range(n):
        ids = [1] + rng.integers(3, VOCAB - 3, int(rng.integers(225, 250))).tolist() + [VOCAB - 2] + [VOCAB - 3] * V_ROWS + [VOCAB - 1] \
            + rng.integers(3, VOCAB - 3, 6).tolist()
        feats = torch.from_numpy(rng.standard_normal((V_ROWS, 1024)).astype(np.float32) * 0.5).to(torch.float16).to(device)
        tasks.append(Task(i, ids, feats, max_new_tokens=int(budgets[i])))
    return tasks


def run_static(m, tasks, width):
    out = {}
    for g0 in range(0, len(tasks), width):
        grp = tasks[g0:g0 + width]
        n = max(t.max_new_tokens for t in grp)
        ids = m.generate([t.ids for t in grp], video_spatio_temporal_features=torch.stack([t.feats for t in grp]), max_new_tokens=n).cpu()
        for r, t in enumerate(grp):
            out[t.task_id] = ids[r, len(t.ids):len(t.ids) + t.max_new_tokens].tolist()
    return out


def run_refill(m, tasks, width, max_new, refill_min):
    from video_llava_amd.continuous import generate_continuous
    return dict(generate_continuous(m, iter(tasks), width, max_new, refill_min=refill_min))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tasks", type=int, default=256)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--max-new-tokens", type=int, default=1024)
    ap.add_argument("--refill-min", type=int, default=None, help="generate_continuous refill_min (default: its own)")
    ap.add_argument("--dists", default="short,tail")
    ap.add_argument("--repeats", type=int, default=2, help="alternated static / refill runs of `short`")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    res = {"width": a.width, "tasks": a.tasks, "layers": a.layers, "refill_min": a.refill_min}
    for dist in a.dists.split(","):
        tasks = make_tasks(a.tasks, dist, a.max_new_tokens, 1 if dist == "short" else 2, dev)
        run_refill(m, tasks[:a.width + 4], a.width, a.max_new_tokens, a.refill_min)        # warm-up: graphs, workspace
        reps = a.repeats if dist == "short" else 1
        rows, ref = [], None
        for _ in range(reps):
            for name, fn in (("static", lambda: run_static(m, tasks, a.width)), ("refill", lambda: run_refill(m, tasks, a.width, a.max_new_tokens, a.refill_min))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ref = got if ref is None else ref
                rows.append({"schedule": name, "s": round(dt, 3), "answers_per_s": round(len(tasks) / dt, 3), "identical": got == ref})
                print(f"[refill_bench] {dist} {name}: {dt:.2f} s", file=sys.stderr, flush=True)
        best = {s: max(r["answers_per_s"] for r in rows if r["schedule"] == s) for s in ("static", "refill")}
        res[dist] = {"runs": rows, "static_answers_per_s": best["static"], "refill_answers_per_s": best["refill"],
                     "speedup": round(best["refill"] / best["static"], 3), "identical_ids": all(r["identical"] for r in rows),
                     "tokens": int(sum(t.max_new_tokens for t in tasks))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
