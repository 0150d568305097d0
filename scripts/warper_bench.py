"""Cost of the sampled decode step with and without top-p / repetition penalty, at PG-Video-LLaVA-7B shapes with random weights.

For each group width (default 8 and 64): prefill ~600-token prompts with a 356-row video run, then time `--steps` sampled decode steps
(model.decode_sample: the captured 8-step graphs, one host call) for every configuration (top_p, repetition_penalty) in (1, 1), (0.6, 1),
(0.6, 1.2) at top_k = 50 and top_k = 0.  Every timed run starts from a fresh prefill of the same prompts (not timed), configurations are
interleaved round-robin over `--repeats` rounds after one warm-up round, and the median per configuration is reported in ms per step,
next to its difference to the (1, 1) line of the same top_k.  One JSON line on stdout.

The script only uses arguments the tree it runs in knows: in a checkout that predates the two parameters it measures the (1, 1)
configurations alone (`--configs neutral`), which is how the parent commit's step is measured on the same machine in the same session.

    python scripts/warper_bench.py [--widths 8,64] [--steps 256] [--repeats 5] [--configs all|neutral] [--top-ks 50,0] [--layers 32]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/warper_bench.py --widths 8 --repeats 1 --top-ks 50     # per-kernel times (its own run)
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.refill_bench import VOCAB, V_ROWS, build_model      # noqa: E402

TEMPERATURE = 0.2


def make_prompts(n: int, seed: int, device):
    rng = np.random.default_rng(seed)
    prompts, feats = [], []
    for _ in range(n):
        prompts.append([1] + rng.integers(3, VOCAB - 3, int(rng.integers(225, 250))).tolist() + [VOCAB - 2] + [VOCAB - 3] * V_ROWS + [VOCAB - 1]
                       + rng.integers(3, VOCAB - 3, 6).tolist())
        feats.append(torch.from_numpy(rng.standard_normal((V_ROWS, 1024)).astype(np.float32) * 0.5).to(torch.float16))
    return prompts, torch.stack(feats).to(device)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--widths", default="8,64")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--configs", choices=("all", "neutral"), default="all")
    ap.add_argument("--top-ks", default="50,0", help="the top_k values to run (a kernel trace of one value keeps its launches apart)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    has_warpers = "top_p" in inspect.signature(m.decode_sample).parameters
    configs = [(k, p, r) for k in [int(x) for x in a.top_ks.split(",")] for p, r in ((1.0, 1.0), (0.6, 1.0), (0.6, 1.2))]
    if a.configs == "neutral" or not has_warpers:
        configs = [c for c in configs if c[1:] == (1.0, 1.0)]
    res = {"steps": a.steps, "layers": a.layers, "repeats": a.repeats, "temperature": TEMPERATURE, "has_warpers": has_warpers, "widths": {}}
    for B in [int(x) for x in a.widths.split(",")]:
        prompts, feats = make_prompts(B, 3, dev)
        max_seq = (max(len(p) for p in prompts) + a.steps + 1 + 63) // 64 * 64
        u = torch.rand(a.steps + 1, B, device=dev, generator=torch.Generator(device=dev).manual_seed(7))

        def run(top_k, top_p, pen):
            kw = {"top_p": top_p, "repetition_penalty": pen} if has_warpers else {}
            kv, _nxt, _ = m.prefill(prompts, feats, max_seq)
            first = m.sample_last(kv, u[0], TEMPERATURE, top_k, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks = m.decode_sample(kv, first, a.steps, -1, TEMPERATURE, top_k, u[1:], **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.steps, toks

        times = {c: [] for c in configs}
        for rnd in range(a.repeats + 1):                              # round 0: warm-up (code objects, graph capture per configuration)
            for c in configs:
                ms, _ = run(*c)
                if rnd > 0:
                    times[c].append(ms)
        rows = []
        for c in configs:
            med = statistics.median(times[c])
            base = statistics.median(times[(c[0], 1.0, 1.0)])
            rows.append({"top_k": c[0], "top_p": c[1], "repetition_penalty": c[2], "ms_per_step_median": round(med, 4),
                         "ms_per_step_min": round(min(times[c]), 4), "ms_per_step_max": round(max(times[c]), 4),
                         "delta_vs_neutral_ms": round(med - base, 4), "delta_vs_neutral_pct": round(100.0 * (med - base) / base, 3)})
            print(f"[warper_bench] B={B} top_k={c[0]} top_p={c[1]} penalty={c[2]}: {med:.4f} ms/step "
                  f"(min {min(times[c]):.4f}, max {max(times[c]):.4f})", file=sys.stderr, flush=True)
        res["widths"][str(B)] = rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
