"""What the filter tail of the sampled pick costs per token step: generate()'s stepping calls with and without `filters`, at PG-Video-LLaVA-7B
shapes with random bf16 weights.  No gate: it measures.

8 sequences of one 461-token prompt (356-row video run), 256 timed steps, cache of 768 positions, temperature 0.2.  Configurations:
  off          pgv_llm_decode_sample, top_k 50 -- the path as it was before the filters existed (the number to hold against an older commit);
  top_p        the same with top_p 0.9: what the nucleus select, the existing stage of the same kind, costs behind top-k 50;
  min_p        min_p 0.05 alone behind top-k 50: one statistics pass;
  all4         min_p 0.05, typical_p 0.9, epsilon_cutoff 3e-4, eta_cutoff 2e-3 behind top-k 50;
  off_k0       top_k 0: the baseline of the two whole-vocabulary configurations;
  top_p_k0     top_p 0.9 on the whole vocabulary;
  typical_k0   typical_p 0.9 on the whole vocabulary: the most expensive route (statistics pass, four mass-histogram passes, band pass).
Every run: prefill, the first pick, 9 untimed steps (they capture the two decode graphs of the configuration), then ONE stepping call of 256 steps
timed with an event pair on the stream.  The configurations alternate over `--repeats` rounds after one warm-up round; medians, minima and maxima are
reported as ms per token step -- the min-max range of a configuration is its run-to-run spread.  On a tree without `filters` (an older commit, for
the comparison of the off numbers: --package-root) only the configurations without them run.  One JSON line on stdout.

    python scripts/bench_filters.py [--repeats 5] [--layers 32] [--steps 256] [--package-root DIR] [--only off,off_k0]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

BATCH, MAX_SEQ, WARM = 8, 768, 9
# name -> (top_k, top_p, filters)
CONFIGS = {"off": (50, 1.0, None), "top_p": (50, 0.9, None), "min_p": (50, 1.0, {"min_p": 0.05}),
           "all4": (50, 1.0, {"min_p": 0.05, "typical_p": 0.9, "epsilon_cutoff": 3e-4, "eta_cutoff": 2e-3}),
           "off_k0": (0, 1.0, None), "top_p_k0": (0, 0.9, None), "typical_k0": (0, 1.0, {"typical_p": 0.9})}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--package-root", default=None, help="import video_llava_amd from this tree (built there) instead of the script's own")
    ap.add_argument("--only", default=None, help="comma-separated configuration names (default: all the tree supports)")
    a = ap.parse_args(argv)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    import video_llava_amd                      # bound before the helper scripts put their own tree in front
    print(f"[bench_filters] package: {os.path.dirname(video_llava_amd.__file__)}", file=sys.stderr, flush=True)
    from scripts.bench_fork import PROMPT_TOKENS, make_prompt
    from scripts.refill_bench import V_ROWS, build_model
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    has_filters = hasattr(m, "set_filters")
    ids, feats = make_prompt(5, dev)
    prompts, feats8 = [ids] * BATCH, feats.expand(BATCH, -1, -1).contiguous()
    N = a.steps
    assert PROMPT_TOKENS + 1 + WARM + N <= MAX_SEQ
    u = torch.rand(1 + WARM + N, BATCH, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def run(name):
        top_k, top_p, filters = CONFIGS[name]
        kv, nxt, _ = m.prefill(prompts, feats8, MAX_SEQ)
        try:
            if filters:
                m.set_filters(kv, filters)
            nxt = m.sample_last(kv, u[0], 0.2, top_k, top_p)
            toks = m.decode_sample(kv, nxt, WARM, -1, 0.2, top_k, u[1:1 + WARM], top_p)
            first = toks[:, WARM - 1].contiguous()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            m.decode_sample(kv, first, N, -1, 0.2, top_k, u[1 + WARM:1 + WARM + N], top_p)
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]) / N
        finally:
            if filters:
                m.set_filters(kv, None)
            m.set_warpers(kv, 1.0, 1.0)

    names = [n for n, c in CONFIGS.items() if has_filters or c[2] is None]
    if a.only:
        names = [n for n in names if n in a.only.split(",")]
    times = {n: [] for n in names}
    for rnd in range(a.repeats + 1):
        for n in names:
            t = run(n)
            if rnd > 0:
                times[n].append(t)
    med = {n: statistics.median(t) for n, t in times.items()}
    res = {"prompt_tokens": PROMPT_TOKENS, "video_rows": V_ROWS, "batch": BATCH, "layers": a.layers, "steps": N, "repeats": a.repeats, "has_filters": has_filters,
           "ms_per_step": {n: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for n, t in times.items()}}
    extra = {}
    for n, base in (("top_p", "off"), ("min_p", "off"), ("all4", "off"), ("top_p_k0", "off_k0"), ("typical_k0", "off_k0")):
        if n in med and base in med:
            extra[f"{n}_minus_{base}_ms"] = round(med[n] - med[base], 4)
    res["cost"] = extra
    for n in names:
        print(f"[bench_filters] {n}: {med[n]:.4f} ms/step (min {min(times[n]):.4f}, max {max(times[n]):.4f})", file=sys.stderr, flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
