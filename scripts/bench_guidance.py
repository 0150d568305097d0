"""What classifier-free guidance costs per token step: generate()'s stepping calls plain and guided, at PG-Video-LLaVA-7B shapes with random bf16
weights.  No gate: it measures.

P prompts of 461 tokens (356-row video run), the no-video negative of each (the same ids without the placeholder run: 103 tokens), 256 timed steps,
cache of 768 positions, P in {1, 8, 32}.  Configurations per P, sampled (temperature 0.2, top_k 50: the reference's default mode, and the same pick
kernel plain and guided) and greedy:
  plain_P      the P prompts alone at width P -- the call without `guidance`;
  plain_2P     prompts + negatives as a plain group of width 2P: the trunk, lm_head and pick a guided step also runs (the pick over 2P rows, not P);
  guided_P     P pairs, scale 1.5: plain_2P's trunk and lm_head, the mix kernel, the pick over P guided rows, the follow kernel.
The expectation to confirm or refute: guided_P = plain_2P + the two launches.  For greedy the pick route differs as well (plain: the arg-max of the
lm_head candidates; guided: the sample-route pick that greedy under a penalty takes), so the sampled rows are the like-for-like comparison.
Every run: prefill, the first pick, 9 untimed steps (they capture the two decode graphs of the configuration), then ONE stepping call of 256 steps
timed with an event pair on the stream.  The configurations alternate over `--repeats` rounds after one warm-up round; medians, minima and maxima are
reported as ms per token step -- the min-max range of a configuration is its run-to-run spread.  On a tree without guidance (an older commit, for
the comparison of the plain numbers: --package-root) only the plain configurations run.  One JSON line on stdout.

    python scripts/bench_guidance.py [--repeats 3] [--layers 32] [--steps 256] [--pairs 1,8,32] [--package-root DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

MAX_SEQ, WARM, SCALE = 768, 9, 1.5


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--pairs", default="1,8,32")
    ap.add_argument("--package-root", default=None, help="import video_llava_amd from this tree (built there) instead of the script's own")
    a = ap.parse_args(argv)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    import video_llava_amd                      # bound before the helper scripts put their own tree in front
    print(f"[bench_guidance] package: {os.path.dirname(video_llava_amd.__file__)}", file=sys.stderr, flush=True)
    from scripts.bench_fork import PROMPT_TOKENS, make_prompt
    from scripts.refill_bench import V_ROWS, VOCAB, build_model
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    has_guidance = hasattr(m, "set_guidance")
    ids, feats = make_prompt(5, dev)
    neg = [t for t in ids if t < VOCAB - 3]                 # "no_video": the prompt without its placeholder run
    N = a.steps
    assert PROMPT_TOKENS + 1 + WARM + N <= MAX_SEQ

    def run(name, P):
        kind, sampled = name.split("/")
        sampled = sampled == "sampled"
        W = P if kind == "plain_P" else 2 * P
        seqs = [ids] * P + ([neg] * P if W > P else [])
        f = feats.expand(P, -1, -1)
        f = torch.cat([f, torch.zeros_like(f)]) if W > P else f
        u = torch.rand(1 + WARM + N, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        kv, nxt, _ = m.prefill(seqs, f.contiguous(), MAX_SEQ)
        if kind == "guided_P":
            m.set_guidance(kv, SCALE, P)
        try:
            if sampled:
                step = lambda first, n, at: m.decode_sample(kv, first, n, -1, 0.2, 50, u[at:at + n])      # noqa: E731
                nxt = m.sample_last(kv, u[0], 0.2, 50)
            else:
                step = lambda first, n, at: m.decode_greedy(kv, first, n, -1)                                # noqa: E731
                if kind == "guided_P":
                    nxt = m.greedy_last(kv, W)
            toks = step(nxt, WARM, 1)
            first = toks[:, WARM - 1].contiguous()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            step(first, N, 1 + WARM)
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]) / N
        finally:
            if kind == "guided_P":
                m.set_guidance(kv, 1.0, 0)

    kinds = ["plain_P", "plain_2P"] + (["guided_P"] if has_guidance else [])
    names = [f"{k}/{mode}" for mode in ("sampled", "greedy") for k in kinds]
    res = {"prompt_tokens": PROMPT_TOKENS, "negative_tokens": len(neg), "video_rows": V_ROWS, "layers": a.layers, "steps": N, "repeats": a.repeats,
           "scale": SCALE, "has_guidance": has_guidance, "ms_per_step": {}}
    for P in [int(x) for x in a.pairs.split(",")]:
        times = {n: [] for n in names}
        for rnd in range(a.repeats + 1):
            for n in names:
                t = run(n, P)
                if rnd > 0:
                    times[n].append(t)
        med = {n: statistics.median(t) for n, t in times.items()}
        row = {n: {"median": round(med[n], 4), "min": round(min(t), 4), "max": round(max(t), 4)} for n, t in times.items()}
        if has_guidance:
            for mode in ("sampled", "greedy"):
                row[f"guided_minus_plain_2P/{mode}"] = round(med[f"guided_P/{mode}"] - med[f"plain_2P/{mode}"], 4)
        res["ms_per_step"][str(P)] = row
        for n in names:
            print(f"[bench_guidance] P={P} {n}: {med[n]:.4f} ms/step (min {min(times[n]):.4f}, max {max(times[n]):.4f})", file=sys.stderr, flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
