"""What logit bans cost per token step: generate()'s stepping calls with and without `bans`, at PG-Video-LLaVA-7B shapes with random bf16 weights.
No gate: it measures.

8 sequences of one 461-token prompt (356-row video run), 256 timed steps, cache of 768 positions.  Configurations:
  greedy_off   pgv_llm_decode_greedy, the arg-max of the lm_head candidates -- the path as it was before bans existed;
  greedy_pen   greedy under repetition_penalty 1.1, no bans: the pick_greedy route (sample kernel over the penalised logits) that greedy under
               bans also takes -- the known price of leaving the candidate arg-max;
  greedy_on    greedy with no_repeat_ngram = 3 + min_new_tokens = 8;
  sampled_off  pgv_llm_decode_sample, temperature 0.2, top_k 50;
  sampled_on   the same with the bans.
sampled_on - sampled_off is the ban kernel alone (a sampled run takes the same pick with and without it); greedy_on - greedy_off is the ban kernel
plus the switch of the pick route, whose size greedy_pen - greedy_off shows.
Every run: prefill, the first pick, 9 untimed steps (they capture the two decode graphs of the configuration), then ONE stepping call of 256 steps
timed with an event pair on the stream.  The configurations alternate over `--repeats` rounds after one warm-up round; medians, minima and maxima are
reported as ms per token step -- the min-max range of a configuration is its run-to-run spread.  On a tree without `bans` (an older commit, for the
comparison of the off numbers: --package-root) only the three configurations without bans run.  One JSON line on stdout.

    python scripts/bench_bans.py [--repeats 7] [--layers 32] [--steps 256] [--package-root DIR]
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys

import torch

BATCH, MAX_SEQ, WARM = 8, 768, 9


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--package-root", default=None, help="import video_llava_amd from this tree (built there) instead of the script's own")
    a = ap.parse_args(argv)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    import video_llava_amd                      # bound before the helper scripts put their own tree in front
    print(f"[bench_bans] package: {os.path.dirname(video_llava_amd.__file__)}", file=sys.stderr, flush=True)
    from scripts.bench_fork import PROMPT_TOKENS, make_prompt
    from scripts.refill_bench import V_ROWS, build_model
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    has_bans = "bans" in inspect.signature(m.prefill).parameters
    ids, feats = make_prompt(5, dev)
    prompts, feats8 = [ids] * BATCH, feats.expand(BATCH, -1, -1).contiguous()
    N = a.steps
    assert PROMPT_TOKENS + 1 + WARM + N <= MAX_SEQ
    u = torch.rand(1 + WARM + N, BATCH, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    ban_kw = {}
    if has_bans:
        from video_llava_amd.logit_bans import LogitBans
        ban_kw = {"bans": LogitBans(no_repeat_ngram=3, min_new_tokens=8).check(m.vocab_size, 2), "eos_id": 2}

    def run(name):
        on, sampled, pen = name.endswith("_on"), name.startswith("sampled"), 1.1 if name == "greedy_pen" else 1.0
        kv, nxt, _ = m.prefill(prompts, feats8, MAX_SEQ, **(ban_kw if on else {}))
        try:
            if sampled:
                step = lambda first, n, at: m.decode_sample(kv, first, n, -1, 0.2, 50, u[at:at + n])      # noqa: E731
                nxt = m.sample_last(kv, u[0], 0.2, 50)
            else:
                step = lambda first, n, at: m.decode_greedy(kv, first, n, -1, pen)                           # noqa: E731
                if on or pen != 1.0:
                    nxt = m.greedy_last(kv, BATCH, pen)
            toks = step(nxt, WARM, 1)
            first = toks[:, WARM - 1].contiguous()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            step(first, N, 1 + WARM)
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]) / N
        finally:
            if on:
                m.set_bans(kv, None)
            m.set_warpers(kv, 1.0, 1.0)

    names = ["greedy_off", "greedy_pen", "sampled_off"] + (["greedy_on", "sampled_on"] if has_bans else [])
    times = {n: [] for n in names}
    for rnd in range(a.repeats + 1):
        for n in names:
            t = run(n)
            if rnd > 0:
                times[n].append(t)
    res = {"prompt_tokens": PROMPT_TOKENS, "video_rows": V_ROWS, "batch": BATCH, "layers": a.layers, "steps": N, "repeats": a.repeats, "has_bans": has_bans,
           "ms_per_step": {n: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for n, t in times.items()}}
    med = {n: statistics.median(t) for n, t in times.items()}
    res["route_switch_ms"] = round(med["greedy_pen"] - med["greedy_off"], 4)
    if has_bans:
        res["ban_kernel_ms"] = round(med["sampled_on"] - med["sampled_off"], 4)
        res["greedy_on_extra_ms"] = round(med["greedy_on"] - med["greedy_off"], 4)
    for n in names:
        print(f"[bench_bans] {n}: {med[n]:.4f} ms/step (min {min(times[n]):.4f}, max {max(times[n]):.4f})", file=sys.stderr, flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
