"""What a beam-search step costs: pgv_llm_decode_beam against pgv_llm_decode_greedy at the same width, at PG-Video-LLaVA-7B shapes with random
bf16 weights.  No gate: it measures.

One prompt of 461 tokens with a 356-row video run, 64 new tokens, K in {2, 4, 8}, cache of 576 positions.  Per K, after one warm-up run of each
(cache allocation, code objects, graph capture):
  (a) greedy: prefill of the prompt + fork([K]) + one pgv_llm_decode_greedy call of 63 steps -- the stepping path as it was before beams existed;
  (b) beams:  prefill + pgv_beam_begin(K) + one pgv_llm_decode_beam call of 63 steps (eos_id = -1: every step runs, early_stopping "never").
Only the stepping call is timed, with an event pair on the stream; (a) and (b) alternate over `--repeats` rounds and the medians and the spread are
reported as ms per token step.  Then ONE run of (b) under the per-family timers (pgv_prof; eager launches, so it is not compared with the graph
replays above) gives the share of the pick (row statistics + beam pick: family decode_small minus the embedding launch, which both paths have) and
of the cache gather (family other, which nothing else in a decode step uses); the same family of an eager greedy run (embedding + arg-max) stands
next to it.  One JSON line on stdout.

    python scripts/bench_beam.py [--repeats 5] [--layers 32] [--ks 2,4,8] [--new 64]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_fork import PROMPT_TOKENS, make_prompt        # noqa: E402
from scripts.refill_bench import V_ROWS, build_model             # noqa: E402

MAX_SEQ = 576


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--new", type=int, default=64)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    ids, feats = make_prompt(5, dev)
    N = a.new
    res = {"prompt_tokens": PROMPT_TOKENS, "video_rows": V_ROWS, "layers": a.layers, "repeats": a.repeats, "new_tokens": N, "max_seq": MAX_SEQ, "rows": []}

    def greedy(K, prof=False):
        kv, nxt, _ = m.prefill([ids], feats, MAX_SEQ, capacity=K)
        m.fork(kv, [K])
        first = nxt.repeat(K).contiguous()
        if prof:
            m.ctx.prof_reset()                  # the timers of the stepping call alone
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        m.decode_greedy(kv, first, N - 1)
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) / (N - 1)

    def beams(K, prof=False):
        kv, _, _ = m.prefill([ids], feats, MAX_SEQ, capacity=K)
        m.beam_begin(kv, K, N, -1, 1.0, "never")
        if prof:
            m.ctx.prof_reset()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        m.decode_beam(kv, N - 1)
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) / (N - 1)

    for K in [int(x) for x in a.ks.split(",")]:
        tg, tb = [], []
        for rnd in range(a.repeats + 1):
            g, b = greedy(K), beams(K)
            if rnd > 0:
                tg.append(g)
                tb.append(b)
        # the shares, from one eager run under the per-family timers
        m.ctx.prof_enable(True)
        greedy(K, prof=True)
        fam_g = m.ctx.prof_get()
        beams(K, prof=True)
        fam = m.ctx.prof_get()
        empty = m.ctx.prof_calibrate()
        m.ctx.prof_enable(False)
        steps = N - 1
        small_g_ms = (fam_g["decode_small"]["ms"] - fam_g["decode_small"]["launches"] * empty) / steps      # embedding + arg-max of the greedy step
        gather = fam["other"]
        small = fam["decode_small"]
        gather_ms = (gather["ms"] - gather["launches"] * empty) / steps
        # decode_small holds two timed scopes per step: the embedding launch and the pick (row statistics + beam pick in ONE scope)
        small_ms = (small["ms"] - small["launches"] * empty) / steps
        total_ms = sum(f["ms"] - f["launches"] * empty for f in fam.values()) / steps
        med_g, med_b = statistics.median(tg), statistics.median(tb)
        row = {"K": K, "greedy_ms_per_step": round(med_g, 4), "beam_ms_per_step": round(med_b, 4), "extra_ms": round(med_b - med_g, 4),
               "extra_share": round((med_b - med_g) / med_g, 4), "greedy_min_max": [round(min(tg), 4), round(max(tg), 4)],
               "beam_min_max": [round(min(tb), 4), round(max(tb), 4)], "prof_gather_ms_per_step": round(gather_ms, 4),
               "prof_embed_plus_pick_ms_per_step": round(small_ms, 4), "prof_greedy_embed_plus_argmax_ms_per_step": round(small_g_ms, 4), "prof_kernels_ms_per_step": round(total_ms, 4),
               "prof_gather_launches": gather["launches"], "prof_small_launches": small["launches"]}
        res["rows"].append(row)
        print(f"[bench_beam] K={K}: greedy {med_g:.4f} ms/step, beams {med_b:.4f} ms/step (+{100 * (med_b - med_g) / med_g:.1f} %); eager shares: gather "
              f"{gather_ms:.4f} ms, embedding + pick {small_ms:.4f} ms of {total_ms:.4f} ms", file=sys.stderr, flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
