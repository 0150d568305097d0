"""What a prompt-lookup step costs: pgv_llm_decode_lookup against pgv_llm_decode_greedy, at PG-Video-LLaVA-7B shapes with random bf16 weights.
No gate: it measures.  The speed-up of lookup decoding is (tokens per step) / (cost ratio); the first factor depends on the answers and cannot be
measured with random weights, so this reports the second and the break-even that follows.

One prompt of 461 tokens with a 356-row video run in every slot, 64 steps, cache of 2048 positions.  Per (B, D), after one warm-up run of each
(cache allocation, code objects), ms per step of
  (a) a plain greedy step at width B;
  (b) a plain greedy step at width R = B x (1 + D): the yardstick of the verify trunk -- same GEMV shapes, the K / V bytes of R sequences;
  (c) a lookup step at (B, D), with the tokens per step this run happened to emit.  Random weights propose next to no drafts, so in (c) only
      row 0 of a slot attends: the LOWER end of a step's cost.
Only the stepping call is timed, with an event pair on the stream ((c) includes its one blocking copy of the lengths); (a), (b), (c) alternate over
`--repeats` rounds, medians and spread are reported.
The upper end, EVERY ROW LIVE, is measured one step per call (`*_1` figures): each call starts from a token that occurs early in the prompt, so the
draft kernel proposes D drafts (checked against lookup_reference.lookup_candidates) and all 1 + D rows of every slot append, attend and are verified;
the model rejects them, the sequence grows by one, and the next call does the same.  Its yardsticks are one-step pgv_llm_decode_greedy calls at
widths B and R, each followed by a stream synchronise like the blocking copy that ends a lookup call.
Then one eager run of (b) and (c) under the per-family timers gives the small kernels' share: family decode_small is embedding + arg-max in (b) and
draft + embedding + row-wise arg-max + accept in (c); the draft and the accept kernel alone: `rocprofv3 --kernel-trace --stats -- python
scripts/bench_lookup.py --child 8:7 --layers 2 --repeats 1` (their time does not depend on the depth).
Every (B, D) pair runs in a child process of its own under `--pair-timeout` seconds; a pair that fails or runs out of time ends the run.
`--plain-only B`: only (a) at width B over 256 steps, one figure -- for A/B runs of the plain path against another build of the library.
`--sampled`: the same (B, D) table for sampled runs (temperature 0.2, top_k 50: the reference's defaults), every row live, one step per call as
above: ms per plain sampled step (pgv_llm_decode_sample) at width B, per sampled lookup step (pgv_llm_decode_lookup_sample) and, beside it, per greedy
lookup step at the same (B, D); the break-even is in tokens beyond the first (sampled lookup / plain sampled at B - 1).  Plain greedy and plain
sampled steps at width R say what the sampled pick costs over the arg-max at the width the lookup step picks at.  Random weights accept next to no
draft: tokens per step on real answers stays unmeasured.
One JSON line on stdout.

    python scripts/bench_lookup.py [--sampled] [--repeats 3] [--layers 32] [--pairs 1:3,1:7,1:15,8:1,8:3,8:7] [--steps 64] [--pair-timeout 240]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_fork import PROMPT_TOKENS, make_prompt        # noqa: E402
from scripts.refill_bench import V_ROWS, build_model             # noqa: E402

MAX_SEQ = 2048
TEMPERATURE, TOP_K = 0.2, 50          # --sampled: the reference's sampling defaults


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--pairs", default="1:3,1:7,1:15,8:1,8:3,8:7")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--pair-timeout", type=int, default=240)
    ap.add_argument("--child", default=None, metavar="B:D", help="measure this pair in this process (what the parent starts per pair)")
    ap.add_argument("--plain-only", type=int, default=0, metavar="B")
    ap.add_argument("--sampled", action="store_true", help="the sampled table: plain sampled step, sampled lookup step, greedy lookup step (every row live)")
    a = ap.parse_args(argv)
    if not a.child and not a.plain_only:
        rows = []
        for pair in a.pairs.split(","):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pair, "--repeats", str(a.repeats), "--layers", str(a.layers), "--steps",
                                str(a.steps)] + (["--sampled"] if a.sampled else []), stdout=subprocess.PIPE, text=True, timeout=a.pair_timeout)
            if r.returncode != 0:
                print(f"[bench_lookup] pair {pair} ended with status {r.returncode}: stopping", file=sys.stderr)
                return 1
            rows += json.loads(r.stdout.strip().splitlines()[-1])["rows"]
        print(json.dumps({"prompt_tokens": PROMPT_TOKENS, "video_rows": V_ROWS, "layers": a.layers, "repeats": a.repeats, "steps": a.steps, "max_seq": MAX_SEQ,
                          **({"sampled": {"temperature": TEMPERATURE, "top_k": TOP_K}} if a.sampled else {}), "rows": rows}))
        return 0
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    ids, feats = make_prompt(5, dev)
    N = a.steps
    res = {"prompt_tokens": PROMPT_TOKENS, "video_rows": V_ROWS, "layers": a.layers, "repeats": a.repeats, "steps": N, "max_seq": MAX_SEQ, "rows": []}

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) / N, out

    # Every variant runs twice on the same cache object: a short call that captures the graphs of its key (the variants before it replaced them),
    # then, from a fresh prefill, the timed call, which only replays.
    def greedy(K, prof=False):
        for n in (9, N):
            kv, nxt, _ = m.prefill([ids], feats, MAX_SEQ, capacity=K)
            m.fork(kv, [K])
            first = nxt.repeat(K).contiguous()
            if prof:
                m.ctx.prof_reset()
            ms = timed(lambda: m.decode_greedy(kv, first, n))[0]
        return ms

    def lookup(B, D, prof=False):
        for n in (9, N):
            kv, nxt, _ = m.prefill([ids] * B, feats.expand(B, -1, -1).contiguous(), MAX_SEQ, lookup=(D, 2))
            budget = [min(n * (1 + D), MAX_SEQ - PROMPT_TOKENS)] * B
            if prof:
                m.ctx.prof_reset()
            ms, (_toks, counts) = timed(lambda: m.decode_lookup(kv, nxt, n, -1, budget))
            m.set_lookup(kv, 0)
        return ms, float(counts.sum()) / (N * B)

    if a.plain_only:
        K, n = a.plain_only, 256
        greedy(K)
        kv, nxt, _ = m.prefill([ids], feats, MAX_SEQ, capacity=K)
        m.fork(kv, [K])
        first = nxt.repeat(K).contiguous()
        ms = timed(lambda: m.decode_greedy(kv, first, n))[0] * N / n
        print(json.dumps({"plain_only": K, "steps": n, "ms_per_step": round(ms, 5)}))
        return 0

    from video_llava_amd.lookup_reference import lookup_candidates
    seed_tok = ids[10]                      # occurs early in the prompt: a 1-gram match with a full continuation behind it

    def one_step_calls(kind, B, D):
        """N calls of ONE step each, a stream synchronise behind every call: plain at width B (kind 'plain': greedy, 'plain_s': sampled), or a
        lookup step whose 1 + D rows per slot are all live (kind 'lookup': greedy, 'lookup_s': sampled)."""
        g = torch.Generator(device=dev).manual_seed(17)
        if kind in ("plain", "plain_s"):
            kv, nxt, _ = m.prefill([ids], feats, MAX_SEQ, capacity=B)
            m.fork(kv, [B])
            first = nxt.repeat(B).contiguous()
            u = torch.rand(1, B, device=dev, generator=g)
            if kind == "plain":
                step = lambda: (m.decode_greedy(kv, first, 1), torch.cuda.synchronize())
            else:
                step = lambda: (m.decode_sample(kv, first, 1, -1, TEMPERATURE, TOP_K, u), torch.cuda.synchronize())
        else:
            kv, _, _ = m.prefill([ids] * B, feats.expand(B, -1, -1).contiguous(), MAX_SEQ, lookup=(D, 1))
            first = torch.full((B,), seed_tok, dtype=torch.int32, device=dev)
            # ngram size 1: the leftmost occurrence of the token, in the prompt's head, whatever the calls before appended behind the prompt
            assert len(lookup_candidates(ids + [seed_tok] * 3, D, 1)) == D
            u = torch.rand(1 + D, B, device=dev, generator=g)
            if kind == "lookup":
                step = lambda: m.decode_lookup(kv, first, 1, -1, [1 + D] * B)
            else:
                step = lambda: m.decode_lookup_sample(kv, first, 1, -1, [1 + D] * B, [0] * B, TEMPERATURE, TOP_K, u)
        for _ in range(3):
            step()
        ms = timed(lambda: [step() for _ in range(N)])[0]
        if kind in ("lookup", "lookup_s"):
            m.set_lookup(kv, 0)
        return ms

    if a.sampled:
        B, D = (int(x) for x in a.child.split(":"))
        R = B * (1 + D)
        kinds = [("plain_s", B), ("lookup_s", B), ("lookup", B), ("plain", R), ("plain_s", R)]
        t = {k: [] for k in kinds}
        for rnd in range(a.repeats + 1):
            for k in kinds:
                ms = one_step_calls(k[0], k[1], D)
                if rnd > 0:
                    t[k].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        span = lambda k: [round(min(t[k]), 4), round(max(t[k]), 4)]
        ps, ls, lg, gr, sr = (med[k] for k in kinds)
        row = {"B": B, "D": D, "rows": R, "plain_sampled_B_1": round(ps, 4), "lookup_sampled_live_1": round(ls, 4), "lookup_greedy_live_1": round(lg, 4),
               "break_even_live": round(ls / ps - 1, 4), "sampled_over_greedy_lookup": round(ls - lg, 4), "plain_greedy_R_1": round(gr, 4),
               "plain_sampled_R_1": round(sr, 4), "sampled_over_greedy_plain_R": round(sr - gr, 4),
               "plain_sampled_B_1_min_max": span(kinds[0]), "lookup_sampled_live_1_min_max": span(kinds[1]), "lookup_greedy_live_1_min_max": span(kinds[2]),
               "plain_greedy_R_1_min_max": span(kinds[3]), "plain_sampled_R_1_min_max": span(kinds[4])}
        res["rows"].append(row)
        res["sampled"] = {"temperature": TEMPERATURE, "top_k": TOP_K}
        print(f"[bench_lookup] sampled B={B} D={D}, every row live, one step per call: plain sampled@{B} {ps:.4f}, sampled lookup {ls:.4f}, greedy lookup {lg:.4f} "
              f"ms/step -> break-even +{ls / ps - 1:.3f} tokens; sampled - greedy: lookup {ls - lg:+.4f}, plain@{R} {sr - gr:+.4f}", file=sys.stderr, flush=True)
        print(json.dumps(res))
        return 0

    for pair in [a.child]:
        B, D = (int(x) for x in pair.split(":"))
        R = B * (1 + D)
        ta, tb, tc, tps, ta1, tb1, tc1 = [], [], [], [], [], [], []
        for rnd in range(a.repeats + 1):
            x, y, (z, t) = greedy(B), greedy(R), lookup(B, D)
            x1, y1, z1 = one_step_calls("plain", B, 0), one_step_calls("plain", R, 0), one_step_calls("lookup", B, D)
            if rnd > 0:
                ta.append(x); tb.append(y); tc.append(z); tps.append(t)
                ta1.append(x1); tb1.append(y1); tc1.append(z1)
        m.ctx.prof_enable(True)
        greedy(R, prof=True)
        small_b = m.ctx.prof_get()["decode_small"]
        lookup(B, D, prof=True)
        small_c = m.ctx.prof_get()["decode_small"]
        empty = m.ctx.prof_calibrate()
        m.ctx.prof_enable(False)
        sb = (small_b["ms"] - small_b["launches"] * empty) / N
        sc = (small_c["ms"] - small_c["launches"] * empty) / N
        ma, mb, mc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
        ma1, mb1, mc1 = statistics.median(ta1), statistics.median(tb1), statistics.median(tc1)
        row = {"B": B, "D": D, "rows": R, "plain_B_ms": round(ma, 4), "plain_R_ms": round(mb, 4), "lookup_ms": round(mc, 4),
               "plain_B_1": round(ma1, 4), "plain_R_1": round(mb1, 4), "lookup_live_1": round(mc1, 4), "live_gap_to_plain_R_1": round(mc1 - mb1, 4),
               "break_even_live": round(mc1 / ma1 - 1, 4), "lookup_live_1_min_max": [round(min(tc1), 4), round(max(tc1), 4)],
               "plain_R_1_min_max": [round(min(tb1), 4), round(max(tb1), 4)], "plain_B_1_min_max": [round(min(ta1), 4), round(max(ta1), 4)],
               "gap_to_plain_R_ms": round(mc - mb, 4), "break_even_extra_tokens_per_step": round(mc / ma - 1, 4),
               "tokens_per_step_this_run": round(statistics.median(tps), 3),
               "plain_B_min_max": [round(min(ta), 4), round(max(ta), 4)], "plain_R_min_max": [round(min(tb), 4), round(max(tb), 4)],
               "lookup_min_max": [round(min(tc), 4), round(max(tc), 4)],
               "prof_small_plain_R_ms": round(sb, 4), "prof_small_lookup_ms": round(sc, 4)}
        res["rows"].append(row)
        print(f"[bench_lookup] B={B} D={D}: plain@{B} {ma:.4f}, plain@{R} {mb:.4f}, lookup {mc:.4f} ms/step ({row['tokens_per_step_this_run']} tokens/step here); "
              f"break-even +{mc / ma - 1:.3f} tokens/step; small kernels {sb:.4f} -> {sc:.4f} ms; every row live, one step per call: plain@{B} {ma1:.4f}, "
              f"plain@{R} {mb1:.4f}, lookup {mc1:.4f} -> break-even +{mc1 / ma1 - 1:.3f}", file=sys.stderr, flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
