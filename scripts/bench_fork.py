"""What pgv_kv_fork saves: n sequences of one prompt from ONE prefill against n prefills, at PG-Video-LLaVA-7B shapes with random bf16 weights.

One prompt of 461 tokens with a 356-row video run, n in {2, 4, 8, 16}, cache of 512 positions.  Per n, event-timed on the stream:
  (a) prefill of the prompt repeated n times -- the only way to n samples without the fork;
  (b) prefill of the one prompt into a cache created for n sequences + fork([n]);
  and the fork on its own (the second part of (b)), with the GB/s of the bytes it reads plus writes (cache rows of every layer, K and V, and the
  slot's logits row / seen-set), next to the 5.5 TB/s the decode GEMVs stream their weights at.
(a) and (b) alternate over `--repeats` rounds after one warm-up round per n (cache allocation, code objects); medians are reported.
The bar: (b) < (a) for every n.  One JSON line on stdout; exit status 1 when the bar is missed.

    python scripts/bench_fork.py [--repeats 7] [--layers 32] [--ns 2,4,8,16]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.refill_bench import VOCAB, V_ROWS, build_model      # noqa: E402

PROMPT_TOKENS, MAX_SEQ, GEMV_TBPS = 461, 512, 5.5


def make_prompt(seed: int, device):
    rng = np.random.default_rng(seed)
    head = PROMPT_TOKENS - 1 - (V_ROWS + 2) - 6
    ids = [1] + rng.integers(3, VOCAB - 3, head).tolist() + [VOCAB - 2] + [VOCAB - 3] * V_ROWS + [VOCAB - 1] + rng.integers(3, VOCAB - 3, 6).tolist()
    assert len(ids) == PROMPT_TOKENS
    feats = torch.from_numpy(rng.standard_normal((1, V_ROWS, 1024)).astype(np.float32) * 0.5).to(torch.float16).to(device)
    return ids, feats


def fork_bytes(m, n: int) -> int:
    """Bytes one fork([n]) reads plus writes: the prompt's cache rows and the slot state, once in and n - 1 times out."""
    c = m.config
    slot = 2 * c.num_hidden_layers * c.num_attention_heads * PROMPT_TOKENS * 256 + 4 * (m.vocab_size + (m.vocab_size + 64 + 31) // 32 + 5)
    return n * slot


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ns", default="2,4,8,16")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    ids, feats = make_prompt(5, dev)
    res = {"prompt_tokens": PROMPT_TOKENS, "video_rows": V_ROWS, "layers": a.layers, "repeats": a.repeats, "max_seq": MAX_SEQ, "rows": []}
    ok = True
    for n in [int(x) for x in a.ns.split(",")]:
        rep_feats = feats.expand(n, -1, -1).contiguous()
        t_rep, t_one, t_fork = [], [], []
        for rnd in range(a.repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            m.prefill([ids] * n, rep_feats, MAX_SEQ)
            ev[1].record()
            ev[2].record()
            kv, _, _ = m.prefill([ids], feats, MAX_SEQ, capacity=n)
            ev[3].record()
            assert m.fork(kv, [n]) == n
            ev[4].record()
            ev[4].synchronize()
            if rnd > 0:
                t_rep.append(ev[0].elapsed_time(ev[1]))
                t_one.append(ev[2].elapsed_time(ev[4]))
                t_fork.append(ev[3].elapsed_time(ev[4]))
        rep, one, fork = statistics.median(t_rep), statistics.median(t_one), statistics.median(t_fork)
        gbs = fork_bytes(m, n) / (fork * 1e-3) / 1e9
        ok = ok and one < rep
        res["rows"].append({"n": n, "prefill_repeated_ms": round(rep, 3), "prefill_plus_fork_ms": round(one, 3), "fork_ms": round(fork, 4),
                            "fork_gb_per_s": round(gbs, 1), "fork_share_of_gemv_rate": round(gbs / (GEMV_TBPS * 1e3), 3), "speedup": round(rep / one, 2),
                            "prefill_repeated_min_max": [round(min(t_rep), 3), round(max(t_rep), 3)],
                            "prefill_plus_fork_min_max": [round(min(t_one), 3), round(max(t_one), 3)]})
        print(f"[bench_fork] n={n}: {n} prefills {rep:.3f} ms, prefill + fork {one:.3f} ms (fork {fork:.4f} ms, {gbs:.0f} GB/s)", file=sys.stderr, flush=True)
    res["bar_met"] = ok
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
