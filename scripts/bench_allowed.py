"""What constrained decoding costs per token step: generate()'s stepping calls with and without a token automaton (`allowed`), at
PG-Video-LLaVA-7B shapes with random bf16 weights.  No gate: it measures.

8 sequences of one 461-token prompt (356-row video run), 256 timed steps, cache of 768 positions.  Configurations:
  greedy_off    pgv_llm_decode_greedy, the arg-max of the lm_head candidates -- the path as it was before `allowed` existed;
  greedy_pen    greedy under repetition_penalty 1.1, no automaton: the pick_greedy route (sample kernel over the processed logits) that greedy under
                an automaton also takes -- the known price of leaving the candidate arg-max;
  sampled_off   pgv_llm_decode_sample, temperature 0.2, top_k 50;
  greedy_trie / sampled_trie    a trie of 1000 random answers of 1 - 4 tokens (a closed answer set).  An answer ends within 4 steps; the stepping call
                runs without a sticky EOS, so the rows then sit behind EOS in the DEAD state, whose allowed set is {EOS}: the kernel still searches an
                edge, marks and rewrites the whole row every step;
  greedy_narrow / sampled_narrow    a cycle whose one state has 10 edges and never accepts: a LIVE narrow state -- every step looks the consumed
                token up, follows its edge and marks 10 ids;
  greedy_wide / sampled_wide    a cycle whose one state has 30000 edges and never accepts: every step searches the 30000 edges for the consumed token
                and marks 30000 ids -- the widest state a real constraint ("any word of a dictionary") is likely to have.
sampled_* - sampled_off is the allow kernel alone (a sampled run takes the same pick with and without it); greedy_* - greedy_off is the kernel plus the
switch of the pick route, whose size greedy_pen - greedy_off shows.
Every run: prefill, the first pick, 9 untimed steps (they capture the two decode graphs of the configuration), then ONE stepping call of 256 steps
timed with an event pair on the stream.  The configurations alternate over `--repeats` rounds after one warm-up round; medians, minima and maxima are
reported as ms per token step -- the min-max range of a configuration is its run-to-run spread.  On a tree without `allowed` (an older commit, for the
comparison of the off numbers: --package-root) only the three configurations without an automaton run.  One JSON line on stdout.

    python scripts/bench_allowed.py [--repeats 5] [--layers 32] [--steps 256] [--package-root DIR]
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys

import numpy as np
import torch

BATCH, MAX_SEQ, WARM, EOS = 8, 768, 9, 2


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--package-root", default=None, help="import video_llava_amd from this tree (built there) instead of the script's own")
    a = ap.parse_args(argv)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    import video_llava_amd                      # bound before the helper scripts put their own tree in front
    print(f"[bench_allowed] package: {os.path.dirname(video_llava_amd.__file__)}", file=sys.stderr, flush=True)
    from scripts.bench_fork import PROMPT_TOKENS, make_prompt
    from scripts.refill_bench import V_ROWS, build_model
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    has_allowed = "allowed" in inspect.signature(m.prefill).parameters
    ids, feats = make_prompt(5, dev)
    prompts, feats8 = [ids] * BATCH, feats.expand(BATCH, -1, -1).contiguous()
    N = a.steps
    assert PROMPT_TOKENS + 1 + WARM + N <= MAX_SEQ
    u = torch.rand(1 + WARM + N, BATCH, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    automata = {}
    if has_allowed:
        from video_llava_amd.allowed import TokenAutomaton, check_allowed
        rng = np.random.default_rng(0)
        words = np.arange(3, m.vocab_size - 3)
        trie = TokenAutomaton.from_sequences([rng.choice(words, int(rng.integers(1, 5))).tolist() for _ in range(1000)])
        wide_tokens = sorted(int(t) for t in rng.choice(words, 30000, replace=False))
        wide = TokenAutomaton.from_edges(2, [(s, t, 1) for s in (0, 1) for t in wide_tokens], [])
        narrow = TokenAutomaton.from_edges(2, [(s, t, 1) for s in (0, 1) for t in wide_tokens[::3000]], [])
        automata = {k: check_allowed(v, BATCH, m.vocab_size, EOS) for k, v in (("trie", trie), ("narrow", narrow), ("wide", wide))}
        for k, al in automata.items():
            print(f"[bench_allowed] {k}: {al.automaton!r}", file=sys.stderr, flush=True)

    def run(name):
        kind = name.split("_")[1]
        on, sampled, pen = kind in automata, name.startswith("sampled"), 1.1 if name == "greedy_pen" else 1.0
        kv, nxt, _ = m.prefill(prompts, feats8, MAX_SEQ, **({"allowed": automata[kind], "eos_id": EOS} if on else {}))
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
            toks = step(first, N, 1 + WARM)
            ev[1].record()
            ev[1].synchronize()
            if kind in ("wide", "narrow"):          # the constraint held: every token of the timed call is one of the state's
                mine = wide_tokens if kind == "wide" else wide_tokens[::3000]
                assert bool(torch.isin(toks.cpu(), torch.tensor(mine, dtype=toks.dtype)).all()), name
            return ev[0].elapsed_time(ev[1]) / N
        finally:
            if on:
                m.set_allowed(kv, None)
            m.set_warpers(kv, 1.0, 1.0)

    names = ["greedy_off", "greedy_pen", "sampled_off"] + ([f"{p}_{k}" for k in automata for p in ("greedy", "sampled")])
    times = {n: [] for n in names}
    for rnd in range(a.repeats + 1):
        for n in names:
            t = run(n)
            if rnd > 0:
                times[n].append(t)
    res = {"prompt_tokens": PROMPT_TOKENS, "video_rows": V_ROWS, "batch": BATCH, "layers": a.layers, "steps": N, "repeats": a.repeats, "has_allowed": has_allowed,
           "ms_per_step": {n: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for n, t in times.items()}}
    med = {n: statistics.median(t) for n, t in times.items()}
    res["route_switch_ms"] = round(med["greedy_pen"] - med["greedy_off"], 4)
    for k in automata:
        res[f"allow_kernel_{k}_ms"] = round(med[f"sampled_{k}"] - med["sampled_off"], 4)
        res[f"greedy_{k}_extra_ms"] = round(med[f"greedy_{k}"] - med["greedy_off"], 4)
    for n in names:
        print(f"[bench_allowed] {n}: {med[n]:.4f} ms/step (min {min(times[n]):.4f}, max {max(times[n]):.4f})", file=sys.stderr, flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
