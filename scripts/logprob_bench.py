"""Cost of generate(output_logprobs=True) per decode token step, at PG-Video-LLaVA-7B shapes with random weights.

`--width` sequences (default 8: ~240-token prompts with a 356-row video run), `--steps` new tokens (default 256), bf16.  For greedy decoding and
for do_sample=True at temperature 0.2 (top_k 50), `timings["decode_s"]` of model.generate with and without `output_logprobs` -- the whole decode
loop as a caller sees it: the captured 8-step graphs, the chunk boundaries, and with the keyword the two device-to-host copies per chunk.  The four
configurations are interleaved round-robin over `--repeats` rounds after one warm-up round (code objects, graph capture per configuration); the
median per configuration is reported as ms per token step next to the difference the keyword makes.  One JSON line on stdout.

    python scripts/logprob_bench.py [--width 8] [--steps 256] [--repeats 5] [--layers 32]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/logprob_bench.py --repeats 1        # per-kernel times (its own run)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.refill_bench import build_model      # noqa: E402
from scripts.warper_bench import make_prompts     # noqa: E402

TEMPERATURE = 0.2


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    m = build_model(a.layers, dev)
    prompts, feats = make_prompts(a.width, 3, dev)
    configs = [(mode, lp) for mode in ("greedy", "sample") for lp in (False, True)]

    def run(mode, lp):
        kw = {"do_sample": True, "temperature": TEMPERATURE, "top_k": 50, "generator": torch.Generator(device=dev).manual_seed(7)} if mode == "sample" else {}
        tm = {}
        out = m.generate(prompts, video_spatio_temporal_features=feats, max_new_tokens=a.steps, eos_token_id=None, timings=tm, output_logprobs=lp, **kw)
        return tm["decode_s"] * 1e3 / (a.steps - 1), (out.sequences if lp else out)     # the first token comes from the prefill

    times = {c: [] for c in configs}
    ids = {}
    for rnd in range(a.repeats + 1):
        for c in configs:
            ms, seq = run(*c)
            if rnd > 0:
                times[c].append(ms)
            ids[c] = seq
    res = {"width": a.width, "steps": a.steps, "layers": a.layers, "repeats": a.repeats, "temperature": TEMPERATURE, "rows": []}
    for mode in ("greedy", "sample"):
        assert torch.equal(ids[(mode, False)], ids[(mode, True)]), f"{mode}: the keyword changed the ids"
        off, on = statistics.median(times[(mode, False)]), statistics.median(times[(mode, True)])
        res["rows"].append({"mode": mode, "ms_per_step_off": round(off, 4), "ms_per_step_on": round(on, 4), "delta_ms_per_step": round(on - off, 4),
                            "delta_pct": round(100.0 * (on - off) / off, 3), "off_min_max": [round(min(times[(mode, False)]), 4), round(max(times[(mode, False)]), 4)],
                            "on_min_max": [round(min(times[(mode, True)]), 4), round(max(times[(mode, True)]), 4)]})
        print(f"[logprob_bench] {mode}: off {off:.4f} ms/step, on {on:.4f} ms/step ({on - off:+.4f})", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
