"""Time teacher-forced scoring against the prefill it extends and against the user-level alternative (forward() + torch.log_softmax + gather).

7B shapes, random weights, bf16 by default: `--seqs` sequences of `--tokens` tokens (a 356-row video run inside), the last `--scored` positions
of each scored.  Four sides, every one warmed, then alternated A B C D A B C D ... in one process, each call between two device events:
  score        model.score(ids, labels)                      -- pgv_llm_score: only the scored rows go through lm_head
  prefill      model.prefill(ids)                            -- what score() adds its tail to
  forward_alt  model(input_ids).logits -> log_softmax of the scored rows -> gather      -- all-position fp32 logits materialised
  score_all    model.score(ids, ids)                         -- every row scored: (tokens - 1) * seqs rows, chunks of _lib.SCORE_CHUNK_ROWS
Prints one JSON line: median / min / max ms per side and score / prefill with its spread.

    python scripts/score_bench.py [--layers 32] [--iters 10] [--dtype bf16]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=560)
    ap.add_argument("--scored", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    a = ap.parse_args(argv)
    from video_llava_amd import _lib
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    from video_llava_amd.random_init import iter_llama_tensors, load_streaming
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    vocab, V = 32003, 356
    m = VideoChatGPTLlamaForCausalLM(VideoChatGPTConfig(vocab_size=vocab, num_hidden_layers=a.layers, eos_token_id=None), VisionConfig(), dtype)
    load_streaming(m, iter_llama_tensors(vocab=vocab, layers=a.layers, dtype=dtype, seed=1))
    vc = m.get_model().vision_config
    vc.vid_patch_token, vc.vid_start_token, vc.vid_end_token, vc.use_vid_start_end = vocab - 3, vocab - 2, vocab - 1, True
    rng = np.random.default_rng(0)
    head = 40
    tail = a.tokens - head - V - 3
    assert tail >= a.scored
    seqs = [[1] + rng.integers(3, 32000, head).tolist() + [vocab - 2] + [vocab - 3] * V + [vocab - 1] + rng.integers(3, 32000, tail).tolist() for _ in range(a.seqs)]
    labels = [[-100] * (a.tokens - a.scored) + s[-a.scored:] for s in seqs]
    feats1 = (torch.randn(1, V, 1024, device=m.device) * 2).to(dtype)
    featsB = feats1.expand(a.seqs, -1, -1).contiguous()
    ids_t = torch.tensor(seqs)
    tgt = ids_t[:, -a.scored:].to(m.device)
    max_seq = (a.tokens + 63) // 64 * 64

    def score():
        return m.score(seqs, labels, video_spatio_temporal_features=feats1)

    def prefill():
        return m.prefill(seqs, featsB, max_seq)

    def forward_alt():
        lg = m(input_ids=ids_t, video_spatio_temporal_features=featsB, max_length=max_seq).logits
        return torch.log_softmax(lg[:, -a.scored - 1:-1], dim=-1).gather(2, tgt[:, :, None]).cpu()

    def score_all():
        return m.score(seqs, seqs, video_spatio_temporal_features=feats1)

    sides = {"score": score, "prefill": prefill, "forward_alt": forward_alt, "score_all": score_all}
    for _ in range(a.warmup):
        for f in sides.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(a.iters):
        for k, f in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    # the two routes agree (same logits, fp32 log-softmax on the device vs the kernel)
    s, alt = score(), forward_alt()
    diff = max(float((s.token_logprobs[b][-a.scored:] - alt[b, :, 0]).abs().max()) for b in range(a.seqs))
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}
    ratios = [x / y for x, y in zip(ms["score"], ms["prefill"])]
    print(json.dumps({"shape": {"layers": a.layers, "seqs": a.seqs, "tokens": a.tokens, "scored_per_seq": a.scored, "dtype": a.dtype,
                                "score_all_rows": a.seqs * (a.tokens - 1), "chunk_rows": _lib.SCORE_CHUNK_ROWS}, "iters": a.iters, **res,
                      "score_over_prefill": {"median": statistics.median(ratios), "min": min(ratios), "max": max(ratios)},
                      "score_vs_forward_alt_max_abs_diff": diff}))


if __name__ == "__main__":
    main()
