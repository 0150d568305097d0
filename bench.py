#!/usr/bin/env python3
"""bench.py -- videos/sec of the PG-Video-LLaVA hot path on MI355X (BASELINE.json metric).

One "step" = one pass of the hot path over one batch of synthetic clips resident in HBM as uint8 frames:
    100x224x224 frames/clip -> fused preprocessing -> CLIP ViT-L/14 (23 layers) -> spatio-temporal pool ->
    mm_projector -> LLaMA-7B-shaped prefill (~450-token ActivityNet-QA-shaped prompt) -> greedy decode of
    `--new-tokens` tokens (EOS disabled so the work is fixed) -> answer collation (all-gather when N > 1).
Random-init weights of the named architectures, bf16 by default (BASELINE config 2/3), synthetic data.

Contract: `python bench.py --gpus N --steps K --warmup W`; one rank per GPU.  For N > 1 either the caller launches it
under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (RANK/LOCAL_RANK/WORLD_SIZE in the
environment), or -- when WORLD_SIZE is unset -- bench.py re-executes ITSELF under torch.distributed.run with N ranks on
127.0.0.1 (launch_self).  Either way rank 0 prints ONE JSON line.  `value` = clips processed by all ranks / max-over-ranks
time; for N > 1 the line carries `collective` (backend, ranks seen in the gathered answers, time of the one all-gather).
`--dry` replaces the GPU work by a deterministic token pattern (real sharding, barriers, all-gather and JSON; gloo, no GPU):
the CPU test of the N > 1 control flow.
A plain run only sets up, warms up, times the K steps and prints the line.  `--full` adds everything else the benchmark measures:
`pcie_inclusive`, `latency_b1`, `runner`, `families` / `roofline` (dominant kernel family, measured with hipEvent pairs around every
launch in a profiled pass on the launch stream), `side` (other dtypes and configurations) and, at N=1, `cpu_baseline` (the reference's
modules timed on the host cores on a bounded sample).
`--dump-outputs DIR` writes what the last timed step returned as DIR/<name>.npy (float32): `answer_tokens` [clips, new_tokens] (the
greedy answers of all clips, in global clip order) for the full workload, `video_tokens` [clips, rows, 4096] (this rank's projected video
tokens) for `--workload vision`.  Inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

if int(os.environ.get("WORLD_SIZE", "1")) > 1 and os.environ.get("PGV_RCCL_DEBUG_CAPTURE", "1") != "0" and "NCCL_DEBUG_FILE" not in os.environ:
    # a rank of an N > 1 run: RCCL's INFO log goes to a per-process file BEFORE `import torch` loads librccl (it caches its debug level on first
    # touch); `collective.transport` of the JSON line is parsed from it (video_llava_amd.parallel.rccl_transport)
    import tempfile
    os.environ["NCCL_DEBUG_FILE"] = os.path.join(tempfile.gettempdir(), "pgv_rccl_%h_%p.log")
    os.environ["NCCL_DEBUG"] = "INFO"

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The CPUs this process may use as it was STARTED: main() narrows the mask to the rank's share of its GPU's NUMA node (parallel.pin_rank_to_numa_node);
# the CPU-baseline child is placed from the original mask (one hardware thread per physical core of one node), not from the rank's slice.
ORIG_AFFINITY = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None

from video_llava_amd.benchlib import PEAK_MFMA_TFLOPS, Workload, dry_pattern, make_prompts, runner_measurement, side_line, time_collective  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips-per-gpu", type=int, default=8, help="clips per GPU per step (BASELINE config 4: 64 clips / 8 GPUs)")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--llm", choices=["7b", "13b"], default="7b")
    ap.add_argument("--image", type=int, choices=[224, 336], default=224,
                    help="336 = the LLaVA-1.5 variant the released PG-Video-LLaVA weights use: ViT-L/14-336 (577 tokens/frame), mlp2x_gelu projector, 676 video tokens")
    ap.add_argument("--weights", choices=["16bit", "fp8"], default="16bit",
                    help="fp8 = BASELINE config 5: decoder matrices quantised to e4m3 (per-row power-of-two scales) for the decode weight stream")
    ap.add_argument("--workload", choices=["full", "vision"], default="full",
                    help="full = BASELINE config 3/4 (frames -> answer); vision = config 2 (ViT + pool + projector)")
    ap.add_argument("--dry", action="store_true",
                    help="no GPU work: every rank fills its shard's answer slots with a deterministic token pattern, then the real barrier / all-gather / "
                         "max-over-ranks / JSON path runs over gloo -- the CPU-testable skeleton of the N > 1 run (never a performance number)")
    ap.add_argument("--no-runner", action="store_true",
                    help="skip the runner-level measurement (side field `runner`: synthetic .npy clips on local disk through "
                         "video_llava_amd.eval.run_inference_qa_activitynet.run_inference -- file discovery, frame sampling, tokenisation, "
                         "detokenisation and the JSON dump included)")
    ap.add_argument("--runner-groups", type=int, default=4, help="groups of --clips-per-gpu clips the runner measurement answers (after one warm-up group)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-port", action="store_true", help="additionally time this repo's own CPU oracle (reported under cpu_baseline.port)")
    ap.add_argument("--no-host-frames", action="store_true",
                    help="skip the second timing of the same steps with the uint8 frames uploaded from pinned host memory inside the timed region "
                         "(reported as pcie_inclusive: BASELINE.md configs 2/3 start at H2D; `value` always has the frames resident in HBM)")
    ap.add_argument("--no-latency", action="store_true", help="skip the batch-1 latency measurement (latency_b1: BASELINE configs[2] proper, one clip -> answer)")
    ap.add_argument("--no-profile-pass", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=4)
    ap.add_argument("--cpu-layers", type=int, default=2)
    ap.add_argument("--no-side", action="store_true",
                    help="skip the guarded side lines of the --full run (`side.fp16`: the reference's dtype, the one the 1e-3 tolerance is stated in; "
                         "`side.cfg5_13b_fp8`: BASELINE configs[4] with its own roofline; `side.clips32` when the decoder batches that many)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure also run every other measurement: pcie_inclusive, latency_b1, runner, the profiled pass "
                         "(families, rooflines), the side lines and the CPU baseline (the --no-* switches above leave single ones out)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step returned to DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--cpu-baseline-child", action="store_true", help=argparse.SUPPRESS)     # internal: the pinned CPU-baseline subprocess
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """--dump-outputs: each array as DIR/<name>.npy in float32 (token ids are exact: the vocabulary is far below 2^24).  An array larger than its
    share of DUMP_BUDGET_BYTES is written as a fixed sample of its flattened elements (seed 0), with the flat indices of the sample in
    DIR/<name>_index.npy (float64)."""
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(len(arrays), 1)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // 12, replace=False))    # 4 bytes of value + 8 of index per element
            np.save(os.path.join(dirname, f"{name}_index.npy"), idx.astype(np.float64))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, f"{name}.npy"), a)


def answers_array(answers):
    """The collated answers (one token-id list per clip, global order) as one [clips, new_tokens] array."""
    assert all(a is not None for a in answers) and len({len(a) for a in answers}) == 1, "answers of unequal length"
    return np.asarray(answers, dtype=np.float32)


def _interleave_host_memory():
    """numactl --interleave=all for this process, without numactl: set_mempolicy(MPOL_INTERLEAVE) over every NUMA node of the box, so the
    27 GB of fp32 weights of the CPU baseline are spread over all memory controllers whichever thread first touches them (a model filled by
    one thread otherwise lands on one socket's DIMMs and the decode GEMVs, which only stream weights, run at a fraction of the box's
    bandwidth -- the round-2 baseline measured 35 GB/s on a 256-thread host).  Returns the number of nodes, 0 if the call is refused."""
    import ctypes
    import glob
    nodes = sorted(int(p.rsplit("node", 1)[1]) for p in glob.glob("/sys/devices/system/node/node[0-9]*"))
    if len(nodes) < 2:
        return len(nodes)
    mask = 0
    for n in nodes:
        mask |= 1 << n
    words = (ctypes.c_ulong * ((max(nodes) // 64) + 1))(*[(mask >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(max(nodes) // 64 + 1)])
    MPOL_INTERLEAVE, SYS_set_mempolicy = 3, 238                     # x86_64
    rc = ctypes.CDLL(None, use_errno=True).syscall(SYS_set_mempolicy, MPOL_INTERLEAVE, words, max(nodes) + 2)
    return len(nodes) if rc == 0 else 0


def _fast_hf_build(cls, cfg):
    """Instantiate an HF model without its per-module random initialisation (the reference's own `disable_torch_init`,
    video_chatgpt/utils.py, does the same before from_pretrained), then fill the matrices from a tiled random block: values do not change
    CPU matmul time, an N(0, 0.02) block keeps every intermediate finite.  The fill is one broadcast copy per tensor, which ATen runs on
    the whole thread pool: pages are first touched by many threads (and interleaved over the NUMA nodes, _interleave_host_memory)."""
    import transformers.modeling_utils as mu
    saved = (torch.nn.Linear.reset_parameters, torch.nn.Embedding.reset_parameters, torch.nn.LayerNorm.reset_parameters, mu.PreTrainedModel.init_weights)
    torch.nn.Linear.reset_parameters = lambda self: None
    torch.nn.Embedding.reset_parameters = lambda self: None
    torch.nn.LayerNorm.reset_parameters = lambda self: None
    mu.PreTrainedModel.init_weights = lambda self: None
    try:
        m = cls(cfg)
    finally:
        torch.nn.Linear.reset_parameters, torch.nn.Embedding.reset_parameters, torch.nn.LayerNorm.reset_parameters, mu.PreTrainedModel.init_weights = saved
    block = torch.randn(1 << 16, generator=torch.Generator().manual_seed(0)) * 0.02
    with torch.no_grad():
        for _n, p in m.named_parameters():
            if p.dim() == 1:
                p.fill_(1.0 if p.numel() in (cfg.hidden_size,) and "bias" not in _n else 0.0)
            else:
                flat = p.view(-1)
                full = flat.numel() // block.numel() * block.numel()
                if full:
                    flat[:full].view(-1, block.numel()).copy_(block.expand(full // block.numel(), -1))
                if full < flat.numel():
                    flat[full:].copy_(block[:flat.numel() - full])
    return m.eval()


def _numa_node_cpus():
    """(node id, one logical CPU per PHYSICAL core of that node) for the NUMA node with the most cores, from sysfs; (None, []) when sysfs has no
    NUMA topology (single-node hosts, containers that hide it)."""
    import glob
    best = (None, [])
    for path in sorted(glob.glob("/sys/devices/system/node/node[0-9]*")):
        try:
            cpus = []
            for part in open(os.path.join(path, "cpulist")).read().strip().split(","):
                lo, _, hi = part.partition("-")
                cpus += list(range(int(lo), int(hi or lo) + 1))
            allowed = ORIG_AFFINITY if ORIG_AFFINITY is not None else os.sched_getaffinity(0)
            phys = []
            for c in cpus:
                if c not in allowed:
                    continue
                sib = open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip().replace("-", ",").split(",")
                if c == min(int(x) for x in sib):               # the first hardware thread of its core
                    phys.append(c)
            if len(phys) > len(best[1]):
                best = (int(path.rsplit("node", 1)[1]), phys)
        except (OSError, ValueError):
            continue
    return best


def _cgroup_cpu_quota():
    """CPUs' worth of time the container may use (cgroup v2 cpu.max / v1 cfs quota), rounded up; None when unlimited or unreadable.  The GPU
    hosts of this pool show 256 logical CPUs but `cpu.max = 1600000 100000`: 16 CPUs -- with 64 runnable threads the eager fp32 path was
    throttled to 4.7 s per decode step against 0.70 s with 16 (gpurun_out/r4c)."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else max(1, -(-int(q) // int(p)))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else max(1, -(-q // p))
    except (OSError, ValueError):
        return None


def cpu_baseline_reference(args):
    """Parent side of the CPU baseline: the measurement runs in a CHILD process whose affinity mask is the physical cores of ONE NUMA node
    (set before the interpreter starts, so every thread of ATen's pool inherits it and the 27 GB of fp32 weights are first-touched on that
    node's DIMMs) -- VERDICT r3 weak #9: the unpinned run measured torch's worst (32 ms per decoder layer on a 256-thread host against
    9.4 ms on the 8-core survey probe).  PGV_CPU_BASELINE_PIN=0 runs the child unpinned for comparison."""
    node, cpus = _numa_node_cpus()
    quota = _cgroup_cpu_quota()
    if quota and quota < len(cpus):
        cpus = cpus[:max(quota, 2)]              # a container limited to `quota` CPUs of time: more runnable threads than that only get throttled
    pin = os.environ.get("PGV_CPU_BASELINE_PIN", "1") != "0" and len(cpus) >= 2
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", "--llm", args.llm, "--frames", str(args.frames), "--new-tokens", str(args.new_tokens)]
    env = dict(os.environ)
    env.pop("OMP_NUM_THREADS", None)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env,
                       preexec_fn=(lambda: os.sched_setaffinity(0, cpus)) if pin else None)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"cpu-baseline child rc={r.returncode}: {(r.stderr or r.stdout)[-400:]}")
    out = json.loads(lines[-1])
    out["pinning"] = {"numa_node": node if pin else None, "cpus_in_mask": len(cpus) if pin else (os.cpu_count() or 1),
                      "policy": ("child process bound to one hardware thread per physical core of one NUMA node before start; weights first-touched there"
                                 if pin else "unpinned")}
    out["cgroup_cpu_quota"] = quota
    out["child_wall_s"] = time.perf_counter() - t0
    return out


def cpu_baseline_child(args):
    """The CPU baseline BASELINE.md 2 specifies: the reference's own path executed by PyTorch on the host cores.  The reference delegates
    ALL arithmetic of this path to HF transformers -- `CLIPVisionModel` (video_chatgpt/eval/model_utils.py:134, inference.py:93) and
    `LlamaForCausalLM.forward` (VideoChatGPTLlamaForCausalLM subclasses it; model/video_chatgpt.py:170-175,219-226) -- plus its own numpy
    pooling; those modules are installed on the GPU box (transformers is part of the image), the reference's glue files are not
    (/root/reference does not travel), so the glue that carries no arithmetic (the splice `torch.cat`, prompt handling) is left out and the
    pooling is the oracle's verbatim restatement of the reference's numpy function.
      (i)  BASELINE config 1 in full: 8 frames, fp32, eager attention, all 24 CLIP layers (what the reference executes) -> hidden_states[-2][:, 1:]
           -> numpy pooling -> [356, 1024] fp16.
      (ii) decoder at FULL DEPTH (32 / 40 layers, fp32 weights: 27 / 52 GB): LlamaForCausalLM.forward, eager attention, lm_head on all
           positions as the reference computes it (model/video_chatgpt.py:226): one prefill of the ~450-token prompt and KV-cached decode
           steps, timed directly (no per-layer differencing).  Thread counts are swept per stage INSIDE the affinity mask the parent set
           (small GEMVs do not scale to every core), the best is kept and every count tried is reported."""
    import transformers
    from transformers import CLIPVisionConfig, CLIPVisionModel, LlamaConfig, LlamaForCausalLM
    from oracle import synth
    from oracle import vision as ovis
    t_all = time.perf_counter()
    ncores = len(os.sched_getaffinity(0))
    numa_nodes = _interleave_host_memory() if os.environ.get("PGV_CPU_BASELINE_INTERLEAVE") == "1" else 0
    default_threads = min(torch.get_num_threads(), ncores)
    # thread counts swept, best-known first: every core the parent's mask grants (already capped at the container's CPU quota), then 3/4 and 1/2
    # of them; the ATen pool's own default goes last and only if the sample's time budget allows
    top = min(ncores, 32)
    cand = list(dict.fromkeys(c for c in (top, max(1, top * 3 // 4), max(1, top // 2)) if c >= 1))

    frames = synth.make_frames(8, 224, seed=0)
    ccfg = CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
                            hidden_act="quick_gelu", layer_norm_eps=1e-5, attn_implementation="eager")
    clip = _fast_hf_build(CLIPVisionModel, ccfg)
    px = ovis.clip_preprocess(frames)
    vit_times = {}
    with torch.no_grad():
        for th in cand[:2]:
            torch.set_num_threads(th)
            clip(px[:1], output_hidden_states=True)                                   # warm-up
            t0 = time.perf_counter()
            feat = clip(px, output_hidden_states=True).hidden_states[-2][:, 1:]
            ovis.spatio_temporal_pool_numpy(feat.numpy().astype(np.float16))
            vit_times[th] = time.perf_counter() - t0
    t_cfg1 = min(vit_times.values())
    del clip
    full_layers, H, I, heads = (32, 4096, 11008, 32) if args.llm == "7b" else (40, 5120, 13824, 40)
    torch.set_num_threads(default_threads)
    t_build = time.perf_counter()
    lcfg = LlamaConfig(vocab_size=32003, hidden_size=H, intermediate_size=I, num_hidden_layers=full_layers, num_attention_heads=heads, num_key_value_heads=heads,
                       max_position_embeddings=4096, rms_norm_eps=1e-5, attn_implementation="eager")
    llm = _fast_hf_build(LlamaForCausalLM, lcfg)
    t_build = time.perf_counter() - t_build
    weight_bytes = sum(p.numel() for n, p in llm.named_parameters() if "embed_tokens" not in n) * 4.0
    ids = torch.tensor([make_prompts(1, 32003, 356, 0)[0]])
    S = ids.shape[1]
    n_step = 2

    def prefill(threads):
        torch.set_num_threads(threads)
        with torch.no_grad():
            t0 = time.perf_counter()
            o = llm(input_ids=ids, use_cache=True)
            return time.perf_counter() - t0, o

    def decode(threads, o):
        torch.set_num_threads(threads)
        with torch.no_grad():
            tok = o.logits[:, -1].argmax(-1, keepdim=True)
            o = llm(input_ids=tok, past_key_values=o.past_key_values, use_cache=True)   # first step warms the decode shapes
            t0 = time.perf_counter()
            for _ in range(n_step):
                tok = o.logits[:, -1].argmax(-1, keepdim=True)
                o = llm(input_ids=tok, past_key_values=o.past_key_values, use_cache=True)
            return (time.perf_counter() - t0) / n_step, o

    # Sweep order: the counts that have won on every host so far first; the pool's default (every core of the mask) LAST and only while the
    # sample's time budget allows -- with all 64 cores of a node the eager M = 1 path of torch collapsed on the GPU hosts (ViT 17.6 s against
    # 1.06 s at 32 threads, a decode step 4.8 s), and a sample that burns its budget there never reaches the good settings.
    BUDGET_S = 32.0
    pre, o = {}, None
    for th in cand[:1]:
        pre[th], o = prefill(th)
    step = {}
    for th in cand:
        step[th], o = decode(th, o)
        if time.perf_counter() - t_all > BUDGET_S:
            break
    if default_threads not in step and time.perf_counter() - t_all < BUDGET_S - 3 * (n_step + 1) * min(step.values()):
        step[default_threads], o = decode(default_threads, o)
    th_pre, th_step = min(pre, key=pre.get), min(step, key=step.get)
    pre_full, step_full = pre[th_pre], step[th_step]
    del llm, o
    clip_s = t_cfg1 * (args.frames / 8.0) + pre_full + step_full * (args.new_tokens - 1)
    probe = 0.0094 if args.llm == "7b" else 0.0146               # BASELINE.md 3 (8-core build container)
    return {"value": 1.0 / clip_s, "unit": "videos/sec", "cores": ncores, "kind": "reference",
            "kind_note": ("HF transformers " + transformers.__version__ + " CLIPVisionModel + LlamaForCausalLM.forward on the host cores: the modules the "
                          "reference's path executes (it has no arithmetic of its own beyond the numpy pooling, restated verbatim); the reference's glue "
                          "files cannot travel to the GPU box"),
            "host_logical_cpus": os.cpu_count(),
            "threads_tried": {"vit": sorted(vit_times), "prefill": sorted(pre), "decode_step": sorted(step)},
            "threads_used": {"vit": min(vit_times, key=vit_times.get), "prefill": th_pre, "decode_step": th_step},
            "numa_nodes_interleaved": numa_nodes, "layers_timed": full_layers, "model_build_s": t_build,
            "config1_8_frames_s": t_cfg1, "config1_by_threads_s": {str(k): v for k, v in vit_times.items()},
            "prefill_s_full_depth": pre_full, "decode_step_s_full_depth": step_full, "prefill_by_threads_s": {str(k): v for k, v in pre.items()},
            "decode_step_by_threads_s": {str(k): v for k, v in step.items()},
            "decode_step_s_per_layer": step_full / full_layers, "decode_weight_stream_gbs": weight_bytes / step_full / 1e9,
            "survey_probe_decode_step_s_per_layer": probe, "decode_per_layer_vs_survey_probe": step_full / full_layers / probe,
            "sample": (f"BASELINE config 1 in full (8 frames, 24-layer ViT-L/14 fp32 eager + numpy pool: {t_cfg1:.2f}s) scaled to {args.frames} frames; "
                       f"{args.llm.upper()}-shaped LlamaForCausalLM fp32 eager at FULL depth ({full_layers} layers, {weight_bytes / 1e9:.1f} GB of weights, "
                       f"first-touch inside the affinity mask{', interleaved over %d NUMA nodes' % numa_nodes if numa_nodes else ''}): prefill S={S} {pre_full:.2f}s + {n_step} timed decode steps of {step_full * 1e3:.0f} ms "
                       f"({step_full / full_layers * 1e3:.1f} ms per layer, {weight_bytes / step_full / 1e9:.0f} GB/s) -> prefill + {args.new_tokens - 1} steps "
                       f"= {clip_s:.1f}s/clip; sample took {time.perf_counter() - t_all:.0f}s"),
            "seconds_per_clip": clip_s}


def cpu_baseline_port(args):
    """Second CPU number: this repo's own oracle (oracle/, a torch-fp32 restatement of the same path) on a bounded sample, scaled to one clip."""
    from oracle import llm as ollm
    from oracle import synth
    from oracle import vision as ovis
    t_all = time.perf_counter()
    threads = torch.get_num_threads()
    ccfg = synth.CLIP_L14_224
    w = synth.make_clip_weights(ccfg, seed=0)
    px = ovis.clip_preprocess(synth.make_frames(args.cpu_frames, 224, seed=0))
    with torch.no_grad():
        ovis.clip_select_features(px[:1], w, ccfg)            # warm-up
        t0 = time.perf_counter()
        feat = ovis.clip_select_features(px, w, ccfg)
        t_vit = time.perf_counter() - t0
        t0 = time.perf_counter()
        pooled = ovis.spatio_temporal_pool_torch(feat)
        t_pool = time.perf_counter() - t0
    del w
    full = synth.LLAMA_7B if args.llm == "7b" else synth.LLAMA_13B
    lcfg = synth.LlamaCfg(**{**full.__dict__, "layers": args.cpu_layers})
    lw = synth.make_llama_weights(lcfg, seed=0)
    ids = make_prompts(1, lcfg.vocab, 356, 0)[0]
    PATCH, START, END = lcfg.vocab - 3, lcfg.vocab - 2, lcfg.vocab - 1
    with torch.no_grad():
        m = ollm.LlamaOracle(lw, lcfg)
        t0 = time.perf_counter()
        lg = m.prefill(ids, pooled.float(), START, END, PATCH)
        t_prefill = time.perf_counter() - t0
        tok = int(lg[0].argmax())
        t0 = time.perf_counter()
        nstep = 4
        for _ in range(nstep):
            tok = int(m.step(tok)[0].argmax())
        t_step = (time.perf_counter() - t0) / nstep
    scale_l = full.layers / args.cpu_layers
    clip_s = t_vit * (args.frames / args.cpu_frames) + t_pool + t_prefill * scale_l + t_step * scale_l * (args.new_tokens - 1)
    return {"value": 1.0 / clip_s, "unit": "videos/sec", "cores": threads, "kind": "port",
            "sample": (f"oracle (torch fp32 CPU restatement): ViT-L/14 23 layers on {args.cpu_frames} of {args.frames} frames "
                       f"({t_vit:.2f}s), {args.cpu_layers} of {full.layers} decoder layers: prefill S={len(ids)} ({t_prefill:.2f}s) "
                       f"+ {nstep} decode steps ({t_step * 1e3:.0f} ms each), scaled linearly to one clip with "
                       f"{args.new_tokens} tokens = {clip_s:.1f}s/clip; sample took {time.perf_counter() - t_all:.0f}s"),
            "seconds_per_clip": clip_s}


def launch_self(args) -> int:
    """`python bench.py --gpus N` with no torchrun environment: start the N ranks ourselves by re-executing this file under
    torch.distributed.run (one process per GPU, LOCAL_RANK -> device, rendezvous on 127.0.0.1 at a free port).  The ranks inherit
    stdout, so rank 0's single JSON line is this process's output; the exit code is the launcher's."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    return subprocess.call(cmd, env=env)


def main_dry(args):
    """--dry: the N-rank skeleton without the GPU.  Each rank owns shard_indices(n_global, rank, world), "answers" them with dry_pattern,
    and the real collation runs; every rank checks the gathered answers against the pattern of ALL clips."""
    from video_llava_amd import parallel
    rank, world, _local = parallel.init_distributed("gloo")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    B, NEW, vocab = args.clips_per_gpu, args.new_tokens, 32003
    n_global = B * world
    mine = parallel.shard_indices(n_global, rank, world)
    dev = torch.device("cpu")

    def sync():
        if world > 1:
            torch.distributed.barrier()

    def step():
        toks = torch.tensor([dry_pattern(i, NEW, vocab) for i in mine], dtype=torch.int32, device=dev)
        lens = torch.full((len(mine),), NEW, dtype=torch.int32, device=dev)
        return parallel.gather_answers(toks, lens, n_global, rank, world), toks, lens

    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        answers, toks, lens = step()
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tt[0])
    for i in range(n_global):
        assert answers[i] == dry_pattern(i, NEW, vocab), f"rank {rank}: clip {i} collated wrongly"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"answer_tokens": answers_array(answers)})
    coll, _ = time_collective(parallel, toks, lens, n_global, rank, world, sync)
    coll.update(parallel.collective_identity(dev, rank, world, allow_shared_device=True))      # the same identity record the GPU run carries (no GPUs here: BDFs are null)
    if coll["world_seen"] != args.gpus or coll["ranks_answered"] != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the all-gather delivered the slots of {coll['world_seen']} ranks ({coll['ranks_answered']} answered)")
    if rank == 0:
        print(json.dumps({"metric": "videos/sec (DRY: no GPU work, control flow only)", "value": n_global * args.steps / elapsed, "unit": "videos/sec",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none", "data": "dry",
                          "config": {"workload": "dry run of the N-rank skeleton", "clips_per_gpu_per_step": B, "new_tokens": NEW, "parallelism": f"dp{world}"},
                          "collective": coll, "clips_checked": n_global}), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def main():
    args = parse()
    if args.cpu_baseline_child:
        print(json.dumps(cpu_baseline_child(args)), flush=True)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_self(args))
    if args.dry:
        return main_dry(args)
    from video_llava_amd import parallel

    if torch.cuda.is_available() and not os.environ.get("PGV_BENCH_SHARE_DEVICE"):
        # host threads of this rank (prefetch, OMP, the process-group backend's own) next to its GPU: BEFORE the backend starts its threads;
        # silent when sysfs says nothing.  (With one shared device every rank would pin to the same GPU's slice: skipped.)
        parallel.pin_rank_to_numa_node(int(os.environ.get("LOCAL_RANK", "0")))
    rank, world, local = parallel.init_distributed()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if os.environ.get("PGV_BENCH_SHARE_DEVICE"):        # control-flow smoke test of the N > 1 path on a 1-GPU box (with PGV_DIST_BACKEND=gloo)
        local = 0
    elif torch.cuda.device_count() < world:
        raise SystemExit(f"--gpus {world} but only {torch.cuda.device_count()} GPU(s) are visible (one rank per GPU; "
                         "PGV_BENCH_SHARE_DEVICE=1 PGV_DIST_BACKEND=gloo runs the ranks on one device as a control-flow check)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    wl = Workload(args, dev, rank, world)
    model, tower, frames = wl.model, wl.tower, wl.frames
    B, T, NEW, S, vocab, n_global, mine = wl.B, wl.T, wl.NEW, wl.S, wl.vocab, wl.n_global, wl.mine
    video_rows, projector, barrier = wl.video_rows, wl.projector, wl.barrier

    elapsed, vit_ms, own_elapsed = wl.timed(args.steps, args.warmup)
    ms_per_step = elapsed / args.steps * 1e3
    value = n_global * args.steps / elapsed
    if args.dump_outputs and rank == 0:
        out = wl.last_out
        dump_outputs(args.dump_outputs, {"answer_tokens": answers_array(out)} if args.workload == "full" else {"video_tokens": out.float().cpu().numpy()})
    rank_ms = None
    if world > 1:                                             # every rank's own ms per step: a straggler shows in the one JSON line
        tt = torch.zeros(world, dtype=torch.float64, device=dev)
        tt[rank] = own_elapsed / args.steps * 1e3
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.SUM)
        rank_ms = [float(x) for x in tt.cpu()]
    pcie = None
    if args.full and not args.no_host_frames:                # same steps, frames handed over as host buffers (the reference's boundary: PIL images on the host)
        host = frames.cpu().pin_memory()
        keep = list(wl.vit_events)
        el, _, _ = wl.timed(args.steps, 1, host_frames=host)
        wl.vit_events[:] = keep
        pcie = {"value": n_global * args.steps / el, "unit": "videos/sec", "ms_per_step": el / args.steps * 1e3,
                "h2d_bytes_per_step_per_gpu": int(host.numel())}
        del host
    latency = wl.latency_b1() if (args.full and not args.no_latency and args.workload == "full" and rank == 0) else None
    runner = None
    if args.full and not args.no_runner and args.workload == "full" and world == 1:
        try:
            runner = runner_measurement(args, model, tower, video_rows, S, rank, world)
            runner["ratio_to_value"] = runner["videos_per_sec"] / value
        except Exception as e:                                   # noqa: BLE001 -- a side field (needs ~250 MB of local disk) never costs the headline line
            runner = {"videos_per_sec": None, "error": f"{type(e).__name__}: {e}"}
    if world > 1:
        torch.distributed.barrier()
    clip_feat_tflops = wl.clip_tflops(vit_ms)
    clip_feat_tflops_total = clip_feat_tflops                 # sum over ranks of each rank's own stage rate
    if world > 1:
        tt = torch.tensor([clip_feat_tflops], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.SUM)
        clip_feat_tflops_total = float(tt[0])

    # ---- the one exchange step, timed alone (N > 1): all-gather of the answer buffer ---------------------------------
    collective = None
    if world > 1 and args.workload == "full":
        toks_c = torch.stack([torch.tensor(dry_pattern(i, NEW, vocab), dtype=torch.int32) for i in mine]).to(dev)
        lens_c = torch.full((B,), NEW, dtype=torch.int32, device=dev)
        collective, ans_c = time_collective(parallel, toks_c, lens_c, n_global, rank, world, barrier)
        assert all(ans_c[i] == dry_pattern(i, NEW, vocab) for i in range(n_global)), f"rank {rank}: collation mismatch"
        # proof of transport: who answered, on which GPUs, over which library and path -- raises when fewer ranks than --gpus took
        # part or two ranks sit on one GPU without PGV_BENCH_SHARE_DEVICE=1, so a mis-launched job cannot produce a scaling number
        collective.update(parallel.collective_identity(dev, rank, world, allow_shared_device=bool(os.environ.get("PGV_BENCH_SHARE_DEVICE"))))
        if collective["world_seen"] != args.gpus or collective["ranks_answered"] != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but the all-gather delivered the slots of {collective['world_seen']} ranks ({collective['ranks_answered']} answered)")
        collective["transport"] = parallel.rccl_transport()        # this rank's captured RCCL INFO log: P2P (xGMI) vs SHM / NET fallbacks
        collective["rank_ms_per_step"] = rank_ms
        free_b, total_b = torch.cuda.mem_get_info(dev)    # device-wide (every process on it): with PGV_BENCH_SHARE_DEVICE=1 the footprint of all N replicas
        collective["device_mem_used_gb"] = round((total_b - free_b) / 2 ** 30, 1)
        collective["shared_device"] = bool(os.environ.get("PGV_BENCH_SHARE_DEVICE"))
        collective["rank_ms_per_step_min_max"] = [min(rank_ms), max(rank_ms)]

    # ---- profiled pass: hipEvent pairs around every launch of each kernel family, on the launch stream -----------------
    fam, roofline = {}, None
    if rank == 0 and args.full and not args.no_profile_pass:
        fam, roofline = wl.profile_pass(ms_per_step)

    if rank == 0:
        line = {
            "metric": f"videos/sec (100x{S}^2 frames->answer)" if args.workload == "full" else f"videos/sec (100x{S}^2 frames->projected video tokens)",
            "value": value, "unit": "videos/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": ("BASELINE configs[2] batched as configs[3]: PG-Video-LLaVA-7B-shaped, "
                                    f"{B} clips/GPU/step x {T} frames {S}x{S} -> ViT-L/14 (23 layers) -> pool -> {projector} projector -> "
                                    f"prefill (~{video_rows + 95} tok) -> {NEW} greedy tokens, random-init weights")
                       if args.workload == "full" else
                       f"BASELINE configs[1]: {B} clips/GPU/step x {T} frames -> ViT-L/14 (23 layers) + pool + Linear(1024,4096)",
                       "clips_per_gpu_per_step": B, "frames_per_clip": T, "new_tokens": NEW, "llm": args.llm if args.workload == "full" else None, "llm_weights": args.weights,
                       "parallelism": f"dp{world}"},
            # CLIP-feature stage (preprocess + ViT 23 layers + pool), algorithmic 155.29 GFLOP/frame, per GPU
            "clip_feat_tflops": clip_feat_tflops, "clip_feat_frac_of_mfma_peak": clip_feat_tflops / PEAK_MFMA_TFLOPS,
            "clip_feat_tflops_all_gpus": clip_feat_tflops_total,
            "clip_feat_ms_per_step": vit_ms,
        }
        if collective:
            line["collective"] = collective
        if pcie:
            line["pcie_inclusive"] = pcie
        if latency:
            line["latency_b1"] = latency
        if runner:
            line["runner"] = runner
        if fam:
            line["families"] = fam
            line["family_share_of_step"] = {k: v["ms_per_step_est"] / ms_per_step for k, v in fam.items()}
        if roofline:
            line["roofline"] = roofline
            if getattr(wl, "roofline_mfma", None):
                line["roofline_mfma"] = wl.roofline_mfma
            if getattr(wl, "roofline_gemv", None):
                line["roofline_gemv"] = wl.roofline_gemv
        headline = (args.workload == "full" and args.llm == "7b" and args.weights == "16bit" and args.dtype == "bf16" and S == 224 and world == 1)
        if headline and args.full and not args.no_side:
            # Guarded side lines: driver-timed numbers for the parity-grade dtype and for BASELINE configs[4]; a failure costs
            # only its own field.  The headline models are freed first.
            wl.free()
            del model, tower, frames
            side = {}
            for key, ov, st, wu, roof in (("fp16", {"dtype": "fp16"}, 5, 1, False),
                                          ("cfg5_13b_fp8", {"llm": "13b", "weights": "fp8"}, 3, 1, True),
                                          # the PRODUCTION configuration of the released PG-Video-LLaVA weights (reference docs/1-CLI_DEMO.md:27-44): ViT-L/14-336
                                          # (577 tokens per frame), mlp2x_gelu projector, 676 video tokens -- with its own rooflines
                                          ("image336", {"image": 336}, 3, 1, True),
                                          ("clips32", {"clips_per_gpu": 32}, 1, 1, False),      # what a long runner queue would use: the weight stream of a token step shared by 32 clips
                                          # ... and by 64: what `--batch auto` picks on an MI355X next to a 7B replica, with the wide-batch GEMV roofline
                                          ("clips64", {"clips_per_gpu": 64}, 1, 1, True)):
                try:
                    side[key] = side_line(args, dev, ov, st, wu, roof)
                except Exception as e:                           # noqa: BLE001
                    side[key] = {"value": None, "error": f"{type(e).__name__}: {e}"}
            if side["fp16"].get("value"):
                side["fp16"]["ratio_to_headline"] = side["fp16"]["value"] / value
            line["side"] = side
        if args.gpus == 1 and args.full and not args.no_cpu_baseline and args.workload == "full":
            try:
                line["cpu_baseline"] = cpu_baseline_reference(args)
                line["gpu_over_cpu"] = value / line["cpu_baseline"]["value"]
                if args.cpu_port:
                    line["cpu_baseline"]["port"] = cpu_baseline_port(args)
            except Exception as e:                               # noqa: BLE001 -- a host-side hiccup (e.g. not enough RAM for the 27 GB fp32 model) must not cost the GPU line
                line["cpu_baseline"] = {"value": None, "unit": "videos/sec", "cores": os.cpu_count(), "kind": "reference", "error": f"{type(e).__name__}: {e}"}
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
