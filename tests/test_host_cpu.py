"""CPU-only: host logic and the C-ABI surface (no compute calls -- there is no GPU here)."""
import ctypes
import json
import os
import re
import socket
import subprocess
import time
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_and_exports_every_header_symbol():
    from video_llava_amd import _lib, build
    path = build.build()
    lib = ctypes.CDLL(path)
    header = open(os.path.join(ROOT, "include", "pgv.h")).read()
    declared = set(re.findall(r"\b(pgv_[a-z0-9_]+)\s*\(", header))
    declared -= {"pgv_epi"}
    assert len(declared) >= 30
    for name in sorted(declared):
        assert hasattr(lib, name), f"libpgv.so does not export {name}"
        assert name in _lib.PROTOTYPES, f"ctypes binding lacks {name}"
    assert set(_lib.PROTOTYPES) <= declared | {"pgv_version"}
    lib.pgv_version.restype = ctypes.c_int
    assert lib.pgv_version() == _lib.ABI_VERSION


def test_release_library_reads_five_switches_and_the_split_merge_lowers_to_sc1():
    """VERDICT r4 item 8 / ADVICE r4: the release libpgv.so reads exactly the five documented environment switches -- every
    launch-shape A/B switch lives behind -DPGV_LAB in libpgv_lab.so -- and the fence-free cross-workgroup merge of the split decode attention
    still lowers to sc1 stores / loads with no cache maintenance (build.check_isa)."""
    from video_llava_amd import build
    data = open(build.build(), "rb").read()
    names = set(re.findall(rb"\x00(PGV_[A-Z0-9_]{3,})\x00", data))        # NUL-delimited C strings: getenv names (PGV_F16 ... inside messages are not)
    assert names == {b"PGV_DATTN_SPLIT", b"PGV_LLM_NORM_FOLD", b"PGV_NO_GRAPH", b"PGV_VIT_LANES", b"PGV_VIT_LN_FOLD"}, names
    found = build.check_isa()
    split = {k: v for k, v in found.items() if k[0] != "vit_attn"}
    assert len(split) == 6 and all(v["cache_maintenance"] == 0 and v["atomics"] == 1 for v in split.values())
    # ... and the two pieces of inline asm of the ViT attention kernel still assemble as written: the half swap keeps its wait state,
    # every LDS-DMA sits directly behind the s_mov_b32 m0 that belongs to it
    attn = {k: v for k, v in found.items() if k[0] == "vit_attn"}
    assert len(attn) == 4 and all(v["half_swaps_with_wait_state"] >= 2 and v["lds_dma"] == v["lds_dma_with_m0"] >= 2 for v in attn.values()), attn


def test_product_path_fails_loudly_without_gpu():
    from video_llava_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.Context.get(0)
    from video_llava_amd.inference import get_spatio_temporal_features_torch
    with pytest.raises(RuntimeError, match="GPU"):
        get_spatio_temporal_features_torch(torch.zeros(2, 4, 1024, dtype=torch.float16))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "video_llava_amd")
    for dp, _dn, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{fn} imports the oracle"
                assert "/root/reference" not in src, f"{fn} reads the reference tree"


def test_prompts_match_reference(golden_dir):
    from video_llava_amd.video_conversation import conv_templates
    ref = json.load(open(os.path.join(golden_dir, "prompts.json")))
    for mode, want in ref.items():
        c = conv_templates[mode].copy()
        c.append_message(c.roles[0], "what is the person doing?\n<vid_start><vid_patch><vid_patch><vid_end>")
        c.append_message(c.roles[1], None)
        assert c.get_prompt() == want, mode


def test_build_prompt_layout():
    from video_llava_amd.inference import build_prompt
    p, stop = build_prompt("what is happening", "pg-video-llava", 356, True)
    assert stop == "</s>" and p.endswith("ASSISTANT:")
    assert p.count("<vid_patch>") == 356 and p.count("<vid_start>") == 1 and p.index("<vid_start>") < p.index("<vid_end>")
    p2, _ = build_prompt("q", "pg-video-llava", 4, True, transcript="hello")
    assert 'The noisy audio transcript of this video is:\n"hello"' in p2
    p3, stop3 = build_prompt("q", "default", 4, False)
    assert stop3 == "###" and "<vid_start>" not in p3


def test_get_seq_frames_golden(golden_dir):
    from video_llava_amd.eval.model_utils import get_seq_frames
    table = json.load(open(os.path.join(golden_dir, "seq_frames.json")))
    for key, ref in table.items():
        n, k = map(int, key.split(","))
        assert get_seq_frames(n, k) == ref


def test_keywords_stopping_criteria_semantics():
    from video_llava_amd.model.utils import KeywordsStoppingCriteria

    class Tok:
        def __call__(self, s):
            class R: pass
            r = R(); r.input_ids = [1, 2] if s == "</s>" else [7]
            return r

        def batch_decode(self, ids, skip_special_tokens=True):
            return ["".join(chr(96 + int(t)) for t in row) for row in ids]
    ids = torch.tensor([[5, 6]])
    c = KeywordsStoppingCriteria(["cd"], Tok(), ids)
    assert c.keyword_ids == [7]
    assert c(ids, None) is False                      # first call only records the prompt length
    assert c(torch.tensor([[5, 6, 1]]), None) is False
    assert c(torch.tensor([[5, 6, 1, 7]]), None) is True          # single-id keyword matched on the last token
    c2 = KeywordsStoppingCriteria(["</s>"], Tok(), ids)
    assert c2.keyword_ids == []                                      # 2-id keyword is dropped, falls back to the substring search
    c3 = KeywordsStoppingCriteria(["cd"], Tok(), ids); c3(ids, None)
    assert c3(torch.tensor([[5, 6, 3, 4]]), None) is True           # "cd" appears in the decoded tail


def test_shard_indices_cover_and_order():
    from video_llava_amd import parallel
    for n, w in ((64, 8), (10, 4), (3, 8), (0, 2), (7, 1)):
        got = [i for r in range(w) for i in parallel.shard_indices(n, r, w)]
        assert got == list(range(n))
        assert max(len(parallel.shard_indices(n, r, w)) for r in range(w)) == (parallel.shard_capacity(n, w) if n else 0)


def test_gather_answers_single_rank():
    from video_llava_amd import parallel
    toks = torch.arange(12, dtype=torch.int32).view(3, 4)
    lens = torch.tensor([4, 0, 2], dtype=torch.int32)
    out = parallel.gather_answers(toks, lens, 3, 0, 1)
    assert out == [[0, 1, 2, 3], [], [8, 9]]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_dp_collation_world2_gloo(tmp_path):
    """world_size-2 run of the shard + all-gather collation on CPU (gloo), incl. a failing clip and a ragged shard."""
    script = tmp_path / "dp.py"
    script.write_text(f'''
import sys, json, torch
sys.path.insert(0, {ROOT!r})
from video_llava_amd import parallel
rank, world, local = parallel.init_distributed("gloo")
N, NEW = 5, 6
def infer(group):
    if 3 in group: raise RuntimeError("bad clip")
    toks = torch.stack([torch.arange(NEW, dtype=torch.int32) + 100 * i for i in group])
    return toks, [NEW - (i % 3) for i in group]
ans = parallel.run_sharded(N, infer, NEW, rank, world, torch.device("cpu"), per_gpu_batch=1, spill_path={str(tmp_path / "preds")!r})
open({str(tmp_path)!r} + f"/result_{{rank}}.json", "w").write(json.dumps(ans))   # files, not stdout: rank lines interleave
torch.distributed.destroy_process_group()
''')
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    results = {rk: json.load(open(tmp_path / f"result_{rk}.json")) for rk in (0, 1) if (tmp_path / f"result_{rk}.json").exists()}
    assert set(results) == {0, 1} and results[0] == results[1]
    ans = results[0]
    want = [[100 * i + t for t in range(6 - (i % 3))] for i in range(5)]
    want[3] = []                                                        # failed clip keeps an empty slot
    assert ans == want
    assert not list(tmp_path.glob("preds.rank*.partial.json"))          # the rank-local spill files are removed once the all-gather succeeded


def _spawn_ranks(script, world, extra_env=None, timeout=180):
    """Start `world` plain processes (no elastic agent: a dying rank must be noticed by OUR code, not by torchrun killing the group)."""
    port = _free_port()
    procs = []
    for rk in range(world):
        env = dict(os.environ, RANK=str(rk), LOCAL_RANK=str(rk), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **(extra_env or {}))
        procs.append(subprocess.Popen([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env))
    outs = []
    for pr in procs:
        try:
            out, _ = pr.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            pr.kill()
            out, _ = pr.communicate()
            out += "\n<<HUNG: killed by the test>>"
        outs.append((pr.returncode, out))
    return outs


def test_dp_rank_raising_mid_shard_keeps_its_slots_failed(tmp_path):
    """one rank's infer raises from its second group on (a GPU fault mid-shard): every rank must still finish, with exactly
    that rank's later slots marked failed (None: distinct from an empty answer) -- the skip-bad-clip policy of the reference's runner
    (video_chatgpt/eval/run_inference_qa_activitynet.py:74,103-104) applied per group."""
    script = tmp_path / "raise.py"
    script.write_text(f'''
import sys, json, torch
sys.path.insert(0, {ROOT!r})
from video_llava_amd import parallel
rank, world, local = parallel.init_distributed("gloo", timeout_s=60)
N, NEW = 12, 4
calls = [0]
def infer(group):
    calls[0] += 1
    if rank == 1 and calls[0] >= 2: raise RuntimeError("device fault on rank 1")
    return torch.stack([torch.arange(NEW, dtype=torch.int32) + 10 * i for i in group]), [NEW + 1 for i in group]
ans = parallel.run_sharded(N, infer, NEW, rank, world, torch.device("cpu"), per_gpu_batch=2, length_offset=1)
open({str(tmp_path)!r} + f"/r_{{rank}}.json", "w").write(json.dumps(ans))
torch.distributed.destroy_process_group()
''')
    outs = _spawn_ranks(script, 2)
    assert all(rc == 0 for rc, _ in outs), outs
    a0, a1 = (json.load(open(tmp_path / f"r_{rk}.json")) for rk in (0, 1))
    assert a0 == a1
    want = [[10 * i + t for t in range(4)] for i in range(12)]
    for i in (8, 9, 10, 11):                       # rank 1 owns clips 6..11; its first group (6, 7) succeeded
        want[i] = None
    assert a0 == want


def test_dp_rank_exiting_fails_the_survivor_loudly_not_forever(tmp_path):
    """A rank that EXITS before the collation (killed, out of memory): the survivor must not hang in the all-gather -- it raises
    parallel.CollationError well inside the process-group timeout (here 20 s) and exits non-zero."""
    script = tmp_path / "exit.py"
    script.write_text(f'''
import os, sys, time, torch
sys.path.insert(0, {ROOT!r})
from video_llava_amd import parallel
rank, world, local = parallel.init_distributed("gloo", timeout_s=20)
def infer(group):
    if rank == 1: os._exit(7)
    return torch.zeros(len(group), 3, dtype=torch.int32), [3] * len(group)
t0 = time.time()
try:
    parallel.run_sharded(4, infer, 3, rank, world, torch.device("cpu"), per_gpu_batch=2, spill_path={str(tmp_path / "preds")!r})
except parallel.CollationError as e:
    print("LOUD after %.1f s:" % (time.time() - t0), e); sys.exit(5)
print("collated?!"); sys.exit(0)
''')
    t0 = time.time()
    outs = _spawn_ranks(script, 2, timeout=150)
    assert outs[1][0] == 7
    assert outs[0][0] == 5 and "LOUD" in outs[0][1] and "HUNG" not in outs[0][1], outs[0]
    assert time.time() - t0 < 120
    # the survivor's finished shard is not lost with the collation -- its rank-local file holds it and the error names it
    kept = json.load(open(tmp_path / "preds.rank0.partial.json"))
    assert kept["indices"] == [0, 1] and kept["tokens"] == [[0, 0, 0], [0, 0, 0]] and kept["lengths"] == [3, 3] and "preds.rank0.partial.json" in outs[0][1]


def test_rank_affinity_slices_and_silent_fallback():
    """Per-rank CPU placement (parallel.pin_rank_to_numa_node): the slices of a node's CPU list are disjoint, contiguous and cover it; with
    no GPU / no sysfs entry the call changes nothing and returns None."""
    from video_llava_amd import parallel
    cpus = list(range(64, 128)) + list(range(192, 256))
    parts = [parallel.affinity_slice(cpus, 4, i) for i in range(4)]
    assert sum(parts, []) == cpus and [len(x) for x in parts] == [32, 32, 32, 32]
    parts = [parallel.affinity_slice(list(range(10)), 3, i) for i in range(3)]
    assert sum(parts, []) == list(range(10)) and [len(x) for x in parts] == [4, 3, 3]
    assert parallel.affinity_slice([1, 2], 4, 3) == [1, 2]                      # fewer CPUs than ranks: share them
    assert parallel._parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]
    before = os.sched_getaffinity(0)
    assert parallel.pin_rank_to_numa_node(0, 1) is None                          # no GPU in the build container
    assert os.sched_getaffinity(0) == before


def test_rank_affinity_from_gpu_position_in_sysfs(tmp_path):
    """the core slice comes from the GPU's position among ALL GPUs of its NUMA node in sysfs, not from the per-job rank order -- two
    jobs on one host (each seeing 4 of 8 GPUs) pin disjoint slices that together cover each node.  Fake sysfs: 8 GPUs, 4 per node, plus a
    non-GPU PCI function and another vendor's display controller that must be ignored; the CPU lists are cut to the cores this process may use."""
    from video_llava_amd import parallel
    allowed = sorted(os.sched_getaffinity(0))
    if len(allowed) < 8:
        pytest.skip("needs 8 usable cores")
    half = len(allowed) // 2
    node_cpus = [allowed[:half], allowed[half:]]
    root = tmp_path / "sys"
    bdfs = [f"0000:{0x10 + 0x10 * i:02x}:00.0" for i in range(8)]
    def dev(bdf, vendor, cls, node):
        d = root / "bus" / "pci" / "devices" / bdf
        d.mkdir(parents=True)
        (d / "vendor").write_text(vendor + "\n"); (d / "class").write_text(cls + "\n"); (d / "numa_node").write_text(f"{node}\n")
    for i, b in enumerate(bdfs):
        dev(b, "0x1002", "0x120000", i // 4)
    dev("0000:05:00.0", "0x8086", "0x030000", 0)                                 # another vendor's display controller
    dev("0000:10:00.1", "0x1002", "0x040300", 0)                                 # audio function of a GPU
    for n in (0, 1):
        d = root / "devices" / "system" / "node" / f"node{n}"
        d.mkdir(parents=True)
        (d / "cpulist").write_text(",".join(str(c) for c in node_cpus[n]) + "\n")
    assert parallel.node_gpu_bdfs(0, str(root)) == bdfs[:4] and parallel.node_gpu_bdfs(1, str(root)) == bdfs[4:]
    before = os.sched_getaffinity(0)
    try:
        got = {}
        for job, visible in (("A", [0, 2, 4, 6]), ("B", [1, 3, 5, 7])):              # two jobs, interleaved GPUs; local rank k of BOTH jobs used to get slice k
            for local, g in enumerate(visible):
                os.sched_setaffinity(0, before)
                share = parallel.pin_rank_to_numa_node(local, sysfs_root=str(root), bdf=bdfs[g], quiet=True)
                assert share and os.sched_getaffinity(0) == set(share)
                got[g] = share
        for n in (0, 1):
            parts = [got[g] for g in range(4 * n, 4 * n + 4)]
            assert sorted(sum(parts, [])) == node_cpus[n], (n, parts)               # disjoint and covering, across the two jobs
    finally:
        os.sched_setaffinity(0, before)


@pytest.mark.parametrize("launcher", ["self", "torchrun"])
def test_bench_launcher_dry_world2(launcher):
    """`python bench.py --gpus 2` with no torchrun environment must start its own two ranks (the driver's command shape) and print
    ONE rank-0 JSON line with n_gpus = 2 and the collective report; the torchrun form must keep working.  --dry: real sharding,
    barriers, all-gather (gloo) and max-over-ranks timing, no GPU work."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry", "--steps", "3", "--warmup", "1", "--clips-per-gpu", "3", "--new-tokens", "5"]
    if launcher == "self":
        cmd = [sys.executable, *tail]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), *tail]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["config"]["parallelism"] == "dp2" and d["scaling"] == "weak"
    assert d["collective"]["backend"] == "gloo" and d["collective"]["world_seen"] == 2 and d["collective"]["gather_ms"] > 0
    assert d["clips_checked"] == 6
    # the identity record of the process group (what proves, on an N-GPU node, that N ranks on N distinct devices took part): gathered over the group
    c = d["collective"]
    assert c["ranks_answered"] == 2 and c["world"] == 2 and [r["rank"] for r in c["ranks"]] == [0, 1] and len({r["pid"] for r in c["ranks"]}) == 2
    assert all(set(r) >= {"host", "device_bdf", "numa_node"} for r in c["ranks"]) and c["rccl_version"] is None and c["distinct_devices"] == 0


@pytest.mark.parametrize("n", [4, 8])
def test_bench_launcher_dry_world_4_8(n):
    """The driver's scaling tier runs N = 1, 2, 4, 8: the same skeleton at 4 and 8 ranks (gloo, --dry) -- every clip of every rank lands in its
    global slot on rank 0 and the per-rank step times are reported for all N ranks."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry", "--steps", "2", "--warmup", "1", "--clips-per-gpu", "2", "--new-tokens", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["config"]["parallelism"] == f"dp{n}" and d["scaling"] == "weak"
    assert d["collective"]["world_seen"] == n and d["clips_checked"] == 2 * n
    assert len(d["collective"].get("rank_ms_per_step", [0] * n)) == n


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs DIR: what the last timed step returned (here the collated answers of both ranks of a --dry run, in global clip order) as
    float32 .npy; --steps is the number of timed steps the line reports.  An output over its share of the 64 MB budget is written as a fixed
    seeded sample with its flat indices."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry", "--steps", "4", "--warmup", "0", "--clips-per-gpu", "3",
           "--new-tokens", "5", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 4 and d["ms_per_step"] > 0
    from video_llava_amd.benchlib import dry_pattern
    got = np.load(tmp_path / "out" / "answer_tokens.npy")
    assert got.dtype == np.float32 and got.tolist() == [dry_pattern(i, 5, 32003) for i in range(6)]

    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1200)
    big = np.arange(1000, dtype=np.float64).reshape(10, 100)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"x": big})
    idx = np.load(tmp_path / "a" / "x_index.npy")
    val = np.load(tmp_path / "a" / "x.npy")
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and val.dtype == np.float32 and np.array_equal(val, big.reshape(-1)[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "x_index.npy"))


def test_collective_identity_refuses_shared_devices_and_parses_the_rccl_log(tmp_path, monkeypatch):
    """parallel.collective_identity: two ranks of one host on one GPU are refused unless the caller allows it (bench.py: PGV_BENCH_SHARE_DEVICE=1);
    parallel.rccl_transport: the channel lines of an RCCL INFO log are counted into a P2P / SHM / NET verdict."""
    from video_llava_amd import parallel
    import torch.distributed as dist

    class FakeDist:
        @staticmethod
        def is_initialized():
            return True

        @staticmethod
        def get_backend():
            return "gloo"

        @staticmethod
        def get_world_size():
            return 2

        @staticmethod
        def all_gather_object(out, me):
            out[0] = dict(me, rank=0, device_bdf="0000:05:00.0")
            out[1] = dict(me, rank=1, device_bdf="0000:05:00.0", pid=me["pid"] + 1)
    monkeypatch.setattr(parallel, "dist", FakeDist)
    with pytest.raises(RuntimeError, match="share a GPU"):
        parallel.collective_identity(torch.device("cpu"), 0, 2)
    ok = parallel.collective_identity(torch.device("cpu"), 0, 2, allow_shared_device=True)
    assert ok["ranks_answered"] == 2 and ok["distinct_devices"] == 1
    with pytest.raises(RuntimeError, match="2 ranks answered, 3 expected"):
        parallel.collective_identity(torch.device("cpu"), 0, 3, allow_shared_device=True)
    monkeypatch.setattr(parallel, "dist", dist)
    log = tmp_path / "rccl.log"
    log.write_text("vm:1:1 [0] NCCL INFO Channel 00/0 : 0[0] -> 1[1] via P2P/IPC comm 0x1 nRanks 02\n"
                   "vm:1:1 [0] NCCL INFO Channel 01/0 : 1[1] -> 0[0] via P2P/IPC comm 0x1 nRanks 02\n"
                   "vm:1:1 [0] NCCL INFO === System : maxBw 48.0 totalBw 48.0 === XGMI\n")
    monkeypatch.setattr(parallel, "_rccl_debug_file", str(log))
    t = parallel.rccl_transport(cleanup=False)
    assert t["p2p"] == 2 and t["shm"] == 0 and t["net"] == 0 and t["verdict"] == "P2P" and t["xgmi_mentions"] == 1 and t["log_lines"] == 3
    log.write_text(log.read_text() + "vm:1:1 [0] NCCL INFO Channel 00 : 0[0] -> 1[1] via SHM/direct/direct\n")
    assert parallel.rccl_transport(cleanup=False)["verdict"] == "SHM"


def test_chat_turn_bookkeeping_follows_the_reference_rules(capsys):
    """Host logic of the chat front end without a device (reference video_chatgpt/chat.py:90-104 add_text, :201-222 print_state / _post_process_code):
    the first turn of a clip is cut at 1200 characters, gets the `<video>` marker once and carries the clip path; later turns are cut at 1536 and
    carry nothing; every turn queues a (user, text) and an open (assistant, None) message; escapes inside paired code fences are undone."""
    from types import SimpleNamespace as NS
    from video_llava_amd.chat import VideoChatGPTInterface
    from video_llava_amd.video_conversation import default_conversation
    model = NS(get_model=lambda: NS(vision_config=NS(use_vid_start_end=True)))
    iface = VideoChatGPTInterface(None, None, components=(model, None, None, NS(crop_size={"height": 224, "width": 224}), 356))
    assert iface.replace_token.count("<vid_patch>") == 356 and iface.replace_token.startswith("<vid_start>") and iface.replace_token.endswith("<vid_end>")
    iface.add_text("q" * 2000, "clip.mp4")
    (role_u, first), (role_a, open_slot) = iface.state.messages[-2:]
    assert (role_u, role_a) == tuple(default_conversation.roles[:2]) and open_slot is None
    assert first == ("q" * 1200 + "\n<video>", "clip.mp4") and iface.state.skip_next is False
    iface.first_run = False                                      # what answer() does after the first turn
    iface.add_text("<video> again " + "r" * 2000, "clip.mp4")
    assert iface.state.messages[-2][1] == ("<video> again " + "r" * 2000)[:1536] and iface.state.messages[-1][1] is None
    n0 = len(default_conversation.messages)                      # the template's own example exchange
    assert len(iface.state.messages) == n0 + 4
    iface.clear_history()
    iface.add_text("what is <video> about", None)                # the marker is not added twice
    assert iface.state.messages[-2][1] == ("what is <video> about", None) and len(iface.state.messages) == n0 + 2
    iface.print_state()
    out = capsys.readouterr().out
    assert out.startswith("SYSTEM: " + str(default_conversation.system)) and f"{default_conversation.roles[0]}: what is <video> about" in out
    post = VideoChatGPTInterface._post_process_code
    assert post("no fences \\_") == "no fences \\_"
    assert post("a\n```py\nx\\_y\n```\nb\\_") == "a\n```py\nx_y\n```\nb\\_"
    assert post("a\n```py\nx\\_y") == "a\n```py\nx\\_y"        # an unpaired fence: untouched


def test_kv_reuse_prefix_rules():
    """generate(kv_reuse_key=...) (round 6; a later chat turn prefills only what is behind the cached prefix, reference chat.py:108-160 re-runs the
    whole conversation): which prefix of the cache a new prompt may start from -- host logic, checked here on a stub without a device."""
    from video_llava_amd.model.video_chatgpt import VideoChatGPTLlamaForCausalLM as M, VisionConfig

    class Stub:
        pass
    m = Stub()
    m.model = Stub()
    vc = m.model.vision_config = VisionConfig()
    vc.vid_patch_token, vc.vid_start_token, vc.vid_end_token = 900, 901, 902
    kvh = object()
    cached = [1, 7, 8, 901, 900, 900, 902, 9, 10, 11, 40, 41, 42]        # prompt (with the video run) + the answer tokens that were fed back
    m._kv = {(1, 64): kvh}
    m._reuse = ("clip-a", kvh, 64, cached)
    f = lambda key, ids, new=8: M._reusable_prefix(m, key, ids, new)
    assert f("clip-a", cached + [50, 51]) == len(cached)                  # the new prompt extends the cache: everything is kept
    assert f("clip-a", cached[:10] + [60, 61, 62]) == 10                   # the answer came back re-tokenised: common prefix only
    assert f("clip-a", list(cached)) == len(cached) - 1                    # nothing new: one token still has to run (its logits pick the next)
    assert f("clip-b", cached + [50]) == 0                                 # another clip's conversation
    assert f("clip-a", [1, 7, 99] + cached[3:] + [50]) == 0                # diverges before the video run: the run would lie in the appended part
    assert f("clip-a", cached[:5]) == 0                                    # cut inside the video run
    assert f("clip-a", cached + [50], new=64) == 0                         # would outgrow the cache
    m._kv = {(1, 64): object()}
    assert f("clip-a", cached + [50]) == 0                                 # the cache the record points at is gone
    m._reuse = None
    assert f("clip-a", cached + [50]) == 0


@pytest.mark.parametrize("rel", ["bench.py", "video_llava_amd/benchlib.py", "__graft_entry__.py"])
def test_measurement_scripts_have_no_undefined_names(rel):
    """bench.py's CPU-baseline child only runs at the end of a GPU bench (it builds a 27 GB fp32 model), so a name that went missing in a refactor
    -- `make_prompts` after the measurement library was split out of the script, round 6 -- shows up as `cpu_baseline.value = null` on the
    driver's box and nowhere else.  Every name a function of these files loads must be defined in the file, imported, or a builtin."""
    import ast
    import builtins
    tree = ast.parse(open(os.path.join(ROOT, rel)).read())
    defined = set(dir(builtins)) | {"__file__", "__name__"}
    for n in ast.walk(tree):
        if isinstance(n, (ast.FunctionDef, ast.ClassDef)):
            defined.add(n.name)
        elif isinstance(n, ast.Import):
            defined.update((a.asname or a.name).split(".")[0] for a in n.names)
        elif isinstance(n, ast.ImportFrom):
            defined.update(a.asname or a.name for a in n.names)
        elif isinstance(n, ast.Name) and isinstance(n.ctx, (ast.Store, ast.Del)):
            defined.add(n.id)
        elif isinstance(n, ast.arg):
            defined.add(n.arg)
        elif isinstance(n, ast.ExceptHandler) and n.name:
            defined.add(n.name)
    used = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load)}
    assert not (used - defined), sorted(used - defined)


def test_bench_gpus_mismatch_is_loud():
    """A WORLD_SIZE that contradicts --gpus is an error, not a silently different run."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_release_library_has_no_lab_switches():
    """Switches that produce garbage by design (timing ablations) must not exist in the library the product loads: they are compiled
    only into libpgv_lab.so (-DPGV_LAB, video_llava_amd.build.build(lab=True)), which nothing under video_llava_amd/ binds."""
    from video_llava_amd import build
    lib = build.build()
    blob = open(lib, "rb").read()
    for needle in (b"PGV_GEMM_ABLATE", b"PGV_ATTN_ABLATE", b"ABLATE"):
        assert needle not in blob, f"{needle!r} found in {lib}"
    src = "".join(open(os.path.join(ROOT, "video_llava_amd", f)).read() for f in os.listdir(os.path.join(ROOT, "video_llava_amd")) if f.endswith(".py") and f != "_lib.py" and f != "build.py")
    assert "use_lab_build" not in src and "libpgv_lab" not in src


def test_sanitizer_build_of_the_host_shim_builds_and_loads():
    """libpgv_ubsan.so -- UBSan (non-recoverable) + libstdc++ container assertions on the host code of every translation unit,
    release kernels -- must build for gfx950 and export the whole C ABI under its preloaded runtime (the GPU suite runs under it with
    scripts/sessions/r4_ubsan.sh: 198 passed, 0 reports, profiles/r04_a_ubsan_gpu_tests.txt).  Nothing in the product binds it."""
    from video_llava_amd import _lib, build
    lib = build.build_sanitizer()
    rt = build.sanitizer_runtime()
    code = ("import ctypes, sys; sys.path.insert(0, %r); from video_llava_amd import _lib; _lib.LIB_PATH = %r; l = _lib.load(build_if_missing=False); "
            "print('OK', l.pgv_version(), len(_lib.PROTOTYPES))" % (ROOT, lib))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, LD_PRELOAD=rt))
    assert r.returncode == 0 and r.stdout.startswith(f"OK {_lib.ABI_VERSION} "), (r.stdout, r.stderr[-2000:])
    src = "".join(open(os.path.join(ROOT, "video_llava_amd", f)).read() for f in os.listdir(os.path.join(ROOT, "video_llava_amd")) if f.endswith(".py") and f != "build.py")
    assert "libpgv_ubsan" not in src and "build_sanitizer" not in src


def test_no_kernel_spills_to_scratch():
    """Every gfx950 kernel of libpgv must fit its registers: a spilled accumulator or DMA offset inside a GEMM/attention loop
    costs 2-3x (seen while building the 4-wave GEMM), so scratch use is a build failure, not a perf note."""
    from video_llava_amd import build
    build.build()
    llvm = "/opt/rocm/lib/llvm/bin"
    if not all(os.path.exists(os.path.join(llvm, t)) for t in ("clang-offload-bundler", "llvm-readelf", "llvm-objcopy")):
        pytest.skip("ROCm llvm tools not present")
    import tempfile
    checked = 0
    bad = []
    regs = {}
    with tempfile.TemporaryDirectory() as td:
        for src in build.sources_present():
            obj = os.path.join(build.OBJ, src.replace(".hip", ".o"))
            fat, co = os.path.join(td, "x.fatbin"), os.path.join(td, "x.co")
            subprocess.run([f"{llvm}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
            if not os.path.exists(fat) or os.path.getsize(fat) == 0:
                continue                                    # host-only translation unit
            r = subprocess.run([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True, text=True)
            assert r.returncode == 0, f"{src}: {r.stderr}"
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            names = re.findall(r"\.name:\s+(\S+)", notes)
            segs = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
            spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)]
            vgprs = [int(x) for x in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
            assert len(names) == len(segs) == len(spills) == len(vgprs), src
            checked += len(names)
            bad += [(n, sg, v) for n, sg, v in zip(names, segs, spills) if v > 0]
            regs.update(zip(names, vgprs))
            os.remove(fat)
    assert checked >= 20, f"only {checked} kernels found"
    assert not bad, f"kernels spilling VGPRs: {bad[:6]}"
    # Register budgets the launch shapes rely on (gfx950: 512 VGPRs per SIMD lane): a kernel that grows past its budget silently halves its
    # occupancy -- two waves per SIMD for the ViT attention (256), three workgroups of 8 waves per CU for the split decode attention (80:
    # all 640 workgroups of a 13B launch resident), one workgroup per CU with two waves per SIMD for the widest GEMV shapes (256).
    def worst(fragment):
        hit = {n: v for n, v in regs.items() if fragment in n}
        assert hit, fragment
        return max(hit.values())
    assert worst("vit_attn_kernel") <= 256
    assert worst("decode_attn_split_kernel") <= 80
    assert worst("decode_attn_kernelI") <= 128
    assert worst("gemv_mfma_kernel") <= 256 and worst("gemv_k8_kernel") <= 168


def test_gemm_tile_order_is_a_bijection(tmp_path):
    """The persistent GEMM's tile order (csrc/gemm.hip tile_coords_v: the W-resident order for wide outputs with an even tile-row count,
    the band order otherwise) must visit every output tile exactly once for every grid the path launches.  The function is not ported: its
    SOURCE TEXT is cut out of gemm.hip and compiled for the host (it is plain integer arithmetic), then brute-forced over the tile grids of
    the ViT passes (224 px: N = 257 tokens, 336 px: 577; 1 .. 1024 frames per lane; qkv 12 / fc1 16 / out_proj, fc2 4 tile columns), the
    LLaMA prefill projections (7B: 48 / 16 / 86; 13B: 60 / 20 / 108 tile columns) and every small grid."""
    import shutil
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src = open(os.path.join(ROOT, "video_llava_amd", "csrc", "gemm.hip")).read()
    i = src.index("__device__ __forceinline__ void tile_coords_v")
    depth, j = 0, src.index("{", i)
    for j in range(j, len(src)):
        depth += src[j] == "{"
        depth -= src[j] == "}"
        if depth == 0:
            break
    fn = src[i:j + 1]
    assert "wn = ntn >> 2" in fn and "band" in fn            # both orders are in the cut
    prog = """#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
#define __forceinline__ inline
using std::min;
""" + fn + """
int main(int argc, char** argv) {
    long checked = 0;
    for (int a = 1; a + 1 < argc; a += 2) {
        const int ntm = atoi(argv[a]), ntn = atoi(argv[a + 1]), total = ntm * ntn;
        std::vector<char> seen(total, 0);
        for (int vb = 0; vb < total; ++vb) {
            int tm = -1, tn = -1;
            tile_coords_v(vb, total, ntm, ntn, tm, tn);
            if (tm < 0 || tm >= ntm || tn < 0 || tn >= ntn || seen[tm * ntn + tn]) { printf("BAD ntm=%d ntn=%d vb=%d -> (%d,%d)\\n", ntm, ntn, vb, tm, tn); return 1; }
            seen[tm * ntn + tn] = 1;
        }
        ++checked;
    }
    printf("OK %ld\\n", checked);
    return 0;
}
"""
    cpp, exe = tmp_path / "tiles.cpp", tmp_path / "tiles"
    cpp.write_text(prog)
    subprocess.run([gxx, "-O1", "-o", str(exe), str(cpp)], check=True)
    grids = set()
    for tokens in (257, 577):
        for frames in list(range(1, 130)) + [200, 256, 399, 400, 401, 512, 799, 800, 1000, 1024]:
            ntm = (frames * tokens + 255) // 256
            for ntn in (4, 12, 16):
                grids.add((ntm, ntn))
        for frames in range(1, 130):
            grids.add(((frames * (tokens - 1) + 255) // 256, 4))                 # patch-embed GEMM: M = frames x patches
    for rows in (1, 2, 441, 454, 3528, 7264):                                   # prefill: sum of prompt lengths (1 .. 16 sequences)
        for ntn in (48, 16, 86, 60, 20, 108, 1, 2, 3, 5, 8, 9, 17):
            grids.add(((rows + 255) // 256, ntn))
    for ntm in range(1, 41):
        for ntn in range(1, 41):
            grids.add((ntm, ntn))
    args = [str(x) for g in sorted(grids) for x in g]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    assert (402, 12) in grids and (804, 16) in grids                           # the two grids bench.py times


def test_llm_weight_table_layouts_and_keys(tmp_path):
    """csrc/llm_weights.h is the one description of the decoder's matrices: compiled on its own with g++ (it must need no HIP header), it has to
    give (1) the byte offset of every item and the total of the 16-bit, fp8 and 12-bit blobs exactly as the hand-written layouts it replaced
    did -- restated below from those formulas, the 12-bit size as in w12_numpy.nbytes -- for the tiny test model, 7B and 13B (the totals decide
    what `--batch auto` fits next to a replica); (2) for each of the seven matrix keys, at the first and the last layer, the matrix, its shape,
    row offset, row count and gate / up interleave that pgv_llm_load_tensor / pgv_llm_get_weight used; (3) a status, not a crash, for malformed
    keys.  Where g++ has the sanitizer runtimes the same stand-alone program runs a second time under ASan + UBSan."""
    import shutil
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    csrc = os.path.join(ROOT, "video_llava_amd", "csrc")
    prog = r"""#include <cstdio>
#include "llm_weights.h"
int main(int argc, char** argv) {
    const LlmDims d{atoll(argv[1]), atoll(argv[2]), atoll(argv[3]), atoi(argv[4])};
    const LlmLayout lo = llm_layout(d);
    printf("mat16"); for (const LlmMatSlot& x : lo.mat) printf(" %zu", x.w16);
    printf("\naux16 %zu %zu %zu", lo.embed, lo.norm_g, lo.rope); for (int l = 0; l < d.L; ++l) printf(" %zu %zu", lo.in_g[l], lo.post_g[l]);
    printf("\nmat8"); for (const LlmMatSlot& x : lo.mat) printf(" %zu", x.w8);
    printf("\naux8"); for (const LlmMatSlot& x : lo.mat) printf(" %zu", x.scale);
    printf("\nmat12"); for (const LlmMatSlot& x : lo.mat) printf(" %zu", x.w12);
    printf("\ntotal16 %zu\ntotal8 %zu\ntotal12 %zu\n", lo.total16, lo.total8, lo.total12);
    for (int i = 5; i < argc; ++i) {
        const LlmLayerKey k = llm_parse_layer_key(argv[i], d.L);
        printf("key %d %d", (int)k.status, k.layer);
        if (k.status == LLM_KEY_MATRIX) {
            const LlmMatSlot& s = lo.mat[llm_mat_index(k.layer, k.mat->kind)];
            printf(" %d %lld %lld %lld %lld %d %d", k.mat->kind, s.N, s.K, llm_dim(k.mat->row_off, d.H, d.I), llm_dim(k.mat->rows, d.H, d.I), k.mat->row_blk, k.mat->blk_stride);
        } else if (k.status == LLM_KEY_OTHER) printf(" rest=%zu", strlen(k.rest));
        printf("\n");
    }
    return 0;
}
"""
    cpp, exe, exe_san = tmp_path / "weights.cpp", tmp_path / "weights", tmp_path / "weights_san"
    cpp.write_text(prog)
    base = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", csrc, str(cpp)]
    subprocess.run([*base, "-o", str(exe)], check=True)
    exes = [exe]
    san = subprocess.run([*base, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe_san)], capture_output=True, text=True)
    if san.returncode == 0:
        exes.append(exe_san)
    else:
        assert "asan" in san.stderr or "ubsan" in san.stderr, san.stderr        # only a missing sanitizer runtime excuses the second build
        print("g++ has no sanitizer runtimes here: plain build only")

    def align(x):
        return (x + 255) // 256 * 256

    def expected(H, I, V, L):
        """The layouts of pgv_llm_create / pgv_llm_quantize_fp8 / w12_slots before the table, item by item in their order."""
        shapes = [(3 * H, H), (H, H), (2 * I, H), (H, I)]
        off, mat16, aux16 = 0, [], []
        for dst, nbytes in [(aux16, V * H * 2), (mat16, V * H * 2), (aux16, H * 4), (aux16, 4096 * 64 * 8)]:
            dst.append(off); off += align(nbytes)
        for _ in range(L):
            for _g in range(2):
                aux16.append(off); off += align(H * 4)
            for N, K in shapes:
                mat16.append(off); off += align(N * K * 2)
        total16 = off
        off, mat8, aux8 = 0, [], []
        for group in [[(V, H)]] + [shapes] * L:
            for N, K in group:
                mat8.append(off); off += align(N * K)
            for N, K in group:
                aux8.append(off); off += align(N * 4)
        total8 = off
        off, mat12 = 0, []
        for N, K in [(V, H)] + shapes * L:
            mat12.append(off); off += align(N * K * 3 // 2 + (N // 16) * 64 * 4 + N)
        return {"mat16": mat16, "aux16": aux16, "total16": [total16], "mat8": mat8, "aux8": aux8, "total8": [total8], "mat12": mat12, "total12": [off]}

    suffixes = ["self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight", "mlp.gate_proj.weight",
                "mlp.up_proj.weight", "mlp.down_proj.weight"]
    NOT_LAYER, BAD_INDEX, OTHER, MATRIX = 0, 1, 2, 3
    for H, I, V, L in [(512, 768, 592, 2), (4096, 11008, 32080, 32), (5120, 13824, 32080, 40)]:
        # (kind, N, K, row_off, rows, row_blk, blk_stride) as the if-ladders of pgv_llm_load_tensor and pgv_llm_get_weight had them
        want_mat = [(0, 3 * H, H, 0, H, 0, 0), (0, 3 * H, H, H, H, 0, 0), (0, 3 * H, H, 2 * H, H, 0, 0), (1, H, H, 0, H, 0, 0),
                    (2, 2 * I, H, 0, I, 32, 64), (2, 2 * I, H, 32, I, 32, 64), (3, H, I, 0, H, 0, 0)]
        keys, want = [], []
        for layer in (0, L - 1):
            for sfx, t in zip(suffixes, want_mat):
                keys.append(f"model.layers.{layer}.{sfx}"); want.append([MATRIX, layer, *t])
        for key, status in [("model.layers..x", BAD_INDEX), ("model.layers.-1.mlp.up_proj.weight", BAD_INDEX), (f"model.layers.{L}.mlp.up_proj.weight", BAD_INDEX),
                            ("model.layers.1", BAD_INDEX), ("model.layers.", BAD_INDEX), ("model.layers." + "9" * 4096 + ".mlp.up_proj.weight", BAD_INDEX),
                            ("model.layers.1.", OTHER), ("model.layers.1.self_attn.q_proj.weightX", OTHER), ("model.layers.1.self_attn.q_proj.weigh", OTHER),
                            ("model.layers.1." + "a" * 4096, OTHER), ("model.layers.0.input_layernorm.weight", OTHER),
                            ("model.layers.0.self_attn.rotary_emb.inv_freq", OTHER), ("x" * 4096, NOT_LAYER), ("", NOT_LAYER), ("lm_head.weight", NOT_LAYER),
                            ("model.layers", NOT_LAYER), ("xmodel.layers.0.mlp.up_proj.weight", NOT_LAYER)]:
            keys.append(key)
            want.append([status, 1 if key.startswith("model.layers.1.") else 0 if status == OTHER else -1])
        exp = expected(H, I, V, L)
        for x in exes:
            r = subprocess.run([str(x), str(H), str(I), str(V), str(L), *keys], capture_output=True, text=True)
            assert r.returncode == 0 and not r.stderr, (x, r.returncode, r.stderr[-2000:])
            lines = [ln.split() for ln in r.stdout.splitlines()]
            got = {ln[0]: [int(v) for v in ln[1:]] for ln in lines if ln[0] != "key"}
            assert got == exp, [(k, got.get(k), exp[k]) for k in exp if got.get(k) != exp[k]][:1]
            got_keys = [[int(v) for v in ln[1:] if not v.startswith("rest=")] for ln in lines if ln[0] == "key"]
            assert got_keys == want, [(k, g, w) for k, g, w in zip(keys, got_keys, want) if g != w][:3]
            rests = [int(ln[-1][5:]) for ln in lines if ln[0] == "key" and ln[-1].startswith("rest=")]
            assert rests == [len(k.split(".", 3)[3]) for k, w in zip(keys, want) if w[0] == OTHER]       # `rest` points at the suffix behind the index
    assert expected(512, 768, 592, 2)["mat8"][1] == align(592 * 512) + align(592 * 4)                # the head's scales sit between its codes and layer 0's
    # nothing but llm.hip reads the table
    users = [f for f in sorted(os.listdir(csrc)) if '#include "llm_weights.h"' in open(os.path.join(csrc, f)).read()]
    assert users == ["llm.hip"], users


def test_pick_params_and_decode_graph_key(tmp_path):
    """csrc/pick_params.h and csrc/kv_features.h, each compiled on its own with g++ (they must need no HIP header): (1) pick_greedy(p) is
    temperature 1, top_k 1, top_p 1, penalty p, greedy; (2) two decode-graph keys, built by the ONE builder llm.hip uses (KvFeatures + the per-call
    values), that differ in exactly one of the key's 21 fields -- B, eos, flags, generation, the log-probability switch, the nine PickParams fields,
    beams, bans, lookup_D, lookup_n, guide_pairs, guide_scale, allowed -- compare unequal: a field left out of the comparison would replay a stale
    graph; (3) the builder's five normalisations, one by one: the keys of two runs without AM_SAMPLE compare equal whatever sampled parameters an
    earlier run left in flight (and differ from a sampled run's), beams is 0 without AM_BEAM, guide_scale is 1 without pairs, lookup_D / lookup_n
    are 0 unless the steps are lookup steps, and bans / allowed are 0 when off; (4) the rule table: for every operation and every single feature
    switched on in an otherwise neutral KvFeatures, refused or not and with which message, against the literal list below, and the three orderings
    (set_guidance: logprobs before beam before lookup; beam_begin: bans before allowed; lookup run: penalty before bans).  Where g++ has the
    sanitizer runtimes the same stand-alone program runs a second time under ASan + UBSan.  llm.hip holds no second copy of a rule text or of
    the key assembly."""
    import shutil
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    csrc = os.path.join(ROOT, "video_llava_amd", "csrc")
    prog = r"""#include <cstdio>
#include <cstring>
#include "kv_features.h"
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad = 1; } } while (0)
// a cache with nothing on but (maybe) the log-probabilities, stepping plain steps: the six values the key had before the features
static DecodeGraphKey key6(int B, int eos, int flags, int generation, bool logprobs, const PickParams& in_flight) {
    KvFeatures f;
    f.logprobs = logprobs;
    return decode_graph_key(f, B, eos, flags, generation, in_flight, false);
}
// the first refusal of an operation, phase 0 before phase 1, "" for none
static const char* first(KvOp op, const KvFeatures& f) {
    static char msg[512];
    if (kv_refusal(op, 0, f, "W", "X", msg, sizeof(msg)) || kv_refusal(op, 1, f, "W", "X", msg, sizeof(msg))) return msg;
    return "";
}
struct Want { KvOp op; KvFeature on; const char* msg; };
int main() {
    const PickParams d;
    EXPECT(d.temperature == 1.f && d.top_k == 0 && d.top_p == 1.f && d.penalty == 1.f && !d.greedy);
    const PickParams g = pick_greedy(1.3f);
    EXPECT(g.temperature == 1.f && g.top_k == 1 && g.top_p == 1.f && g.penalty == 1.3f && g.greedy);
    EXPECT((g == PickParams{1.f, 1, 1.f, 1.3f, true}) && !(g == pick_greedy(1.2f)));
    const PickParams p{0.7f, 50, 0.9f, 1.2f, false};
    const int F = AM_INC_POS | AM_RECORD | AM_SAMPLE;
    const DecodeGraphKey k = key6(2, 7, F, 3, false, p);
    EXPECT(k == key6(2, 7, F, 3, false, p));
    EXPECT(k.B == 2 && k.eos == 7 && k.flags == F && k.generation == 3 && !k.logprobs && k.pick == p);
    EXPECT(!(DecodeGraphKey{} == k) && DecodeGraphKey{}.generation == -1);
    int differ = 0;
    differ += !(k == key6(3, 7, F, 3, false, p));
    differ += !(k == key6(2, -1, F, 3, false, p));
    differ += !(k == key6(2, 7, F & ~AM_RECORD, 3, false, p));
    differ += !(k == key6(2, 7, F, 4, false, p));
    differ += !(k == key6(2, 7, F, 3, true, p));
    differ += !(k == key6(2, 7, F, 3, false, {0.8f, 50, 0.9f, 1.2f, false}));
    differ += !(k == key6(2, 7, F, 3, false, {0.7f, 49, 0.9f, 1.2f, false}));
    differ += !(k == key6(2, 7, F, 3, false, {0.7f, 50, 0.8f, 1.2f, false}));
    differ += !(k == key6(2, 7, F, 3, false, {0.7f, 50, 0.9f, 1.3f, false}));
    differ += !(k == key6(2, 7, F, 3, false, {0.7f, 50, 0.9f, 1.2f, true}));
    EXPECT(differ == 10);
    const int G = AM_INC_POS | AM_RECORD;
    const DecodeGraphKey a = key6(2, 7, G, 3, false, p), b = key6(2, 7, G, 3, false, pick_greedy(2.f));
    EXPECT(a == b && a.pick == PickParams{} && !(a == k));

    // (2) all 21 fields, from a key in which none is normalised away: a sampled beam flag set, lookup steps, every feature on
    KvFeatures on;
    on.bans = 4; on.allowed = 6; on.guide_pairs = 3; on.guide_scale = 1.5f; on.lookup_D = 3; on.lookup_n = 2; on.beams = 2; on.penalty = 1.2f;
    const PickParams q{0.7f, 50, 0.9f, 1.2f, false, 0.05f, 0.9f, 1e-3f, 2e-3f};
    const int FB = F | AM_BEAM;
    const DecodeGraphKey full = decode_graph_key(on, 4, 7, FB, 3, q, true);
    EXPECT(full == decode_graph_key(on, 4, 7, FB, 3, q, true));
    EXPECT(full.beams == 2 && full.bans == 4 && full.allowed == 6 && full.guide_pairs == 3 && full.guide_scale == 1.5f && full.lookup_D == 3 && full.lookup_n == 2 && full.pick == q);
    int all = 0;
    all += !(full == decode_graph_key(on, 5, 7, FB, 3, q, true));
    all += !(full == decode_graph_key(on, 4, -1, FB, 3, q, true));
    all += !(full == decode_graph_key(on, 4, 7, FB & ~AM_RECORD, 3, q, true));
    all += !(full == decode_graph_key(on, 4, 7, FB, 4, q, true));
    { KvFeatures f = on; f.logprobs = true; all += !(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    const PickParams qs[9] = {{0.8f, 50, 0.9f, 1.2f, false, 0.05f, 0.9f, 1e-3f, 2e-3f}, {0.7f, 49, 0.9f, 1.2f, false, 0.05f, 0.9f, 1e-3f, 2e-3f},
                              {0.7f, 50, 0.8f, 1.2f, false, 0.05f, 0.9f, 1e-3f, 2e-3f}, {0.7f, 50, 0.9f, 1.3f, false, 0.05f, 0.9f, 1e-3f, 2e-3f},
                              {0.7f, 50, 0.9f, 1.2f, true, 0.05f, 0.9f, 1e-3f, 2e-3f},  {0.7f, 50, 0.9f, 1.2f, false, 0.06f, 0.9f, 1e-3f, 2e-3f},
                              {0.7f, 50, 0.9f, 1.2f, false, 0.05f, 0.8f, 1e-3f, 2e-3f}, {0.7f, 50, 0.9f, 1.2f, false, 0.05f, 0.9f, 2e-3f, 2e-3f},
                              {0.7f, 50, 0.9f, 1.2f, false, 0.05f, 0.9f, 1e-3f, 3e-3f}};
    for (const PickParams& x : qs) all += !(full == decode_graph_key(on, 4, 7, FB, 3, x, true));
    { KvFeatures f = on; f.beams = 3; all += !(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    { KvFeatures f = on; f.bans = 5; all += !(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    { KvFeatures f = on; f.lookup_D = 4; all += !(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    { KvFeatures f = on; f.lookup_n = 3; all += !(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    { KvFeatures f = on; f.guide_pairs = 2; all += !(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    { KvFeatures f = on; f.guide_scale = 2.5f; all += !(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    { KvFeatures f = on; f.allowed = 7; all += !(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    EXPECT(all == 21);
    { KvFeatures f = on; f.penalty = 1.3f; EXPECT(full == decode_graph_key(f, 4, 7, FB, 3, q, true)); }      // the penalty reaches a step through the PickParams in flight only

    // (3) the normalisations, one by one
    EXPECT(decode_graph_key(on, 4, 7, FB & ~AM_SAMPLE, 3, q, true).pick == PickParams{});                    // without AM_SAMPLE: default PickParams
    EXPECT(decode_graph_key(on, 4, 7, FB & ~AM_SAMPLE, 3, q, true) == decode_graph_key(on, 4, 7, FB & ~AM_SAMPLE, 3, qs[0], true));
    EXPECT(decode_graph_key(on, 4, 7, F, 3, q, true).beams == 0);                                            // without AM_BEAM: beams 0
    { KvFeatures f = on; f.beams = 3; EXPECT(decode_graph_key(on, 4, 7, F, 3, q, true) == decode_graph_key(f, 4, 7, F, 3, q, true)); }
    { KvFeatures f = on; f.guide_pairs = 0; f.guide_scale = 2.5f;                                            // without pairs: scale 1
      const DecodeGraphKey x = decode_graph_key(f, 4, 7, FB, 3, q, true);
      EXPECT(x.guide_pairs == 0 && x.guide_scale == 1.f);
      f.guide_scale = 1.5f; EXPECT(x == decode_graph_key(f, 4, 7, FB, 3, q, true)); }
    { const DecodeGraphKey x = decode_graph_key(on, 4, 7, FB, 3, q, false);                                  // plain steps: D and n stay out
      EXPECT(x.lookup_D == 0 && x.lookup_n == 0 && !(x == full));
      KvFeatures f = on; f.lookup_D = 7; f.lookup_n = 4; EXPECT(x == decode_graph_key(f, 4, 7, FB, 3, q, false)); }
    { KvFeatures f = on; f.bans = 0; f.allowed = 0;                                                          // off: 0, and 0 is what a neutral cache gives
      const DecodeGraphKey x = decode_graph_key(f, 4, 7, FB, 3, q, true);
      EXPECT(x.bans == 0 && x.allowed == 0 && key6(2, 7, F, 3, false, p).bans == 0 && key6(2, 7, F, 3, false, p).allowed == 0); }

    // (4) the rule table: every (operation, single feature) that refuses, with its text; every other pair passes
    const Want want[] = {
        {KV_SET_ALLOWED, KF_BEAM, "W: a beam run is in flight in this cache (the beam pick applies no logits processor)"},
        {KV_SET_ALLOWED, KF_LOOKUP, "W: pgv_kv_set_lookup is on in this cache (lookup steps verify drafts against the unconstrained pick)"},
        {KV_SET_LOGPROBS, KF_GUIDANCE, "W: guidance is on in this cache (a guided pick records no log-probabilities)"},
        {KV_SET_GUIDANCE, KF_LOGPROBS, "W: pgv_kv_set_logprobs is on in this cache (a guided pick records no log-probabilities)"},
        {KV_SET_GUIDANCE, KF_BEAM, "W: a beam run is in flight in this cache"},
        {KV_SET_GUIDANCE, KF_LOOKUP, "W: pgv_kv_set_lookup is on in this cache (lookup steps verify drafts against the unguided pick)"},
        {KV_SET_LOOKUP, KF_GUIDANCE, "W: guidance is on in this cache (pgv_kv_set_guidance(kv, 1, 0) turns it off)"},
        {KV_SET_LOOKUP, KF_ALLOWED, "W: a token automaton is set on this cache (pgv_kv_set_allowed); lookup steps verify drafts against the unconstrained pick"},
        {KV_PREFILL_SLOTS, KF_GUIDANCE, "W: guidance is on in this cache (pgv_kv_set_guidance(kv, 1, 0) turns it off)"},
        {KV_FORK, KF_GUIDANCE, "W: guidance is on in this cache (pgv_kv_set_guidance(kv, 1, 0) turns it off)"},
        {KV_BEAM_BEGIN, KF_GUIDANCE, "W: guidance is on in this cache (pgv_kv_set_guidance(kv, 1, 0) turns it off)"},
        {KV_BEAM_BEGIN, KF_BANS, "W: logit bans are set on this cache (pgv_kv_set_bans); the beam pick applies no logits processor"},
        {KV_BEAM_BEGIN, KF_ALLOWED, "W: a token automaton is set on this cache (pgv_kv_set_allowed); the beam pick applies no logits processor"},
        {KV_LOOKUP_RUN, KF_GUIDANCE, "W: guidance is on in this cache (pgv_kv_set_guidance(kv, 1, 0) turns it off)"},
        {KV_LOOKUP_RUN, KF_PENALTY, "W: a repetition penalty is set on this cache (pgv_kv_set_warpers); lookup steps verify X"},
        {KV_LOOKUP_RUN, KF_BANS, "W: logit bans are set on this cache (pgv_kv_set_bans); lookup steps verify X"},
        {KV_LOOKUP_RUN, KF_ALLOWED, "W: a token automaton is set on this cache (pgv_kv_set_allowed); lookup steps verify X"},
        {KV_LOOKUP_RUN, KF_LOGPROBS, "W: log-probabilities are on (pgv_kv_set_logprobs); lookup steps record none"},
        {KV_LOOKUP_RUN, KF_BEAM, "W: a beam run is in flight on this cache"},
    };
    const KvOp ops[] = {KV_SET_ALLOWED, KV_SET_LOGPROBS, KV_SET_GUIDANCE, KV_SET_LOOKUP, KV_PREFILL_SLOTS, KV_FORK, KV_BEAM_BEGIN, KV_LOOKUP_RUN};
    const KvFeature feats[] = {KF_LOGPROBS, KF_BANS, KF_ALLOWED, KF_GUIDANCE, KF_LOOKUP, KF_BEAM, KF_PENALTY};
    int refused = 0;
    for (KvOp op : ops) {
        EXPECT(!strcmp(first(op, KvFeatures{}), ""));                     // a neutral cache: nothing refuses
        for (KvFeature x : feats) {
            KvFeatures f;
            if (x == KF_LOGPROBS) f.logprobs = true;
            if (x == KF_BANS) f.bans = 1;
            if (x == KF_ALLOWED) f.allowed = 1;
            if (x == KF_GUIDANCE) { f.guide_pairs = 1; f.guide_scale = 2.f; }
            if (x == KF_LOOKUP) { f.lookup_D = 3; f.lookup_n = 2; }
            if (x == KF_BEAM) f.beams = 2;
            if (x == KF_PENALTY) f.penalty = 1.2f;
            const char* expect = "";
            for (const Want& w : want) if (w.op == op && w.on == x) expect = w.msg;
            const char* got = first(op, f);
            if (strcmp(got, expect)) { printf("FAILED op %d feature %d: got '%s', want '%s'\n", (int)op, (int)x, got, expect); bad = 1; }
            refused += got[0] != 0;
        }
    }
    EXPECT(refused == 19);
    // the phases: the rules behind an operation's own state checks are not reported before them
    { KvFeatures f; f.bans = 1; f.allowed = 1; char m[512];
      EXPECT(!kv_refusal(KV_BEAM_BEGIN, 0, f, "W", "X", m, sizeof(m)) && kv_refusal(KV_BEAM_BEGIN, 1, f, "W", "X", m, sizeof(m)));
      f.penalty = 1.2f; f.logprobs = true; f.beams = 2;
      EXPECT(!kv_refusal(KV_LOOKUP_RUN, 0, f, "W", "X", m, sizeof(m)) && kv_refusal(KV_LOOKUP_RUN, 1, f, "W", "X", m, sizeof(m))); }
    // the orderings
    { KvFeatures f; f.logprobs = true; f.beams = 2; f.lookup_D = 3; f.lookup_n = 2;
      EXPECT(!strcmp(first(KV_SET_GUIDANCE, f), "W: pgv_kv_set_logprobs is on in this cache (a guided pick records no log-probabilities)"));
      f.logprobs = false; EXPECT(!strcmp(first(KV_SET_GUIDANCE, f), "W: a beam run is in flight in this cache")); }
    { KvFeatures f; f.bans = 1; f.allowed = 1;
      EXPECT(!strcmp(first(KV_BEAM_BEGIN, f), "W: logit bans are set on this cache (pgv_kv_set_bans); the beam pick applies no logits processor")); }
    { KvFeatures f; f.penalty = 1.2f; f.bans = 1;
      EXPECT(!strcmp(first(KV_LOOKUP_RUN, f), "W: a repetition penalty is set on this cache (pgv_kv_set_warpers); lookup steps verify X")); }
    { KvFeatures f; f.guide_pairs = 1; f.guide_scale = 2.f; f.bans = 1; f.penalty = 1.2f;                   // guidance is reported before everything
      EXPECT(!strcmp(first(KV_LOOKUP_RUN, f), "W: guidance is on in this cache (pgv_kv_set_guidance(kv, 1, 0) turns it off)"));
      EXPECT(!strcmp(first(KV_BEAM_BEGIN, f), "W: guidance is on in this cache (pgv_kv_set_guidance(kv, 1, 0) turns it off)")); }
    { char m[64];                                                        // the caller's name and the verify tail are substituted
      KvFeatures f; f.penalty = 1.2f;
      char big[512];
      EXPECT(kv_refusal(KV_LOOKUP_RUN, 1, f, "pgv_llm_decode_lookup", "the plain arg-max", big, sizeof(big)));
      EXPECT(!strcmp(big, "pgv_llm_decode_lookup: a repetition penalty is set on this cache (pgv_kv_set_warpers); lookup steps verify the plain arg-max"));
      EXPECT(kv_refusal(KV_LOOKUP_RUN, 1, f, "pgv_llm_decode_lookup", "the plain arg-max", m, sizeof(m)) && strlen(m) == sizeof(m) - 1); }   // a short buffer truncates
    if (!bad) printf("OK %d\n", all);
    return bad;
}
"""
    cpp, exe, exe_san = tmp_path / "pick.cpp", tmp_path / "pick", tmp_path / "pick_san"
    cpp.write_text(prog)
    base = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", csrc]
    for header in ("pick_params.h", "kv_features.h"):                  # each header alone: no HIP header, nothing it forgot to include
        alone = tmp_path / (header + ".cpp")
        alone.write_text(f'#include "{header}"\nint main() {{ return 0; }}\n')
        subprocess.run([*base, "-fsyntax-only", str(alone)], check=True)
    base.append(str(cpp))
    subprocess.run([*base, "-o", str(exe)], check=True)
    exes = [exe]
    san = subprocess.run([*base, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe_san)], capture_output=True, text=True)
    if san.returncode == 0:
        exes.append(exe_san)
    else:
        assert "asan" in san.stderr or "ubsan" in san.stderr, san.stderr        # only a missing sanitizer runtime excuses the second build
        print("g++ has no sanitizer runtimes here: plain build only")
    for x in exes:
        r = subprocess.run([str(x)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr and r.stdout == "OK 21\n", (x, r.returncode, r.stdout, r.stderr[-2000:])
    # the header is what the library uses: llm.hip includes it, builds its key from the cache's snapshot alone, and holds no rule text of its own
    users = [f for f in sorted(os.listdir(csrc)) if '#include "kv_features.h"' in open(os.path.join(csrc, f)).read()]
    assert users == ["llm.hip"], users
    llm, table = open(os.path.join(csrc, "llm.hip")).read(), open(os.path.join(csrc, "kv_features.h")).read()
    for phrase in ("is on in this cache", "are set on this cache", "in flight"):
        assert phrase not in llm and phrase in table, phrase
    assert llm.count("decode_graph_key(") == 1 and "decode_graph_key(kv_features(kv), " in llm
    assert llm.count("kv_features(kv)") == 2 and llm.count("static KvFeatures kv_features(const pgv_kv* kv)") == 1      # the key and kv_allows
    for read in ("kv->ban.gen : 0", "kv->allow.gen : 0"):
        assert llm.count(read) == 1, read


def test_prefill_plan_row_maps_and_refusals(tmp_path):
    """csrc/prefill_plan.h, compiled on its own with g++ (it must need no HIP header), owns the int block of row maps a prefill uploads: (1) the
    section offsets and the total for (M, B, nscore), the same accessor over a mutable and a const base; (2) every section of the built block,
    element by element against arrays written out below by hand, for a plain call, one with a video run (a placeholder id beyond the vocabulary is
    accepted on a video row and kept in raw_ids), an appended one (positions, lengths and the attention FLOP count behind a cached prefix), a
    refill into slots, a scored one (-1 / -100 targets skipped; srows / stgts follow raw_ids) and the id-less form of pgv_prefill_attention;
    (3) every refusal of the loops prefill_impl had, with its message and class, the accepted neighbour of each bound next to it.  Where g++ has
    the sanitizer runtimes the same stand-alone program runs a second time under ASan + UBSan."""
    import shutil
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    csrc = os.path.join(ROOT, "video_llava_amd", "csrc")
    prog = r"""#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "prefill_plan.h"
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad = 1; } } while (0)
typedef std::initializer_list<int> L;
// section `off` of the block holds exactly `want` up to the next section `end`
static bool sec(const std::vector<int>& meta, size_t off, size_t end, L want) {
    if (end - off != want.size() || end > meta.size()) return false;
    size_t i = off;
    for (int v : want) if (meta[i++] != v) return false;
    return true;
}
static const int lens35[2] = {3, 5}, ids8[8] = {5, 6, 7, 8, 9, 10, 11, 12};
static PrefillRows rows35(const int* ids) {
    PrefillRows r;
    r.who = "who"; r.ids = ids; r.seq_lens = lens35; r.B = 2; r.vocab = 20; r.max_seq = 16; r.hidden = 4;
    return r;
}
static std::vector<int> meta;
static PrefillPlan plan;
static char err[256];
static bool ok(const PrefillRows& r) { err[0] = 0; return prefill_plan_build(r, meta, plan, err, sizeof(err)) == PLAN_OK && !err[0]; }
static bool refused(const PrefillRows& r, const char* msg) {
    err[0] = 0;
    const bool hit = prefill_plan_build(r, meta, plan, err, sizeof(err)) == PLAN_EINVAL && !strncmp(err, "who: ", 5) && strstr(err, msg);
    if (!hit) printf("got \"%s\", want \"%s\"\n", err, msg);
    return hit;
}
int main() {
    {   // layout: row_src | row_b | row_pos | cu | last | lens | offs | slots | raw_ids | srows | stgts
        const PrefillLayout lo(8, 2, 5);
        EXPECT(lo.row_src == 0 && lo.row_b == 8 && lo.row_pos == 16 && lo.cu == 24 && lo.last == 27 && lo.lens == 29 && lo.offs == 31 && lo.slots == 33);
        EXPECT(lo.raw_ids == 35 && lo.srows == 43 && lo.stgts == 48 && lo.total == 53);
        int base[53];
        const PrefillMaps<int> a = lo.maps(base);
        const PrefillMaps<const int> c = lo.maps((const int*)base);
        EXPECT(a.row_src == base && a.row_b == base + 8 && a.row_pos == base + 16 && a.cu == base + 24 && a.last == base + 27 && a.lens == base + 29);
        EXPECT(a.offs == base + 31 && a.slots == base + 33 && a.raw_ids == base + 35 && a.srows == base + 43 && a.stgts == base + 48);
        EXPECT(c.row_src == a.row_src && c.row_b == a.row_b && c.row_pos == a.row_pos && c.cu == a.cu && c.last == a.last && c.lens == a.lens);
        EXPECT(c.offs == a.offs && c.slots == a.slots && c.raw_ids == a.raw_ids && c.srows == a.srows && c.stgts == a.stgts);
        EXPECT(PrefillLayout(0, 0, 0).total == 1 && PrefillLayout(1, 1, 0).total == 10);
    }
    {   // plain
        EXPECT(ok(rows35(ids8)));
        const PrefillLayout& lo = plan.lo;
        EXPECT(plan.M == 8 && plan.max_len == 5 && plan.nscore == 0 && lo.total == 4 * 8 + 5 * 2 + 1 && meta.size() == 43);
        EXPECT(sec(meta, lo.row_src, lo.row_b, {5, 6, 7, 8, 9, 10, 11, 12}));
        EXPECT(sec(meta, lo.row_b, lo.row_pos, {0, 0, 0, 1, 1, 1, 1, 1}));
        EXPECT(sec(meta, lo.row_pos, lo.cu, {0, 1, 2, 0, 1, 2, 3, 4}));
        EXPECT(sec(meta, lo.cu, lo.last, {0, 3, 8}) && sec(meta, lo.last, lo.lens, {2, 7}) && sec(meta, lo.lens, lo.offs, {3, 5}));
        EXPECT(sec(meta, lo.offs, lo.slots, {0, 0}) && sec(meta, lo.slots, lo.raw_ids, {0, 1}));
        EXPECT(sec(meta, lo.raw_ids, lo.srows, {5, 6, 7, 8, 9, 10, 11, 12}) && sec(meta, lo.srows, lo.stgts, {}) && sec(meta, lo.stgts, lo.total, {}));
        EXPECT(plan.attn_flops == 2.0 * 3 * 3 * 4 + 2.0 * 5 * 5 * 4);
    }
    {   // video: sequence 0 has none, sequence 1 its 2 rows behind row 1; the placeholder id 25 is beyond the vocabulary of 20
        const int ids[8] = {5, 6, 7, 8, 9, 25, 19, 12}, vp[2] = {-1, 1};
        PrefillRows r = rows35(ids);
        r.vid_pos = vp; r.Vt = 2;
        EXPECT(ok(r));
        const PrefillLayout& lo = plan.lo;
        EXPECT(lo.total == 43 && sec(meta, lo.row_src, lo.row_b, {5, 6, 7, 8, 9, -3, -4, 12}));
        EXPECT(sec(meta, lo.raw_ids, lo.srows, {5, 6, 7, 8, 9, 25, 19, 12}));
        EXPECT(sec(meta, lo.row_b, lo.row_pos, {0, 0, 0, 1, 1, 1, 1, 1}) && sec(meta, lo.row_pos, lo.cu, {0, 1, 2, 0, 1, 2, 3, 4}));
        const int late[2] = {-1, 2};            // 2 + 2 + 1 rows do not fit in front of the last of 5
        r.vid_pos = late;
        EXPECT(refused(r, "video run of sequence 1 (start 2, 2 rows) overruns its 5 tokens"));
        const int vp0[2] = {0, -1};             // the same id on a row outside the run
        r.vid_pos = vp0; r.Vt = 1;
        EXPECT(refused(r, "token id 25 at row 5 outside the vocabulary (20)"));
    }
    {   // append behind prefixes of 4 and 0 positions
        const int start[2] = {4, 0};
        PrefillRows r = rows35(ids8);
        r.start = start;
        EXPECT(ok(r));
        const PrefillLayout& lo = plan.lo;
        EXPECT(sec(meta, lo.row_pos, lo.cu, {4, 5, 6, 0, 1, 2, 3, 4}) && sec(meta, lo.lens, lo.offs, {7, 5}) && sec(meta, lo.offs, lo.slots, {4, 0}));
        EXPECT(sec(meta, lo.cu, lo.last, {0, 3, 8}) && sec(meta, lo.last, lo.lens, {2, 7}) && sec(meta, lo.row_b, lo.row_pos, {0, 0, 0, 1, 1, 1, 1, 1}));
        EXPECT(plan.attn_flops == 2.0 * 3 * (3 + 2 * 4) * 4 + 2.0 * 5 * 5 * 4 && plan.attn_flops == 464.0);
        const int full[2] = {13, 11}, over[2] = {14, 0};
        r.start = full;
        EXPECT(ok(r) && sec(meta, plan.lo.lens, plan.lo.offs, {16, 16}));
        r.start = over;
        EXPECT(refused(r, "sequence 0 has 14 + 3 tokens (cache holds 16)"));
        const int neg[2] = {0, -1};
        r.start = neg;
        EXPECT(refused(r, "sequence 1 has -1 + 5 tokens (cache holds 16)"));
    }
    {   // slots of a live group of 3
        const int slots[2] = {2, 0}, out[2] = {3, 0}, below[2] = {0, -1}, twice[2] = {1, 1};
        PrefillRows r = rows35(ids8);
        r.slots = slots; r.active = 3;
        EXPECT(ok(r));
        const PrefillLayout& lo = plan.lo;
        EXPECT(sec(meta, lo.row_b, lo.row_pos, {2, 2, 2, 0, 0, 0, 0, 0}) && sec(meta, lo.slots, lo.raw_ids, {2, 0}) && sec(meta, lo.cu, lo.last, {0, 3, 8}));
        r.slots = out;
        EXPECT(refused(r, "slot 3 outside the 3 of the live group"));
        r.slots = below;
        EXPECT(refused(r, "slot -1 outside the 3 of the live group"));
        r.slots = twice;
        EXPECT(refused(r, "slot 1 listed twice"));
    }
    {   // score: five rows have a target
        const int tg[8] = {-1, 6, 7, -1, -100, 10, 19, 0};
        PrefillRows r = rows35(ids8);
        r.targets = tg;
        EXPECT(ok(r));
        const PrefillLayout& lo = plan.lo;
        EXPECT(plan.nscore == 5 && lo.total == 4 * 8 + 5 * 2 + 1 + 2 * 5 && lo.srows == lo.raw_ids + 8 && lo.stgts == lo.srows + 5 && lo.total == lo.stgts + 5);
        EXPECT(sec(meta, lo.srows, lo.stgts, {1, 2, 5, 6, 7}) && sec(meta, lo.stgts, lo.total, {6, 7, 10, 19, 0}));
        EXPECT(sec(meta, lo.raw_ids, lo.srows, {5, 6, 7, 8, 9, 10, 11, 12}) && sec(meta, lo.row_src, lo.row_b, {5, 6, 7, 8, 9, 10, 11, 12}));
        const int tg_out[8] = {-1, 6, 20, -1, -100, 10, 19, 0};
        r.targets = tg_out;
        EXPECT(refused(r, "target 20 of row 2 outside the vocabulary (20)"));
    }
    {   // lengths and token ids
        const int zero[2] = {3, 0};
        PrefillRows r = rows35(ids8);
        r.seq_lens = zero;
        EXPECT(refused(r, "sequence 1 has 0 + 0 tokens (cache holds 16)"));
        const int minus[8] = {-1, 6, 7, 8, 9, 10, 11, 12}, at_vocab[8] = {5, 6, 7, 8, 9, 10, 11, 20}, top[8] = {0, 6, 7, 8, 9, 10, 11, 19};
        EXPECT(refused(rows35(minus), "token id -1 at row 0 outside the vocabulary (20)"));
        EXPECT(refused(rows35(at_vocab), "token id 20 at row 7 outside the vocabulary (20)"));
        EXPECT(ok(rows35(top)));
        char tiny[8];                           // a short message buffer is not overrun
        EXPECT(prefill_plan_build(rows35(minus), meta, plan, tiny, sizeof(tiny)) == PLAN_EINVAL && !strcmp(tiny, "who: to"));
    }
    {   // the id-less form of pgv_prefill_attention
        const int lens[2] = {2, 1}, start[2] = {3, 0};
        PrefillRows r;
        r.who = "who"; r.seq_lens = lens; r.B = 2; r.start = start; r.max_seq = 8; r.hidden = 4;
        EXPECT(ok(r));
        const PrefillLayout& lo = plan.lo;
        EXPECT(plan.M == 3 && plan.max_len == 2 && plan.nscore == 0 && lo.total == 4 * 3 + 5 * 2 + 1);
        EXPECT(sec(meta, lo.row_b, lo.row_pos, {0, 0, 1}) && sec(meta, lo.row_pos, lo.cu, {3, 4, 0}) && sec(meta, lo.cu, lo.last, {0, 2, 3}));
        EXPECT(sec(meta, lo.offs, lo.slots, {3, 0}) && sec(meta, lo.lens, lo.offs, {5, 1}) && sec(meta, lo.last, lo.lens, {1, 2}));
        EXPECT(sec(meta, lo.row_src, lo.row_b, {0, 0, 0}) && sec(meta, lo.raw_ids, lo.srows, {0, 0, 0}));
        EXPECT(plan.attn_flops == 2.0 * 2 * (2 + 2 * 3) * 4 + 2.0 * 1 * 1 * 4);
    }
    if (!bad) printf("OK\n");
    return bad;
}
"""
    cpp, exe, exe_san = tmp_path / "plan.cpp", tmp_path / "plan", tmp_path / "plan_san"
    cpp.write_text(prog)
    base = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", csrc, str(cpp)]
    subprocess.run([*base, "-o", str(exe)], check=True)
    exes = [exe]
    san = subprocess.run([*base, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe_san)], capture_output=True, text=True)
    if san.returncode == 0:
        exes.append(exe_san)
    else:
        assert "asan" in san.stderr or "ubsan" in san.stderr, san.stderr        # only a missing sanitizer runtime excuses the second build
        print("g++ has no sanitizer runtimes here: plain build only")
    for x in exes:
        r = subprocess.run([str(x)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr and r.stdout == "OK\n", (x, r.returncode, r.stdout, r.stderr[-2000:])
    # nothing but llm.hip builds row maps
    users = [f for f in sorted(os.listdir(csrc)) if '#include "prefill_plan.h"' in open(os.path.join(csrc, f)).read()]
    assert users == ["llm.hip"], users


def test_gemv_plan_shapes_totality_sizes_and_refusals(tmp_path):
    """csrc/gemv_plan.h, compiled on its own with g++ (it must need no HIP header), owns the launch plan of a decode GEMV: (1) the launch shape
    (tl, ct, x2, k8, nwb) and the streamed weight format of the five matrices of the 7B and 13B decoders on 256 CUs at B = 1, 8, 9, 16, 17, 32,
    33, 64, 16-bit and fp8, against literals written out below (what choose_gemv returned before it moved here), and no 8-phase choice anywhere
    without its scratch; (2) totality: over every mode, both formats, B 1..64, 1..2600 row blocks, six K, four CU counts, scratch on and off,
    every choice has an instantiation by the predicates the kernel list is expanded with, a GV_STORE16 tl divides the row-block count, an 8-phase
    choice implies mode 5, scratch and whole row groups (and fp8 at one column tile, which pgv_llm_weight_stream_bytes leans on), x2 implies
    B <= 8, one tile and tl < 6, and ct is gemv_col_tiles(B); (3) the 8-phase scratch and LDS sizes; (4) every refusal of the two check
    functions with its message, the accepted neighbour of each bound next to it.  Where g++ has the sanitizer runtimes the same stand-alone
    program runs a second time under ASan + UBSan."""
    import shutil
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    csrc = os.path.join(ROOT, "video_llava_amd", "csrc")
    prog = r"""#include <cstdio>
#include <cstring>
#include "gemv_plan.h"
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad = 1; } } while (0)
static GemvPlan plan;
static char err[512];
static bool ok(const GemvCall& c) { err[0] = 0; const bool r = gemv_plan_build(c, plan, err, sizeof(err)) == GEMV_PLAN_OK && !err[0]; if (!r) printf("refused: \"%s\"\n", err); return r; }
static bool refused(const GemvCall& c, const char* msg) {
    err[0] = 0;
    const bool hit = gemv_plan_build(c, plan, err, sizeof(err)) == GEMV_PLAN_EINVAL && !strcmp(err, msg);
    if (!hit) printf("got \"%s\", want \"%s\"\n", err, msg);
    return hit;
}
static bool dok(const GemvDescShape& d) { err[0] = 0; const bool r = gemv_check_desc(d, err, sizeof(err)) == GEMV_PLAN_OK && !err[0]; if (!r) printf("refused: \"%s\"\n", err); return r; }
static bool drefused(const GemvDescShape& d, const char* msg) {
    err[0] = 0;
    const bool hit = gemv_check_desc(d, err, sizeof(err)) == GEMV_PLAN_EINVAL && !strcmp(err, msg);
    if (!hit) printf("got \"%s\", want \"%s\"\n", err, msg);
    return hit;
}
// a decode step's call of one matrix on 256 CUs
static GemvCall call(int mode, int N, int K, int B, bool w8, bool scratch, bool w12) {
    GemvCall c;
    c.mode = mode; c.N = N; c.K = K; c.B = B; c.w8 = w8; c.bf16 = true; c.W = true; c.w12 = w12; c.rows12 = (N + 15) / 16 * 16;
    c.norm = true; c.ssq_ts = 8192; c.amax_ts = 32064; c.nparts_in = mode == GV_RESIDNORM ? 0 : 256;
    c.gamma = c.xg = c.ssq_out = mode == GV_RESIDNORM; c.k8_part = scratch && mode == GV_RESIDNORM; c.x_blocked = true;
    return c;
}
static bool shape_is(int tl, int ct, int x2, int k8, int nwb, int wf) {
    const bool r = plan.tl == tl && plan.ct == ct && plan.x2 == x2 && plan.k8 == k8 && plan.nwb == nwb && plan.wf == wf;
    if (!r) printf("shape (%d %d %d %d %d %d), want (%d %d %d %d %d %d)\n", plan.tl, plan.ct, plan.x2, plan.k8, plan.nwb, plan.wf, tl, ct, x2, k8, nwb, wf);
    return r;
}
int main() {
    {   // (1) the launch shapes of the 7B and 13B decoders
        const int Bs[8] = {1, 8, 9, 16, 17, 32, 33, 64};
        for (int big = 0; big < 2; ++big) for (int w8 = 0; w8 < 2; ++w8) for (int w12 = 0; w12 < 2 - w8; ++w12) for (int bi = 0; bi < 8; ++bi) for (int scratch = 0; scratch < 2; ++scratch) {
            const int H = big ? 5120 : 4096, I = big ? 13824 : 11008, B = Bs[bi];
            const int ct = B <= 16 ? 1 : (B <= 32 ? 2 : 4), x2 = B <= 8;
            const int wf = w8 ? WF_FP8 : WF_16, wf1 = (w12 && ct == 1) ? WF_12 : wf;        // wf1: the format of a launch that is not 8-phase
            EXPECT(ok(call(GV_STORE16, 3 * H, H, B, w8, scratch, w12)) && shape_is(big ? 4 : 3, ct, x2, 0, 0, wf1) && plan.units == 3 * H / 16 && plan.grid * plan.tl == plan.units);
            EXPECT(ok(call(GV_SWIGLU, 2 * I, H, B, w8, scratch, w12)) && shape_is(B <= 16 ? 2 : (big ? 8 : 6), ct, x2, 0, 0, wf1) && plan.units == I / 16);
            EXPECT(plan.grid == (B <= 16 ? I / 16 : (big ? 216 : 230)));
            EXPECT(ok(call(GV_F32, 2001 * 16 - 5, H, B, w8, scratch, w12)) && shape_is(B <= 8 ? 1 : 8, ct, x2, 0, 0, wf1) && plan.units == 2001 && plan.grid == (B <= 8 ? 2001 : 251));
            EXPECT(plan.xblk == (B > 8) && !plan.xgblk);
            const bool o8 = scratch && (B >= 33 || (big && w8 && B <= 16)), d8 = scratch && (B >= 17 || (big && w8));
            const int nwb = big ? 10 : 8;
            EXPECT(ok(call(GV_RESIDNORM, H, H, B, w8, scratch, w12)) && shape_is(1, ct, x2 && !o8, o8, o8 ? nwb : 0, o8 ? wf : wf1) && plan.units == H / 16 && plan.grid == H / 16);
            EXPECT(ok(call(GV_RESIDNORM, H, I, B, w8, scratch, w12)) && shape_is(1, ct, x2 && !d8, d8, d8 ? nwb : 0, d8 ? wf : wf1));
            EXPECT(plan.xgblk == (B > 8) && !plan.xblk);
            // the one predicate, also where a 12-bit copy next to fp8 weights is refused as an argument
            GemvChoice c; c.ct = ct;
            EXPECT(gemv_weight_format(w8, true, c) == (w8 ? WF_FP8 : (ct == 1 ? WF_12 : WF_16)) && gemv_weight_format(w8, false, c) == wf);
            c.k8 = true;
            EXPECT(gemv_weight_format(w8, true, c) == wf);
        }
    }
    {   // (2) totality
        const int modes[5] = {GV_STORE16, GV_RESID, GV_SWIGLU, GV_F32, GV_RESIDNORM}, Ks[6] = {32, 64, 4096, 5120, 11008, 13824}, cus[4] = {1, 64, 256, 304};
        long long points = 0, holes = 0;
        for (int mi = 0; mi < 5; ++mi) for (int w8 = 0; w8 < 2; ++w8) for (int B = 1; B <= 64; ++B) for (int ki = 0; ki < 6; ++ki) for (int ci = 0; ci < 4; ++ci)
            for (int scratch = 0; scratch < 2; ++scratch) for (int units = 1; units <= 2600; ++units, ++points) {
                const int mode = modes[mi];
                const GemvChoice c = choose_gemv(mode, w8, B, units, Ks[ki], cus[ci], scratch);
                bool good = c.ct == gemv_col_tiles(B);
                if (c.k8) good = good && mode == GV_RESIDNORM && scratch && units % c.nwb == 0 && gemv_has_k8_kernel(c.ct, c.nwb) && (c.ct > 1 || w8);
                else {
                    const bool x2 = c.x2 && c.ct == 1;
                    good = good && gemv_has_kernel(mode, c.tl, c.ct, w8 ? WF_FP8 : WF_16, x2) && (w8 || c.ct > 1 || gemv_has_kernel(mode, c.tl, c.ct, WF_12, x2));
                }
                if (mode == GV_STORE16) good = good && units % c.tl == 0;
                if (c.x2) good = good && B <= 8 && c.ct == 1 && c.tl < 6;
                if (!good && holes++ < 10) printf("mode %d w8 %d B %d units %d K %d CUs %d scratch %d -> tl %d ct %d x2 %d k8 %d nwb %d\n", mode, w8, B, units, Ks[ki], cus[ci], scratch, c.tl, c.ct, c.x2, c.k8, c.nwb);
            }
        EXPECT(holes == 0 && points == 5LL * 2 * 64 * 6 * 4 * 2 * 2600);
        // the predicates themselves: what the list holds and what it forbids
        EXPECT(gemv_has_kernel(GV_F32, 8, 1, WF_12, false) && !gemv_has_kernel(GV_F32, 8, 1, WF_12, true) && !gemv_has_kernel(GV_F32, 8, 1, WF_16, true));
        EXPECT(gemv_has_kernel(GV_STORE16, 4, 1, WF_12, true) && !gemv_has_kernel(GV_STORE16, 4, 2, WF_12, false) && !gemv_has_kernel(GV_STORE16, 4, 2, WF_FP8, true));
        EXPECT(gemv_has_kernel(GV_SWIGLU, 6, 4, WF_FP8, false) && !gemv_has_kernel(GV_SWIGLU, 6, 1, WF_16, false) && !gemv_has_kernel(GV_STORE16, 2, 1, WF_16, false));
        EXPECT(!gemv_has_kernel(4, 1, 1, WF_16, false) && gemv_has_k8_kernel(4, 10) && !gemv_has_k8_kernel(3, 8) && !gemv_has_k8_kernel(1, 9));
        int rows = 0, k8s = 0;
#define COUNT_ROW(M, TL, CT) ++rows;
#define COUNT_K8(CT, NWB) ++k8s;
        GEMV_KERNELS(COUNT_ROW, COUNT_K8)
        EXPECT(rows == 30 && k8s == 6);
        EXPECT(gemv_col_tiles(1) == 1 && gemv_col_tiles(16) == 1 && gemv_col_tiles(17) == 2 && gemv_col_tiles(32) == 2 && gemv_col_tiles(33) == 4 && gemv_col_tiles(64) == 4);
        EXPECT(gemv_xblk_tiles(1) == 0 && gemv_xblk_tiles(8) == 0 && gemv_xblk_tiles(9) == 1 && gemv_xblk_tiles(16) == 1 && gemv_xblk_tiles(17) == 2 && gemv_xblk_tiles(33) == 4);
        EXPECT(gemv_grid(GV_SWIGLU, 25, 8) == 7 && gemv_grid(GV_SWIGLU, 24, 8) == 6 && gemv_grid(GV_F32, 2001, 8) == 251 && gemv_grid(GV_STORE16, 768, 3) == 256);
        EXPECT(kGemvSsqChunks == 1536);
    }
    {   // (3) sizes
        for (int H = 4096; H <= 5120; H += 1024) for (int ct = 1; ct <= 4; ct *= 2) {
            const size_t nrb = (size_t)H / 16;
            EXPECT(gemv_k8_part_bytes(H / 16, ct) == nrb * 8 * ct * 64 * 16 && gemv_k8_part_bytes(H / 16, ct) == nrb * 8 * ct * 1024);
        }
        for (int K = 32; K <= 13824; K += 32) for (int ct = 1; ct <= 4; ct *= 2) {
            const unsigned lds = gemv_k8_lds_bytes(K, ct), group = ct * 16 * 128;
            EXPECT(lds >= group && lds <= 98304 && lds % group == 0);
        }
        EXPECT(gemv_k8_lds_bytes(4096, 1) == 8 * 2048 && gemv_k8_lds_bytes(13824, 4) == 98304 && gemv_k8_lds_bytes(13824, 2) == 98304 && gemv_k8_lds_bytes(5120, 4) == 10 * 8192 && gemv_k8_lds_bytes(11008, 4) == 12 * 8192);
    }
    {   // (4a) the refusals of a launch
        GemvCall c = call(GV_STORE16, 64, 64, 1, false, false, false);
        EXPECT(ok(c));
        c.B = 0;  EXPECT(refused(c, "gemv: batch 0 outside [1,64]"));
        c.B = 65; EXPECT(refused(c, "gemv: batch 65 outside [1,64]"));
        c.B = 64; EXPECT(ok(c));
        c.K = 48; EXPECT(refused(c, "gemv: K=48 must be a multiple of 32"));
        c.K = 96; EXPECT(ok(c));
        c.w8 = true; EXPECT(refused(c, "gemv fp8: K=96 must be a multiple of 64"));
        c.K = 128; EXPECT(ok(c) && plan.wf == WF_FP8);
        c = call(4, 64, 64, 1, false, false, false); EXPECT(refused(c, "gemv: bad mode 4"));
        c.mode = 6; EXPECT(refused(c, "gemv: bad mode 6"));
        c.mode = -1; EXPECT(refused(c, "gemv: bad mode -1"));
        // the tile strides of the side arrays
        c = call(GV_F32, 64, 64, 17, false, false, false);
        c.amax_val = true; EXPECT(ok(c));
        c.amax_ts = 0; EXPECT(refused(c, "gemv: batches beyond 16 need the tile strides of the side arrays"));
        c.amax_val = false; EXPECT(ok(c));
        c.ssq_ts = 0; EXPECT(refused(c, "gemv: batches beyond 16 need the tile strides of the side arrays"));
        c.B = 16; EXPECT(ok(c));
        c.B = 17; c.norm = false; EXPECT(ok(c) && !plan.xblk);
        // sum-of-squares partials
        c = call(GV_STORE16, 64, 64, 1, false, false, false);
        c.nparts_in = 384; EXPECT(ok(c));
        c.nparts_in = 385; EXPECT(refused(c, "gemv: 385 sum-of-squares partials exceed what a consumer workgroup loads (hidden <= 6144)"));
        // row counts
        c = call(GV_STORE16, 40, 64, 1, false, false, false); EXPECT(refused(c, "gemv: N=40 must be a multiple of 16"));
        c.mode = GV_RESID; EXPECT(refused(c, "gemv: N=40 must be a multiple of 16"));
        c.mode = GV_F32; EXPECT(ok(c) && plan.units == 3);
        c = call(GV_SWIGLU, 96, 64, 1, false, false, false); EXPECT(refused(c, "gemv swiglu: N=96 must be a multiple of 64"));
        c.N = 128; EXPECT(ok(c) && plan.units == 4 && plan.grid == 4 && plan.tl == 2);
        // the producer
        c = call(GV_RESIDNORM, 48, 64, 9, false, false, false); EXPECT(refused(c, "gemv: a blocked xg needs N in multiples of 32"));
        c.B = 8; EXPECT(ok(c) && !plan.xgblk);
        c.B = 9; c.x_blocked = false; EXPECT(ok(c) && !plan.xgblk);
        c.x_blocked = true; c.N = 64; EXPECT(ok(c) && plan.xgblk);
        c.gamma = false; EXPECT(refused(c, "gemv: the residual+norm producer needs gamma / xg / ssq_out"));
        c.gamma = true; c.xg = false; EXPECT(refused(c, "gemv: the residual+norm producer needs gamma / xg / ssq_out"));
        c.xg = true; c.ssq_out = false; EXPECT(refused(c, "gemv: the residual+norm producer needs gamma / xg / ssq_out"));
        c.ssq_out = true; c.norm = false; EXPECT(refused(c, "gemv: the residual+norm producer needs gamma / xg / ssq_out"));
        // the 12-bit copy
        c = call(GV_STORE16, 64, 64, 16, false, false, true); EXPECT(ok(c) && plan.wf == WF_12);
        c.w8 = true; EXPECT(refused(c, "gemv: bad 12-bit weight copy (64 rows for N = 64, K = 64)"));
        c.w8 = false; c.bf16 = false; EXPECT(refused(c, "gemv: bad 12-bit weight copy (64 rows for N = 64, K = 64)"));
        c.bf16 = true; c.K = 96; EXPECT(refused(c, "gemv: bad 12-bit weight copy (64 rows for N = 64, K = 96)"));
        c.K = 64; c.rows12 = 72; EXPECT(refused(c, "gemv: bad 12-bit weight copy (72 rows for N = 64, K = 64)"));
        c.rows12 = 48; EXPECT(refused(c, "gemv: bad 12-bit weight copy (48 rows for N = 64, K = 64)"));
        c.rows12 = 80; EXPECT(ok(c));
        c.mode = GV_F32; c.N = 70; EXPECT(ok(c));
        c.N = 81; EXPECT(refused(c, "gemv: bad 12-bit weight copy (80 rows for N = 81, K = 64)"));
        c = call(GV_STORE16, 64, 64, 16, false, false, true); c.W = false; EXPECT(ok(c) && plan.wf == WF_12);
        c.B = 17; EXPECT(refused(c, "gemv: 17 sequences need the 16-bit matrix (the 12-bit copy serves one column tile)"));
        c.W = true; EXPECT(ok(c) && plan.wf == WF_16);
        char tiny[8];                           // a short message buffer is not overrun
        c.B = 0; EXPECT(gemv_plan_build(c, plan, tiny, sizeof(tiny)) == GEMV_PLAN_EINVAL && !strcmp(tiny, "gemv: b"));
    }
    {   // (4b) the refusals of the test entry
        GemvDescShape g;
        g.mode = GV_STORE16; g.N = 64; g.K = 64; g.B = 33; g.ldx = 64; g.ldo = 64; g.W = g.x = g.out = true;
        GemvDescShape d = g;
        EXPECT(dok(d));
        d.W = false; EXPECT(drefused(d, "pgv_gemv_ex: null W / x / out"));
        d.W12 = true; EXPECT(dok(d));
        d = g; d.x = false; EXPECT(drefused(d, "pgv_gemv_ex: null W / x / out"));
        d = g; d.out = false; EXPECT(drefused(d, "pgv_gemv_ex: null W / x / out"));
        d = g; d.mode = 4; EXPECT(drefused(d, "pgv_gemv_ex: mode 4 is none of 0..3, 5"));
        d.mode = -1; EXPECT(drefused(d, "pgv_gemv_ex: mode -1 is none of 0..3, 5"));
        d.mode = 6; EXPECT(drefused(d, "pgv_gemv_ex: mode 6 is none of 0..3, 5"));
        d = g; d.B = 65; EXPECT(drefused(d, "pgv_gemv_ex: bad shape N = 64, K = 64, B = 65"));
        d.B = 0; EXPECT(drefused(d, "pgv_gemv_ex: bad shape N = 64, K = 64, B = 0"));
        d.B = 64; EXPECT(dok(d));
        d.B = 1; EXPECT(dok(d));
        d.N = 0; EXPECT(drefused(d, "pgv_gemv_ex: bad shape N = 0, K = 64, B = 1"));
        d = g; d.K = 31; d.ldx = 32; EXPECT(drefused(d, "pgv_gemv_ex: bad shape N = 64, K = 31, B = 33"));
        d.K = 32; EXPECT(dok(d));
        d = g; d.ldx = 56; EXPECT(drefused(d, "pgv_gemv_ex: ldx = 56 for K = 64 (row-major x: 16-byte rows)"));
        d.ldx = 68; EXPECT(drefused(d, "pgv_gemv_ex: ldx = 68 for K = 64 (row-major x: 16-byte rows)"));
        d.ldx = 72; EXPECT(dok(d));
        d.ldx = 0; d.x_blocked = true; EXPECT(dok(d));                 // a blocked consumer operand has no row stride
        d.B = 8; EXPECT(drefused(d, "pgv_gemv_ex: ldx = 0 for K = 64 (row-major x: 16-byte rows)"));      // up to 8 sequences x stays row-major
        d = g; d.ldo = 60; EXPECT(drefused(d, "pgv_gemv_ex: ldo = 60 for N = 64, mode 0"));
        d.ldo = 66; EXPECT(drefused(d, "pgv_gemv_ex: ldo = 66 for N = 64, mode 0"));
        d.mode = GV_F32; EXPECT(dok(d));
        d.mode = GV_SWIGLU; d.ldo = 32; EXPECT(dok(d));
        d.ldo = 28; EXPECT(drefused(d, "pgv_gemv_ex: ldo = 28 for N = 64, mode 2"));
        d = g; d.ssq_ts = -1; EXPECT(drefused(d, "pgv_gemv_ex: negative stride or count"));
        d = g; d.amax_ts = -1; EXPECT(drefused(d, "pgv_gemv_ex: negative stride or count"));
        d = g; d.nparts_in = -1; EXPECT(drefused(d, "pgv_gemv_ex: negative stride or count"));
        // the consumer side
        d = g; d.ssq_in = true; d.nparts_in = 4; d.hidden = 64; d.ssq_ts = 64; EXPECT(dok(d));
        d.ssq_ts = 63; EXPECT(drefused(d, "pgv_gemv_ex: ssq_in needs a consumer mode, nparts_in >= 1, hidden >= 1 and ssq_ts >= 16 nparts_in (mode 0, 4 parts, ssq_ts 63)"));
        d.ssq_ts = 64; d.hidden = 0; EXPECT(drefused(d, "pgv_gemv_ex: ssq_in needs a consumer mode, nparts_in >= 1, hidden >= 1 and ssq_ts >= 16 nparts_in (mode 0, 4 parts, ssq_ts 64)"));
        d.hidden = 1; d.nparts_in = 0; EXPECT(drefused(d, "pgv_gemv_ex: ssq_in needs a consumer mode, nparts_in >= 1, hidden >= 1 and ssq_ts >= 16 nparts_in (mode 0, 0 parts, ssq_ts 64)"));
        d.nparts_in = 1; EXPECT(dok(d));
        d.mode = GV_RESID; EXPECT(drefused(d, "pgv_gemv_ex: ssq_in needs a consumer mode, nparts_in >= 1, hidden >= 1 and ssq_ts >= 16 nparts_in (mode 1, 1 parts, ssq_ts 64)"));
        // the producer side
        GemvDescShape p = g;
        p.mode = GV_RESIDNORM; p.gamma = p.xg = p.ssq_out = true; p.ssq_ts = 64;
        d = p; EXPECT(dok(d));
        d.ssq_ts = 63; EXPECT(drefused(d, "pgv_gemv_ex: a producer needs gamma, xg, ssq_out and ssq_ts >= N (63 < 64)"));
        d = p; d.gamma = false; EXPECT(drefused(d, "pgv_gemv_ex: a producer needs gamma, xg, ssq_out and ssq_ts >= N (64 < 64)"));
        d = p; d.xg = false; EXPECT(drefused(d, "pgv_gemv_ex: a producer needs gamma, xg, ssq_out and ssq_ts >= N (64 < 64)"));
        d = p; d.ssq_out = false; EXPECT(drefused(d, "pgv_gemv_ex: a producer needs gamma, xg, ssq_out and ssq_ts >= N (64 < 64)"));
        d = p; d.gamma = d.xg = d.ssq_out = false; EXPECT(drefused(d, "pgv_gemv_ex: gamma / xg / ssq_out belong to mode 5, and mode 5 needs all three"));
        d = g; d.gamma = true; EXPECT(drefused(d, "pgv_gemv_ex: gamma / xg / ssq_out belong to mode 5, and mode 5 needs all three"));
        d = p; d.x_blocked = true; d.ldx = 0; EXPECT(drefused(d, "pgv_gemv_ex: ldx = 0 for K = 64 (row-major x: 16-byte rows)"));       // a producer reads x row-major
        d = p; d.k8_part = true; d.k8_part_bytes = 4 * 8 * 4 * 1024; EXPECT(dok(d));
        d.k8_part_bytes -= 1; EXPECT(drefused(d, "pgv_gemv_ex: k8_part belongs to mode 5 and holds (N / 16) * 8 * ct * 1024 = 131072 bytes (131071 given)"));
        d.B = 32; EXPECT(dok(d));                                       // two column tiles: half the scratch
        d = g; d.k8_part = true; d.k8_part_bytes = 1 << 20; EXPECT(drefused(d, "pgv_gemv_ex: k8_part belongs to mode 5 and holds (N / 16) * 8 * ct * 1024 = 131072 bytes (1048576 given)"));
        // the arg-max candidates
        GemvDescShape h = g;
        h.mode = GV_F32; h.N = 70; h.ldo = 70; h.amax_val = h.amax_idx = true; h.amax_ts = 80;
        d = h; EXPECT(dok(d));
        d.amax_ts = 79; EXPECT(drefused(d, "pgv_gemv_ex: the candidates need mode 3, both arrays and amax_ts >= 16 ceil(N / 16) (79 < 80)"));
        d = h; d.amax_idx = false; EXPECT(drefused(d, "pgv_gemv_ex: the candidates need mode 3, both arrays and amax_ts >= 16 ceil(N / 16) (80 < 80)"));
        d = h; d.amax_val = false; EXPECT(drefused(d, "pgv_gemv_ex: the candidates need mode 3, both arrays and amax_ts >= 16 ceil(N / 16) (80 < 80)"));
        d = g; d.amax_val = d.amax_idx = true; d.amax_ts = 64; EXPECT(drefused(d, "pgv_gemv_ex: the candidates need mode 3, both arrays and amax_ts >= 16 ceil(N / 16) (64 < 64)"));
    }
    if (!bad) printf("OK\n");
    return bad;
}
"""
    cpp, exe, exe_san = tmp_path / "gemv_plan.cpp", tmp_path / "gemv_plan", tmp_path / "gemv_plan_san"
    cpp.write_text(prog)
    base = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", csrc, str(cpp)]
    subprocess.run([*base, "-o", str(exe)], check=True)
    exes = [exe]
    san = subprocess.run([*base, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe_san)], capture_output=True, text=True)
    if san.returncode == 0:
        exes.append(exe_san)
    else:
        assert "asan" in san.stderr or "ubsan" in san.stderr, san.stderr        # only a missing sanitizer runtime excuses the second build
        print("g++ has no sanitizer runtimes here: plain build only")
    for x in exes:
        r = subprocess.run([str(x)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr and r.stdout == "OK\n", (x, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    # the column-tile rule is written once
    tiles = [f for f in sorted(os.listdir(csrc)) if "<= 32 ? 2 : 4" in open(os.path.join(csrc, f)).read()]
    assert tiles == ["gemv_plan.h"], tiles


# --------------------------------------------------------------------------------------------------
# offline feature extraction (scripts/save_spatio_temporal_clip_features.py) and the QA runner: host logic
# --------------------------------------------------------------------------------------------------
def test_extraction_cli_and_numpy_twin(tmp_path, golden_dir):
    from video_llava_amd import feature_extraction as fx
    a = fx.parse_args(["--llava", "1.5", "--video_dir_path", "v", "--clip_feat_path", "o"])
    assert a.infer_batch == 32 and fx.LLAVA_VERSIONS[a.llava][1] == (336, 336)
    with pytest.raises(SystemExit):
        fx.parse_args(["--llava", "2.0", "--video_dir_path", "v", "--clip_feat_path", "o"])
    # numpy twin == the golden produced by the reference's own function
    g = np.load(os.path.join(golden_dir, "pool.npz"))                      # outputs of the reference script's own function
    for name, (T, P) in {"t8_p16": (8, 16), "t100_p16": (100, 16), "t3_p4": (3, 4)}.items():
        rng = np.random.default_rng(int(g[name + "_seed"]))
        f16 = (rng.standard_normal((T, P, 1024), dtype=np.float32) * 1.5).astype(np.float16)
        assert np.array_equal(fx.get_spatio_temporal_features(f16), g[name + "_numpy"])
    x = np.random.default_rng(0).standard_normal((7, 16, 1024)).astype(np.float16)
    y = fx.get_spatio_temporal_features(x)
    assert y.dtype == np.float16 and y.shape == (116, 1024) and not y[7:100].any()
    assert np.array_equal(y[:7], np.mean(x, axis=1)) and np.array_equal(y[100:], np.mean(x, axis=0))


def test_extraction_load_video_npy_sampling_and_resize(tmp_path):
    from video_llava_amd import feature_extraction as fx
    rng = np.random.default_rng(1)
    clip = rng.integers(0, 256, (130, 60, 80, 3), dtype=np.uint8)
    p = tmp_path / "clip.npy"
    np.save(p, clip)
    out = fx.load_video(str(p), num_frm=100, shape=(224, 224))
    assert out.shape == (100, 224, 224, 3) and out.dtype == np.uint8
    idx = fx.get_seq_frames(130, 100)
    ref = torch.nn.functional.interpolate(torch.from_numpy(clip[idx]).permute(0, 3, 1, 2).float(), size=(224, 224))
    assert np.array_equal(out, ref.permute(0, 2, 3, 1).to(torch.uint8).numpy())          # the reference's nearest resize
    short = fx.load_video(str(p), num_frm=200, shape=(60, 80))
    assert short.shape == (130, 60, 80, 3) and np.array_equal(short, clip[fx.get_seq_frames(130, 130)])


def test_extraction_loop_skips_flushes_and_survives_failures(tmp_path):
    """run(): idempotent skip of existing .pkl, periodic flush, a broken clip is reported and skipped; pkl = np.float16 array."""
    import pickle
    from video_llava_amd import feature_extraction as fx
    vd, od = tmp_path / "videos", tmp_path / "feats"
    vd.mkdir(); od.mkdir()
    for name in ("a.npy", "b.npy", "c.npy", "bad.npy"):
        np.save(vd / name, np.zeros((3, 8, 8, 3), np.uint8))
    (vd / "bad.npy").write_bytes(b"not a numpy file")
    with open(od / "a.pkl", "wb") as f:
        pickle.dump(np.ones((2, 2), np.float16), f)
    calls = []
    orig = fx.extract_clip_features
    fx.extract_clip_features = lambda path, tower, size: (calls.append(os.path.basename(path)), np.load(path),
                                                          np.full((356, 1024), len(calls), np.float16))[2]
    try:
        logs = []
        args = fx.parse_args(["--llava", "1.1", "--video_dir_path", str(vd), "--clip_feat_path", str(od)])
        n = fx.run(args, vision_tower=object(), save_every=2, log=logs.append)
    finally:
        fx.extract_clip_features = orig
    assert n == 2 and calls == ["b.npy", "bad.npy", "c.npy"] and len(logs) == 1 and "bad.npy" in logs[0]
    assert pickle.load(open(od / "a.pkl", "rb")).shape == (2, 2)                        # untouched
    for key in ("b", "c"):
        arr = pickle.load(open(od / f"{key}.pkl", "rb"))
        assert isinstance(arr, np.ndarray) and arr.dtype == np.float16 and arr.shape == (356, 1024)
    assert not (od / "bad.pkl").exists()


def test_qa_runner_host_logic(tmp_path):
    from video_llava_amd.eval import run_inference_qa_activitynet as qa
    a = qa.parse_args(["--video_dir", "v", "--gt_file_question", "q", "--gt_file_answers", "a", "--output_dir", "o", "--output_name", "n",
                       "--model-name", "m", "--projection_path", "p"])
    assert a.conv_mode == "pg-video-llava" and not a.use_asr
    vd = tmp_path / "v"; vd.mkdir()
    (vd / "v_x1.mov").write_bytes(b""); (vd / "v_x1.mkv").write_bytes(b""); (vd / "v_y.npy").write_bytes(b"")
    assert qa.find_video(str(vd), "x1").endswith("v_x1.mov")           # reference order: mp4, avi, mov, mkv
    assert qa.find_video(str(vd), "y").endswith("v_y.npy") and qa.find_video(str(vd), "zz") is None
    q = [{"video_name": "x1", "question": "what?", "question_id": "x1_0"}, {"video_name": "zz", "question": "why?", "question_id": "zz_0"}]
    an = [{"answer": "yes"}, {"answer": "no"}]
    (tmp_path / "q.json").write_text(json.dumps(q)); (tmp_path / "a.json").write_text(json.dumps(an))
    samples = qa.load_samples(str(tmp_path / "q.json"), str(tmp_path / "a.json"))
    assert samples[1] == {"video_name": "zz", "question": "why?", "id": "zz_0", "answer": "no"}
    out = qa.build_output(samples, ["a dog", None])
    assert out == [{"id": "x1_0", "question": "what?", "answer": "yes", "pred": "a dog"}]


def test_sibling_runners_host_logic(tmp_path, monkeypatch):
    """Dataset adapters of the other eval runners (file naming, sample / output schema, drop-on-failure policy) with the sharded
    answering core stubbed out: reference video_chatgpt/eval/run_inference_{benchmark_general,benchmark_consistency,qa_msrvtt,qa_msvd,qa_tgif}.py."""
    from PIL import Image
    from video_llava_amd.eval import _sharded
    from video_llava_amd.eval import run_inference_benchmark_consistency as cons
    from video_llava_amd.eval import run_inference_benchmark_general as gen
    from video_llava_amd.eval import run_inference_qa_msrvtt as msrvtt
    from video_llava_amd.eval import run_inference_qa_msvd as msvd
    from video_llava_amd.eval import run_inference_qa_tgif as tgif

    class _IP:
        crop_size = {"height": 224, "width": 224}
    seen = {}

    def fake_setup(args, components=None):
        return 0, 1, (None, None, None, _IP(), 356)

    def fake_answer(args, tasks, components, load_frames, rank, world):
        seen["tasks"] = tasks
        return [None if t["path"] is None else f"ans:{t['question']}" for t in tasks]
    monkeypatch.setattr(_sharded, "setup", fake_setup)
    monkeypatch.setattr(_sharded, "answer_tasks", fake_answer)
    vd = tmp_path / "v"; vd.mkdir()
    out = tmp_path / "o"
    common = ["--video_dir", str(vd), "--output_dir", str(out), "--output_name", "r", "--model-name", "m", "--projection_path", "p"]

    # general + consistency: {video_name}.{mp4,avi,mov,mkv}; a sample with any failed question is dropped
    (vd / "a.avi").write_bytes(b""); (vd / "a.mkv").write_bytes(b"")
    gt = [{"video_name": "a", "Q": "q?", "A": "x", "Q1": "q1?", "Q2": "q2?"}, {"video_name": "missing", "Q": "z?", "A": "y", "Q1": "m1", "Q2": "m2"}]
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    r = gen.run_inference(gen.parse_args(common + ["--gt_file", str(tmp_path / "gt.json")]))
    assert seen["tasks"][0]["path"].endswith("a.avi") and seen["tasks"][1]["path"] is None
    assert r == [dict(gt[0], pred="ans:q?")] and json.load(open(out / "r.json")) == r
    r = cons.run_inference(cons.parse_args(common + ["--gt_file", str(tmp_path / "gt.json")]))
    assert [t["question"] for t in seen["tasks"]] == ["q1?", "q2?", "m1", "m2"]
    assert r == [dict(gt[0], pred1="ans:q1?", pred2="ans:q2?")]

    # MSRVTT: video{video_id}.mp4; MSVD: mapper lines "<name> vid<id>" and .avi
    (vd / "video7.mp4").write_bytes(b""); (vd / "clipA.avi").write_bytes(b"")
    gt2 = [{"video_id": 7, "question": "who?", "answer": "man", "id": 1}, {"video_id": 8, "question": "what?", "answer": "dog", "id": 2}]
    (tmp_path / "gt2.json").write_text(json.dumps(gt2))
    r = msrvtt.run_inference(msrvtt.parse_args(common + ["--gt_file", str(tmp_path / "gt2.json")]))
    assert seen["tasks"][0]["path"].endswith("video7.mp4") and r == [dict(gt2[0], pred="ans:who?")]
    (tmp_path / "map.txt").write_text("clipA vid7\nclipB vid8\n")
    a = msvd.parse_args(common + ["--gt_file", str(tmp_path / "gt2.json"), "--mapper", str(tmp_path / "map.txt")])
    assert msvd.load_mapper(a.mapper) == {7: "clipA", 8: "clipB"}
    r = msvd.eval_model(a)
    assert seen["tasks"][0]["path"].endswith("clipA.avi") and seen["tasks"][1]["path"] is None and r == [dict(gt2[0], pred="ans:who?")]

    # TGIF: tab-separated rows, {gif_name}.gif, 8 segment-centred frames at native size
    assert tgif.gif_frame_indices(40) == [2, 7, 12, 17, 22, 26, 31, 36] and tgif.gif_frame_indices(3) == [0, 0, 0, 1, 1, 1, 2, 2]
    frames = [Image.fromarray(np.full((20, 30, 3), 10 * i, dtype=np.uint8)) for i in range(12)]
    frames[0].save(vd / "g1.gif", save_all=True, append_images=frames[1:], duration=50, loop=0)
    imgs = tgif.load_video_from_gif(str(vd / "g1.gif"))
    assert len(imgs) == 8 and imgs[0].size == (30, 20) and imgs[0].mode == "RGB"
    (tmp_path / "t.tsv").write_text("gif_name\tquestion\tdescription\tanswer\ng1\thow many?\ta cat\t2\ng9\twhere?\ta dog\tpark\n")
    r = tgif.run_inference(tgif.parse_args(common + ["--gt_file", str(tmp_path / "t.tsv")]))
    assert r == [{"gif_name": "g1", "question": "how many?", "description": "a cat", "answer": "2", "pred": "ans:how many?"}]


def test_first_stop_length_equals_per_token_criterion_loop():
    """_sharded's batched path cuts an answer where the reference's per-token loop would have stopped: first_stop_length must agree with
    driving KeywordsStoppingCriteria token by token (HF calls it after every appended token; its first call only records the start)."""
    from video_llava_amd.model.utils import KeywordsStoppingCriteria, first_stop_length

    class Tok:
        def __call__(self, s):
            class R: pass
            r = R(); r.input_ids = [1] + [ord(c) for c in s]
            return r

        def batch_decode(self, ids, skip_special_tokens=True):
            return ["".join(chr(int(t)) for t in row if int(t) > 2) for row in ids]

    tok = Tok()
    rng = np.random.default_rng(0)
    prompt = torch.tensor([[1, 70, 71]])
    for trial in range(300):
        n = int(rng.integers(1, 30))
        toks = rng.choice([ord("a"), ord("b"), ord("#"), ord(" ")], n, p=[0.4, 0.3, 0.2, 0.1]).tolist()
        stop = ["###", "#", "ab#"][trial % 3]
        crit = KeywordsStoppingCriteria([stop], tok, prompt)
        want = None
        for i in range(1, n + 1):
            if crit(torch.tensor([prompt[0].tolist() + toks[:i]]), None):
                want = i
                break
        assert first_stop_length(toks, tok, [stop]) == want, (toks, stop)


def test_gather_answers_distinguishes_empty_from_failed():
    from video_llava_amd import parallel
    toks = torch.tensor([[5, 6, 7], [0, 0, 0], [0, 0, 0], [9, 0, 0]], dtype=torch.int32)
    lens = torch.tensor([4, 1, 0, 2], dtype=torch.int32)              # length + 1; 0 = failed
    out = parallel.gather_answers(toks, lens, 4, 0, 1, length_offset=1)
    assert out == [[5, 6, 7], [], None, [9]]


def test_nearest_resize_index_rule():
    """pgv_ingest_u8 implements F.interpolate(mode='nearest') as src = min(floorf(dst * (float)in / out), in - 1) per axis; pin that rule
    against torch itself on the shapes load_video meets (reference eval/model_utils.py:38-43), including up-sampling and odd ratios."""
    from video_llava_amd.feature_extraction import resize_nearest
    rng = np.random.default_rng(0)
    for (h, w, s) in ((360, 640, 224), (360, 640, 336), (20, 20, 56), (481, 853, 224), (224, 224, 224), (112, 112, 224), (1080, 1920, 336)):
        a = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        got = resize_nearest(a, (s, s))
        sh, sw = np.float32(h) / np.float32(s), np.float32(w) / np.float32(s)
        iy = np.minimum(np.floor(np.arange(s, dtype=np.float32) * sh).astype(np.int64), h - 1)
        ix = np.minimum(np.floor(np.arange(s, dtype=np.float32) * sw).astype(np.int64), w - 1)
        assert np.array_equal(got, a[:, iy][:, :, ix]), (h, w, s)


def test_frame_directory_front_end(tmp_path):
    """load_video without decord: a directory of image files (one frame per file) is sampled with get_seq_frames exactly like a decoded
    video (reference eval/model_utils.py:27-36) and resized with the reference's nearest rule."""
    from PIL import Image
    from video_llava_amd import feature_extraction as fx
    from video_llava_amd.eval.model_utils import get_seq_frames
    rng = np.random.default_rng(3)
    clip = rng.integers(0, 256, (130, 24, 40, 3), dtype=np.uint8)
    d = tmp_path / "clip_frames"
    d.mkdir()
    for i, f in enumerate(clip):
        Image.fromarray(f).save(d / f"{i:06d}.png")                      # lossless
    (d / "notes.txt").write_text("ignored")
    native = fx.sample_frames(str(d))
    assert native.shape == (100, 24, 40, 3) and np.array_equal(native, clip[get_seq_frames(130, 100)])
    got = fx.load_video(str(d), shape=(14, 14))
    assert got.shape == (100, 14, 14, 3) and np.array_equal(got, fx.resize_nearest(native, (14, 14)))
    nf = fx.load_video(str(d), shape=(14, 14), device_resize=True)
    assert isinstance(nf, fx.NativeFrames) and nf.shape == (14, 14) and np.array_equal(nf.resized(), got)
    with pytest.raises(ValueError, match="no image files"):
        (tmp_path / "empty").mkdir()
        fx.sample_frames(str(tmp_path / "empty"))


def test_animated_gif_front_end(tmp_path):
    """The TGIF runner's files are .gif: without decord they are decoded by Pillow.  Frames are sampled with get_seq_frames and must equal an
    independent frame-by-frame decode of the same file (GIF itself is lossy: compare against the file, not against the source array)."""
    from PIL import Image
    from video_llava_amd import feature_extraction as fx
    from video_llava_amd.eval import _sharded
    from video_llava_amd.eval.model_utils import get_seq_frames
    rng = np.random.default_rng(5)
    src = [Image.fromarray(rng.integers(0, 256, (20, 28, 3), dtype=np.uint8)) for _ in range(120)]
    path = tmp_path / "tumblr_x.gif"
    src[0].save(path, save_all=True, append_images=src[1:], duration=40, loop=0)
    with Image.open(path) as im:
        assert im.n_frames == 120
        ref = []
        for i in range(120):
            im.seek(i)
            ref.append(np.asarray(im.convert("RGB")))
    ref = np.stack(ref)
    got = fx.sample_frames(str(path))
    assert got.shape == (100, 20, 28, 3) and np.array_equal(got, ref[get_seq_frames(120, 100)])
    small = fx.load_video(str(path), shape=(14, 14))
    assert small.shape == (100, 14, 14, 3) and np.array_equal(small, fx.resize_nearest(got, (14, 14)))
    # runner-side discovery: the reference's extension order first, then the decord-free forms (array, directory of frames)
    assert _sharded.first_existing(str(tmp_path), "tumblr_x", [".gif", *_sharded.DECORD_FREE_FORMATS]) == str(path)
    (tmp_path / "clip7").mkdir()
    assert _sharded.first_existing(str(tmp_path), "clip7", [".mp4", *_sharded.DECORD_FREE_FORMATS]) == str(tmp_path / "clip7")
    assert _sharded.first_existing(str(tmp_path), "absent", [".mp4", *_sharded.DECORD_FREE_FORMATS]) is None


def test_load_video_decord_branches_match_reference(golden_dir, tmp_path):
    """The decord branches of both `load_video` mirrors (reference video_chatgpt/eval/model_utils.py:12-52 and
    scripts/save_spatio_temporal_clip_features.py:13-32) executed through a stub `decord.VideoReader` (decord is not installable offline):
    frame sampling -> get_batch -> nearest resize -> PIL / uint8 array, byte-identical to what the REFERENCE's own functions returned
    for the same stub clips (tests/golden/load_video.npz, written by oracle/gen_golden.py::gen_load_video)."""
    from oracle import decord_stub
    from video_llava_amd import feature_extraction as fx
    from video_llava_amd.eval import model_utils as mu
    g = np.load(os.path.join(golden_dir, "load_video.npz"))
    decord_stub.install()
    try:
        for i, (path, shape) in enumerate(zip(g["paths"].tolist(), g["shapes"].tolist())):
            want = g[f"case{i}"]
            shape = tuple(int(x) for x in shape)
            pil = mu.load_video(path, shape=shape)                           # eval/model_utils.py mirror: list of PIL images
            assert len(pil) == want.shape[0] and all(im.size == (shape[1], shape[0]) and im.mode == "RGB" for im in pil)
            assert np.array_equal(np.stack([np.asarray(im) for im in pil]), want), path
            arr = fx.load_video(path, shape=shape)                           # extraction-script mirror: uint8 [k, h, w, 3]
            assert arr.dtype == np.uint8 and np.array_equal(arr, want), path
            nat = fx.load_video(path, shape=shape, device_resize=True)       # runner front end: native frames, resized on the device later
            assert isinstance(nat, fx.NativeFrames) and np.array_equal(nat.resized(), want), path
        # a real file path goes through the same branch (the stub reads .npy): the eval runners' route for v_<name>.mp4
        clip = np.random.default_rng(9).integers(0, 256, (12, 9, 11, 3), dtype=np.uint8)
        p = tmp_path / "v_x.npy"
        np.save(p, clip)
        os.rename(p, tmp_path / "v_x.mp4")
        got = fx.sample_frames(str(tmp_path / "v_x.mp4"))
        assert np.array_equal(got, clip[mu.get_seq_frames(12, 12)])          # note: not the identity -- the reference's midpoint rule repeats frames
    finally:
        decord_stub.uninstall()
    with pytest.raises(RuntimeError, match="decord"):                        # without decord the error names what is missing
        mu.load_video("synth:3x4x4:1")


def test_run_sharded_prefetches_one_group_ahead():
    """parallel.run_sharded with a `prepare` half: the host half of group g + 1 runs on a background thread while the device half of group g
    runs; results and failure isolation are those of the serial loop (a prepare() exception fails only its own group)."""
    import threading
    import time
    from video_llava_amd import parallel
    events, lock = [], threading.Lock()

    def log(*e):
        with lock:
            events.append(e)

    def prepare(group):
        log("prep_start", tuple(group), threading.current_thread().name)
        time.sleep(0.05)
        if 4 in group:
            raise IOError("corrupt clip")
        log("prep_end", tuple(group))
        return {i: i * 10 for i in group}

    def infer(group, prepared):
        log("infer_start", tuple(group), threading.current_thread().name)
        time.sleep(0.1)
        toks = torch.tensor([[prepared[i], prepared[i] + 1, 0] for i in group], dtype=torch.int32)
        log("infer_end", tuple(group))
        return toks, [3 if i % 2 else 2 for i in group]           # length_offset 1: answers of 2 / 1 tokens

    ans = parallel.run_sharded(7, infer, 3, 0, 1, torch.device("cpu"), per_gpu_batch=2, length_offset=1, prepare=prepare)
    assert ans == [[0], [10, 11], [20], [30, 31], None, None, [60]]            # group (4, 5) failed in prepare; the rest is intact
    names = [e[0:2] for e in events]
    # overlap: the preparation of group 1 starts before the inference of group 0 ends, on another thread
    assert names.index(("prep_start", (2, 3))) < names.index(("infer_end", (0, 1)))
    main = threading.current_thread().name
    assert all(e[2] != main for e in events if e[0] == "prep_start") and all(e[2] == main for e in events if e[0] == "infer_start")
    # never more than one group ahead
    assert names.index(("prep_start", (4, 5))) > names.index(("infer_start", (0, 1)))


def test_first_stop_length_survives_a_non_monotone_decoder():
    """`keyword in decode(tokens[:n])` need not be monotone (byte-fallback pieces decode to U+FFFD until complete).  The search
    result is verified and a linear scan takes over: the answer must equal the reference's per-token loop for such a decoder too."""
    from video_llava_amd.model.utils import first_stop_length

    class Tok:
        """Token 9 followed by token 8 decodes to 'ab'; a trailing lone 9 decodes to U+FFFD (an incomplete byte-fallback piece); 5 erases the
        previous character only when it directly follows 8 at the END of the sequence (a decoder that strips a trailing piece)."""
        def __call__(self, s):
            class R: pass
            r = R(); r.input_ids = [1, 2, 3]; return r
        def batch_decode(self, rows, skip_special_tokens=True):
            out = []
            for row in rows:
                t = ""
                for i, x in enumerate(row):
                    if x == 9:
                        t += "a" if i + 1 < len(row) else "�"
                    elif x == 8:
                        t += "b"
                    elif x == 5:
                        t = t[:-1] if i + 1 == len(row) else t + "y"
                    else:
                        t += "x"
                out.append(t)
            return out

    def per_token(toks, kw):                       # the reference's loop: stop at the first n >= 2 whose decoded prefix holds the keyword
        tk = Tok()
        return next((n for n in range(2, len(toks) + 1) if kw in tk.batch_decode([toks[:n]])[0]), None)

    for toks in ([7, 9, 8, 7, 7], [7, 7, 9, 8, 5, 7, 7, 7], [7, 9, 8, 5], [7, 7, 7], [7, 9], [9, 8], [7, 7, 7, 9, 8, 9], [9, 8, 9, 8, 9]):
        assert first_stop_length(toks, Tok(), ["ab"]) == per_token(toks, "ab"), toks


def test_device_resize_upload_is_bounded(tmp_path):
    """the native-resolution upload of the runners (`device_resize=True`) is capped; above the cap the frames are resized on the host."""
    from video_llava_amd import feature_extraction as fx
    small = np.zeros((4, 48, 64, 3), np.uint8); np.save(tmp_path / "s.npy", small)
    assert isinstance(fx.load_video(str(tmp_path / "s.npy"), shape=(14, 14), device_resize=True), fx.NativeFrames)
    old = fx.DEVICE_RESIZE_MAX_BYTES
    fx.DEVICE_RESIZE_MAX_BYTES = small.nbytes - 1
    try:
        out = fx.load_video(str(tmp_path / "s.npy"), shape=(14, 14), device_resize=True)
        assert isinstance(out, np.ndarray) and out.shape == (4, 14, 14, 3)
    finally:
        fx.DEVICE_RESIZE_MAX_BYTES = old


def test_runner_batch_auto_picks_the_widest_group_that_fits():
    """`--batch auto` (the runners' default since round 5): the largest of 8 / 16 / 32 / 64 clips per group whose KV cache + tower workspace
    fit 70 % of the free device memory; explicit values still parse, out-of-range ones are rejected."""
    import argparse
    from video_llava_amd.eval import _sharded
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig
    c7 = VideoChatGPTConfig(vocab_size=32003)
    c13 = VideoChatGPTConfig(vocab_size=32003, hidden_size=5120, intermediate_size=13824, num_hidden_layers=40, num_attention_heads=40)
    GiB = 2 ** 30
    need = [_sharded.batch_bytes(b, c7, 224, 1024) for b in (8, 16, 32, 64)]
    assert need == sorted(need) and 4 * GiB < need[0] < 20 * GiB and 40 * GiB < need[3] < 160 * GiB, [n / GiB for n in need]
    assert _sharded.pick_batch(c7, 224, 1024, 270 * GiB) == 64                 # a free MI355X next to 13.5 GB of weights
    assert _sharded.pick_batch(c7, 224, 1024, int(need[2] / 0.7) + GiB) == 32
    assert _sharded.pick_batch(c7, 224, 1024, 8 * GiB) == 8                    # never below 8: a too-small GPU fails in the allocation, loudly
    assert _sharded.batch_bytes(64, c13, 336, 1024) > _sharded.batch_bytes(64, c7, 224, 1024)
    p = _sharded.add_runtime_arguments(argparse.ArgumentParser())
    assert p.parse_args([]).batch == "auto" and p.parse_args(["--batch", "16"]).batch == 16
    with pytest.raises(SystemExit):
        p.parse_args(["--batch", "65"])


def test_generate_stop_string_ahead_of_eos_in_the_same_chunk():
    """`generate(stop_strings=...)` at B = 1 whose chunk ends with the sequence at EOS must still cut at a stop string that appears
    BEFORE that EOS in the same chunk (the reference's per-token loop, model/utils.py:6-26, stops at the string first).  Host logic only: the
    device calls (prefill / decode_greedy) are scripted, so this runs without a GPU."""
    import torch.nn as nn
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM
    script = [11, 12, 13, 14, 15, 16, 17, 18] + [19] * 60             # 14 decodes to the stop string, 16 plays EOS: both inside the first chunk of 32
    STOP_ID, EOS = 14, 16

    class Tok:
        def __call__(self, text):                                     # "###" is not a single-id keyword: only the decoded-tail branch can see it
            class R:
                input_ids = [1, 40, 41, 42]
            return R()

        def batch_decode(self, ids, skip_special_tokens=True):
            return [" ".join("###" if int(t) == STOP_ID else str(int(t)) for t in row) for row in ids]

    def fake_model(eos):
        m = object.__new__(VideoChatGPTLlamaForCausalLM)
        nn.Module.__init__(m)
        m.config = VideoChatGPTConfig(eos_token_id=eos)
        m.device_ = torch.device("cpu")
        cur = {"i": 0, "done": False}

        def prefill(seqs, feats, max_seq, want_logits=False):
            cur.update(i=1, done=script[0] == eos)
            return None, torch.tensor([script[0]], dtype=torch.int32), None

        def decode_greedy(kv, first, n, eos_id=-1):                   # the device loop: EOS is sticky (csrc/sampling.hip argmax_parts_kernel)
            out = []
            for _ in range(n):
                t = eos_id if cur["done"] else script[cur["i"]]
                cur["i"] += 1
                cur["done"] = cur["done"] or (eos_id >= 0 and t == eos_id)
                out.append(t)
            return torch.tensor([out], dtype=torch.int32)
        m.prefill, m.decode_greedy = prefill, decode_greedy
        return m
    ids = [1, 5, 6]
    out = fake_model(EOS).generate([ids], max_new_tokens=40, stop_strings=["###"], tokenizer=Tok(), chunk=32)
    assert out[0, len(ids):].tolist() == script[:4], out                # cut at the stop string (token 14), not at the EOS two tokens later
    out = fake_model(EOS).generate([ids], max_new_tokens=40, chunk=32)  # without a stop string the same run ends at the EOS
    assert out[0, len(ids):].tolist() == script[:6]
    out = fake_model(None).generate([ids], max_new_tokens=40, stop_strings=["###"], tokenizer=Tok(), chunk=32, eos_token_id=None)
    assert out[0, len(ids):].tolist() == script[:4]                     # no EOS at all: still one chunk, cut at the string
    timings = {}
    fake_model(EOS).generate([ids], max_new_tokens=40, stop_strings=["###"], tokenizer=Tok(), chunk=4, timings=timings)
    assert timings["steps"] <= 8                                        # chunk of 4: the stop at token 4 ends the loop after the first chunk


def test_generate_chunk_bookkeeping_per_sequence():
    """The per-chunk token bookkeeping of generate() (vectorised per sequence in round 5): every sequence keeps its tokens up to and including
    its first EOS, finished sequences ignore later chunks, the loop ends with the chunk in which the last sequence finishes, `steps` counts up
    to that token.  Scripted device calls (no GPU): three sequences whose EOS falls in the first chunk, in the second chunk, never / late."""
    import torch.nn as nn
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM
    EOS = 9

    def run(eos_at, max_new, chunk):
        B = len(eos_at)
        scripts = [[100 * (b + 1) + i for i in range(200)] for b in range(B)]
        for b, k in enumerate(eos_at):
            if k is not None:
                scripts[b][k] = EOS
        m = object.__new__(VideoChatGPTLlamaForCausalLM)
        nn.Module.__init__(m)
        m.config = VideoChatGPTConfig(eos_token_id=EOS)
        m.device_ = torch.device("cpu")
        st = {"i": 0, "done": [False] * B, "calls": 0}

        def prefill(seqs, feats, max_seq, want_logits=False):
            st["i"] = 1
            st["done"] = [scripts[b][0] == EOS for b in range(B)]
            return None, torch.tensor([scripts[b][0] for b in range(B)], dtype=torch.int32), None

        def decode_greedy(kv, first, n, eos_id=-1):
            st["calls"] += 1
            out = [[0] * n for _ in range(B)]
            for j in range(n):
                for b in range(B):
                    t = eos_id if st["done"][b] else scripts[b][st["i"]]
                    st["done"][b] = st["done"][b] or t == eos_id
                    out[b][j] = t
                st["i"] += 1
            return torch.tensor(out, dtype=torch.int32)
        m.prefill, m.decode_greedy = prefill, decode_greedy
        tm = {}
        out = m.generate([[1, 2, 3]] * B, max_new_tokens=max_new, chunk=chunk, timings=tm)
        return out[:, 3:].tolist(), tm["steps"], st["calls"], scripts

    rows, steps, calls, sc = run([2, 40, None], 50, 32)
    assert steps == 50 and calls == 2                                             # 1 + 32 + 17 tokens
    assert rows[0][:3] == sc[0][:3] and rows[0][3:] == [EOS] * 47                  # finished at its EOS, padded with EOS
    assert rows[1][:41] == sc[1][:41] and rows[1][41:] == [EOS] * 9
    assert rows[2] == sc[2][:50]
    rows, steps, calls, sc = run([2, 40, 45], 120, 32)
    assert steps == 46 and calls == 2 and len(rows[0]) == 46                      # ends with the chunk in which the last sequence finished; steps up to its EOS
    assert rows[2] == sc[2][:46] and rows[1] == sc[1][:41] + [EOS] * 5
    rows, steps, calls, sc = run([0, 0], 20, 8)
    assert steps == 1 and calls == 0 and rows == [[EOS], [EOS]]                   # both finished by the prefill's token
