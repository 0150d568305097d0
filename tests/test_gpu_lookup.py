"""GPU: prompt-lookup speculative decoding and its building block, the row-wise decode step -- several consecutive positions of a sequence in one
pass over the weights.  A row is bit for bit the plain decode step at its position, so everything here is torch.equal against plain greedy
decoding; no tolerances.  Every cache is filled by another group first (`poison`): a row that was not written cannot hide behind identical leftovers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import synth

from helpers import make_model  # noqa: E402
from lookup_cases import check_rows_equal_steps, poison  # noqa: E402
from video_llava_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 128


def ints(xs):
    return (C.c_int32 * len(xs))(*[int(x) for x in xs])


def bits(x):
    return x.contiguous().view(torch.int16)


# --------------------------------------------------------------------------------------------------
# 1. the attention building block
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attn_models(ctx):
    """One weightless 1-layer model per (dtype, heads): the entries only take its dtype, head count and RoPE table."""
    made = {}
    for dt in (torch.float16, torch.bfloat16):
        for heads in (32, 40):
            cfg = _lib.LlmConfig(vocab=64, hidden=heads * HD, inter=11008 if heads == 32 else 13824, layers=1, heads=heads, eps=1e-5, rope_theta=10000.0)
            h = C.c_void_p()
            _lib.check(ctx.lib.pgv_llm_create(ctx.handle, C.byref(cfg), _lib.dtype_code(dt), C.byref(h)), "pgv_llm_create")
            made[(dt, heads)] = h
    yield made
    for h in made.values():
        ctx.lib.pgv_llm_destroy(h)


POISON = -7.25          # exact in fp16 and bf16; no q / k / v value (|randn| * 0.5 never rounds to it by design of the check below)


@pytest.mark.parametrize("dt,heads,split", [(dt, heads, split) for dt in (torch.float16, torch.bfloat16) for heads in (32, 40) for split in (1, 0)]
                         + [(torch.float16, 40, 4), (torch.bfloat16, 40, 8), (torch.bfloat16, 32, 2)],       # the forced splits' row instantiations too
                         ids=lambda v: {torch.float16: "fp16", torch.bfloat16: "bf16"}.get(v, str(v)))
def test_attention_rows_equal_sequential_decode_attention(ctx, attn_models, dt, heads, split):
    """Two slots in one launch, 8 rows each (slot 1: 5 valid rows and 3 that are no row); the start positions make pos + j cross the 64-key round and
    the 256-key ring period of the unsplit kernel and the 16-key groups of the split one.  Outputs of the valid rows and the whole cache equal those of
    8 consecutive pgv_decode_attention calls on the same q / k / v; the outputs of the absent rows and every cache row nobody owns keep their
    poison value."""
    llm = attn_models[(dt, heads)]
    H, max_seq, n = heads * HD, 320, 8
    lib, st = ctx.lib, _lib.stream_ptr()
    for case, (p0, p1) in enumerate([(57, 250), (0, 300), (62, 1)]):
        g = torch.Generator(device=DEV).manual_seed(100 * heads + 10 * case + split)
        valid = [n, 5]
        row_slot = [0] * n + [1] * 5 + [-1] * 3
        row_j = list(range(n)) + list(range(5)) + [0, 0, 0]
        R = len(row_slot)
        qkv = (torch.randn(R, 3 * H, device=DEV, generator=g) * 0.5).to(dt)
        K0 = torch.full((2, heads, max_seq, HD), POISON, device=DEV, dtype=dt)
        V0 = K0.clone()
        for b, p in enumerate((p0, p1)):
            K0[b, :, :p] = (torch.randn(heads, p, HD, device=DEV, generator=g) * 0.5).to(dt)
            V0[b, :, :p] = (torch.randn(heads, p, HD, device=DEV, generator=g) * 0.5).to(dt)
        assert not (qkv == POISON).any()
        # reference: consecutive plain steps (slot 1 drops out after its 5 rows; the plain kernel is batch-invariant)
        Kr, Vr = K0.clone(), V0.clone()
        ref = torch.full((R, H), POISON, device=DEV, dtype=dt)
        part = torch.zeros(R * heads * 8 * 130, device=DEV, dtype=torch.float32)
        ticket = torch.zeros(R * heads, device=DEV, dtype=torch.int32)
        for j in range(n):
            live = [b for b in (0, 1) if j < valid[b]]
            rows = [j] + ([n + j] if 1 in live else [])
            q = qkv[rows].contiguous()
            o = torch.empty(len(rows), H, device=DEV, dtype=dt)
            _lib.check(lib.pgv_decode_attention(ctx.handle, llm, q.data_ptr(), ints([(p0, p1)[b] + j for b in live]), Kr.data_ptr(), Vr.data_ptr(), o.data_ptr(),
                                                len(live), max_seq, split, part.data_ptr(), ticket.data_ptr(), st), "pgv_decode_attention")
            ref[rows] = o
        # the row form, one launch
        Kg, Vg = K0.clone(), V0.clone()
        out = torch.full((R, H), POISON, device=DEV, dtype=dt)
        _lib.check(lib.pgv_decode_attention_rows(ctx.handle, llm, qkv.data_ptr(), ints([p0, p1]), 2, ints(row_slot), ints(row_j), Kg.data_ptr(), Vg.data_ptr(),
                                                 out.data_ptr(), R, max_seq, split, part.data_ptr(), ticket.data_ptr(), st), "pgv_decode_attention_rows")
        torch.cuda.synchronize()
        assert torch.isfinite(ref[:n + 5].float()).all()
        assert torch.equal(bits(out), bits(ref)), (case, (bits(out) != bits(ref)).any(dim=1).nonzero().flatten().tolist())
        assert (out[n + 5:] == POISON).all()
        assert torch.equal(bits(Kg), bits(Kr)) and torch.equal(bits(Vg), bits(Vr)), case
        assert (Kg[1, :, p1 + 5:] == POISON).all() and (Vg[0, :, p0 + n:] == POISON).all()
        assert not ticket.any()


def test_attention_rows_refusals(ctx, attn_models):
    llm = attn_models[(torch.float16, 32)]
    buf = torch.zeros(1 << 16, device=DEV, dtype=torch.float16)
    p = buf.data_ptr()
    call = lambda pos, rs, rj, max_seq, split=1: ctx.lib.pgv_decode_attention_rows(ctx.handle, llm, p, ints(pos), len(pos), ints(rs), ints(rj), p, p, p, len(rs),
                                                                                   max_seq, split, p, p, _lib.stream_ptr())
    assert call([3], [0, 0], [0, 0], 16) == _lib.PGV_EINVAL and b"two rows" in ctx.lib.pgv_last_error()
    assert call([14], [0, 0], [0, 2], 16) == _lib.PGV_EINVAL and b"outside" in ctx.lib.pgv_last_error()
    assert call([3], [1], [0], 16) == _lib.PGV_EINVAL
    assert call([3], [0], [0], 16, split=3) == _lib.PGV_EINVAL
    assert not buf.any()


# --------------------------------------------------------------------------------------------------
# 2. decode_rows
# --------------------------------------------------------------------------------------------------
ROW_CASES = {
    "2x8": ([37, 52], [8, 8], 96),
    "3x6_ragged": ([5, 61, 30], [6, 3, 5], 96),
    "8x8": ([9, 17, 33, 64, 65, 70, 3, 48], [8] * 8, 96),           # 64 rows: crosses the 16- and 32-column tiles of the GEMVs
}


@pytest.fixture(scope="module")
def tiny(ctx):
    cfg = synth.LLAMA_TINY
    w = synth.make_llama_weights(cfg, seed=3, head_std=0.08)
    return {dt: make_model(cfg, w, dt) for dt in (torch.float16, torch.bfloat16)}, cfg.vocab


@pytest.mark.parametrize("case", list(ROW_CASES))
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_decode_rows_equal_consecutive_decode_steps(tiny, dt, case):
    models, vocab = tiny
    lens, rows, max_seq = ROW_CASES[case]
    check_rows_equal_steps(models[dt], vocab, lens, rows, max_seq, seed=41)


def test_decode_rows_unfolded_norm_path():
    """PGV_LLM_NORM_FOLD=0 is read once per process: the same cases in a child process."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f'''
import sys, torch
sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r})
from oracle import synth
from helpers import make_model
from lookup_cases import check_rows_equal_steps
cfg = synth.LLAMA_TINY
w = synth.make_llama_weights(cfg, seed=3, head_std=0.08)
for dt in (torch.float16, torch.bfloat16):
    m = make_model(cfg, w, dt)
    check_rows_equal_steps(m, cfg.vocab, [37, 52], [8, 8], 96, seed=41)
    check_rows_equal_steps(m, cfg.vocab, [5, 61, 30], [6, 3, 5], 96, seed=41)
    check_rows_equal_steps(m, cfg.vocab, [9, 17, 33, 64, 65, 70, 3, 48], [8] * 8, 96, seed=41)
print("unfolded rows ok")
'''
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, PGV_LLM_NORM_FOLD="0"))
    assert r.returncode == 0 and "unfolded rows ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_decode_rows_13b_shaped_two_layers(ctx):
    """40 heads: the context-split attention with its cross-workgroup merge, and the 10-row-block residual producers, 12-bit weight stream (16 rows)."""
    from video_llava_amd import random_init as ri
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    vocab = 32003
    cfg = VideoChatGPTConfig(vocab_size=vocab, hidden_size=5120, intermediate_size=13824, num_hidden_layers=2, num_attention_heads=40, eos_token_id=None)
    m = VideoChatGPTLlamaForCausalLM(cfg, VisionConfig(frame_size=224), torch.bfloat16, torch.device(DEV))
    ri.load_streaming(m, ri.iter_llama_tensors(vocab=vocab, hidden=5120, inter=13824, layers=2, device=DEV, dtype=torch.bfloat16, seed=13, head_std=0.05))
    check_rows_equal_steps(m, vocab, [59, 250], [8, 8], 272, seed=7)


# --------------------------------------------------------------------------------------------------
# refusals and the unchanged path
# --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_cache_unchanged(tiny):
    models, vocab = tiny
    m = models[torch.float16]
    rng = np.random.default_rng(5)
    prompts = [[1] + rng.integers(3, vocab - 3, n - 1).tolist() for n in (20, 28)]
    kv, nxt, _ = m.prefill(prompts, None, 32)
    lib, h = m.ctx.lib, m.ctx.handle
    tok = torch.tensor([5, 6, 7, 8, 9, 10], dtype=torch.int32, device=DEV)
    lg = torch.full((6, vocab), 3.0, device=DEV)
    rows = lambda slots: lib.pgv_llm_decode_rows(h, m.handle, kv, ints(slots), tok.data_ptr(), len(slots), lg.data_ptr(), _lib.stream_ptr())
    from lookup_cases import peek
    assert rows([0, 0]) == _lib.PGV_ESTATE and b"pgv_kv_set_lookup" in lib.pgv_last_error()          # no row scratch yet
    assert lib.pgv_kv_set_lookup(kv, 16, 2) == _lib.PGV_EINVAL and lib.pgv_kv_set_lookup(kv, -1, 2) == _lib.PGV_EINVAL
    assert lib.pgv_kv_set_lookup(kv, 3, 0) == _lib.PGV_EINVAL and lib.pgv_kv_set_lookup(kv, 3, 5) == _lib.PGV_EINVAL
    assert rows([0, 0]) == _lib.PGV_ESTATE                                                            # the refused settings changed nothing
    m.set_lookup(kv, 2)
    assert rows([0, 0, 0, 0]) == _lib.PGV_EINVAL and b"rows per slot" in lib.pgv_last_error()          # more than 1 + D rows
    assert rows([0, 1, 0]) == _lib.PGV_EINVAL and b"consecutive" in lib.pgv_last_error()
    assert rows([0, 2]) == _lib.PGV_EINVAL and b"outside" in lib.pgv_last_error()
    assert rows([1, 1, 1]) == _lib.PGV_OK                                                               # 28 + 3 rows fit 32 ...
    m.decode_step(kv, nxt)
    m.decode_step(kv, nxt)
    before = [peek(m, kv, b, 0, 32) for b in (0, 1)]
    assert rows([1, 1, 1]) == _lib.PGV_EINVAL and b"cache holds" in lib.pgv_last_error()               # ... 30 + 3 do not
    # pgv_llm_decode_lookup: every refusal, nothing launched
    out = torch.full((2, 8), -5, dtype=torch.int32, device=DEV)
    cnt = torch.full((2, 2), -5, dtype=torch.int32, device=DEV)
    look = lambda budget, steps=2: lib.pgv_llm_decode_lookup(h, m.handle, kv, nxt.data_ptr(), steps, -1, ints(budget), out.data_ptr(), cnt.data_ptr(), _lib.stream_ptr())
    assert look([1, 1]) == _lib.PGV_ESTATE and b"id record" in lib.pgv_last_error()                     # prefilled before lookup was set, stepped since
    assert lib.pgv_kv_set_lookup(kv, 0, 0) == _lib.PGV_OK and rows([0]) == _lib.PGV_ESTATE
    assert look([1, 1]) == _lib.PGV_ESTATE and b"lookup is off" in lib.pgv_last_error()
    kv2, nxt, _ = m.prefill(prompts, None, 32, lookup=(3, 2))
    assert kv2.value == kv.value
    before = [peek(m, kv, b, 0, 32) for b in (0, 1)]
    assert look([13, 4]) == _lib.PGV_EINVAL and b"cache holds" in lib.pgv_last_error()                  # 20 + 13 > 32
    assert look([1, 1], steps=0) == _lib.PGV_EINVAL
    m.set_warpers(kv, 1.0, 1.3)
    assert look([1, 1]) == _lib.PGV_ESTATE and b"repetition penalty" in lib.pgv_last_error()
    m.set_warpers(kv, 1.0, 1.0)
    m.set_logprobs(kv, True)
    assert look([1, 1]) == _lib.PGV_ESTATE and b"log-probabilities" in lib.pgv_last_error()
    m.set_logprobs(kv, False)
    from video_llava_amd.logit_bans import LogitBans
    m.set_bans(kv, LogitBans(suppress=[7]))
    assert look([1, 1]) == _lib.PGV_ESTATE and b"bans" in lib.pgv_last_error()
    m.set_bans(kv, None)
    # a beam run in flight
    m.beam_begin(kv, 1, 4, -1, 1.0, False)
    assert look([1, 1]) == _lib.PGV_ESTATE and b"beam run" in lib.pgv_last_error()
    kv2, nxt, _ = m.prefill(prompts, None, 32, lookup=(3, 2))                                           # a prefill ends the beam run
    before = [peek(m, kv, b, 0, 32) for b in (0, 1)]
    # more rows than a step takes: 5 sequences x (1 + 15) in a cache whose row scratch holds 64
    kv5, nxt5, _ = m.prefill([p[:6] for p in prompts + prompts + prompts[:1]], None, 32, lookup=(15, 2))
    out5, cnt5 = torch.full((5, 32), -5, dtype=torch.int32, device=DEV), torch.full((2, 5), -5, dtype=torch.int32, device=DEV)
    before5 = [peek(m, kv5, b, 0, 32) for b in range(5)]
    assert lib.pgv_llm_decode_lookup(h, m.handle, kv5, nxt5.data_ptr(), 2, -1, ints([1] * 5), out5.data_ptr(), cnt5.data_ptr(), _lib.stream_ptr()) == _lib.PGV_EINVAL
    assert b"5 sequences x 16 rows" in lib.pgv_last_error()
    torch.cuda.synchronize()
    assert (out5 == -5).all() and (cnt5 == -5).all() and [m.kv_len(kv5, b) for b in range(5)] == [6] * 5
    assert all(torch.equal(a, peek(m, kv5, b, 0, 32)) for b, a in enumerate(before5))
    m.set_lookup(kv5, 0)
    kv2, nxt, _ = m.prefill(prompts, None, 32, lookup=(3, 2))                                           # back to the two-sequence cache
    kv = kv2
    before = [peek(m, kv, b, 0, 32) for b in (0, 1)]
    assert (out == -5).all() and (cnt == -5).all() and [m.kv_len(kv, b) for b in (0, 1)] == [20, 28]
    assert look([1, 1]) == _lib.PGV_OK and (cnt.cpu() == torch.tensor([[1, 1], [0, 0]])).all()          # the budget ends both runs after one token
    m.prefill(prompts, None, 32)
    m.decode_step(kv, nxt)
    m.decode_step(kv, nxt)
    m.set_lookup(kv, 0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, peek(m, kv, b, 0, 32)) for b, a in enumerate(before))
    assert [m.kv_len(kv, b) for b in (0, 1)] == [22, 30] and (lg[3:] == 3.0).all()


# --------------------------------------------------------------------------------------------------
# 3. / 4. end to end: generate(lookup=D) is generate()
# --------------------------------------------------------------------------------------------------
V_TINY, NEW = 20, 40


def _prompts(vocab, seeds):
    """Small-vocabulary prompts made of repeated spans (the tiny model then loops, so drafts get accepted); every third one carries a video run."""
    out = []
    for sd in seeds:
        rng = np.random.default_rng(sd)
        base = rng.integers(3, 11, 6).tolist()
        n = int(rng.integers(12, 50))
        ids = [1]
        while len(ids) < n:
            ids += base[:int(rng.integers(2, 7))]
        ids = ids[:n]
        if sd % 3 == 2:
            ids = ids[:5] + [vocab - 2] + [vocab - 3] * V_TINY + [vocab - 1] + ids[5:]
        out.append(ids)
    return out


def _feats(B):
    g = torch.Generator().manual_seed(77)
    return (torch.randn(B, V_TINY, 1024, generator=g) * 0.5).to(torch.float16).to(DEV)


def _new_tokens(out, prompts, eos):
    rows = []
    for b, p in enumerate(prompts):
        new = out[b, len(p):len(p) + NEW].tolist()
        if eos is not None and eos in new:
            new = new[:new.index(eos) + 1]
        rows.append(new)
    return rows


def _pick_eos(prompts, answers, D, n):
    """An id whose first occurrence in some plain answer sits inside an accepted run of the numpy trace: (eos, slot) or None."""
    from video_llava_amd.lookup_reference import lookup_trace
    for b, (p, a) in enumerate(zip(prompts, answers)):
        for k in range(4, len(a)):
            v = a[k]
            if v in a[:k] or any(v in q for q in prompts):
                continue
            tr = lookup_trace(p + a[:1], a[1:k + 1], D, n, v, NEW - 1)
            if tr and tr[-1] > 1:
                return v, b
    return None


@pytest.mark.parametrize("D", [1, 3, 7])
def test_generate_lookup_equals_generate(tiny, D):
    """B in {1, 3, 8}, ragged prompts with and without video rows, EOS off and on, chunks of 1, 5 and 32 lookup steps: the ids are those of the
    call without `lookup`, and the device's per-step emit counts are lookup_trace of the PLAIN answer, step for step.  What the inputs must
    exercise is asserted from the plain answers and the numpy rule alone: steps that accept a draft, steps that reject one, a sequence that meets
    its EOS inside an accepted run and one that exhausts its budget inside one."""
    from video_llava_amd.lookup_reference import lookup_candidates, lookup_trace
    models, vocab = tiny
    m = models[torch.float16]
    n = 2
    seen = {"accept": False, "reject": False, "eos_in_run": False, "budget_in_run": False}
    for iB, B in enumerate((1, 3, 8)):
        prompts = _prompts(vocab, range(10 * iB, 10 * iB + B))
        feats = _feats(B) if any(vocab - 3 in p for p in prompts) else None
        chunk = (1, 5, 32)[(iB + D) % 3]
        max_seq = (max(len(p) for p in prompts) + NEW + 63) // 64 * 64          # generate's own choice: the poisoned cache is the one it uses
        plain = m.generate(prompts, feats, max_new_tokens=NEW, eos_token_id=None, chunk=chunk)
        answers = _new_tokens(plain, prompts, None)
        picked = _pick_eos(prompts, answers, D, n)
        for eos in [None] + ([picked[0]] if picked else []):
            if eos is not None:
                plain = m.generate(prompts, feats, max_new_tokens=NEW, eos_token_id=eos, chunk=chunk)
                answers = _new_tokens(plain, prompts, eos)
            poison(m, vocab, B, max_seq)
            tm = {}
            got = m.generate(prompts, feats, max_new_tokens=NEW, eos_token_id=eos, chunk=chunk, lookup=D, lookup_ngram=n, timings=tm)
            assert torch.equal(got, plain), (B, D, eos, chunk)
            traces = [lookup_trace(p + a[:1], a[1:], D, n, eos, NEW - 1) for p, a in zip(prompts, answers)]
            assert tm["lookup_emitted"] == sum(len(a) - 1 for a in answers) and tm["lookup_steps"] == max(len(t) for t in traces), (tm, B, D, eos)
            # the device's own counts, from one decode_lookup call on a fresh prefill
            kv, nxt, _ = m.prefill(prompts, feats, max_seq, lookup=(D, n))
            toks, counts = m.decode_lookup(kv, nxt, NEW - 1, -1 if eos is None else eos, [NEW - 1] * B)
            m.set_lookup(kv, 0)
            toks = toks.cpu()
            for b in range(B):
                assert int(nxt[b]) == answers[b][0]
                steps = counts[:, b].tolist()
                assert steps[:len(traces[b])] == traces[b] and not any(steps[len(traces[b]):]), (B, D, eos, b, steps, traces[b])
                assert toks[b, :sum(traces[b])].tolist() == answers[b][1:]
                assert m.kv_len(kv, b) == len(prompts[b]) + len(answers[b]) - 1
                # accepted / rejected drafts per step, from the numpy rule on the plain answer
                e, seq = 0, prompts[b] + answers[b][:1]
                for c in traces[b]:
                    drafts = lookup_candidates(seq, D, n, eos)[:max(0, NEW - 1 - e - 1)]
                    rest = answers[b][1 + e:]
                    a = 0
                    while a < len(drafts) and a < len(rest) and drafts[a] == rest[a]:
                        a += 1
                    seen["accept"] |= a > 0
                    seen["reject"] |= a < len(drafts)
                    seq += answers[b][1 + e:1 + e + c]
                    e += c
                if eos is not None and answers[b][-1] == eos and traces[b][-1] > 1:
                    seen["eos_in_run"] = True
                if len(answers[b]) == NEW and traces[b][-1] > 1 and (eos is None or answers[b][-1] != eos):
                    seen["budget_in_run"] = True
    assert all(seen.values()), (D, seen)


def test_generate_lookup_with_stop_string_and_stopping_criterion(tiny):
    from helpers import SynthTokenizer
    models, vocab = tiny
    m = models[torch.bfloat16]
    tok = SynthTokenizer(vocab)
    prompts = _prompts(vocab, [3])
    plain = m.generate(prompts, None, max_new_tokens=NEW, eos_token_id=None)
    new = plain[0, len(prompts[0]):].tolist()
    stop = f" {new[17]} {new[18]}"
    a = m.generate(prompts, None, max_new_tokens=NEW, eos_token_id=None, stop_strings=[stop], tokenizer=tok, chunk=5)
    b = m.generate(prompts, None, max_new_tokens=NEW, eos_token_id=None, stop_strings=[stop], tokenizer=tok, chunk=5, lookup=3)
    assert torch.equal(a, b) and a.shape[1] < plain.shape[1]
    crit = lambda ids, scores: ids.shape[1] >= len(prompts[0]) + 23
    a = m.generate(prompts, None, max_new_tokens=NEW, eos_token_id=None, stopping_criteria=[crit])
    b = m.generate(prompts, None, max_new_tokens=NEW, eos_token_id=None, stopping_criteria=[crit], lookup=7, lookup_ngram=3)
    assert torch.equal(a, b) and a.shape[1] == len(prompts[0]) + 23


def test_plain_greedy_after_row_steps_is_a_fresh_run(tiny):
    """Row steps use a scratch of their own and capture nothing: plain decode_greedy on the same cache object afterwards, graphs included, is bit for bit
    the run of a cache that never saw one."""
    models, vocab = tiny
    m = models[torch.bfloat16]
    rng = np.random.default_rng(9)
    prompts = [[1] + rng.integers(3, vocab - 3, n - 1).tolist() for n in (12, 31, 7)]
    kv, nxt, _ = m.prefill(prompts, None, 128)
    want = m.decode_greedy(kv, nxt, 20).clone()
    kv, nxt2, _ = m.prefill(prompts, None, 128)
    assert torch.equal(nxt, nxt2)
    warm = m.decode_greedy(kv, nxt2, 9)                    # eager step + both graphs
    assert torch.equal(warm, want[:, :9])
    kv, nxt2, _ = m.prefill(prompts, None, 128)
    m.set_lookup(kv, 3)
    m.decode_rows(kv, [0, 0, 0, 0, 1, 2, 2], torch.arange(3, 10, dtype=torch.int32))
    m.set_lookup(kv, 0)
    assert torch.equal(m.decode_greedy(kv, nxt2, 20), want)
    # ... and after a whole lookup run with its own captured graphs on the same cache object (3 sequences, 128 positions)
    m.generate(prompts, None, max_new_tokens=40, eos_token_id=None, chunk=9, lookup=3)
    kv3, nxt3, _ = m.prefill(prompts, None, 128)
    assert kv3.value == kv.value and torch.equal(nxt3, nxt)
    assert torch.equal(m.decode_greedy(kv3, nxt3, 20), want)


def test_runner_and_infer_take_the_lookup_flag(ctx, tmp_path):
    """The QA runner with `--lookup 3` writes the predictions of the run without it, its --timings lines say how many tokens a step emitted, and
    video_chatgpt_infer(lookup=) is video_chatgpt_infer()."""
    import json
    from helpers import SynthTokenizer
    from test_gpu_runners import _tiny_components
    from video_llava_amd.eval import run_inference_qa_activitynet as qa
    from video_llava_amd.inference import video_chatgpt_infer
    ccfg, lcfg, cw, lw, tower, model, ip, V = _tiny_components()
    vd = tmp_path / "v"; vd.mkdir()
    names = ["s1", "s2", "s3"]
    frames = {n: synth.make_frames(5 + i, ccfg.image, seed=60 + i) for i, n in enumerate(names)}
    for n in names:
        np.save(vd / f"v_{n}.npy", frames[n])
    qs = [{"video_name": n, "question": f"what happens {i}?", "question_id": f"{n}_q"} for i, n in enumerate(names)]
    (tmp_path / "q.json").write_text(json.dumps(qs)); (tmp_path / "a.json").write_text(json.dumps([{"answer": "a"}] * 3))
    tok = SynthTokenizer(lcfg.vocab)
    outs = {}
    for tag, extra in (("plain", []), ("lookup", ["--lookup", "3", "--lookup_ngram", "2"])):
        args = qa.parse_args(["--video_dir", str(vd), "--gt_file_question", str(tmp_path / "q.json"), "--gt_file_answers", str(tmp_path / "a.json"),
                              "--output_dir", str(tmp_path / tag), "--output_name", "p", "--model-name", "x", "--projection_path", "y",
                              "--conv-mode", "default", "--batch", "3", "--max_new_tokens", "48", "--timings", str(tmp_path / f"{tag}.jsonl")] + extra)
        outs[tag] = qa.run_inference(args, components=(model, tower, tok, ip, V))
    assert [o["pred"] for o in outs["lookup"]] == [o["pred"] for o in outs["plain"]] and all(len(o["pred"].split()) > 5 for o in outs["plain"])
    lines = [json.loads(x) for x in open(tmp_path / "lookup.jsonl")]
    assert len(lines) == 3 and all(x["lookup_emitted_group"] >= x["lookup_steps_group"] >= 1 for x in lines)
    assert all("lookup_steps_group" not in json.loads(x) for x in open(tmp_path / "plain.jsonl"))
    for n, o in zip(names, outs["plain"]):
        got = video_chatgpt_infer(frames[n], o["question"], "default", model, tower, tok, ip, V, do_sample=False, max_new_tokens=48, lookup=3)
        assert got == o["pred"], (n, got, o["pred"])
