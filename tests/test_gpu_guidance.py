"""GPU: classifier-free guidance on the device (csrc/guidance.hip), from the kernel (pgv_guidance_logits) up to model.generate(guidance=).

Yardstick: video_llava_amd.guidance.guided_scores, HF's rule in fp64 numpy (held to the installed HF by tests/test_guidance_cpu.py).
 1. The kernel, entry by entry.  Tolerance, derived: the two log-softmax terms carry the per-row bound tests/test_gpu_score.py uses for a device
    log-softmax (tol = 5e-5 + 2^-21 max |x|: two v_exp / v_log evaluations and an fp32 sum of V terms), weighted by how the rule uses them
    (out = s lc + (1 - s) lu), plus four fp32 roundings of the mix itself (the two subtractions inside lc - lu count once each, the product, the sum):
        |s| tol_c + |1 - s| tol_u + 4 * 2^-23 (|s (lc - lu)| + |lu| + |out|).
 2. / 3.  End to end by a teacher-forced replay: a plain 2B-wide cache is stepped with the guided run's own tokens, the rule is applied to the
    returned logits in fp64, and the guided run's token must be the arg-max (the oracle's inverse-CDF pick) wherever the decision is not within
    rounding: an fp64 top-1 / top-2 gap above 1e-3 (a draw farther than 1e-4 from a CDF step).  The share of steps that close is bounded and asserted.
 4. Exact properties, no tolerance.   5. The penalty and the bans read the guided row (HF's processors on the reference row).   6. Refusals.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import llm as ollm
from oracle import synth
from video_llava_amd.guidance import Guidance, guided_scores, stack_features

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = float("-inf")
SCALES = (0.0, 0.5, 1.5, 3.0)
VR = 20                     # video rows of every prompt


def bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------------------------
def _rows(P, V, seed):
    """cond / uncond [P, V]: N(0, 1) scaled 1.5 - 3.5 sigma by row, the maximum repeated at a later index (a tie at the top) in every third row."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(2):
        x = torch.randn(P, V, generator=g) * (1.5 + 2.0 * torch.rand(P, 1, generator=g))
        for r in range(k, P, 3):
            if V > 2:
                x[r, V - 1 - k] = x[r].max()
        out.append(x)
    return out


def _launch(ctx, cond, uncond, scale, V, ld, ld_out_pad=3):
    """One call on buffers of row stride ld (columns [V, ld) and the output's spare columns hold a sentinel that must survive)."""
    P = cond.shape[0]
    SENT = 12345.0
    bufs = []
    for x in (cond, uncond):
        b = torch.full((P, ld), SENT, dtype=torch.float32, device=DEV)
        b[:, :V] = x.to(DEV)
        bufs.append(b)
    out = torch.full((P + 1, V + ld_out_pad), SENT, dtype=torch.float32, device=DEV)
    ctx.guidance_logits(bufs[0][:, :V], bufs[1][:, :V], scale, V=V, out=out[:P])
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[:, V:] == SENT).all()) and bool((o[P] == SENT).all()), "the kernel wrote outside its rows"
    assert bool((bufs[0].cpu()[:, V:] == SENT).all())
    return o[:P, :V]


def _row_tol(x):
    a = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).double()
    return (5e-5 + 2.0 ** -21 * a.max(dim=-1).values)[:, None]


@pytest.mark.parametrize("V,ld", [(7, 7), (515, 515), (32003, 32003), (32003, 32004)])
def test_kernel_equals_the_rule(ctx, V, ld):
    cond32, uncond32 = _rows(32, V, V + ld)
    worst = 0.0
    for scale in SCALES:
        cond = cond32.clone()
        if scale > 0:
            g = torch.Generator().manual_seed(int(scale * 10))
            for r in range(32):
                cond[r, torch.randint(0, V, (max(1, V // 50),), generator=g)] = NEG
                cond[r, int(cond32[r].argmax())] = cond32[r].max()              # the row keeps a finite maximum
        whole = None
        for P in (32, 3, 1):
            got = _launch(ctx, cond[:P], uncond32[:P], scale, V, ld)
            if P == 32:
                whole = got
                want = torch.from_numpy(guided_scores(cond.numpy(), uncond32.numpy(), scale))
                lc = torch.log_softmax(cond.double(), -1)
                lu = torch.log_softmax(uncond32.double(), -1)
                inf = torch.isinf(cond)
                assert bool((got[inf] == NEG).all()) and bool((want[inf] == NEG).all()), "-inf in the conditional row must come out -inf"
                fin = ~inf
                mix = torch.where(fin, (scale * (lc - lu)).abs(), torch.zeros_like(lu))
                bound = abs(scale) * _row_tol(cond) + abs(1 - scale) * _row_tol(uncond32) + 4 * 2.0 ** -23 * (mix + lu.abs() + torch.where(fin, want.abs(), torch.zeros_like(want)))
                err = (got.double() - want).abs()
                assert not torch.isnan(got[fin]).any()
                ratio = float((err[fin] / bound.expand_as(err)[fin]).max())
                worst = max(worst, ratio)
                print(f"V={V} ld={ld} scale={scale}: worst err / bound = {ratio:.3f}")
                assert ratio <= 1.0, (V, ld, scale, ratio)
            else:
                assert torch.equal(bits(got), bits(whole[:P])), (V, ld, scale, P, "a row depends on the pair count")
    assert worst > 0.0


def test_kernel_scale_zero_with_inf_is_nan_and_same_rows_give_the_log_softmax(ctx):
    """IEEE results stand (0 * -inf is NaN, as in HF's tensors); with d_uncond == d_cond the output is (x - M) - ls bit for bit -- the value
    pgv_logprob_rows gives for that target (same statistics, same order)."""
    V, ld, P = 32003, 32004, 3
    cond, uncond = _rows(P, V, 5)
    c = cond.clone()
    c[1, 17] = NEG
    got = _launch(ctx, c, uncond, 0.0, V, ld)
    want = guided_scores(c.numpy(), uncond.numpy(), 0.0)
    assert np.isnan(want[1, 17]) and bool(torch.isnan(got[1, 17])) and int(torch.isnan(got).sum()) == 1
    buf = torch.zeros(P, ld, dtype=torch.float32, device=DEV)
    buf[:, :V] = cond.to(DEV)
    same = ctx.guidance_logits(buf[:, :V], buf[:, :V], 1.5, V=V).cpu()
    for t in (0, 1, 5000, 31999, V - 1):
        lp, _lse, _am = ctx.logprob_rows(buf, torch.full((P,), t, dtype=torch.int32, device=DEV), V=V)
        assert torch.equal(bits(same[:, t]), bits(lp)), t


def test_kernel_refuses_bad_arguments(ctx):
    from video_llava_amd import _lib
    x = torch.zeros(2, 16, device=DEV)
    o = torch.zeros(2, 16, device=DEV)
    call = lambda ld, V, P, s, ldo: ctx.lib.pgv_guidance_logits(ctx.handle, x.data_ptr(), x.data_ptr(), ld, V, P, s, o.data_ptr(), ldo, _lib.stream_ptr())   # noqa: E731
    assert call(15, 16, 2, 1.5, 16) == _lib.PGV_EINVAL and call(16, 16, 2, 1.5, 15) == _lib.PGV_EINVAL
    assert call(16, 16, 2, float("inf"), 16) == _lib.PGV_EINVAL and call(16, 16, 2, float("nan"), 16) == _lib.PGV_EINVAL
    assert call(16, 0, 2, 1.5, 16) == _lib.PGV_EINVAL and call(16, 16, -1, 1.5, 16) == _lib.PGV_EINVAL
    assert call(16, 16, 0, 1.5, 16) == _lib.PGV_OK
    torch.cuda.synchronize()
    assert float(o.abs().sum()) == 0.0


# ---- the model, prompts, negatives and the replay ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(head_x: float):
    from helpers import make_model
    cfg = synth.LLAMA_TINY
    w = synth.make_llama_weights(cfg, seed=3, head_std=0.08)
    w["lm_head.weight"] = (w["lm_head.weight"] * np.float32(head_x)).astype(np.float32)
    return cfg, make_model(cfg, w, torch.float16)


def _prompts(cfg, seed, extras):
    rng = np.random.default_rng(seed)
    PATCH, START, END = cfg.vocab - 3, cfg.vocab - 2, cfg.vocab - 1
    prompts, feats = [], []
    for extra in extras:
        prompts.append([1] + rng.integers(3, cfg.vocab - 3, 5 + extra).tolist() + [START] + [PATCH] * VR + [END] + rng.integers(3, cfg.vocab - 3, 4).tolist())
        feats.append(torch.from_numpy(rng.standard_normal((VR, 1024), dtype=np.float32)))
    return prompts, torch.stack(feats).half()


def _negatives(cfg, prompts, kind):
    if kind == "last_token":
        return "last_token", [[p[-1]] for p in prompts]
    video = {cfg.vocab - 3, cfg.vocab - 2, cfg.vocab - 1}
    ids = [[t for t in p if t not in video] for p in prompts]                  # "no_video": the same prompt without the placeholder run
    return ids, ids


def _new(out, prompts, n):
    return [out[b, len(p):len(p) + n].tolist() for b, p in enumerate(prompts)]


def _replay(m, cfg, prompts, negs, feats_t, new, n):
    """The logits a plain 2B-wide cache returns when both twins are fed the guided run's tokens: [n] x (cond [B, V], uncond [B, V]) on the host."""
    B = len(prompts)
    both = stack_features(feats_t, None, negs, cfg.vocab - 3)
    kv, _nxt, logits = m.prefill(list(prompts) + [list(x) for x in negs], both, 128, want_logits=True)
    steps = []
    for i in range(n):
        lg = logits.cpu()
        steps.append((lg[:B], lg[B:]))
        tok = torch.tensor([new[b][i] for b in range(B)] * 2, dtype=torch.int32, device=DEV)
        _nxt, logits = m.decode_step(kv, tok, want_logits=True)
    return steps


# ---- 2. greedy ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no_video", "last_token"])
def test_greedy_guided_run_equals_the_replayed_rule(ctx, kind):
    cfg, m = _model(4.0)
    prompts, feats_t = _prompts(cfg, 2, (3, 40, 0))
    n, B = 24, 3
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=None)
    plain = _new(m.generate(prompts, **kw), prompts, n)
    neg_arg, negs = _negatives(cfg, prompts, kind)
    close = total = 0
    for scale in SCALES:
        g = Guidance(scale=scale, negative=neg_arg)
        out = m.generate(prompts, guidance=g, chunk=32, **kw)
        for chunk in (1, 5):
            assert torch.equal(m.generate(prompts, guidance=g, chunk=chunk, **kw), out), (scale, chunk)
        new = _new(out, prompts, n)
        for b in range(B):
            assert out[b, :len(prompts[b])].tolist() == prompts[b]
            assert new[b] != plain[b], (scale, b, "guidance did not change the answer")
        for i, (cond, uncond) in enumerate(_replay(m, cfg, prompts, negs, feats_t, new, n)):
            ref = guided_scores(cond.numpy(), uncond.numpy(), scale)
            for b in range(B):
                top = np.sort(ref[b])[-2:]
                total += 1
                if top[1] - top[0] > 1e-3:
                    assert new[b][i] == int(np.argmax(ref[b])), (kind, scale, i, b, new[b][i], int(np.argmax(ref[b])), float(top[1] - top[0]))
                else:
                    close += 1
    print(f"{kind}: {close} of {total} steps with an fp64 top-1 / top-2 gap below 1e-3")
    assert total == len(SCALES) * n * B and close <= 0.02 * total, (close, total)


# ---- 3. sampled --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_p", [1.0, 0.9])
@pytest.mark.parametrize("kind", ["no_video", "last_token"])
def test_sampled_guided_run_equals_the_replayed_oracle_pick(ctx, kind, top_p):
    from test_gpu_warpers import band, cdf_of, hf_chain
    cfg, m = _model(1.0)
    prompts, feats_t = _prompts(cfg, 2, (3, 40, 0))
    n, B, temp, top_k = 24, 3, 0.9, 50
    neg_arg, negs = _negatives(cfg, prompts, kind)
    gen = torch.Generator(device=DEV).manual_seed(11)
    kw = dict(video_spatio_temporal_features=feats_t, do_sample=True, temperature=temp, top_k=top_k, max_new_tokens=n, generator=gen, eos_token_id=None,
              **({"top_p": top_p} if top_p < 1 else {}))
    sure = total = 0
    for scale in SCALES:
        g = Guidance(scale=scale, negative=neg_arg)
        gen.manual_seed(11)
        out = m.generate(prompts, guidance=g, chunk=32, **kw)
        gen.manual_seed(11)
        assert torch.equal(m.generate(prompts, guidance=g, chunk=5, **kw), out), scale
        gen.manual_seed(11)
        u = torch.rand(n, B, device=DEV, generator=gen).cpu()                  # the call's uniforms stay [max_new_tokens, B]
        new = _new(out, prompts, n)
        for i, (cond, uncond) in enumerate(_replay(m, cfg, prompts, negs, feats_t, new, n)):
            ref = torch.from_numpy(guided_scores(cond.numpy(), uncond.numpy(), scale))
            got = torch.tensor([new[b][i] for b in range(B)])
            if top_p == 1.0:
                want, dist = ollm.sample_pick(ref, u[i], temp, top_k)
                ok = dist > 1e-4
            else:
                x2, y = hf_chain(ref, None, temp, top_k, top_p, 1.0)
                n_lo, n_hi, _ = band(x2, top_p)
                cdf = cdf_of(y)
                want = (cdf <= u[i].double()[:, None]).sum(-1).clamp_max(cfg.vocab - 1)
                ok = ((cdf - u[i].double()[:, None]).abs().min(-1).values > 1e-4) & (n_lo == n_hi)
            assert torch.equal(got[ok], want[ok]), (kind, scale, i, got.tolist(), want.tolist())
            sure += int(ok.sum())
            total += B
    print(f"{kind} top_p={top_p}: {sure} of {total} draws farther than 1e-4 from a CDF step")
    assert sure >= 0.95 * total, (sure, total)


# ---- 4. exact properties -----------------------------------------------------------------------------------------------------------------------------
def _drive(m, cfg, prompts, negs, feats_t, scale, n, u=None, eos=-1, chunks=(None,), temp=0.9, top_k=50):
    """A guided run over the model's step methods, with explicit uniforms u [n, B] (None: greedy) -> (kv, tokens [2B, n] on the host)."""
    B = len(prompts)
    both = stack_features(feats_t, None, negs, cfg.vocab - 3)
    kv, _nxt, _ = m.prefill(list(prompts) + [list(x) for x in negs], both, 128)
    m.set_guidance(kv, scale, B)
    try:
        if u is not None:
            uw = torch.nn.functional.pad(u.to(DEV), (0, B))
            nxt = m.sample_last(kv, uw[0], temp, top_k)
        else:
            nxt = m.greedy_last(kv, 2 * B)
        cols, done = [nxt.cpu()[:, None]], 1
        sizes = [n - 1] if chunks == (None,) else list(chunks)
        for k in sizes:
            toks = m.decode_sample(kv, nxt, k, eos, temp, top_k, uw[done:done + k]) if u is not None else m.decode_greedy(kv, nxt, k, eos)
            cols.append(toks.cpu())
            nxt, done = toks[:, k - 1].contiguous(), done + k
    finally:
        m.set_guidance(kv, 1.0, 0)
    return kv, torch.cat(cols, dim=1)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_a_batch_equals_every_prompt_alone(ctx, B):
    cfg, m = _model(4.0)
    prompts, feats_t = _prompts(cfg, 20 + B, [int(x) for x in np.random.default_rng(B).integers(0, 30, B)])
    _arg, negs = _negatives(cfg, prompts, "no_video")
    n = 12
    u = torch.stack([torch.rand(n, generator=torch.Generator().manual_seed(100 + b)) for b in range(B)], dim=1)       # one generator per prompt
    for uu in (None, u):
        _kv, whole = _drive(m, cfg, prompts, negs, feats_t, 1.5, n, uu)
        assert torch.equal(whole[B:], whole[:B]), "the twins' rows repeat the answers'"
        for b in range(B):
            _kv, alone = _drive(m, cfg, prompts[b:b + 1], negs[b:b + 1], feats_t[b:b + 1], 1.5, n, None if uu is None else uu[:, b:b + 1])
            assert torch.equal(alone[0], whole[b]), (B, b, uu is not None)
    if B > 1:           # the same through generate(): greedy rows do not depend on the batch
        kw = dict(max_new_tokens=n, eos_token_id=None, guidance=Guidance(1.5, negs))
        out = m.generate(prompts, video_spatio_temporal_features=feats_t, **kw)
        _kv, whole = _drive(m, cfg, prompts, negs, feats_t, 1.5, n)
        assert _new(out, prompts, n) == whole[:B].tolist()


def test_neutral_negative_and_neutral_records(ctx):
    cfg, m = _model(4.0)
    prompts, feats_t = _prompts(cfg, 2, (3, 40, 0))
    kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=16, eos_token_id=None)
    plain = m.generate(prompts, **kw)
    # a negative equal to the prompt, ids and features: lc == lu bit for bit, the guided row is the log-softmax of the prompt's own
    for scale in (0.0, 1.5, 3.0):
        assert torch.equal(m.generate(prompts, guidance=Guidance(scale, [list(p) for p in prompts]), **kw), plain), scale
    for neutral in (None, Guidance(scale=1.0), Guidance(1.0, "last_token"), 1.0, {"scale": 1.0}):
        assert torch.equal(m.generate(prompts, guidance=neutral, **kw), plain), neutral
    gen = torch.Generator(device=DEV).manual_seed(2)
    skw = dict(kw, do_sample=True, temperature=0.9, generator=gen)
    s_plain = m.generate(prompts, **skw)
    gen.manual_seed(2)
    assert torch.equal(m.generate(prompts, guidance=Guidance(scale=1.0), **skw), s_plain)
    # a guided call, then one without: the cache's setting was cleared
    assert not torch.equal(m.generate(prompts, guidance=1.5, **kw), plain)
    assert torch.equal(m.generate(prompts, **kw), plain)


def test_twin_slots_hold_the_negative_prompts_cache_rows(ctx):
    cfg, m = _model(4.0)
    prompts, feats_t = _prompts(cfg, 2, (3, 40, 0))
    _arg, negs = _negatives(cfg, prompts, "no_video")
    n, B, L = 10, 3, synth.LLAMA_TINY.layers
    kv, toks = _drive(m, cfg, prompts, negs, feats_t, 1.5, n, chunks=(4, 5))
    lens = [m.kv_len(kv, B + b) for b in range(B)]
    assert lens == [len(x) + n - 1 for x in negs] and [m.kv_len(kv, b) for b in range(B)] == [len(p) + n - 1 for p in prompts]
    mine = [[m.kv_peek(kv, layer, which, B + b, 0, lens[b]).cpu() for layer in (0, L - 1) for which in (0, 1)] for b in range(B)]
    kv2, _nxt, _ = m.prefill([list(x) for x in negs], None, 128)
    for i in range(n - 1):
        m.decode_step(kv2, toks[:B, i].to(DEV).contiguous())
    for b in range(B):
        assert m.kv_len(kv2, b) == lens[b]
        theirs = [m.kv_peek(kv2, layer, which, b, 0, lens[b]).cpu() for layer in (0, L - 1) for which in (0, 1)]
        for a, c in zip(mine[b], theirs):
            assert torch.equal(a.view(torch.int16), c.view(torch.int16)), b


def test_eos_ends_both_twins(ctx):
    cfg, m = _model(4.0)
    prompts, feats_t = _prompts(cfg, 2, (3, 40, 0))
    _arg, negs = _negatives(cfg, prompts, "no_video")
    B, n = 3, 12
    _kv, free = _drive(m, cfg, prompts, negs, feats_t, 1.5, n)
    eos = int(free[0, 2])
    _kv, toks = _drive(m, cfg, prompts, negs, feats_t, 1.5, n, eos=eos, chunks=(3, 4, 4))     # the last chunks start after the EOS of row 0
    assert torch.equal(toks[B:], toks[:B])
    row = toks[0].tolist()
    k = row.index(eos)
    assert k <= 2 and row[:k] == free[0, :k].tolist() and all(t == eos for t in row[k:]), row
    for b in range(1, B):
        r, f = toks[b].tolist(), free[b].tolist()
        cut = f.index(eos) + 1 if eos in f else n
        assert r[:cut] == f[:cut] and all(t == eos for t in r[cut:]), (b, r, f)
    out = m.generate(prompts, video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=eos, guidance=Guidance(1.5, negs), chunk=4)
    assert out[0, len(prompts[0]):len(prompts[0]) + k + 1].tolist() == row[:k + 1]


# ---- 5. combinations ---------------------------------------------------------------------------------------------------------------------------------
def test_repetition_penalty_and_bans_read_the_guided_row(ctx):
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    from bans_hf import hf_scores
    from video_llava_amd.logit_bans import LogitBans
    n, B, scale = 24, 3, 1.5
    raw = LogitBans(no_repeat_ngram=2, min_new_tokens=4)
    # The penalty multiplies a guided score (<= 0) of a seen id by 1.3: it moves the arg-max only where the top score is well below 0, which the
    # peaked rows of the x 4 head rarely are -- that case runs on the unscaled head, on the first prompt set whose answer the penalty changes.
    cases = {"penalty": (1.0, None), "bans": (4.0, raw)}
    for name, (head_x, ban) in cases.items():
        cfg, m = _model(head_x)
        for seed in range(2, 10):
            prompts, feats_t = _prompts(cfg, seed, (3, 40, 0))
            neg_arg, negs = _negatives(cfg, prompts, "no_video")
            kw = dict(video_spatio_temporal_features=feats_t, max_new_tokens=n, eos_token_id=None, guidance=Guidance(scale, neg_arg))
            base = _new(m.generate(prompts, **kw), prompts, n)
            eos = base[0][1]                     # min_new_tokens bans a token the unbanned run emits at once
            extra = dict(repetition_penalty=1.3) if ban is None else dict(bans=raw, eos_token_id=eos)
            out = m.generate(prompts, chunk=7, **dict(kw, **extra))
            new = _new(out, prompts, n)
            if new != base:
                break
        print(f"{name}: prompt set {seed}")
        assert new != base, (name, "no prompt set whose answer the processor changes")
        close = total = 0
        live = [True] * B
        for i, (cond, uncond) in enumerate(_replay(m, cfg, prompts, negs, feats_t, new, n)):
            ref = torch.from_numpy(guided_scores(cond.numpy(), uncond.numpy(), scale))
            for b in range(B):
                if not live[b]:
                    assert new[b][i] == eos
                    continue
                seen = prompts[b] + new[b][:i]
                if ban is None:
                    x = RepetitionPenaltyLogitsProcessor(1.3)(torch.tensor([seen]), ref[b][None].clone())[0]
                else:
                    x = hf_scores(ban, seen, len(prompts[b]), eos, ref[b]).double()
                    assert x[new[b][i]] > NEG, (name, i, b, "a banned token was picked")
                top = torch.sort(x).values[-2:]
                total += 1
                if float(top[1] - top[0]) > 1e-3:
                    assert new[b][i] == int(torch.argmax(x)), (name, i, b)
                else:
                    close += 1
                if ban is not None and new[b][i] == eos:
                    live[b] = False
        print(f"{name}: {close} of {total} steps below the gap")
        assert close <= 0.02 * total, (name, close, total)
        if ban is not None:
            assert all(eos not in row[:4] for row in new)


# ---- 6. refusals at the library level ----------------------------------------------------------------------------------------------------------------
def test_library_refusals_leave_the_state_alone(ctx):
    from video_llava_amd import _lib
    cfg, m = _model(4.0)
    prompts, feats_t = _prompts(cfg, 2, (3, 40, 0))
    _arg, negs = _negatives(cfg, prompts, "no_video")
    B = 3
    _kv, want = _drive(m, cfg, prompts, negs, feats_t, 1.5, 5)          # first: the prefill below replaces the model's one cache
    both = stack_features(feats_t, None, negs, cfg.vocab - 3)
    kv, nxt, _ = m.prefill(list(prompts) + [list(x) for x in negs], both, 128, capacity=8)
    lib = ctx.lib
    guide = lambda: int(lib.pgv_kv_guidance(kv))            # noqa: E731
    try:
        assert guide() == 0
        with pytest.raises(ValueError, match="not finite"):
            m.set_guidance(kv, float("nan"), B)
        with pytest.raises(ValueError, match="5 pairs need 10 slots"):
            m.set_guidance(kv, 1.5, 5)
        assert guide() == 0
        m.set_logprobs(kv, True)
        with pytest.raises(RuntimeError, match="pgv_kv_set_logprobs is on"):
            m.set_guidance(kv, 1.5, B)
        assert guide() == 0
        m.set_logprobs(kv, False)
        m.set_guidance(kv, 1.5, 2)                          # the live group has 6 sequences, not 4
        lens = [m.kv_len(kv, b) for b in range(2 * B)]
        for call in (lambda: m.greedy_last(kv, 2 * B), lambda: m.decode_greedy(kv, nxt, 2),
                     lambda: m.sample_last(kv, torch.zeros(2 * B), 0.9), lambda: m.decode_sample(kv, nxt, 2, -1, 0.9, 50, torch.zeros(2, 2 * B))):
            with pytest.raises(RuntimeError, match="guidance is on for 2 pairs, the live group has 6 sequences"):
                call()
        m.set_guidance(kv, 1.5, B)
        assert guide() == B
        refused = {"pgv_kv_fork": lambda: m.fork(kv, [1] * (2 * B - 1) + [2]),
                   "pgv_llm_prefill_slots": lambda: m.prefill_slots(kv, [0], prompts[:1], feats_t[:1]),
                   "pgv_beam_begin": lambda: m.beam_begin(kv, 1, 4),
                   "pgv_kv_set_lookup": lambda: m.set_lookup(kv, 3, 2),
                   "pgv_kv_set_logprobs": lambda: m.set_logprobs(kv, True)}
        for name, call in refused.items():
            with pytest.raises(RuntimeError, match=f"{name}: guidance is on"):
                call()
            assert guide() == B and [m.kv_len(kv, b) for b in range(2 * B)] == lens, name
        # ... and the guided step still runs, equal to a run that met no refusal
        toks = m.decode_greedy(kv, m.greedy_last(kv, 2 * B), 4).cpu()
        m.set_guidance(kv, 1.0, 0)
        assert guide() == 0
        assert torch.equal(toks, want[:, 1:])
        # lookup on first: guidance is refused
        m.set_lookup(kv, 3, 2)
        with pytest.raises(RuntimeError, match="pgv_kv_set_lookup is on"):
            m.set_guidance(kv, 1.5, B)
        assert guide() == 0
    finally:
        m.set_lookup(kv, 0)
        m.set_logprobs(kv, False)
        m.set_guidance(kv, 1.0, 0)
