"""GPU: teacher-forced scoring -- pgv_logprob_rows (csrc/score.hip), pgv_llm_score, VideoChatGPTLlamaForCausalLM.score and
inference.video_chatgpt_score -- against fp64 on the same fp32 logits, against this model's own forward() and against the fixture the
REFERENCE's forward produced (tests/golden/llama_tiny.npz).

Tolerance of one row's log-probability / logsumexp against fp64 on the same fp32 logits: TOL(row) = 5e-5 + 2^-21 max|x|.  Worst-case budget
(eps = 2^-24): <= 40 eps relative per term from the rounded argument (x - M) log2(e) -- terms below e^-40 of the largest cannot reach fp32
resolution even V of them together -- <= 140 eps for 126 strided adds plus 8 tree levels, 2 eps for the log: ~2.4e-5 for |x| <= 64, doubled;
plus three roundings at the magnitude of the logits (x - M, M + log, x[t] - M).
"""
import os

import numpy as np
import pytest
import torch

from oracle import synth

from helpers import SynthTokenizer as _Tok, make_model as _model, make_tower as _tower  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ref64(x: torch.Tensor, targets):
    """fp64 reference on fp32 logits x [R, V] (host): (logprob [R] with 0 where the target is negative, logsumexp [R], first-index argmax [R], TOL [R])."""
    x = x.detach().cpu().float()
    xd = x.double()
    lse = torch.logsumexp(xd, dim=1)
    t = torch.as_tensor(np.asarray(targets), dtype=torch.long)
    lp = torch.where(t >= 0, xd.gather(1, t.clamp_min(0)[:, None])[:, 0] - lse, torch.zeros_like(lse))
    am = torch.from_numpy(np.argmax(x.numpy(), axis=1).astype(np.int32))            # numpy: first index on ties
    finite = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))
    tol = 5e-5 + 2.0 ** -21 * finite.max(dim=1).values.double()
    return lp, lse, am, tol


def assert_close_rows(got: torch.Tensor, want: torch.Tensor, tol: torch.Tensor, what: str):
    got, want = got.detach().cpu().double(), want.double()
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), what                      # a target on -inf is -inf exactly
    err = (got[~inf] - want[~inf]).abs()
    assert not torch.isnan(err).any(), what
    if err.numel():
        worst = int(torch.argmax(err - tol[~inf]))
        print(f"{what}: max |err| {float(err.max()):.3e} (tolerance there {float(tol[~inf][int(torch.argmax(err))]):.3e})")
        assert bool((err <= tol[~inf]).all()), (what, float(err[worst]), float(tol[~inf][worst]))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


def make_rows(R: int, V: int, seed: int, fill: float):
    """[R, ceil16(V) + 16] fp32 logits whose columns [V, ld) hold `fill`, and int32 targets.  Row kinds by r % 5: N(0, 3) with the maximum
    repeated at a later index; all equal; one dominant logit; magnitudes +-3e4; a few -inf entries (the target of such a row sits on one)."""
    g = torch.Generator().manual_seed(seed)
    ld = (V + 15) // 16 * 16 + 16
    x = torch.full((R, ld), fill, dtype=torch.float32)
    t = torch.empty(R, dtype=torch.int32)
    cyc = [0, V - 1, -100, V // 2, V // 3]
    for r in range(R):
        kind = r % 5
        row = torch.randn(V, generator=g) * 3.0
        tgt = cyc[(r // 5 + r) % 5]
        if kind == 0 and V > 2:
            first = int(torch.argmax(row))
            if first + 1 < V:
                row[V - 1] = row[first]                                 # a tie: the first index must win
        elif kind == 1:
            row[:] = 2.5
        elif kind == 2:
            j = int(torch.randint(0, V, (1,), generator=g))
            row /= 3.0
            row[j] = 50.0
            tgt = j
        elif kind == 3:
            row *= 1e4
        elif kind == 4 and V > 4:
            idx = torch.randperm(V, generator=g)[:max(1, V // 5)]
            row[idx] = -float("inf")
            if r % 2 == 0:
                tgt = int(idx[0])
        x[r, :V] = row
        t[r] = tgt
    return x, t


@pytest.mark.parametrize("R", [1, 3, 257])
@pytest.mark.parametrize("V,fill", [(1, float("nan")), (15, float("nan")), (16, float("nan")), (17, float("nan")), (515, float("nan")),
                                    (515, 1e30), (32003, float("nan"))])
def test_logprob_rows_against_fp64(ctx, V, fill, R):
    """pgv_logprob_rows on caller buffers.  Columns [V, ld) hold NaN (once +1e30): any read past V shows in every output."""
    x, t = make_rows(R, V, seed=1000 * V + R, fill=fill)
    lp, lse, am = ctx.logprob_rows(x.to(DEV), t.to(DEV), V)
    lp_r, lse_r, am_r, tol = ref64(x[:, :V], t)
    assert_close_rows(lse, lse_r, tol, f"lse V={V} R={R}")
    assert_close_rows(lp, lp_r, tol, f"logprob V={V} R={R}")
    assert torch.equal(am.cpu(), am_r)                                   # exact, first index on ties
    lp = lp.cpu()
    assert bool((lp[t < 0] == 0).all()) and bool((lp <= 0).all())
    for r in range(R):
        if r % 5 == 1 and t[r] >= 0:
            assert abs(float(lp[r]) + np.log(V)) <= float(tol[r]), r    # all equal: -log V
        if r % 5 == 2:
            assert -1e-3 < float(lp[r]) <= 0.0, (r, float(lp[r]))       # one dominant logit: <= 0 and ~ 0
    # NULL outputs are skipped, the others unchanged
    lib = ctx.lib
    from video_llava_amd import _lib
    only = torch.full((R,), 7.0, device=DEV)
    xd, td = x.to(DEV), t.to(DEV)
    _lib.check(lib.pgv_logprob_rows(ctx.handle, xd.data_ptr(), xd.shape[1], V, R, td.data_ptr(), only.data_ptr(), None, None, _lib.stream_ptr()))
    assert torch.equal(bits(only), bits(lp))


@pytest.mark.parametrize("V", [17, 32003])
def test_logprob_rows_is_launch_invariant(ctx, V):
    """The same row in launches of different R and at another row index: bitwise equal results (fixed reduction order)."""
    x, t = make_rows(257, V, seed=5, fill=float("nan"))
    big = ctx.logprob_rows(x.to(DEV), t.to(DEV), V)
    for r in (0, 3, 129, 256):
        one = ctx.logprob_rows(x[r:r + 1].to(DEV), t[r:r + 1].to(DEV), V)
        three = ctx.logprob_rows(torch.cat([x[7:9], x[r:r + 1]]).to(DEV), torch.cat([t[7:9], t[r:r + 1]]).to(DEV), V)
        for a, b, c in zip(big, one, three):
            assert torch.equal(bits(a[r:r + 1]), bits(b)) and torch.equal(bits(b), bits(c[2:3])), r
    # timed under profiling family 6 (the short decode kernels)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        ctx.logprob_rows(x[:3].to(DEV), t[:3].to(DEV), V)
        prof = ctx.prof_get()
    finally:
        ctx.prof_enable(False)
    assert prof["decode_small"]["launches"] == 1 and prof["decode_small"]["ms"] > 0 and all(v["launches"] == 0 for k, v in prof.items() if k != "decode_small")
    with pytest.raises(ValueError, match="multiple of 4"):
        from video_llava_amd import _lib
        bad = torch.zeros(2, 18, device=DEV)
        _lib.check(ctx.lib.pgv_logprob_rows(ctx.handle, bad.data_ptr(), 18, 17, 2, t[:2].to(DEV).data_ptr(), None, None, None, _lib.stream_ptr()))


# ---- the reference's fixture ------------------------------------------------------------------------------------------------------------
_FIX = {}


def fixture_model(golden_dir, tag):
    """fp16 model of the `lin` / `mlp` fixture, its sequence (prompt + the reference's greedy tokens), features and -- computed once, shared,
    never written to -- this model's own forward() logits for that sequence."""
    if tag not in _FIX:
        g = np.load(os.path.join(golden_dir, "llama_tiny.npz"))
        proj, image = {"lin": ("linear", 224), "mlp": ("mlp2x_gelu", 336)}[tag]
        cfg = synth.LlamaCfg(**{**synth.LLAMA_TINY.__dict__, "projector": proj})
        w = synth.make_llama_weights(cfg, seed=int(g[tag + "_weight_seed"]), head_std=float(g["head_std"]))
        m = _model(cfg, w, torch.float16, image)
        seq = g[tag + "_ids"].tolist() + g[tag + "_tokens"].tolist()
        feats = torch.from_numpy(g[tag + "_feats"]).half()[None]
        fwd = m(input_ids=torch.tensor([seq]), video_spatio_temporal_features=feats).logits[0].clone()
        _FIX[tag] = (g, cfg, m, seq, feats, fwd)
    return _FIX[tag]


def padded(logits: torch.Tensor) -> torch.Tensor:
    """[R, V] -> [R, ceil16(V) + 16] with NaN behind column V (pgv_logprob_rows wants ld % 4 == 0)."""
    R, V = logits.shape
    out = torch.full((R, (V + 15) // 16 * 16 + 16), float("nan"), dtype=torch.float32, device=logits.device)
    out[:, :V] = logits
    return out


def check_against_own_logits(ctx, out, lens, all_logits, targets, what):
    """Checks 2(a): score()'s numbers are BITWISE pgv_logprob_rows applied to the model's own all-position logits [sum lens, V] for the same
    batch (alignment, the vocabulary extent -- 515 of 528 columns --, chunk scatter) and within TOL of fp64 on those logits."""
    V = all_logits.shape[1]
    t = torch.from_numpy(np.asarray(targets, dtype=np.int32))
    lp, _lse, am = ctx.logprob_rows(padded(all_logits.float()), t.to(all_logits.device), V)
    lp, am = lp.cpu(), am.cpu()
    lp_r, _lse_r, am_r, tol = ref64(all_logits, t)
    off = 0
    for b, n in enumerate(lens):
        on = t[off:off + n - 1] >= 0
        assert torch.equal(out.scored[b][1:], on) and not bool(out.scored[b][0])
        assert torch.equal(bits(out.token_logprobs[b][1:][on]), bits(lp[off:off + n - 1][on])), (what, b)
        assert torch.equal(out.argmax[b][1:][on], am[off:off + n - 1][on]) and torch.equal(am[off:off + n - 1][on], am_r[off:off + n - 1][on]), (what, b)
        assert bool((out.token_logprobs[b][~out.scored[b]] == 0).all()) and bool((out.argmax[b][~out.scored[b]] == -1).all())
        assert_close_rows(out.token_logprobs[b][1:][on], lp_r[off:off + n - 1][on], tol[off:off + n - 1][on], f"{what} seq {b} vs fp64")
        assert int(out.counts[b]) == int(on.sum())
        assert float(out.sequence_logprob[b]) == float(out.token_logprobs[b][out.scored[b]].double().sum())
        off += n
    return lp_r, tol


@pytest.mark.parametrize("tag", ["lin", "mlp"])
def test_score_against_forward_and_the_reference_fixture(ctx, golden_dir, tag):
    """Sequence = the fixture's prompt + the reference's greedy tokens, labels = the sequence itself (every row but the last is scored).
    (a) against this model's forward() logits: bitwise pgv_logprob_rows of them, within TOL of their fp64 log-softmax;
    (b) against the REFERENCE's logits (prompt rows: *_prefill_logits, continuation rows: *_step_logits):
        |d logprob| <= 2 max_v |forward_logit - ref_logit| of that row + TOL -- log-softmax is 1-Lipschitz in the max norm for the lse part and
        the target's own logit moves by at most the same amount; the right-hand side is computed here from forward(), whose distance to the
        fixture the existing tests bound.  Largest measured |d| (LAB.md): 2.5e-3 (lin) / 2.9e-3 (mlp) under bounds of 7.9e-3 / 7.3e-3;
    (c) the argmax of the continuation rows is the reference's greedy tokens (fixture margins > 0.02)."""
    g, cfg, m, seq, feats, fwd = fixture_model(golden_dir, tag)
    S, P = len(seq), len(g[tag + "_ids"])
    out = m.score(torch.tensor([seq]), torch.tensor([seq]), video_spatio_temporal_features=feats)
    targets = seq[1:] + [-1]
    check_against_own_logits(ctx, out, [S], fwd, targets, f"{tag} (a)")
    assert int(out.counts[0]) == S - 1
    # (b)
    ref = torch.cat([torch.from_numpy(g[tag + "_prefill_logits"]), torch.from_numpy(g[tag + "_step_logits"])[1:]]).float()
    assert ref.shape == (S, cfg.vocab)
    lp_ref, _, _, tol = ref64(ref, targets)
    dist = (fwd.cpu().double() - ref.double()).abs().max(dim=1).values
    d = (out.token_logprobs[0][1:].double() - lp_ref[:-1]).abs()
    bound = 2.0 * dist[:-1] + tol[:-1]
    print(f"{tag} (b): largest |logprob - reference's| {float(d.max()):.3e} (bound there {float(bound[int(torch.argmax(d))]):.3e}; "
          f"largest forward-vs-fixture logit distance {float(dist.max()):.3e})")
    assert bool((d <= bound).all()), (int(torch.argmax(d - bound)), float((d - bound).max()))
    # (c)
    assert out.argmax[0][P:].tolist() == g[tag + "_tokens"].tolist()


def test_loss_is_cross_entropy_of_forward_logits(ctx, golden_dir):
    """ScoreOutput.loss == fp64 CrossEntropyLoss on forward()'s logits with HF's shift (the reference's video_chatgpt.py:228-239), labels -100 on
    the prompt (placeholder run included); unscored positions hold 0 and are masked out."""
    g, cfg, m, seq, feats, fwd = fixture_model(golden_dir, "lin")
    P = len(g["lin_ids"])
    labels = [-100] * P + seq[P:]
    out = m.score([seq], [labels], video_spatio_temporal_features=feats)
    ce = torch.nn.functional.cross_entropy(fwd.cpu().double()[:-1], torch.tensor(labels[1:]), ignore_index=-100)
    tol = float(ref64(fwd, [0] * len(seq))[3].max())
    print(f"loss {out.loss:.6f} vs fp64 cross_entropy {float(ce):.6f}")
    assert abs(out.loss - float(ce)) <= tol
    assert out.scored[0].tolist() == [False] * P + [True] * (len(seq) - P) and int(out.counts[0]) == len(seq) - P
    assert bool((out.token_logprobs[0][:P] == 0).all()) and bool((out.token_logprobs[0][P:] < 0).all())
    # a two-sequence batch with different label sets: the batch mean is over all scored tokens
    lab2 = [-100] * (P + 3) + seq[P + 3:]
    out2 = m.score([seq, seq], [labels, lab2], video_spatio_temporal_features=feats)
    both = torch.cat([fwd.cpu().double()[:-1], fwd.cpu().double()[:-1]])
    ce2 = torch.nn.functional.cross_entropy(both, torch.tensor(labels[1:] + lab2[1:]), ignore_index=-100)
    assert abs(out2.loss - float(ce2)) <= tol and out2.counts.tolist() == [len(seq) - P, len(seq) - P - 3]
    # nothing scored: nan, like torch's mean over no element
    assert np.isnan(m.score([seq], [[-100] * len(seq)], video_spatio_temporal_features=feats).loss)


def test_score_is_batch_invariant(ctx, golden_dir):
    """Three ragged sequences, one of them text-only: scored together they are bitwise what each gives alone; a label set that scores only
    the last row of a sequence works."""
    g, cfg, m, seq, feats, _fwd = fixture_model(golden_dir, "lin")
    P = len(g["lin_ids"])
    seqs = [seq, seq[:P + 5], [1] + list(range(20, 29))]
    labels = [list(seqs[0]), [-100] * (len(seqs[1]) - 1) + [seqs[1][-1]], list(seqs[2])]
    f3 = torch.cat([feats, feats, torch.zeros_like(feats)])
    tog = m.score(seqs, labels, video_spatio_temporal_features=f3)
    assert tog.counts.tolist() == [len(seqs[0]) - 1, 1, len(seqs[2]) - 1]
    assert tog.scored[1].tolist() == [False] * (len(seqs[1]) - 1) + [True]
    for b in range(3):
        one = m.score([seqs[b]], [labels[b]], video_spatio_temporal_features=feats if b < 2 else None)
        assert torch.equal(bits(one.token_logprobs[0]), bits(tog.token_logprobs[b])), b
        assert torch.equal(one.argmax[0], tog.argmax[b]) and torch.equal(one.scored[0], tog.scored[b])
        assert float(one.sequence_logprob[0]) == float(tog.sequence_logprob[b])
    # one clip for all sequences: projected once and broadcast -- the same numbers as a feature set per sequence
    two = m.score(seqs[:2], labels[:2], video_spatio_temporal_features=feats)
    assert all(torch.equal(bits(two.token_logprobs[b]), bits(tog.token_logprobs[b])) for b in range(2))


def test_score_chunks(ctx):
    """2 * SCORE_CHUNK_ROWS + 3 scored rows in 5 sequences: three chunks, the last one of 3 rows; every number lands on its own row."""
    from video_llava_amd import _lib
    assert _lib.SCORE_CHUNK_ROWS == 1024
    cfg = synth.LLAMA_TINY
    m = _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16)
    lens = [411, 412, 411, 411, 411]
    assert sum(n - 1 for n in lens) == 2 * _lib.SCORE_CHUNK_ROWS + 3
    rng = np.random.default_rng(7)
    seqs = [[1] + rng.integers(3, cfg.vocab - 3, n - 1).tolist() for n in lens]
    _kv, _nxt, _lg, all_lg = m.prefill(seqs, None, 448, want_all_logits=True)
    all_lg = all_lg.clone()
    out = m.score(seqs, seqs)
    targets = np.concatenate([np.asarray(s[1:] + [-1]) for s in seqs])
    check_against_own_logits(ctx, out, lens, all_lg, targets, "chunks")
    assert int(out.counts.sum()) == 2 * _lib.SCORE_CHUNK_ROWS + 3


def test_score_fp8(ctx):
    """quantize_weights_fp8(): score equals fp64 on that model's own forward() logits."""
    cfg = synth.LLAMA_TINY
    m = _model(cfg, synth.make_llama_weights(cfg, seed=3, head_std=0.08), torch.float16)
    m.quantize_weights_fp8()
    assert m.is_fp8
    rng = np.random.default_rng(8)
    seq = [1] + rng.integers(3, cfg.vocab - 3, 40).tolist()
    fwd = m(input_ids=torch.tensor([seq])).logits[0].clone()
    out = m.score([seq], [seq])
    check_against_own_logits(ctx, out, [len(seq)], fwd, seq[1:] + [-1], "fp8")


def test_score_real_vocabulary_bf16(ctx):
    """A two-layer 7B-shaped model (hidden 4096, vocabulary 32003: 32016 lm_head columns), bf16, one sequence of 80 tokens, the last 20 scored."""
    from video_llava_amd.random_init import iter_llama_tensors, load_streaming
    cfg = synth.LlamaCfg(layers=2)
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    m = VideoChatGPTLlamaForCausalLM(VideoChatGPTConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2,
                                                        num_attention_heads=cfg.heads, eos_token_id=None), VisionConfig(), torch.bfloat16)
    load_streaming(m, iter_llama_tensors(vocab=cfg.vocab, hidden=cfg.hidden, inter=cfg.inter, layers=2, dtype=torch.bfloat16, seed=5, head_std=0.05))
    rng = np.random.default_rng(9)
    seq = [1] + rng.integers(3, 32000, 79).tolist()
    labels = [-100] * 60 + seq[60:]
    _kv, _nxt, _lg, all_lg = m.prefill([seq], None, 128, want_all_logits=True)
    all_lg = all_lg.clone()
    out = m.score([seq], [labels])
    assert int(out.counts[0]) == 20
    check_against_own_logits(ctx, out, [80], all_lg, [-1] * 59 + seq[60:] + [-1], "7B-shaped bf16")


def test_score_state(ctx, golden_dir):
    """score() is a prefill: earlier past_key_values go stale, the cache it leaves continues like prefill's, a label beyond the vocabulary is
    refused with the cache unchanged."""
    g, cfg, m, seq, feats, _fwd = fixture_model(golden_dir, "lin")
    ids = g["lin_ids"].tolist()
    old = m(input_ids=torch.tensor([ids]), video_spatio_temporal_features=feats)
    out = m.score([ids], [ids], video_spatio_temporal_features=feats)
    with pytest.raises(RuntimeError, match="stale"):
        m(input_ids=torch.tensor([[5]]), past_key_values=old.past_key_values)
    n = len(g["lin_tokens"])
    out = m.score([ids], [ids], video_spatio_temporal_features=feats)
    assert m.kv_len(out.kv, 0) == len(ids)
    first = m.sample_last(out.kv, torch.zeros(1), 1.0, 1)              # the greedy token of the last row's logits (top_k 1, u 0)
    toks = [int(first[0])] + m.decode_greedy(out.kv, first, n - 1)[0].tolist()
    gen = m.generate(torch.tensor([ids]), video_spatio_temporal_features=feats, max_new_tokens=n, eos_token_id=None)[0, len(ids):].tolist()
    assert toks == gen == g["lin_tokens"].tolist()
    out = m.score([ids], [ids], video_spatio_temporal_features=feats)
    before = m.kv_len(out.kv, 0)
    with pytest.raises(ValueError, match="outside the vocabulary"):     # same cache shape: the refused call reaches the library with this cache
        m.score([ids], [ids[:-1] + [cfg.vocab]], video_spatio_temporal_features=feats)
    assert m.kv_len(out.kv, 0) == before == len(ids)
    with pytest.raises(ValueError, match="labels for"):
        m.score([ids], [ids[:-1]])
    with pytest.raises(NotImplementedError):                             # forward(labels=) stays refused: score() is the way
        m(input_ids=torch.tensor([ids]), labels=torch.tensor([ids]))


class _RoundTripTok(_Tok):
    """SynthTokenizer whose decode can be encoded back: id t <-> the private-use character U+E000 + t."""

    def _encode(self, s):
        ids, i = [1], 0
        while i < len(s):
            for name, tid in self.special.items():
                if s.startswith(name, i):
                    ids.append(tid); i += len(name)
                    break
            else:
                o = ord(s[i])
                ids.append(o - 0xE000 if 0xE000 <= o < 0xE000 + self.vocab else 3 + (o % (self.vocab - 8))); i += 1
        return ids

    def batch_decode(self, ids, skip_special_tokens=True):
        return ["".join(chr(0xE000 + int(t)) for t in row) for row in ids]


def test_video_chatgpt_score(ctx):
    """inference.video_chatgpt_score on the tiny tower + decoder of the QA-runner test (weight seeds 21 / 22: every greedy step's oracle margin
    is 0.9+): equals a manual score() call; candidate order changes no candidate's numbers; the greedy answer of video_chatgpt_infer scores
    greedy = True (with a tokenizer in which the stop string is one token, as "</s>" is in LLaMA's: here the token the model emits next)."""
    from video_llava_amd.inference import build_prompt, video_chatgpt_infer, video_chatgpt_score, video_features
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    from video_llava_amd.scoring import continuation_labels
    ccfg, lcfg = synth.CLIP_TINY, synth.LLAMA_TINY
    tower = _tower(ccfg, synth.make_clip_weights(ccfg, seed=21))
    model = VideoChatGPTLlamaForCausalLM(VideoChatGPTConfig(vocab_size=lcfg.vocab, hidden_size=lcfg.hidden, intermediate_size=lcfg.inter,
                                                            num_hidden_layers=lcfg.layers, num_attention_heads=lcfg.heads, eos_token_id=None,
                                                            max_position_embeddings=2048), VisionConfig(frame_size=ccfg.image), torch.float16)
    model.load_state_dict(synth.make_llama_weights(lcfg, seed=22, head_std=0.08))
    vc = model.get_model().vision_config
    vc.vid_patch_token, vc.vid_start_token, vc.vid_end_token, vc.use_vid_start_end = lcfg.vocab - 3, lcfg.vocab - 2, lcfg.vocab - 1, True
    tok = _RoundTripTok(lcfg.vocab)

    class IP:
        crop_size = {"height": ccfg.image, "width": ccfg.image}
    V = 100 + (ccfg.image // ccfg.patch) ** 2
    frames = synth.make_frames(5, ccfg.image, seed=30)
    q, mode = "what happens 0?", "pg-video-llava"
    text = video_chatgpt_infer(frames, q, mode, model, tower, tok, IP(), V, do_sample=False, max_new_tokens=6)
    gen = [ord(c) - 0xE000 for c in text]
    assert len(gen) == 6 and all(0 <= t < lcfg.vocab - 3 for t in gen), gen
    prompt, stop_str = build_prompt(q, mode, V, True)
    tok.special[stop_str] = gen[5]                                       # the stop string is ONE token: the one greedy decoding emits after text[:5]
    cands = [text[:5], "yes", text[:4] + "no", "a longer wrong answer"]
    res = video_chatgpt_score(frames, q, cands, mode, model, tower, tok, IP(), V)
    assert [set(r) for r in res] == [{"logprob", "tokens", "mean_logprob", "greedy"}] * 4
    assert res[0]["greedy"] is True and res[0]["tokens"] == 6 and not any(r["greedy"] for r in res[1:])
    assert all(r["logprob"] < 0 for r in res)
    assert [r["tokens"] for r in res] == [6, 4, 7, len(cands[3]) + 1]
    # a manual score() call
    feats = video_features(frames, tower, IP())
    pid = tok([prompt]).input_ids[0]
    full = [tok([prompt + c + stop_str]).input_ids[0] for c in cands]
    man = model.score(full, [continuation_labels(pid, f) for f in full], video_spatio_temporal_features=feats[None])
    for b, r in enumerate(res):
        assert r["logprob"] == float(man.sequence_logprob[b]) and r["tokens"] == int(man.counts[b])
        assert r["mean_logprob"] == r["logprob"] / r["tokens"]
    # candidate order (and the features given up front: CLIP is skipped)
    rev = video_chatgpt_score(None, q, cands[::-1], mode, model, tower, tok, IP(), V, features=feats)
    assert rev[::-1] == res


def test_score_answers_runner(ctx, tmp_path):
    """eval/score_answers.py at world 1: two samples (and one whose video is missing) through run_inference(components=...); the JSON's
    numbers are those of direct video_chatgpt_score calls."""
    import json
    from video_llava_amd.eval import score_answers as sa
    from video_llava_amd.feature_extraction import load_video
    from video_llava_amd.inference import video_chatgpt_score
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig
    ccfg, lcfg = synth.CLIP_TINY, synth.LLAMA_TINY
    tower = _tower(ccfg, synth.make_clip_weights(ccfg, seed=21))
    model = VideoChatGPTLlamaForCausalLM(VideoChatGPTConfig(vocab_size=lcfg.vocab, hidden_size=lcfg.hidden, intermediate_size=lcfg.inter,
                                                            num_hidden_layers=lcfg.layers, num_attention_heads=lcfg.heads, eos_token_id=None,
                                                            max_position_embeddings=2048), VisionConfig(frame_size=ccfg.image), torch.float16)
    model.load_state_dict(synth.make_llama_weights(lcfg, seed=22, head_std=0.08))
    vc = model.get_model().vision_config
    vc.vid_patch_token, vc.vid_start_token, vc.vid_end_token, vc.use_vid_start_end = lcfg.vocab - 3, lcfg.vocab - 2, lcfg.vocab - 1, True
    tok = _Tok(lcfg.vocab)

    class IP:
        crop_size = {"height": ccfg.image, "width": ccfg.image}
    V = 100 + (ccfg.image // ccfg.patch) ** 2
    vd = tmp_path / "v"; vd.mkdir()
    names = ["k1", "k2"]
    for i, n in enumerate(names):
        np.save(vd / f"v_{n}.npy", synth.make_frames(5 + i, ccfg.image, seed=30 + i))
    qs = [{"video_name": "k1", "question": "what happens 0?", "question_id": "k1_q"}, {"video_name": "missing", "question": "gone?", "question_id": "m_q"},
          {"video_name": "k2", "question": "what happens 1?", "question_id": "k2_q"}]
    ans = [{"answer": "a dog runs"}, {"answer": "nothing"}, {"answer": "yes"}]
    (tmp_path / "q.json").write_text(json.dumps(qs)); (tmp_path / "a.json").write_text(json.dumps(ans))
    args = sa.parse_args(["--video_dir", str(vd), "--gt_file_question", str(tmp_path / "q.json"), "--gt_file_answers", str(tmp_path / "a.json"),
                          "--output_dir", str(tmp_path / "out"), "--output_name", "scores", "--model-name", "x", "--projection_path", "y", "--batch", "2"])
    out = sa.run_inference(args, components=(model, tower, tok, IP(), V))
    assert json.load(open(tmp_path / "out" / "scores.json")) == out and [o["id"] for o in out] == ["k1_q", "k2_q"]
    assert all(set(o) == {"id", "question", "answer", "answer_logprob", "answer_tokens", "answer_ppl"} for o in out)
    for o, n in zip(out, names):
        frames = load_video(str(vd / f"v_{n}.npy"), shape=(ccfg.image, ccfg.image), device_resize=True)     # the runner's loader (it samples frames)
        direct = video_chatgpt_score(frames, o["question"], [o["answer"]], "pg-video-llava", model, tower, tok, IP(), V)[0]
        assert o["answer_logprob"] == direct["logprob"] and o["answer_tokens"] == direct["tokens"] == len(o["answer"]) + 4
        assert o["answer_ppl"] == float(np.exp(-direct["logprob"] / direct["tokens"]))
