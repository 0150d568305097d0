"""Classifier-free guidance, host side: the fp64 rule (video_llava_amd/guidance.py: guided_scores -- what the GPU tests hold the kernel to) against
HF's own generate(guidance_scale=, negative_prompt_ids=) and its processor class on a tiny CPU LlamaForCausalLM; the host checks of
generate(guidance=), the negatives of a call, the chunk loop over a scripted backend, and the callers' flags.  No GPU."""
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_generate_loop_cpu import LoopLM, _gen, _ids, _new                      # noqa: E402
from test_runner_core_cpu import EOS as SEOS, CharTok, V as VROWS                # noqa: E402
from video_llava_amd import generation as G                                     # noqa: E402
from video_llava_amd.guidance import Guidance, check_guidance, guided_scores, stack_features      # noqa: E402

VOCAB, EOS, PAD, MAX_NEW, PROMPT = 41, 2, 40, 7, 5
SCALES = (0.0, 0.5, 1.5, 3.0)


@pytest.fixture(scope="module")
def hf_models():
    """The tiny random llamas of tests/test_beam_cpu.py: vocabulary 41, lm_head x 40 so that candidates are apart."""
    transformers = pytest.importorskip("transformers")
    out = {}
    for seed in range(8):
        torch.manual_seed(seed)
        cfg = transformers.LlamaConfig(vocab_size=VOCAB, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                                       num_key_value_heads=2, max_position_embeddings=64, eos_token_id=EOS, pad_token_id=PAD, bos_token_id=1)
        m = transformers.LlamaForCausalLM(cfg).eval()
        with torch.no_grad():
            m.lm_head.weight.mul_(40.0)
        out[seed] = m
    return out


def _last_logits(model, ids):
    with torch.no_grad():
        return model(torch.tensor([ids])).logits[0, -1].double().numpy()


def reference_run(model, prompt, negative, scale, penalty):
    """The numpy rule and this project's pick rules (repetition penalty on the guided scores over the conditional ids, first-index arg-max, EOS
    ends the answer) driven with the HF model's own logits, both streams re-run in full every step.  -> (tokens, smallest top-1 / top-2 gap)."""
    seq, neg, new, gap = list(prompt), list(negative), [], float("inf")
    for _ in range(MAX_NEW):
        x = guided_scores(_last_logits(model, seq), _last_logits(model, neg), scale) if scale != 1.0 else _last_logits(model, seq)
        if penalty != 1.0:
            seen = sorted(set(seq))
            x[seen] = np.where(x[seen] < 0, x[seen] * penalty, x[seen] / penalty)
        top = np.sort(x)[-2:]
        gap = min(gap, float(top[1] - top[0]))
        t = int(np.argmax(x))
        new.append(t)
        seq.append(t)
        neg.append(t)
        if t == EOS:
            break
    return new, gap


def test_rule_and_pick_rules_equal_hf_generate(hf_models):
    """s x negative x repetition_penalty x seeds 0-7 = 128 cases: HF's greedy generate(guidance_scale=s, negative_prompt_ids=...) returns, token for
    token, what guided_scores gives when driven with the model's logits; every decision has a top-1 / top-2 gap >= 1e-3; at least half the
    answers differ from the unguided one."""
    differ, smallest = 0, float("inf")
    cases = list(itertools.product(SCALES, ("last_token", "explicit"), (1.0, 1.3), range(8)))
    for scale, kind, pen, seed in cases:
        m = hf_models[seed]
        rng = np.random.default_rng(seed)
        prompt = [1] + [int(v) for v in rng.integers(3, VOCAB - 1, PROMPT - 1)]
        negative = [prompt[-1]] if kind == "last_token" else [1] + [int(v) for v in rng.integers(3, VOCAB - 1, 3)]
        kw = {} if kind == "last_token" else {"negative_prompt_ids": torch.tensor([negative])}
        with torch.no_grad():
            hf = m.generate(torch.tensor([prompt]), guidance_scale=scale, max_new_tokens=MAX_NEW, do_sample=False, repetition_penalty=pen,
                            pad_token_id=PAD, eos_token_id=EOS, **kw)
        row = hf[0, len(prompt):].tolist()
        new, gap = reference_run(m, prompt, negative, scale, pen)
        assert Guidance(scale, None if kind == "last_token" else [negative]).negatives([prompt]) == [negative]
        assert row[:len(new)] == new and all(t == PAD for t in row[len(new):]), (scale, kind, pen, seed, row, new)
        assert gap >= 1e-3, (scale, kind, pen, seed, gap)
        smallest = min(smallest, gap)
        plain, _ = reference_run(m, prompt, negative, 1.0, pen)
        differ += plain != new
    print(f"{differ} of {len(cases)} guided answers differ from the unguided one; smallest top-1 / top-2 gap {smallest:.3g}")
    assert differ >= len(cases) // 2, differ


def test_rule_equals_hf_processor_class(hf_models):
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    m = hf_models[3]
    prompt, negative = [1, 5, 9, 30, 12, 7], [1, 17, 4]
    with torch.no_grad():
        cond = m(torch.tensor([prompt])).logits[:, -1].float()
    for scale in SCALES:
        proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(scale, m, unconditional_ids=torch.tensor([negative]), use_cache=False)
        with torch.no_grad():
            got = proc(torch.tensor([prompt]), cond.clone())[0].double().numpy()
        want = guided_scores(cond[0].numpy(), _last_logits(m, negative), scale)
        assert np.abs(got - want).max() <= 1e-6 * max(1.0, float(np.abs(want).max())), (scale, float(np.abs(got - want).max()))
    # IEEE: -inf in the conditional row is -inf under a positive scale, NaN under 0
    c = np.array([0.5, NEG_INF, 1.0]); u = np.array([0.1, 0.2, 0.3])
    assert guided_scores(c, u, 1.5)[1] == NEG_INF and np.isnan(guided_scores(c, u, 0.0)[1]) and np.isfinite(guided_scores(c, u, 0.0)[[0, 2]]).all()


NEG_INF = float("-inf")
ONE, TWO = [[1, 2, 3]], [[1, 2, 3], [1, 2, 3, 4]]


# ---- host checks -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,msg", [
    (dict(guidance=float("nan")), "`guidance` scale has to be a finite float, but is nan"),
    (dict(guidance=Guidance(float("inf"))), "`guidance` scale has to be a finite float, but is inf"),
    (dict(guidance="strong"), "`guidance` has to be a Guidance, a scale, a dict of its fields or None"),
    (dict(guidance={"guidance_scale": 2.0}), r"`guidance` has no field `guidance_scale` \(HF's `guidance_scale` is `scale` here\)"),
    (dict(guidance=Guidance(1.5, "no_video")), "`guidance` negative has to be None, \"last_token\" or one id list per prompt"),
    (dict(guidance=Guidance(1.5, [[1], [2]])), r"one id list per prompt \(1\)"),
    (dict(guidance=Guidance(1.5, [[]])), "`guidance` negative 0 has to be a non-empty id list"),
    (dict(guidance=Guidance(1.5, [[1, 256]])), "`guidance` negative 0 holds 256: not a token id below the vocabulary size 256"),
    (dict(guidance=1.5, beams=2), r"`beams` cannot be combined with `guidance` scale 1.5 \(a beam step already runs K rows per prompt"),
    (dict(guidance=1.5, lookup=3), r"`lookup` cannot be combined with `guidance` scale 1.5 \(the drafts are verified against the unguided pick\)"),
    (dict(guidance=0.0, do_sample=True, samples_per_prompt=2), r"`samples_per_prompt` cannot be combined with `guidance` scale 0 \(a fork"),
    (dict(guidance=1.5, kv_reuse_key="clip"), r"`kv_reuse_key` cannot be combined with `guidance` scale 1.5 \(the kept cache would hold the negative"),
    (dict(guidance=1.5, output_logprobs=True), r"`output_logprobs` cannot be combined with `guidance` scale 1.5 \(a guided pick records no"),
])
def test_refusals_and_their_wording(kw, msg):
    with pytest.raises(ValueError, match=msg):
        G.plan_generate(LoopLM(), ONE, max_new_tokens=4, **kw)


def test_more_than_32_prompts_and_long_negatives_are_refused():
    many = [[1, 2, 3]] * 33
    with pytest.raises(ValueError, match="33 prompts under `guidance` need 66 sequences, beyond the 64 of one decode group"):
        G.plan_generate(LoopLM(), many, max_new_tokens=4, guidance=2.0)
    assert G.plan_generate(LoopLM(), [[1, 2, 3]] * 32, max_new_tokens=4, guidance=2.0).settings.guidance == (2.0, 32)
    with pytest.raises(ValueError, match="`guidance` negative \\+ max_new_tokens = 604 exceeds max_position_embeddings 512"):
        G.plan_generate(LoopLM(), ONE, max_new_tokens=4, guidance=Guidance(2.0, [[5] * 600]))
    # a negative longer than every prompt sizes the cache
    assert G.plan_generate(LoopLM(), ONE, max_new_tokens=4, guidance=Guidance(2.0, [[5] * 100])).max_seq == 128


def test_the_new_check_comes_after_every_existing_one():
    """A call that is faulty twice keeps the error it has always had."""
    for kw, msg in ((dict(top_p=1.5), "`top_p` has to be a float"), (dict(beams=9), "`beams`=9 has to be an integer"),
                    (dict(lookup=99), "`lookup`=99 has to be an integer"), (dict(max_new_tokens=4096), "exceeds max_position_embeddings"),
                    (dict(stop_strings=["x"]), "stop_strings needs one entry per sequence and the tokenizer")):
        with pytest.raises(ValueError, match=msg):
            G.plan_generate(LoopLM(), ONE, **dict(dict(max_new_tokens=4, guidance=float("nan")), **kw))


def test_a_neutral_record_is_the_call_without_the_keyword():
    prompts = [_ids("tell me {abcabc abcab$}"), _ids("q {hi$}")]
    for neutral in (None, Guidance(), Guidance(1.0, "last_token"), Guidance(1.0, [[7], [8]]), 1.0, 1, {"scale": 1.0}, {}):
        assert check_guidance(neutral, prompts) is None
        assert G.plan_generate(LoopLM(), prompts, max_new_tokens=9, guidance=neutral) == G.plan_generate(LoopLM(), prompts, max_new_tokens=9)
        for mode in ({}, {"do_sample": True, "temperature": 0.2}):
            a, b = LoopLM(), LoopLM()
            out_a, tm_a = _gen(a, prompts, max_new_tokens=9, guidance=neutral, **mode)
            out_b, tm_b = _gen(b, prompts, max_new_tokens=9, **mode)
            assert torch.equal(out_a, out_b) and a.calls == b.calls and a.sets == b.sets == [] and tm_a["steps"] == tm_b["steps"]
    p = G.plan_generate(LoopLM(), prompts, max_new_tokens=9)
    assert p.guidance is None and p.negatives is None and p.settings.guidance is None and p.settings == G.CacheSettings(eos_id=SEOS)


def test_negatives_of_a_call():
    prompts = [[1, 5, 9], [1, 7]]
    assert Guidance(2.0).negatives(prompts) == Guidance(2.0, "last_token").negatives(prompts) == [[9], [7]]
    assert Guidance(2.0, [[1, 4], (3,)]).negatives(prompts) == [[1, 4], [3]]
    p = G.plan_generate(LoopLM(), prompts, max_new_tokens=4, guidance=Guidance(0.5, [[1, 4], [3]]))
    assert p.negatives == ((1, 4), (3,)) and p.guidance.scale == 0.5 and p.settings.guidance == (0.5, 2)
    # features of the 2B rows: the call's, then per negative its own video features (or negative_feats) where it carries patch tokens, zeros where not
    f = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4) + 1
    both = stack_features(f, None, [[1, 99, 99, 99], [1, 4]], 99)
    assert both.shape == (4, 3, 4) and torch.equal(both[:2], f) and torch.equal(both[2], f[0]) and float(both[3].abs().sum()) == 0.0
    nf = -f
    both = stack_features(f, nf, [[1, 99, 99, 99], [1, 4]], 99)
    assert torch.equal(both[2], nf[0]) and float(both[3].abs().sum()) == 0.0
    assert stack_features(None, None, [[1]], 99) is None
    with pytest.raises(ValueError, match="1 video feature sets for 2 prompts"):
        stack_features(f[:1], None, [[1], [2]], 99)


def test_no_video_negative_of_the_single_clip_entry_points():
    import inspect
    from video_llava_amd import inference
    tok = CharTok()
    g = inference.guidance_for(1.5, "no_video", "what happens?", "video-chatgpt_v1", tok, 5, True)
    with_video, _ = inference.build_prompt("what happens?", "video-chatgpt_v1", 5, True)
    without, stop = inference.build_prompt("what happens?", "video-chatgpt_v1", 5, True, video=False)
    assert "<vid_patch>" in with_video and "<vid" not in without and without.replace("what happens?\n", "what happens?\n" + with_video[with_video.index("<vid_start>"):with_video.index("<vid_end>") + 9]) == with_video
    assert g.scale == 1.5 and g.negative == [tok([without]).input_ids[0]] and stop == inference.build_prompt("q", "video-chatgpt_v1", 5, True)[1]
    assert inference.guidance_for(1.5, "last_token", "q", "video-chatgpt_v1", tok, 5, True) == Guidance(1.5, "last_token")
    assert inference.guidance_for(0.0, "worse answer", "q", "video-chatgpt_v1", tok, 5, True).negative == [tok(["worse answer"]).input_ids[0]]
    assert inference.guidance_for(None, "no_video", "q", "video-chatgpt_v1", tok, 5, True) is None
    assert inference.guidance_for(1.0, "no_video", "q", "video-chatgpt_v1", tok, 5, True) is None
    assert inference.guidance_kwargs(None, "no_video") == {} and inference.guidance_kwargs(1.0, "last_token") == {}
    assert inference.guidance_kwargs(2.0, "last_token") == {"guidance_scale": 2.0, "guidance_negative": "last_token"}
    for fn in (inference.video_chatgpt_infer, inference.video_chatgpt_infer_logprobs):
        prm = inspect.signature(fn).parameters
        assert prm["guidance_scale"].default is None and prm["guidance_negative"].default == "no_video"
    from video_llava_amd.model.video_chatgpt import VideoChatGPTLlamaForCausalLM as M
    assert inspect.signature(M.generate).parameters["guidance"].default is None and callable(M.set_guidance) and callable(M.guidance_logits)


class GuidedLM(LoopLM):
    """LoopLM with the guidance switch; every step method checks the width it is driven at."""

    def set_guidance(self, kv, scale=1.0, pairs=0):
        self.sets.append(("guidance", pairs > 0))
        self.pairs = (float(scale), int(pairs))

    def greedy_last(self, kv, width, repetition_penalty=1.0):
        assert width == len(kv.g)
        return super().greedy_last(kv, width, repetition_penalty)

    def decode_greedy(self, kv, first, n, eos_id=-1, repetition_penalty=1.0):
        assert first.shape == (len(kv.g),)
        return super().decode_greedy(kv, first, n, eos_id, repetition_penalty)


def test_the_loop_runs_prompts_and_negatives_as_one_group():
    prompts = [_ids("tell me {abcabc abcab$}"), _ids("q {hi$}"), _ids("a much longer question {}")]
    negs = [_ids("n {zzzzzzzzzzzzzzzzzzzz}"), _ids("n {yy$}"), _ids("n {xxxxxxxxxxxxxxxxxxxx}")]
    for mode in ({}, {"do_sample": True, "temperature": 0.2}):
        plain, tm0 = _gen(LoopLM(), prompts, max_new_tokens=17, chunk=5, **mode)
        m = GuidedLM()
        tm = {}
        kw = dict(mode, generator=torch.Generator().manual_seed(5)) if mode else {}
        feats = torch.full((3, VROWS, 8), 65.0)
        out = m.generate([list(p) for p in prompts], video_spatio_temporal_features=feats, timings=tm, max_new_tokens=17, chunk=5,
                         guidance=Guidance(2.0, negs), **kw)
        # the scripted backend knows no guidance: rows [0, B) answer as ever, B answers come back, the twins ran alongside
        assert torch.equal(out, plain) and _new(out, prompts) == _new(plain, prompts)
        assert m.calls == [("prefill", 6)] and m.pairs == (1.0, 0) and m.sets == [("guidance", True), ("guidance", False)]
        assert tm["batch"] == 3 and tm["steps"] == tm0["steps"]
    # the switch is cleared when a step fails
    m = GuidedLM(fail=("decode_greedy",))
    with pytest.raises(RuntimeError, match="injected"):
        _gen(m, prompts, max_new_tokens=17, guidance=Guidance(2.0, negs))
    assert m.sets == [("guidance", True), ("guidance", False)]


def test_runner_and_chat_flags():
    from video_llava_amd.chat import guidance_from_flags, parse_args
    from video_llava_amd.eval import _sharded
    assert guidance_from_flags(None, "no_video") is None and guidance_from_flags(1.0, "last_token") is None and guidance_from_flags(1.5, "no_video") == 1.5
    for kw, msg in ((dict(schedule="refill"), r"--guidance_scale 1.5 cannot be combined with --schedule refill \(a refill"),
                    (dict(beams=2), r"--guidance_scale 1.5 cannot be combined with --beams 2 \(a beam step"),
                    (dict(lookup=3), r"--guidance_scale 1.5 cannot be combined with --lookup 3 \(the drafts"),
                    (dict(samples_per_prompt=4), r"--guidance_scale 1.5 cannot be combined with --samples_per_prompt 4 \(a fork")):
        with pytest.raises(ValueError, match=msg):
            guidance_from_flags(1.5, "no_video", **kw)
        assert guidance_from_flags(1.0, "no_video", **kw) is None           # a neutral scale combines with everything
    with pytest.raises(ValueError, match="--guidance_negative has to be no_video or last_token"):
        guidance_from_flags(1.5, "none")
    with pytest.raises(ValueError, match="--guidance_scale has to be a finite float"):
        guidance_from_flags(float("nan"), "no_video")
    base = ["--model-name", "m", "--projection_path", "p"]
    a = parse_args(base + ["--guidance_scale", "1.5"])
    assert a.guidance_scale == 1.5 and a.guidance_negative == "no_video" and parse_args(base).guidance_scale is None
    with pytest.raises(SystemExit):
        parse_args(base + ["--guidance_scale", "1.5", "--lookup", "3"])
    ns = types.SimpleNamespace(guidance_scale=1.5, guidance_negative="last_token", lookup=0, beams=1, samples_per_prompt=1, schedule="group", batch=32)
    assert _sharded.guidance_scale_from_args(ns) == 1.5
    ns.batch = 33
    with pytest.raises(ValueError, match="--batch 33 clips x 2 rows under --guidance_scale exceed the 64 rows of a decode step"):
        _sharded.guidance_scale_from_args(ns)
    ns.batch, ns.schedule = "auto", "refill"
    with pytest.raises(ValueError, match="--schedule refill"):
        _sharded.guidance_scale_from_args(ns)
    assert _sharded.guidance_scale_from_args(types.SimpleNamespace()) is None


def test_decode_graph_key_carries_the_guidance_state(tmp_path):
    """Two decode-graph keys that differ only in the pair count or the scale compare unequal (the mix and follow launches bake both in); with no
    pairs the scale plays no part, so a cache that never switches guidance on keeps the key it has always had."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    prog = r"""#include <cstdio>
#include "pick_params.h"
int main() {
    const PickParams p{0.7f, 50, 0.9f, 1.2f, false};
    const int F = AM_INC_POS | AM_RECORD | AM_SAMPLE;
    const DecodeGraphKey off = decode_graph_key(6, 7, F, 3, false, p), a = decode_graph_key(6, 7, F, 3, false, p, 0, 0, 0, 0, 3, 1.5f);
    int bad = 0;
    bad |= !(off.guide_pairs == 0 && off.guide_scale == 1.f && a.guide_pairs == 3 && a.guide_scale == 1.5f && DecodeGraphKey{}.guide_pairs == 0);
    bad |= (off == a) || !(a == decode_graph_key(6, 7, F, 3, false, p, 0, 0, 0, 0, 3, 1.5f));
    bad |= a == decode_graph_key(6, 7, F, 3, false, p, 0, 0, 0, 0, 3, 3.f);
    bad |= a == decode_graph_key(6, 7, F, 3, false, p, 0, 0, 0, 0, 2, 1.5f);
    bad |= !(off == decode_graph_key(6, 7, F, 3, false, p, 0, 0, 0, 0, 0, 2.5f));
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
"""
    src = tmp_path / "key.cpp"
    src.write_text(prog)
    exe = tmp_path / "key"
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "video_llava_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout
