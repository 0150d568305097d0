"""Beam search, host side: the numpy restatement of the rules (video_llava_amd/beam_reference.py -- what the GPU tests compare the kernel with)
against HF's own generate(num_beams=K) on a tiny CPU LlamaForCausalLM; the host checks of generate(beams=K) and of the sharded runner's flags."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from video_llava_amd import beam_reference as br                      # noqa: E402
from video_llava_amd.generation import REFUSED, GenerateBeamsOutput, check_beams, check_generate_kwargs      # noqa: E402

VOCAB, EOS, PAD, MAX_NEW, PROMPT = 41, 2, 40, 7, 5          # (HF fills with `pad_token_id or eos`: a pad id of 0 would read as none)


@pytest.fixture(scope="module")
def hf_models():
    """One tiny random llama per seed; the lm_head is scaled so that candidates are apart, and EOS gets a head row that follows ten other tokens so that it reaches
    the top K at several steps (a third of the cases must end a hypothesis on it)."""
    transformers = pytest.importorskip("transformers")
    out = {}
    for seed in range(8):
        torch.manual_seed(seed)
        cfg = transformers.LlamaConfig(vocab_size=VOCAB, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                                       num_key_value_heads=2, max_position_embeddings=64, eos_token_id=EOS, pad_token_id=PAD, bos_token_id=1)
        m = transformers.LlamaForCausalLM(cfg).eval()
        with torch.no_grad():
            m.lm_head.weight.mul_(40.0)
            m.lm_head.weight[EOS] = 0.7 * m.lm_head.weight[3:13].sum(0)       # high wherever several of ten other tokens are
        out[seed] = m
    return out


def reference_run(model, prompt, K, early, lp):
    """The numpy rules driven with the HF model's own logits: every step re-runs the K running sequences in full (no cache to reorder)."""
    run = br.BeamRun(K, MAX_NEW, EOS, lp, early)
    seqs = [list(prompt) for _ in range(K)]
    while run.open:
        with torch.no_grad():
            logits = model(torch.tensor(seqs)).logits[:, -1, :].float().numpy()
        tok, par = run.step(logits)
        seqs = [seqs[int(par[i])] + [int(tok[i])] for i in range(K)]
    return run


CASES = list(itertools.product((2, 3, 4), (False, True, "never"), (0.0, 1.0, 2.0)))


def test_numpy_rules_equal_hf_beam_search(hf_models):
    """K x early_stopping x length_penalty x seeds 0-7 = 216 cases: the K returned sequences are HF's, sequences_scores within 1e-5; at least a third
    of the cases hold a hypothesis that ended on EOS."""
    eos_cases = 0
    worst = 0.0
    for (K, early, lp), seed in itertools.product(CASES, range(8)):
        m = hf_models[seed]
        prompt = [1] + [int(v) for v in np.random.default_rng(seed).integers(3, VOCAB, PROMPT - 1)]
        with torch.no_grad():
            hf = m.generate(torch.tensor([prompt]), num_beams=K, num_return_sequences=K, max_new_tokens=MAX_NEW, do_sample=False, early_stopping=early,
                            length_penalty=lp, output_scores=True, return_dict_in_generate=True, pad_token_id=PAD, eos_token_id=EOS)
        run = reference_run(m, prompt, K, early, lp)
        res = run.results()
        hf_new = hf.sequences[:, len(prompt):].tolist()
        for i, (toks, score, fin) in enumerate(res):
            assert fin, (K, early, lp, seed, i)
            row = hf_new[i]
            assert row[:len(toks)] == toks and all(v == PAD for v in row[len(toks):]), (K, early, lp, seed, i, row, toks)
            d = abs(float(hf.sequences_scores[i]) - score)
            worst = max(worst, d)
            assert d <= 1e-5, (K, early, lp, seed, i, float(hf.sequences_scores[i]), score)
        eos_cases += any(toks and toks[-1] == EOS for toks, _s, _f in res)
    print(f"cases with an EOS hypothesis: {eos_cases} of {8 * len(CASES)}; largest score difference {worst:.3g}")
    assert 3 * eos_cases >= 8 * len(CASES), eos_cases


def test_state_words_round_trip_and_start():
    st = br.BeamState(3)
    assert st.run.tolist() == [0.0, -1e9, -1e9] and (st.fin_score == br.NEG).all() and not st.fin_flag.any() and st.unsat and st.open
    w = st.to_words()
    assert w.size == br.state_words(3) == 20 and w[18] == 1 and w[19] == 1
    st.fin_len[:] = [4, 2, 0]; st.fin_flag[:] = [1, 1, 0]; st.unsat = False
    back = br.BeamState.from_words(st.to_words(), 3)
    assert back.fin_len.tolist() == [4, 2, 0] and back.fin_flag.tolist() == [1, 1, 0] and not back.unsat and back.open


def test_tie_rule_and_nan():
    """Equal scores go to the lower flat index, inside a row and across beams; a NaN never outranks a number (it poisons its row's ln sum exp, as in
    torch: the whole row ranks as -inf, behind every number, in index order)."""
    st = br.BeamState(2)
    st.run[:] = [-1.0, -1.0]
    x = np.full((2, 9), -40.0, dtype=np.float32)
    x[0, 5] = x[0, 2] = x[1, 2] = x[1, 7] = 0.0
    res = br.beam_step(st, x, 1, 10, -1, 1.0, False)
    assert res.top_index.tolist() == [2, 5, 9 + 2, 9 + 7] and res.tokens.tolist() == [2, 5] and res.parents.tolist() == [0, 0]
    st = br.BeamState(2)
    st.run[:] = [0.0, -5.0]
    x[0, 0] = np.nan
    res = br.beam_step(st, x, 1, 10, -1, 1.0, False)
    assert res.top_index.tolist() == [9 + 2, 9 + 7, 9 + 0, 9 + 1] and res.parents.tolist() == [1, 1] and np.isfinite(res.top_scores).all()


def test_check_beams_refusals_and_resolution():
    assert check_beams(1, 64, do_sample=True, repetition_penalty=1.3, early_stopping="whatever") == (1, 1.0, False)       # greedy: everything inert
    assert check_beams(4, 16) == (4, 1.0, False)
    assert check_beams(2, 1, length_penalty=2.0, early_stopping="never") == (2, 2.0, "never")
    assert check_beams(2, 1, generation_config={"length_penalty": 0.5, "early_stopping": True}) == (2, 0.5, True)
    assert check_beams(2, 1, length_penalty=0.0, generation_config={"length_penalty": 0.5}) == (2, 0.0, False)
    for name, kw in [("do_sample", dict(do_sample=True)), ("samples_per_prompt", dict(samples_per_prompt=2)), ("repetition_penalty", dict(repetition_penalty=1.1)),
                     ("output_logprobs", dict(output_logprobs=True)), ("stopping_criteria", dict(has_criteria=True)), ("stop_strings", dict(has_stop_strings=True)),
                     ("kv_reuse_key", dict(has_reuse_key=True))]:
        with pytest.raises(ValueError, match=f"`{name}`"):
            check_beams(3, 2, **kw)
    for bad in (0, 9, -1, 2.5, True):
        with pytest.raises(ValueError, match="`beams`"):
            check_beams(bad, 1)
    with pytest.raises(ValueError, match="exceed the 64"):
        check_beams(8, 9)
    with pytest.raises(ValueError, match="early_stopping"):
        check_beams(2, 1, early_stopping="sometimes")
    assert GenerateBeamsOutput(1, 2).new_lengths is None


def test_num_beams_stays_refused_and_names_beams():
    assert REFUSED["num_beams"](2) and not REFUSED["num_beams"](1)
    with pytest.raises(ValueError, match=r"argument `num_beams`=3 .*`beams`"):
        check_generate_kwargs({"num_beams": 3})
    with pytest.raises(ValueError, match=r"generation_config field `num_beams`=4 .*`beams`"):
        check_generate_kwargs({}, {"num_beams": 4})


def test_generate_refuses_before_any_device_work():
    """generate(beams=...) validates on the host: a model object without weights or GPU raises the ValueError of check_beams, not a device error."""
    from video_llava_amd.model.video_chatgpt import VideoChatGPTLlamaForCausalLM
    m = VideoChatGPTLlamaForCausalLM.__new__(VideoChatGPTLlamaForCausalLM)
    m.generation_config = None
    with pytest.raises(ValueError, match="`do_sample` cannot be combined with `beams`=2"):
        m.generate([[1, 2, 3]], beams=2, do_sample=True)
    with pytest.raises(ValueError, match="`beams`=9"):
        m.generate([[1, 2, 3]], beams=9)
    with pytest.raises(ValueError, match="`output_beam_scores` needs `beams`"):
        m.generate([[1, 2, 3]], output_beam_scores=True)


def test_runner_flags(capsys):
    """--beams K --length_penalty F --early_stopping {false,true,never}: group schedule only; the refusals name the flag."""
    import argparse
    from video_llava_amd.eval import _sharded
    ap = _sharded.add_runtime_arguments(argparse.ArgumentParser())
    ok = ap.parse_args(["--beams", "4", "--length_penalty", "0.5", "--early_stopping", "never", "--batch", "16"])
    assert _sharded.check_beam_args(ok) == (4, 0.5, "never")
    assert _sharded.check_beam_args(ap.parse_args([])) == (1, None, None)
    assert _sharded.check_beam_args(ap.parse_args(["--beams", "2", "--early_stopping", "true"])) == (2, None, True)
    for argv, word in [(["--beams", "2", "--do_sample"], "--do_sample"), (["--beams", "2", "--schedule", "refill"], "--schedule refill"),
                       (["--beams", "2", "--schedule", "refill", "--do_sample", "--samples_per_prompt", "3"], "--do_sample"),
                       (["--beams", "9"], "--beams 9"), (["--beams", "8", "--batch", "9"], "--batch 9")]:
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
        assert word in capsys.readouterr().err, argv
    ns = ap.parse_args(["--beams", "2"])
    ns.samples_per_prompt = 3
    with pytest.raises(ValueError, match="--samples_per_prompt 3"):
        _sharded.check_beam_args(ns)
