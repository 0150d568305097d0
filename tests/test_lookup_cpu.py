"""Host side of the row-wise decode step and of prompt-lookup drafting: the numpy drafting rule against HF's own generator, the step trace against a
token-by-token restatement, and the C ABI of the row step."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from video_llava_amd.lookup_reference import lookup_candidates, lookup_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _search(ids, D, n, eos):
    """The rule once more, in plain loops, with what happened on the way: (drafts, kind flags)."""
    L = len(ids)
    kinds = set()
    for g in range(min(n, L - 1), 0, -1):
        for idx in range(L - g + 1):
            if ids[idx:idx + g] != ids[L - g:]:
                continue
            start, end = idx + g, min(idx + g + D, L)
            if start >= end:
                continue
            out = ids[start:end]
            if g < min(n, L - 1):
                kinds.add("smaller_ngram")
            if idx + g + D > L:
                kinds.add("clipped")
            if eos is not None and eos in out:
                kinds.add("eos_cut")
                out = out[:out.index(eos)]
            return out, kinds
    return [], {"no_match"}


def _cases():
    rng = np.random.default_rng(2024)
    for i in range(400):
        vocab = int(rng.integers(6, 13))
        L = int(rng.integers(2, 61))
        ids = rng.integers(0, vocab, L).tolist()
        D = (1, 3, 7, 15)[i % 4]
        n = (1, 2, 3, 4)[(i // 4) % 4]
        eos = int(rng.integers(0, vocab)) if i % 2 else None
        yield ids, D, n, eos


def test_candidates_equal_hf_prompt_lookup():
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    seen = set()
    count = 0
    for ids, D, n, eos in _cases():
        gen = PromptLookupCandidateGenerator(eos_token_id=None if eos is None else torch.tensor([eos]), num_output_tokens=D, max_matching_ngram_size=n,
                                             max_length=10 ** 6)
        inp = torch.tensor([ids], dtype=torch.long)
        hf = gen.get_candidates(inp)[0][0, len(ids):].tolist()
        want, kinds = _search(ids, D, n, eos)
        got = lookup_candidates(ids, D, n, eos)
        assert got == hf == want, (ids, D, n, eos, got, hf, want)
        assert len(got) <= D and (eos is None or eos not in got)
        seen |= kinds
        count += 1
    assert count >= 200
    assert seen >= {"no_match", "smaller_ngram", "eos_cut", "clipped"}, seen


def test_candidates_stop_at_the_first_window_even_when_the_eos_cut_empties_it():
    # the 2-gram (1, 2) recurs at index 0 and is followed by eos: HF drafts nothing and does not fall back to the 1-gram match at index 3
    assert lookup_candidates([1, 2, 9, 2, 5, 1, 2], D=3, n=2, eos=9) == []
    assert lookup_candidates([1, 2, 9, 2, 5, 1, 2], D=3, n=2, eos=None) == [9, 2, 5]
    assert lookup_candidates([4], 3, 2) == [] and lookup_candidates([4, 4], 3, 2) == [4]
    with pytest.raises(ValueError):
        lookup_candidates([1, 2], 0, 2)


def _trace_by_token(prompt, answer, D, n, eos, budget):
    """One token at a time: what a lookup loop that verifies drafts against the true answer emits per step."""
    seq, counts, e, done = list(prompt), [], 0, False
    while e < budget and not done:
        drafts = lookup_candidates(seq, D, n, eos)
        c = 0
        for j in range(len(drafts) + 1):          # row j: the current token (j = 0) or draft j
            if j > 0 and (drafts[j - 1] != answer[e - 1] or e >= budget):
                break
            if e >= budget:
                break
            tok = answer[e]
            seq.append(tok); e += 1; c += 1
            if eos is not None and tok == eos:
                done = True
                break
        counts.append(c)
    return counts


def test_trace_equals_token_by_token_restatement():
    rng = np.random.default_rng(7)
    multi = cut_eos = cut_budget = 0
    for i in range(300):
        vocab = int(rng.integers(4, 9))
        prompt = rng.integers(0, vocab, int(rng.integers(2, 30))).tolist()
        # a looping answer (copies a span of the prompt now and then) so that drafts get accepted
        answer = []
        while len(answer) < 48:
            if rng.random() < 0.6:
                src = prompt + answer
                s = int(rng.integers(0, len(src)))
                answer += src[s:s + int(rng.integers(1, 9))]
            else:
                answer.append(int(rng.integers(0, vocab)))
        eos = int(rng.integers(0, vocab)) if i % 3 else None
        D, n, budget = (1, 3, 7, 15)[i % 4], (1, 2, 3, 4)[(i // 4) % 4], int(rng.integers(1, 41))
        got = lookup_trace(prompt, answer, D, n, eos, budget)
        assert got == _trace_by_token(prompt, answer, D, n, eos, budget), (prompt, answer, D, n, eos, budget)
        want = answer[:budget]
        if eos is not None and eos in want:
            want = want[:want.index(eos) + 1]
        assert sum(got) == len(want) and all(1 <= c <= D + 1 for c in got)
        multi += any(c > 1 for c in got)
        cut_eos += eos is not None and want[-1] == eos and got[-1] > 1
        cut_budget += len(want) == budget and got[-1] > 1
    assert multi > 50 and cut_eos > 5 and cut_budget > 5, (multi, cut_eos, cut_budget)
    with pytest.raises(ValueError):
        lookup_trace([1, 2], [3], 3, 2, None, 5)


def test_abi_symbols_of_the_row_step():
    from video_llava_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "pgv.h")).read()
    lib = ctypes.CDLL(build.build())
    for name, nargs in (("pgv_kv_set_lookup", 3), ("pgv_kv_lookup", 1), ("pgv_llm_decode_rows", 8), ("pgv_llm_decode_lookup", 10), ("pgv_decode_attention_rows", 16)):
        assert re.search(r"\bint %s\s*\(" % name, header), f"pgv.h does not declare {name}"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, f"ctypes binding of {name}"
        assert hasattr(lib, name), f"libpgv.so does not export {name}"


def test_check_lookup_refusals():
    from video_llava_amd.generation import check_lookup
    assert check_lookup(0) == (0, 0) and check_lookup(None) == (0, 0) and check_lookup(3, 2, 8) == (3, 2) and check_lookup(15, 4, 4) == (15, 4)
    assert check_lookup(0, 2, 8, do_sample=True, beams=4, repetition_penalty=1.2) == (0, 0)          # off: combines with everything
    for kw, word in ((dict(do_sample=True), "do_sample"), (dict(beams=2), "beams"), (dict(samples_per_prompt=2), "samples_per_prompt"),
                     (dict(repetition_penalty=1.1), "repetition_penalty"), (dict(has_bans=True), "bans"), (dict(output_logprobs=True), "output_logprobs")):
        with pytest.raises(ValueError, match=f"`{word}` cannot be combined with `lookup`=3"):
            check_lookup(3, 2, 2, **kw)
    with pytest.raises(ValueError, match="exceed the 64"):
        check_lookup(3, 2, 17)
    for bad in (16, -1, 2.5, True):
        with pytest.raises(ValueError, match="`lookup`"):
            check_lookup(bad)
    for bad in (0, 5, True):
        with pytest.raises(ValueError, match="`lookup_ngram`"):
            check_lookup(3, bad)


def test_front_ends_take_the_flag_and_refuse_what_generate_refuses(capsys):
    import argparse
    import inspect
    from video_llava_amd import chat, inference
    from video_llava_amd.eval import _sharded
    for fn in (inference.video_chatgpt_infer, inference.video_chatgpt_infer_logprobs, chat.VideoChatGPTInterface.__init__):
        prm = inspect.signature(fn).parameters
        assert prm["lookup"].default == 0 and prm["lookup_ngram"].default == 2
    parse = lambda argv: _sharded.add_runtime_arguments(argparse.ArgumentParser()).parse_args(argv)
    ns = parse(["--lookup", "3", "--batch", "8"])
    assert _sharded.lookup_from_args(ns) == {"lookup": 3, "lookup_ngram": 2} and _sharded.lookup_from_args(parse([])) == {}
    assert _sharded.lookup_from_args(parse(["--lookup", "7", "--lookup_ngram", "4"])) == {"lookup": 7, "lookup_ngram": 4}
    for argv, word in ((["--lookup", "3", "--do_sample"], "--do_sample"), (["--lookup", "3", "--beams", "2"], "--beams"),
                       (["--lookup", "3", "--schedule", "refill"], "--schedule refill"), (["--lookup", "3", "--repetition_penalty", "1.2"], "--repetition_penalty"),
                       (["--lookup", "3", "--no_repeat_ngram", "2"], "--no_repeat_ngram"), (["--lookup", "7", "--batch", "9"], "rows exceed"),
                       (["--lookup", "16"], "`lookup`"), (["--lookup", "3", "--lookup_ngram", "5"], "`lookup_ngram`")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert word in capsys.readouterr().err, argv
    base = ["--model-name", "m", "--projection_path", "p"]
    a = chat.parse_args(base + ["--lookup", "5", "--lookup_ngram", "3"])
    assert (a.lookup, a.lookup_ngram, a.do_sample) == (5, 3, False) and chat.parse_args(base).lookup == 0
    for argv in (["--lookup", "5", "--do_sample"], ["--lookup", "16"]):
        with pytest.raises(SystemExit):
            chat.parse_args(base + argv)
    capsys.readouterr()
    with pytest.raises(ValueError, match="do_sample"):
        chat.VideoChatGPTInterface("m", "p", components=(None,) * 5, do_sample=True, lookup=3)


def test_decode_graph_key_carries_the_lookup_setting(tmp_path):
    """csrc/pick_params.h compiled on its own with g++: captured lookup steps and captured plain steps never share a key, nor do two (D, n)."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src = tmp_path / "key.cpp"
    src.write_text('''
#include <cstdio>
#include "pick_params.h"
int main() {
    const int F = AM_INC_POS | AM_RECORD;
    const PickParams p;
    const DecodeGraphKey plain = decode_graph_key(2, 7, F, 3, false, p);
    int bad = 0;
    bad += !(plain == decode_graph_key(2, 7, F, 3, false, p, 0, 0, 0, 0));
    bad += plain.lookup_D != 0 || plain.lookup_n != 0;
    bad += plain == decode_graph_key(2, 7, F, 3, false, p, 0, 0, 3, 2);
    bad += decode_graph_key(2, 7, F, 3, false, p, 0, 0, 3, 2) == decode_graph_key(2, 7, F, 3, false, p, 0, 0, 7, 2);
    bad += decode_graph_key(2, 7, F, 3, false, p, 0, 0, 3, 2) == decode_graph_key(2, 7, F, 3, false, p, 0, 0, 3, 3);
    bad += !(decode_graph_key(2, 7, F, 3, false, p, 0, 0, 3, 2) == decode_graph_key(2, 7, F, 3, false, p, 0, 0, 3, 2));
    std::printf("%d\\n", bad);
    return bad;
}
''')
    exe = tmp_path / "key"
    subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "video_llava_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0", (r.stdout, r.stderr)


def test_row_form_of_the_split_kernel_passes_the_lowering_check():
    """The row map is a template flag of the two decode attention kernels; the fence-free merge of the context-split one must lower the same way
    in the row form (build.check_isa raises otherwise).  Its register budget is held by test_host_cpu.py::test_no_kernel_spills_to_scratch, whose
    name match covers every instantiation."""
    from video_llava_amd import build
    found = {k: v for k, v in build.check_isa().items() if k[0] != "vit_attn"}
    assert len(found) == 6 and all(v["instantiations"] == 2 and v["atomics"] == 1 and v["cache_maintenance"] == 0 for v in found.values()), found
