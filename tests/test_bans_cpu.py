"""Host side of generate(bans=...): the rules of video_llava_amd/logit_bans.py against the installed HF processors, the validation, the refusals,
the runner flags and the decode-graph key.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from bans_hf import hf_banned
from video_llava_amd import generation as G
from video_llava_amd.logit_bans import LogitBans, banned_ids, check_bans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(bans, ids, prompt_len, eos, V):
    """(ours, HF's): ours from the CHECKED record (its [eos] filter), HF's from the raw one (HF's own filter)."""
    return banned_ids(bans.check(V, eos), ids, prompt_len, eos, V), hf_banned(bans, ids, prompt_len, eos, V)


def test_banned_ids_equal_hf_on_seeded_cases():
    """>= 200 seeded cases: V in {50, 1000}, L in 0..200 over an 8-symbol alphabet (n-grams repeat), n in 1..5, bad words of 1..5 ids -- one longer
    than the sequence, one equal to [eos] --, prompt_len in 0..L.  At least half of the n-gram cases ban something through the n-gram rule."""
    rng = np.random.default_rng(20)
    cases = ngram_nonempty = 0
    for case in range(240):
        V = (50, 1000)[case % 2]
        L = int(rng.integers(0, 201)) if case % 6 else int(rng.integers(0, 6))
        alphabet = rng.choice(np.arange(3, V), 8, replace=False)
        ids = [int(t) for t in rng.choice(alphabet, L)]
        n = int(rng.integers(1, 6))
        eos = 2 if case % 5 else -1
        prompt_len = int(rng.integers(0, L + 1))
        words = [[int(t) for t in rng.choice(alphabet, int(rng.integers(1, 6)))] for _ in range(int(rng.integers(1, 5)))]
        if L >= 2:
            k = int(rng.integers(1, min(4, L) + 1))
            words.append(ids[L - k:] + [int(rng.choice(alphabet))])              # a word whose prefix IS the end of the sequence
        words.append([int(t) for t in rng.choice(alphabet, min(L + 2, 16))])    # longer than the sequence (or the limit): skipped
        if eos >= 0:
            words.append([eos])                                                  # HF drops it
        bans = LogitBans(no_repeat_ngram=n, bad_words=words, suppress=[int(t) for t in rng.integers(0, V, 3)],
                         begin_suppress=[int(t) for t in rng.integers(0, V, 2)], min_length=int(rng.integers(0, 2 * L + 2)),
                         min_new_tokens=int(rng.integers(0, 8)))
        ours, hf = _both(bans, ids, prompt_len, eos, V)
        assert ours == hf, (case, sorted(ours ^ hf))
        only_ngram = LogitBans(no_repeat_ngram=n)
        o2, h2 = _both(only_ngram, ids, prompt_len, eos, V)
        assert o2 == h2, (case, "ngram alone")
        cases += 1
        ngram_nonempty += bool(o2)
    assert cases >= 200 and 2 * ngram_nonempty >= cases, (cases, ngram_nonempty)


def test_named_edge_cases_equal_hf():
    V, eos = 50, 2
    a, b, c = 5, 6, 7
    for n in (2, 3, 4):
        seq = [a, b, c, a, b, c, a, b, c]
        for L in (n - 1, n):                                                    # L == n - 1: nothing; L == n: the first full window exists, the suffix never bans its own successor
            ours, hf = _both(LogitBans(no_repeat_ngram=n), seq[:L], 0, eos, V)
            assert ours == hf and (L == n - 1) <= (ours == set()), (n, L, ours, hf)
    # [a, b, a, b] with n = 2: the suffix is [b]; the only window that starts with b is j = 1 and bans a -- the last window, j = 2, ends the
    # sequence and starts with a
    ours, hf = _both(LogitBans(no_repeat_ngram=2), [a, b, a, b], 0, eos, V)
    assert ours == hf == {a}
    ours, hf = _both(LogitBans(no_repeat_ngram=3), [a, b, c, a, b], 0, eos, V)
    assert ours == hf == {c}
    ours, hf = _both(LogitBans(no_repeat_ngram=3), [a, a, a], 0, eos, V)       # the last window [a, a, a] ends the sequence and matches the suffix [a, a]
    assert ours == hf == {a}
    # n = 1: every id of the sequence
    ours, hf = _both(LogitBans(no_repeat_ngram=1), [a, b, a], 0, eos, V)
    assert ours == hf == {a, b}
    ours, hf = _both(LogitBans(no_repeat_ngram=1), [], 0, eos, V)
    assert ours == hf == set()
    # begin_suppress: only at L == prompt_len
    for L, want in ((3, {9, 11}), (4, set())):
        ours, hf = _both(LogitBans(begin_suppress=[9, 11]), [a, b, c, a][:L], 3, eos, V)
        assert ours == hf == want
    # the length rules, and a run without EOS makes both empty
    for bans, ids, plen, want in ((LogitBans(min_length=4), [a, b, c], 1, {eos}), (LogitBans(min_length=3), [a, b, c], 1, set()),
                                  (LogitBans(min_new_tokens=2), [a, b, c], 2, {eos}), (LogitBans(min_new_tokens=2), [a, b, c], 1, set())):
        ours, hf = _both(bans, ids, plen, eos, V)
        assert ours == hf == want, bans
        assert banned_ids(bans, ids, plen, -1, V) == set() == hf_banned(bans, ids, plen, -1, V)
    # bad words: one id always, m ids only behind their prefix, longer than the context never; suppress has no EOS filter
    ours, hf = _both(LogitBans(bad_words=[[a], [b, c], [a, b, c, a, b]], suppress=[eos]), [c, a, b], 0, eos, V)
    assert ours == hf == {a, c, eos}


def test_validation_messages_and_eos_filter():
    with pytest.raises(ValueError, match="`ngram_size` has to be a strictly positive integer"):
        LogitBans(no_repeat_ngram=-1).check(100)
    with pytest.raises(ValueError, match="`ngram_size` has to be a strictly positive integer"):
        LogitBans(no_repeat_ngram=2.5).check(100)
    with pytest.raises(ValueError, match="`bad_words_ids` has to be a list of lists"):
        LogitBans(bad_words=[3, 4]).check(100)
    with pytest.raises(ValueError, match="`bad_words_ids` has to be a non-empty list"):
        LogitBans(bad_words="ab").check(100)
    with pytest.raises(ValueError, match="has to be a list of positive integers"):
        LogitBans(bad_words=[[3, -4]]).check(100)
    with pytest.raises(ValueError, match="has to be a list of positive integers"):
        LogitBans(bad_words=[[]]).check(100)
    with pytest.raises(ValueError, match=r"vocabulary size is 100, but the following tokens were being biased: \[100\]"):
        LogitBans(bad_words=[[3, 100]]).check(100)
    with pytest.raises(ValueError, match="`suppress` lists the tokens"):
        LogitBans(suppress=[100]).check(100)
    with pytest.raises(ValueError, match="`min_new_tokens` has to be a positive integer"):
        LogitBans(min_new_tokens=-1).check(100)
    with pytest.raises(ValueError, match="`min_length` has to be a non-negative integer"):
        LogitBans(min_length=-2).check(100)
    with pytest.raises(ValueError, match="257 words exceed the limit of 256"):
        LogitBans(bad_words=[[i % 90, 1] for i in range(257)]).check(100)
    with pytest.raises(ValueError, match="a word of 17 ids exceeds the limit of 16"):
        LogitBans(bad_words=[[1] * 17]).check(100)
    with pytest.raises(ValueError, match="1025 ids in total, the limit is 1024"):
        LogitBans(suppress=[1] * 1025).check(100)
    with pytest.raises(ValueError, match="HF's `no_repeat_ngram_size` is `no_repeat_ngram` here"):
        LogitBans.coerce({"no_repeat_ngram_size": 3})
    # HF's EOS filter: a bad word equal to [eos] is dropped, nothing else
    b = LogitBans(bad_words=[[7], [2], [2, 3], [3, 2]], suppress=[2]).check(100, eos=2)
    assert b.bad_words == ((7,), (2, 3), (3, 2)) and b.suppress == (2,)
    assert LogitBans(bad_words=[[2]]).check(100, eos=-1).bad_words == ((2,),)
    assert LogitBans.coerce({"no_repeat_ngram": 3, "suppress": [4]}) == LogitBans(no_repeat_ngram=3, suppress=[4])


def test_neutral():
    assert LogitBans().neutral and LogitBans.coerce(None).neutral and LogitBans().check(10).neutral
    for kw in (dict(no_repeat_ngram=2), dict(bad_words=[[1]]), dict(suppress=[1]), dict(begin_suppress=[1]), dict(min_length=1), dict(min_new_tokens=1)):
        assert not LogitBans(**kw).neutral, kw
    # only length rules in a run without EOS: nothing is asked of the device
    assert LogitBans(min_length=3, min_new_tokens=2).effective_neutral(-1) and not LogitBans(min_length=3).effective_neutral(2)
    assert not LogitBans(min_length=3, suppress=[1]).effective_neutral(-1)
    # a bad word list that is only [eos] becomes neutral once checked
    assert LogitBans(bad_words=[[2]]).check(10, eos=2).neutral


def test_bans_are_refused_under_beams_and_named_in_the_refusals():
    with pytest.raises(ValueError, match=r"`bans` cannot be combined with `beams`=2"):
        check_bans(LogitBans(no_repeat_ngram=3), 100, 2, beams=2)
    assert check_bans(None, 100, 2, beams=2).neutral and check_bans(LogitBans(), 100, 2, beams=4).neutral
    assert check_bans({"min_new_tokens": 3}, 100, 2, beams=1).min_new_tokens == 3
    with pytest.raises(ValueError, match="ngram_size"):
        check_bans({"no_repeat_ngram": -3}, 100, 2)
    # the four HF names stay refused, and the message now names this package's keyword
    for name, bad in (("no_repeat_ngram_size", 3), ("bad_words_ids", [[5]]), ("min_length", 4), ("min_new_tokens", 2)):
        with pytest.raises(ValueError, match=name) as e:
            G.check_generate_kwargs({name: bad})
        assert "`bans`" in str(e.value) and G.BANS_HINT[name] in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="min_p") as e:
        G.check_generate_kwargs({"min_p": 0.1})
    assert "`bans`" not in str(e.value)
    # suppress_tokens / begin_suppress_tokens are NOT refused: what existing callers get does not change
    assert "suppress_tokens" not in G.REFUSED and "begin_suppress_tokens" not in G.REFUSED
    G.check_generate_kwargs({"suppress_tokens": [3], "begin_suppress_tokens": [4]})


def test_generate_and_continuous_take_bans():
    import inspect
    from video_llava_amd import continuous, inference
    from video_llava_amd.model.video_chatgpt import VideoChatGPTLlamaForCausalLM as M
    assert inspect.signature(M.generate).parameters["bans"].default is None
    assert inspect.signature(M.prefill).parameters["bans"].default is None
    assert inspect.signature(continuous.generate_continuous).parameters["bans"].default is None
    assert inspect.signature(inference.video_chatgpt_infer).parameters["bans"].default is None
    for meth in ("set_bans", "ids_peek"):
        assert callable(getattr(M, meth))


def test_runner_flags_parse_and_default_to_off():
    import argparse
    from video_llava_amd.eval._sharded import add_runtime_arguments, bans_from_args
    parser = add_runtime_arguments(argparse.ArgumentParser())
    ns, _ = parser.parse_known_args([])
    assert ns.no_repeat_ngram == 0 and ns.min_new_tokens == 0 and tuple(ns.suppress_tokens) == () and bans_from_args(ns) == {}
    ns, _ = parser.parse_known_args(["--no_repeat_ngram", "3", "--min_new_tokens", "8", "--suppress_tokens", "5,17"])
    assert bans_from_args(ns) == {"bans": LogitBans(no_repeat_ngram=3, min_new_tokens=8, suppress=(5, 17))}
    for bad in (["--suppress_tokens", "5,x"], ["--suppress_tokens", "-3"], ["--beams", "2", "--no_repeat_ngram", "3"], ["--no_repeat_ngram", "-1"]):
        with pytest.raises((SystemExit, ValueError)):
            parser.parse_known_args(bad)


def test_binding_and_header_carry_the_ban_entry_points():
    import ctypes
    import re
    from video_llava_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "pgv.h")).read()
    lib = ctypes.CDLL(build.build())
    for name, nargs in (("pgv_kv_set_bans", 2), ("pgv_ban_logits", 11), ("pgv_kv_ids_peek", 6)):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert len(_lib.PROTOTYPES[name][1]) == nargs and hasattr(lib, name), name
    assert "logit_ban.hip" in build.sources_present()
    for macro, v in (("PGV_BAN_MAX_IDS", _lib.BAN_MAX_IDS), ("PGV_BAN_MAX_WORDS", _lib.BAN_MAX_WORDS), ("PGV_BAN_MAX_WORD_LEN", _lib.BAN_MAX_WORD_LEN)):
        assert re.search(r"#define %s %d\b" % (macro, v), header), macro
    cfg = _lib.BanConfig.from_bans(LogitBans(no_repeat_ngram=3, bad_words=((4, 5), (6,)), suppress=(7,), min_new_tokens=2).check(100), 2)
    assert (cfg.no_repeat_ngram, cfg.n_bad_words, cfg.n_suppress, cfg.n_begin_suppress, cfg.min_length, cfg.min_new_tokens, cfg.eos_id) == (3, 2, 1, 0, 0, 2, 2)
    assert [cfg.h_bad_words[i] for i in range(3)] == [4, 5, 6] and [cfg.h_bad_word_lens[i] for i in range(2)] == [2, 1]


def test_pick_params_compiles_alone_and_the_key_carries_the_ban_generation(tmp_path):
    """csrc/pick_params.h still needs no HIP header, and two decode-graph keys that differ only in the ban generation compare unequal (a field left
    out of the comparison would replay a graph that bakes in the lists of another configuration)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    prog = r"""#include <cstdio>
#include "pick_params.h"
int main() {
    const PickParams p{0.7f, 50, 0.9f, 1.2f, false};
    const int F = AM_INC_POS | AM_RECORD | AM_SAMPLE;
    const DecodeGraphKey off = decode_graph_key(2, 7, F, 3, false, p), a = decode_graph_key(2, 7, F, 3, false, p, 0, 1), b = decode_graph_key(2, 7, F, 3, false, p, 0, 2);
    int bad = 0;
    bad |= !(off.bans == 0 && a.bans == 1 && b.bans == 2 && DecodeGraphKey{}.bans == 0);
    bad |= (off == a) || (a == b) || !(a == decode_graph_key(2, 7, F, 3, false, p, 0, 1));
    bad |= !(off == decode_graph_key(2, 7, F, 3, false, p, 0, 0));
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
