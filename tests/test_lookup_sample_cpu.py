"""CPU: the host side of sampled prompt-lookup decoding -- generate(lookup=D, lookup_sample=True): check_lookup's two forms, the new C entry's
declaration, binding and export, the front ends' flag, and the key of the captured graphs.  The device side is tests/test_gpu_lookup_sample.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_lookup_takes_the_sampled_form():
    from video_llava_amd.generation import check_lookup
    assert check_lookup(3, 2, 2, do_sample=True, lookup_sample=True) == (3, 2)
    assert check_lookup(15, 4, 4, do_sample=True, lookup_sample=True) == (15, 4)
    for kw, word in ((dict(beams=2), "beams"), (dict(samples_per_prompt=2), "samples_per_prompt"), (dict(repetition_penalty=1.1), "repetition_penalty"),
                     (dict(has_bans=True), "bans"), (dict(output_logprobs=True), "output_logprobs")):
        with pytest.raises(ValueError, match=f"`{word}` cannot be combined with `lookup`=3"):
            check_lookup(3, 2, 2, do_sample=True, lookup_sample=True, **kw)
    with pytest.raises(ValueError, match="exceed the 64"):
        check_lookup(3, 2, 17, do_sample=True, lookup_sample=True)
    with pytest.raises(ValueError, match="`lookup_sample` needs `do_sample`"):
        check_lookup(3, 2, 2, do_sample=False, lookup_sample=True)
    for off in (0, None):
        with pytest.raises(ValueError, match="`lookup_sample` needs `lookup`"):
            check_lookup(off, 2, 2, do_sample=True, lookup_sample=True)
    for bad in (16, -1, True):
        with pytest.raises(ValueError, match="`lookup`"):
            check_lookup(bad, 2, 1, do_sample=True, lookup_sample=True)
    # without the flag nothing moved: do_sample is refused, and the message now names the way out
    with pytest.raises(ValueError, match="`do_sample` cannot be combined with `lookup`=3") as e:
        check_lookup(3, 2, 2, do_sample=True)
    assert "lookup_sample" in str(e.value) and "speculative sampling is not implemented" in str(e.value)
    assert check_lookup(3, 2, 8) == (3, 2) and check_lookup(0, 2, 8, do_sample=True) == (0, 0)


def test_abi_symbol_of_the_sampled_lookup_entry():
    from video_llava_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "pgv.h")).read()
    name = "pgv_llm_decode_lookup_sample"
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header)
    assert m, f"pgv.h does not declare {name}"
    assert len(m.group(1).split(",")) == 15
    assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == 15, f"ctypes binding of {name}"
    args = _lib.PROTOTYPES[name][1]
    assert args[8] is ctypes.c_float and args[9] is ctypes.c_int and args[11] is ctypes.c_int          # temperature, top_k, u_rows
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, name), f"libpgv.so does not export {name}"
    assert "u[h_u_base[b] + e + j][b]" in header, "pgv.h states the uniform indexing rule"


def test_front_ends_take_lookup_sample(capsys):
    import argparse
    import inspect
    from video_llava_amd import chat, inference
    from video_llava_amd.eval import _sharded
    from video_llava_amd.model.video_chatgpt import VideoChatGPTLlamaForCausalLM
    for fn in (inference.video_chatgpt_infer, chat.VideoChatGPTInterface.__init__, VideoChatGPTLlamaForCausalLM.generate):
        assert inspect.signature(fn).parameters["lookup_sample"].default is False
    assert list(inspect.signature(VideoChatGPTLlamaForCausalLM.decode_lookup_sample).parameters) == [
        "self", "kv", "first", "steps", "eos_id", "budget", "u_base", "temperature", "top_k", "u"]
    parse = lambda argv: _sharded.add_runtime_arguments(argparse.ArgumentParser()).parse_args(argv)
    ns = parse(["--lookup", "3", "--do_sample", "--lookup_sample"])
    assert _sharded.lookup_from_args(ns) == {"lookup": 3, "lookup_ngram": 2, "lookup_sample": True}
    assert _sharded.lookup_from_args(parse(["--lookup", "3"])) == {"lookup": 3, "lookup_ngram": 2}
    for argv, word in ((["--lookup", "3", "--lookup_sample"], "--lookup_sample"), (["--do_sample", "--lookup_sample"], "--lookup_sample"),
                       (["--lookup", "3", "--do_sample"], "--lookup 3 cannot be combined with --do_sample (a sampled token has no draft to verify)"),
                       (["--lookup", "3", "--do_sample", "--lookup_sample", "--repetition_penalty", "1.2"], "--repetition_penalty"),
                       (["--lookup", "3", "--do_sample", "--lookup_sample", "--no_repeat_ngram", "2"], "--no_repeat_ngram"),
                       (["--lookup", "3", "--do_sample", "--lookup_sample", "--schedule", "refill"], "--schedule refill")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert word in capsys.readouterr().err, argv
    base = ["--model-name", "m", "--projection_path", "p"]
    a = chat.parse_args(base + ["--lookup", "3", "--do_sample", "--lookup_sample"])
    assert (a.lookup, a.do_sample, a.lookup_sample) == (3, True, True) and chat.parse_args(base).lookup_sample is False
    for argv, word in ((["--lookup", "3", "--lookup_sample"], "--lookup_sample"), (["--do_sample", "--lookup_sample"], "--lookup_sample"),
                       (["--lookup", "5", "--do_sample"], "--lookup 5 cannot be combined with --do_sample (a sampled token has no draft to verify)")):
        with pytest.raises(SystemExit):
            chat.parse_args(base + argv)
        assert word in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="lookup_sample"):
        chat.VideoChatGPTInterface("m", "p", components=(None,) * 5, do_sample=False, lookup=3, lookup_sample=True)


def test_decode_graph_key_separates_sampled_lookup_steps(tmp_path):
    """csrc/pick_params.h compiled on its own with g++: the key of a captured sampled lookup step differs from the greedy lookup key and from the
    plain sampled key at the same parameters, and between two temperatures, top_k, top_p, filter values, D and n."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src = tmp_path / "key.cpp"
    src.write_text('''
#include <cstdio>
#include "pick_params.h"
int main() {
    const int G = AM_INC_POS | AM_RECORD, S = G | AM_SAMPLE;
    PickParams p; p.temperature = 0.2f; p.top_k = 50;
    PickParams hot = p; hot.temperature = 0.7f;
    PickParams k5 = p; k5.top_k = 5;
    PickParams nucleus = p; nucleus.top_p = 0.9f;
    PickParams minp = p; minp.min_p = 0.05f;
    const DecodeGraphKey look = decode_graph_key(2, 7, S, 3, false, p, 0, 0, 3, 2);
    int bad = 0;
    bad += !(look == decode_graph_key(2, 7, S, 3, false, p, 0, 0, 3, 2));
    bad += look == decode_graph_key(2, 7, G, 3, false, p, 0, 0, 3, 2);            // the greedy lookup step, whatever run is in flight
    bad += look == decode_graph_key(2, 7, S, 3, false, p);                       // the plain sampled step
    bad += look == decode_graph_key(2, 7, S, 3, false, hot, 0, 0, 3, 2);
    bad += look == decode_graph_key(2, 7, S, 3, false, k5, 0, 0, 3, 2);
    bad += look == decode_graph_key(2, 7, S, 3, false, nucleus, 0, 0, 3, 2);
    bad += look == decode_graph_key(2, 7, S, 3, false, minp, 0, 0, 3, 2);
    bad += look == decode_graph_key(2, 7, S, 3, false, p, 0, 0, 7, 2);
    bad += look == decode_graph_key(2, 7, S, 3, false, p, 0, 0, 3, 3);
    bad += !(look.pick == p) || look.lookup_D != 3 || look.lookup_n != 2 || !(look.flags & AM_SAMPLE);
    std::printf("%d\\n", bad);
    return bad;
}
''')
    exe = tmp_path / "key"
    subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "video_llava_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0", (r.stdout, r.stderr)
