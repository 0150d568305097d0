"""Host side of generate(filters=...): the rules of video_llava_amd/sample_filters.py against the installed HF warper classes, the record, its
precedence over a generation config, the refusals, the runner flags and the decode-graph key.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from filters_hf import FAMILIES, HARSH, chain_kept, filters_of, hf_front, hf_kept
from video_llava_amd import generation as G
from video_llava_amd.sample_filters import SampleFilters, check_filters, filter_chain, resolve_filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_chain_equals_hf_warper_classes_in_fp64():
    """Kept set, row for row, against MinP / Typical / Epsilon / Eta LogitsWarper run in fp64 in HF's order behind Temperature / TopK / TopP:
    V = 32003 / 515 / 50, the eight families of the kernel test plus three harsh ones, logits randn * (1.5 + r % 3).  At least a third of the rows
    with typical_p on lose their largest logit: otherwise "the top of the CURRENT survivors" in the stages behind it would not be exercised."""
    rows = typical_rows = typical_lost_top = 0
    # most rows at the real vocabulary: that is where the typical band sits below the maximum (at V = 50 behind a sharp temperature it rarely does)
    for V, B, rounds in ((32003, 8, 3), (515, 4, 3), (50, 4, 3)):
        g = torch.Generator().manual_seed(V)
        for fi, family in enumerate(FAMILIES + HARSH):
            for r in range(rounds):
                scores = torch.randn(B, V, generator=g, dtype=torch.float64) * (1.5 + r % 3)
                ours, hf = chain_kept(scores, family), hf_kept(scores, family)
                for b in range(B):
                    assert (ours[b] == hf[b]).all(), (V, fi, r, b, int(ours[b].sum()), int(hf[b].sum()), np.flatnonzero(ours[b] != hf[b])[:8])
                    assert ours[b].any()
                rows += B
                if family[4] < 1.0:
                    typical_rows += B
                    top = scores.argmax(dim=1).numpy()
                    typical_lost_top += int((~ours[np.arange(B), top]).sum())
    assert rows >= 500 and typical_rows >= 300
    assert 3 * typical_lost_top >= typical_rows, (typical_lost_top, typical_rows)


def test_filter_chain_named_edges():
    y = np.log(np.array([0.5, 0.2, 0.2, 0.05, 0.05]))
    # min_p = 1: exactly the maxima, tied ones together
    assert filter_chain(np.log(np.array([0.3, 0.3, 0.3, 0.1])), SampleFilters(min_p=1.0)).tolist() == [True, True, True, False]
    assert filter_chain(y, SampleFilters(min_p=0.4)).tolist() == [True, True, True, False, False]
    # epsilon: a floor on the probability, the top always stays
    assert filter_chain(y, SampleFilters(epsilon_cutoff=0.1)).tolist() == [True, True, True, False, False]
    assert filter_chain(y, SampleFilters(epsilon_cutoff=0.999)).tolist() == [True, False, False, False, False]
    # typical: H = 1.289; -ln p = 0.69, 1.61, 1.61, 3.0, 3.0 -> d = 0.60, 0.32, 0.32, 1.71, 1.71: the two 0.2 entries are nearest, the maximum is not
    assert filter_chain(y, SampleFilters(typical_p=0.05)).tolist() == [False, True, True, False, False]
    assert filter_chain(y, SampleFilters(typical_p=0.45)).tolist() == [True, True, True, False, False]
    # ... and epsilon behind it keeps the top of what is LEFT, not the row's maximum
    assert filter_chain(y, SampleFilters(typical_p=0.05, epsilon_cutoff=0.9)).tolist() == [False, True, True, False, False]
    # removed entries stay removed; an empty row stays empty; the neutral record keeps every finite entry
    z = y.copy()
    z[0] = -np.inf
    assert not filter_chain(z, SampleFilters(min_p=0.1))[0]
    assert not filter_chain(np.full(4, -np.inf), SampleFilters(min_p=0.1, typical_p=0.5)).any()
    assert filter_chain(z, SampleFilters()).tolist() == [False, True, True, True, True]
    # the perturbations move the boundaries: p = 0.2 against min_p * p_max = 0.2
    assert not filter_chain(y, SampleFilters(min_p=0.4), rel=1e-3)[1] and filter_chain(y, SampleFilters(min_p=0.4), rel=-1e-3)[1]


def test_record_checks_wording_and_neutrality():
    assert SampleFilters().neutral and SampleFilters.coerce(None).neutral and SampleFilters(min_p=0.0).neutral and SampleFilters().check().neutral
    for kw in (dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)):
        assert not SampleFilters(**kw).neutral and SampleFilters(**kw).check() == SampleFilters(**kw), kw
    assert SampleFilters.coerce({"min_p": 0.1, "eta_cutoff": 2e-3}) == SampleFilters(min_p=0.1, eta_cutoff=2e-3)
    for bad in (-0.1, 1.5, "a"):
        with pytest.raises(ValueError, match=r"`min_p` has to be a float in the \[0, 1\] interval, but is " + str(bad)):
            SampleFilters(min_p=bad).check()
    for bad in (0.0, 1.2, -1.0, None):
        with pytest.raises(ValueError, match=r"`typical_p` has to be a float > 0 and < 1, but is " + str(bad)):
            SampleFilters(typical_p=bad).check()
    for name in ("epsilon_cutoff", "eta_cutoff"):
        for bad in (-1e-3, 1.0, 3.0):
            with pytest.raises(ValueError, match=r"`%s` has to be a float > 0 and < 1, but is %s" % (name, bad)):
                SampleFilters(**{name: bad}).check()
    SampleFilters(min_p=1.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.999).check()
    with pytest.raises(ValueError, match="`filters` has no field `top_h`"):
        SampleFilters.coerce({"top_h": 0.3})
    with pytest.raises(ValueError, match="has to be a SampleFilters, a dict of its fields or None"):
        SampleFilters.coerce(0.1)


def test_precedence_over_a_generation_config():
    cfg = G.GenerationDefaults(min_p=0.07, typical_p=0.8, temperature=0.5)
    # no `filters`: neutral (and the config's fields are refused by check_generate_kwargs, as before)
    assert resolve_filters(None, cfg).neutral
    with pytest.raises(ValueError, match="generation_config field `min_p`=0.07"):
        G.check_generate_kwargs({}, cfg)
    # with `filters`: the call's fields win, the rest comes from the config, then neutral
    G.check_generate_kwargs({}, cfg, filters_given=True)
    assert resolve_filters({}, cfg) == SampleFilters(min_p=0.07, typical_p=0.8)
    assert resolve_filters(SampleFilters(), cfg) == SampleFilters(min_p=0.07, typical_p=0.8)
    assert resolve_filters({"min_p": 0.2}, cfg) == SampleFilters(min_p=0.2, typical_p=0.8)
    assert resolve_filters(SampleFilters(eta_cutoff=1e-3), {"min_p": 0.07}) == SampleFilters(min_p=0.07, eta_cutoff=1e-3)
    assert resolve_filters({"typical_p": 1.0, "min_p": None}, cfg).neutral          # a dict can give the neutral value
    assert resolve_filters({"epsilon_cutoff": 1e-3}, None) == SampleFilters(epsilon_cutoff=1e-3)
    with pytest.raises(ValueError, match="`typical_p` has to be a float > 0 and < 1, but is 1.5"):
        resolve_filters({}, {"typical_p": 1.5})
    # the other refused fields of a config stay refused, and the four names as ARGUMENTS of the call too
    with pytest.raises(ValueError, match="penalty_alpha"):
        G.check_generate_kwargs({}, G.GenerationDefaults(min_p=0.07, penalty_alpha=0.6), filters_given=True)
    with pytest.raises(ValueError, match="argument `min_p`"):
        G.check_generate_kwargs({"min_p": 0.1}, cfg, filters_given=True)


def test_refusals_name_filters():
    for name, bad in (("min_p", 0.1), ("typical_p", 0.9), ("epsilon_cutoff", 1e-3), ("eta_cutoff", 1e-3)):
        assert name in G.REFUSED
        with pytest.raises(ValueError, match=name) as e:
            G.check_generate_kwargs({name: bad})
        assert "`filters`" in str(e.value) and f"SampleFilters({name}=...)" in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="penalty_alpha") as e:
        G.check_generate_kwargs({"penalty_alpha": 0.6})
    assert "`filters`" not in str(e.value)
    with pytest.raises(ValueError, match=r"`filters` cannot be combined with `beams`=2"):
        check_filters(SampleFilters(min_p=0.1), None, beams=2)
    assert check_filters(None, None, beams=2).neutral and check_filters(SampleFilters(), None, beams=4).neutral


def _deviceless_model():
    import torch.nn as nn
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM
    m = object.__new__(VideoChatGPTLlamaForCausalLM)
    nn.Module.__init__(m)
    m.config = VideoChatGPTConfig()
    return m


def test_generate_checks_filters_before_it_touches_the_device():
    m = _deviceless_model()
    with pytest.raises(ValueError, match=r"`filters` cannot be combined with `beams`=2"):
        m.generate([[1, 2, 3]], filters=SampleFilters(min_p=0.1), beams=2)
    with pytest.raises(ValueError, match=r"`min_p` has to be a float in the \[0, 1\] interval, but is 1.5"):
        m.generate([[1, 2, 3]], do_sample=True, filters={"min_p": 1.5})
    with pytest.raises(ValueError, match=r"`eta_cutoff` has to be a float > 0 and < 1, but is 1.0"):
        m.generate([[1, 2, 3]], do_sample=True, filters=SampleFilters(eta_cutoff=1.0))
    with pytest.raises(ValueError, match="`filters` has no field `min_tokens_to_keep`"):
        m.generate([[1, 2, 3]], do_sample=True, filters={"min_tokens_to_keep": 2})
    with pytest.raises(ValueError, match="argument `typical_p`=0.9 is not implemented"):
        m.generate([[1, 2, 3]], do_sample=True, typical_p=0.9)


def test_entry_points_take_the_keyword():
    import inspect
    from video_llava_amd import continuous, inference
    from video_llava_amd.model.video_chatgpt import VideoChatGPTLlamaForCausalLM as M
    assert inspect.signature(M.generate).parameters["filters"].default is None
    assert inspect.signature(M.prefill_slots).parameters["filters"].default is None
    assert inspect.signature(continuous.generate_continuous).parameters["filters"].default is None
    assert inspect.signature(inference.video_chatgpt_infer).parameters["filters"].default is None
    assert callable(M.set_filters)


def test_runner_flags_parse_and_default_to_off():
    import argparse
    from video_llava_amd.eval._sharded import add_runtime_arguments, filters_from_args
    parser = add_runtime_arguments(argparse.ArgumentParser())
    ns, _ = parser.parse_known_args([])
    assert ns.min_p is None and ns.typical_p is None and ns.epsilon_cutoff is None and ns.eta_cutoff is None and filters_from_args(ns) == {}
    ns, _ = parser.parse_known_args(["--do_sample", "--min_p", "0.1"])
    assert filters_from_args(ns) == {"filters": {"min_p": 0.1}}
    ns, _ = parser.parse_known_args(["--do_sample", "--schedule", "refill", "--samples_per_prompt", "2", "--typical_p", "0.9", "--epsilon_cutoff", "3e-4",
                                     "--eta_cutoff", "2e-3"])
    assert filters_from_args(ns) == {"filters": {"typical_p": 0.9, "epsilon_cutoff": 3e-4, "eta_cutoff": 2e-3}}
    for bad in (["--min_p", "0.1"], ["--do_sample", "--min_p", "1.5"], ["--do_sample", "--typical_p", "0"], ["--do_sample", "--eta_cutoff", "1"],
                ["--beams", "2", "--min_p", "0.1"], ["--do_sample", "--min_p", "x"]):
        with pytest.raises((SystemExit, ValueError)):
            parser.parse_known_args(bad)


def test_binding_and_header_carry_the_filter_entry_points():
    import ctypes
    import re
    from video_llava_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "pgv.h")).read()
    lib = ctypes.CDLL(build.build())
    for name, nargs in (("pgv_kv_set_filters", 2), ("pgv_sample_logits_filtered", 20)):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert len(_lib.PROTOTYPES[name][1]) == nargs and hasattr(lib, name), name
    assert re.search(r"typedef struct pgv_filter_config \{ float min_p, typical_p, epsilon_cutoff, eta_cutoff; \}", header)
    cfg = _lib.FilterConfig.from_filters(SampleFilters(typical_p=0.5, eta_cutoff=0.25))
    assert (cfg.min_p, cfg.typical_p, cfg.epsilon_cutoff, cfg.eta_cutoff) == (0.0, 0.5, 0.0, 0.25) and ctypes.sizeof(cfg) == 16


def test_pick_params_carry_the_filters_in_the_graph_key(tmp_path):
    """csrc/pick_params.h, stand-alone with g++ (and a second time under ASan + UBSan where g++ has the runtimes): the four fields default to their
    neutral values behind `greedy`, each of them alone makes two decode-graph keys unequal -- a field left out of the comparison would replay a graph
    that bakes in another filter -- and a run without AM_SAMPLE ignores them."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    csrc = os.path.join(ROOT, "video_llava_amd", "csrc")
    prog = r"""#include <cstdio>
#include "pick_params.h"
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad = 1; } } while (0)
int main() {
    const PickParams d;
    EXPECT(d.min_p == 0.f && d.typical_p == 1.f && d.epsilon == 0.f && d.eta == 0.f && !d.filtered());
    const PickParams p{0.7f, 50, 0.9f, 1.2f, false};            // the brace initialisers of before still mean what they meant
    EXPECT(p.min_p == 0.f && p.typical_p == 1.f && p.epsilon == 0.f && p.eta == 0.f && !p.filtered());
    EXPECT(!pick_greedy(1.3f).filtered());
    const int F = AM_INC_POS | AM_RECORD | AM_SAMPLE;
    const DecodeGraphKey k = decode_graph_key(2, 7, F, 3, false, p);
    PickParams q[4] = {p, p, p, p};
    q[0].min_p = 0.05f; q[1].typical_p = 0.9f; q[2].epsilon = 3e-4f; q[3].eta = 2e-3f;
    int differ = 0;
    for (int i = 0; i < 4; ++i) {
        EXPECT(q[i].filtered() && !(q[i] == p));
        differ += !(k == decode_graph_key(2, 7, F, 3, false, q[i]));
        EXPECT(decode_graph_key(2, 7, F, 3, false, q[i]) == decode_graph_key(2, 7, F, 3, false, q[i]));
        for (int j = 0; j < i; ++j) EXPECT(!(decode_graph_key(2, 7, F, 3, false, q[i]) == decode_graph_key(2, 7, F, 3, false, q[j])));
        PickParams g = q[i];
        g.greedy = true;
        EXPECT(!g.filtered());                                   // a greedy pick ignores them
    }
    EXPECT(differ == 4);
    const int G = AM_INC_POS | AM_RECORD;                        // without AM_SAMPLE the key holds the defaults
    for (int i = 0; i < 4; ++i) EXPECT(decode_graph_key(2, 7, G, 3, false, q[i]) == decode_graph_key(2, 7, G, 3, false, p));
    if (!bad) printf("OK %d\n", differ);
    return bad;
}
"""
    cpp, exe, exe_san = tmp_path / "filt.cpp", tmp_path / "filt", tmp_path / "filt_san"
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
        assert r.returncode == 0 and not r.stderr and r.stdout == "OK 4\n", (x, r.returncode, r.stdout, r.stderr[-2000:])
