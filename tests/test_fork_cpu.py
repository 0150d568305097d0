"""Host side of sampling N answers per prompt from one prefill (pgv_kv_fork): the C-ABI surface, the slot map and what
generate(samples_per_prompt=) refuses before it touches the device.  No GPU."""
import ctypes
import os
import re

import pytest

from video_llava_amd import generation as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fork_entry_points_are_declared_bound_and_exported():
    from video_llava_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "pgv.h")).read()
    lib = ctypes.CDLL(build.build())
    for name in ("pgv_kv_fork", "pgv_kv_peek"):
        assert re.search(r"\bint %s\s*\(" % name, header), f"pgv.h does not declare {name}"
        assert name in _lib.PROTOTYPES, f"ctypes binding lacks {name}"
        assert hasattr(lib, name), f"libpgv.so does not export {name}"
    assert len(_lib.PROTOTYPES["pgv_kv_fork"][1]) == 6 and len(_lib.PROTOTYPES["pgv_kv_peek"][1]) == 8
    lib.pgv_version.restype = ctypes.c_int
    assert lib.pgv_version() == 328 == _lib.ABI_VERSION
    assert "kv_fork.hip" in build.sources_present()
    assert "#define PGV_NFAMILY 7" in header                  # the fork belongs to no profiling family


def test_fork_sources_is_repeat_interleave():
    assert G.fork_sources([2, 1, 3]) == [0, 0, 1, 2, 2, 2]
    assert G.fork_sources([1, 1]) == [0, 1] and G.fork_sources([4]) == [0] * 4 and G.fork_sources([]) == []
    for bad in ([1, 0], [-1], [2, 1.5]):
        with pytest.raises(ValueError):
            G.fork_sources(bad)


def _deviceless_model():
    import torch.nn as nn
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM
    m = object.__new__(VideoChatGPTLlamaForCausalLM)
    nn.Module.__init__(m)
    m.config = VideoChatGPTConfig()
    return m


def test_generate_checks_samples_per_prompt_before_it_touches_the_device():
    m = _deviceless_model()
    with pytest.raises(ValueError, match="samples_per_prompt"):
        m.generate([[1, 2, 3]], do_sample=True, samples_per_prompt=0)
    with pytest.raises(ValueError, match="do_sample"):
        m.generate([[1, 2, 3]], samples_per_prompt=2)
    with pytest.raises(ValueError, match="72 sequences"):
        m.generate([[1, 2, 3]] * 9, do_sample=True, samples_per_prompt=8)
    with pytest.raises(ValueError, match="stopping_criteria"):
        m.generate([[1, 2, 3]], do_sample=True, samples_per_prompt=2, stopping_criteria=[lambda ids, scores: False])
    with pytest.raises(ValueError, match="kv_reuse_key"):
        m.generate([[1, 2, 3]], do_sample=True, samples_per_prompt=2, kv_reuse_key="clip")


def test_num_return_sequences_stays_refused_by_name():
    m = _deviceless_model()
    with pytest.raises(ValueError, match="`num_return_sequences`"):
        m.generate([[1, 2, 3]], do_sample=True, num_return_sequences=2)
    assert G.REFUSED["num_return_sequences"](2) and not G.REFUSED["num_return_sequences"](1)
    with pytest.raises(ValueError, match="samples_per_prompt"):        # ... and points to the package's own keyword
        G.check_generate_kwargs({"num_return_sequences": 2})


def test_best_sample_picks_the_largest_logprob_first_on_ties():
    from video_llava_amd.inference import best_sample
    assert best_sample([{"logprob": -3.0}, {"logprob": -1.5}, {"logprob": -1.5}, {"logprob": -2.0}]) == 1
    assert best_sample([{"logprob": -0.25}]) == 0
    with pytest.raises(ValueError):
        best_sample([])
