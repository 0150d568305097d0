"""Host side of the sampling parameters: HF's precedence (call over generation_config.json over HF's default), the refused generate() arguments,
the loader's generation_config.json and the runners' flags.  No GPU."""
import argparse
import json

import pytest

from video_llava_amd import generation as G


def test_precedence_call_over_file_over_hf_default():
    assert G.resolve_sampling() == (1.0, 50, 1.0, 1.0)                                     # HF's GenerationConfig defaults
    cfg = G.GenerationDefaults(temperature=0.9, top_p=0.6)
    assert G.resolve_sampling(generation_config=cfg) == (0.9, 50, 0.6, 1.0)
    # the reference's call: temperature 0.2 in the call, the rest from the file / HF
    assert G.resolve_sampling(temperature=0.2, generation_config=cfg) == (0.2, 50, 0.6, 1.0)
    assert G.resolve_sampling(0.2, 7, 0.95, 1.3, cfg) == (0.2, 7, 0.95, 1.3)
    assert G.resolve_sampling(top_p=1.0, generation_config=cfg) == (0.9, 50, 1.0, 1.0)     # an explicit neutral value still wins over the file
    assert G.resolve_sampling(generation_config={"repetition_penalty": 1.1, "top_k": 0}) == (1.0, 0, 1.0, 1.1)      # a plain dict works too


def test_resolve_validates_with_hf_wording():
    for bad in (0.0, -0.5, 1.01):
        with pytest.raises(ValueError, match="`top_p` has to be a float > 0 and <= 1"):
            G.resolve_sampling(top_p=bad)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="`penalty` has to be a strictly positive float"):
            G.resolve_sampling(repetition_penalty=bad)
    with pytest.raises(ValueError, match="top_p"):
        G.resolve_sampling(generation_config=G.GenerationDefaults(top_p=0.0))


def test_generation_config_json_is_read_and_absent_file_changes_nothing(tmp_path):
    assert G.load_generation_config(str(tmp_path)) is None
    (tmp_path / "generation_config.json").write_text(json.dumps({"bos_token_id": 1, "eos_token_id": 2, "temperature": 0.9, "top_p": 0.6,
                                                                 "max_length": 4096, "transformers_version": "4.31.0"}))
    cfg = G.load_generation_config(str(tmp_path))
    assert cfg.temperature == 0.9 and cfg.top_p == 0.6 and cfg.top_k is None and cfg.num_beams is None
    assert G.resolve_sampling(temperature=0.2, generation_config=cfg) == (0.2, 50, 0.6, 1.0)
    G.check_generate_kwargs({}, cfg)                                                       # nothing refused in it


REFUSED_CASES = [("num_beams", 4, 1), ("min_p", 0.05, None), ("typical_p", 0.9, 1.0), ("penalty_alpha", 0.6, None), ("no_repeat_ngram_size", 3, 0),
                 ("bad_words_ids", [[5]], None), ("min_length", 4, 0), ("min_new_tokens", 2, 0), ("num_return_sequences", 2, 1),
                 ("epsilon_cutoff", 3e-4, 0.0), ("eta_cutoff", 3e-4, 0.0), ("encoder_repetition_penalty", 1.5, 1.0)]


@pytest.mark.parametrize("name,bad,neutral", REFUSED_CASES)
def test_refused_arguments_raise_by_name_and_neutral_values_pass(name, bad, neutral, tmp_path):
    with pytest.raises(ValueError, match=f"`{name}`"):
        G.check_generate_kwargs({name: bad})
    G.check_generate_kwargs({name: neutral})
    # the same field in the checkpoint's file: loading is fine, generate() raises; the call's own neutral value overrides it
    (tmp_path / "generation_config.json").write_text(json.dumps({name: bad}))
    cfg = G.load_generation_config(str(tmp_path))
    with pytest.raises(ValueError, match=f"generation_config field `{name}`"):
        G.check_generate_kwargs({}, cfg)
    G.check_generate_kwargs({name: neutral}, cfg)


def test_inert_arguments_are_ignored():
    import torch
    G.check_generate_kwargs({"use_cache": True, "pad_token_id": 0, "output_scores": False, "return_dict_in_generate": False,
                             "attention_mask": torch.ones(2, 5, dtype=torch.long), "some_future_flag": 3})
    with pytest.raises(ValueError, match="attention_mask"):
        G.check_generate_kwargs({"attention_mask": torch.tensor([[0, 1, 1]])})
    with pytest.raises(ValueError, match="output_scores"):
        G.check_generate_kwargs({"output_scores": True})


def test_generate_resolves_before_it_touches_the_device():
    """generate() on an object without a device: a refused argument and a bad top_p raise first, from the model's generation config too."""
    import torch.nn as nn
    from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM
    m = object.__new__(VideoChatGPTLlamaForCausalLM)
    nn.Module.__init__(m)
    m.config = VideoChatGPTConfig()
    assert m.generation_config is None
    with pytest.raises(ValueError, match="num_beams"):
        m.generate([[1, 2, 3]], num_beams=3)
    with pytest.raises(ValueError, match="top_p"):
        m.generate([[1, 2, 3]], do_sample=True, top_p=0.0)
    m.generation_config = G.GenerationDefaults(no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        m.generate([[1, 2, 3]])


def test_runner_flags_default_to_the_generation_config():
    from video_llava_amd.eval import _sharded
    args = _sharded.add_runtime_arguments(argparse.ArgumentParser()).parse_args([])
    assert args.top_p is None and args.repetition_penalty is None
    args = _sharded.add_runtime_arguments(argparse.ArgumentParser()).parse_args(["--top_p", "0.6", "--repetition_penalty", "1.2"])
    assert args.top_p == 0.6 and args.repetition_penalty == 1.2
    run = object.__new__(_sharded._Runner)
    run.args = argparse.Namespace(top_p=None, repetition_penalty=1.1)
    assert run.warpers() == {"repetition_penalty": 1.1}                                    # only what was given: the rest is generate()'s precedence
    run.args = argparse.Namespace()
    assert run.warpers() == {}


def test_vision_tower_refuses_arguments_that_change_its_output():
    from video_llava_amd.vision_tower import CLIPVisionTower
    t = object.__new__(CLIPVisionTower)
    for name, bad in (("output_attentions", True), ("interpolate_pos_encoding", True), ("return_dict", False)):
        with pytest.raises(ValueError, match=name):
            CLIPVisionTower.__call__(t, None, output_hidden_states=True, **{name: bad})
