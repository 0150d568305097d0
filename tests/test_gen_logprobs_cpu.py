"""Host side of generate(output_logprobs=True): the assembly of the result (cuts, zeros past a sequence's end, fp64 sums), the C ABI table, and
what generate() still refuses.  No GPU."""
import numpy as np
import pytest
import torch

from video_llava_amd import _lib
from video_llava_amd import generation as G


def test_assemble_cuts_pads_and_sums():
    seqs = torch.arange(12).reshape(3, 4)
    # per sequence: every value the device emitted (a whole number of chunks); kept: 2 of 5, all 5, none
    model = [np.array([-1.5, -2.25, -9.0, -9.0, -9.0], dtype=np.float32), np.array([-0.1] * 5, dtype=np.float32), np.array([-3.0] * 5, dtype=np.float32)]
    pick = [np.array([-0.5, 0.0, -8.0, -8.0, -8.0], dtype=np.float32), np.array([-0.2] * 5, dtype=np.float32), np.array([-4.0] * 5, dtype=np.float32)]
    out = G.GenerateLogprobsOutput.assemble(seqs, [2, 5, 0], model, pick)
    assert out.sequences is seqs
    assert out.token_logprobs.shape == (3, 5) and out.token_logprobs.dtype == torch.float32 and out.transition_scores.dtype == torch.float32
    assert out.token_logprobs[0].tolist() == [-1.5, -2.25, 0.0, 0.0, 0.0] and out.transition_scores[0].tolist() == [-0.5, 0.0, 0.0, 0.0, 0.0]
    assert out.token_logprobs[2].tolist() == [0.0] * 5 and out.transition_scores[2].tolist() == [0.0] * 5
    assert torch.equal(out.token_logprobs[1], torch.full((5,), -0.1)) and torch.equal(out.transition_scores[1], torch.full((5,), -0.2))
    assert out.sequence_logprob.dtype == torch.float64 and out.sequence_logprob.shape == (3,)
    assert out.sequence_logprob.tolist() == [-3.75, float(np.float64(np.float32(-0.1)) * 5), 0.0]
    # fp64 sums of the fp32 values: 2^24 + 1 + 1 is not representable in fp32
    big = G.GenerateLogprobsOutput.assemble(seqs[:1], [3], [np.array([-16777216.0, -1.0, -1.0], dtype=np.float32)], [np.zeros(3, dtype=np.float32)])
    assert float(big.sequence_logprob[0]) == -16777218.0
    # nothing generated at all: empty arrays, zero sums
    none = G.GenerateLogprobsOutput.assemble(seqs[:2], [0, 0], [np.zeros(0), np.zeros(0)], [np.zeros(0), np.zeros(0)])
    assert none.token_logprobs.shape == (2, 0) and none.sequence_logprob.tolist() == [0.0, 0.0]
    # fewer values than kept ids is a bookkeeping error, not a silent zero
    with pytest.raises(ValueError, match="log-probabilities"):
        G.GenerateLogprobsOutput.assemble(seqs[:1], [3], [np.zeros(2)], [np.zeros(2)])


def test_abi_table_holds_the_new_symbols():
    assert _lib.ABI_VERSION >= 326
    for name, nargs in (("pgv_kv_set_logprobs", 2), ("pgv_kv_logprobs_last", 4), ("pgv_kv_logprobs_steps", 5), ("pgv_llm_pick_greedy", 5),
                        ("pgv_sample_logits_lp", 18)):
        assert name in _lib.PROTOTYPES, name
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib._i and len(args) == nargs, name
    # the building block = pgv_sample_logits_ex + (greedy, d_lp_model, d_lp_pick) in front of the stream
    ex, lp = _lib.PROTOTYPES["pgv_sample_logits_ex"][1], _lib.PROTOTYPES["pgv_sample_logits_lp"][1]
    assert lp[:len(ex) - 1] == ex[:-1] and lp[len(ex) - 1:] == [_lib._i, _lib._vp, _lib._vp, _lib._vp]


def test_generate_still_refuses_hf_score_outputs_and_names_the_keyword():
    for name in ("output_scores", "return_dict_in_generate"):
        with pytest.raises(ValueError, match=name) as e:
            G.check_generate_kwargs({name: True})
        assert "output_logprobs" in str(e.value)
    G.check_generate_kwargs({"output_scores": False, "return_dict_in_generate": False})


def test_generate_and_continuous_take_the_keyword():
    import inspect
    from video_llava_amd import continuous, inference
    from video_llava_amd.model.video_chatgpt import VideoChatGPTLlamaForCausalLM as M
    assert inspect.signature(M.generate).parameters["output_logprobs"].default is False
    assert inspect.signature(continuous.generate_continuous).parameters["logprobs"].default is None
    a, b = inspect.signature(inference.video_chatgpt_infer).parameters, inspect.signature(inference.video_chatgpt_infer_logprobs).parameters
    assert list(b)[:len(a)] == list(a)
    for meth in ("set_logprobs", "logprobs_last", "logprobs_steps", "greedy_last"):
        assert callable(getattr(M, meth))
