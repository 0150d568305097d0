"""HF's PrefixConstrainedLogitsProcessor on the CPU with a callback that closes over a token automaton: what tests/test_allowed_cpu.py holds
allowed.allowed_ids to.  The callback is HF's `prefix_allowed_tokens_fn(batch_id, input_ids) -> list of ids`."""
import torch
from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor

from video_llava_amd.allowed import allowed_ids


def prefix_fn(automaton, roots, prompt_len: int, eos: int):
    """HF's callback for `automaton`: sequence `batch_id` starts at roots[batch_id]; everything behind `prompt_len` is the answer so far (HF hands
    the finished rows of a batch on with their pad ids behind EOS: the walk is DEAD there and the rule allows EOS, never an empty list)."""
    def fn(batch_id, input_ids):
        return sorted(allowed_ids(automaton, roots[int(batch_id)], [int(t) for t in input_ids[prompt_len:]], eos))
    return fn


def hf_scores(automaton, root: int, generated, eos: int, scores: torch.Tensor) -> torch.Tensor:
    """`scores` [V] fp32 through HF's processor for a sequence whose answer so far is `generated` (no prompt: prompt_len 0)."""
    proc = PrefixConstrainedLogitsProcessor(prefix_fn(automaton, [root], 0, eos), 1)
    ids = torch.tensor([list(generated)], dtype=torch.long).reshape(1, len(generated))
    return proc(ids, scores[None].clone().float())[0]


def hf_allowed(automaton, root: int, generated, eos: int, vocab: int) -> set:
    """The ids HF leaves finite, from finite scores."""
    out = hf_scores(automaton, root, generated, eos, torch.zeros(vocab))
    return set(torch.nonzero(torch.isfinite(out)).flatten().tolist())
