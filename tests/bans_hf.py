"""HF's -inf processors as a LogitsProcessorList on the CPU: what tests/test_bans_cpu.py holds logit_bans.banned_ids to, and what the host loops
of tests/test_gpu_bans.py apply to the stepped logits."""
import torch
from transformers import LogitsProcessorList
from transformers.generation.logits_process import (MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                    NoRepeatNGramLogitsProcessor, SuppressTokensAtBeginLogitsProcessor,
                                                    SuppressTokensLogitsProcessor)


def hf_chain(bans, prompt_len: int, eos: int) -> LogitsProcessorList:
    """The processors HF's generate() builds for the arguments `bans` stands for, in HF's order (GenerationMixin._get_logits_processor).  `bans` is
    given UNCHECKED: the [eos] filter of the bad words is HF's own here.  A processor HF would not build (value 0 / None / empty) is left out."""
    chain = LogitsProcessorList()
    if bans.no_repeat_ngram:
        chain.append(NoRepeatNGramLogitsProcessor(int(bans.no_repeat_ngram)))
    words = [list(w) for w in bans.bad_words]
    if words and not (eos >= 0 and all(w == [eos] for w in words)):       # HF's own filter would leave an empty list, which its constructor refuses
        chain.append(NoBadWordsLogitsProcessor(words, eos_token_id=eos if eos >= 0 else None))
    if eos >= 0 and bans.min_length > 0:
        chain.append(MinLengthLogitsProcessor(int(bans.min_length), eos))
    if eos >= 0 and bans.min_new_tokens > 0:
        chain.append(MinNewTokensLengthLogitsProcessor(int(prompt_len), int(bans.min_new_tokens), eos))
    if len(bans.suppress):
        chain.append(SuppressTokensLogitsProcessor(list(bans.suppress)))
    if len(bans.begin_suppress):
        chain.append(SuppressTokensAtBeginLogitsProcessor(list(bans.begin_suppress), int(prompt_len)))
    return chain


def hf_scores(bans, ids, prompt_len: int, eos: int, scores: torch.Tensor) -> torch.Tensor:
    """`scores` [V] fp32 through the chain for the sequence `ids`."""
    inp = torch.tensor([list(ids)], dtype=torch.long).reshape(1, len(ids))
    return hf_chain(bans, prompt_len, eos)(inp, scores[None].clone().float())[0]


def hf_banned(bans, ids, prompt_len: int, eos: int, vocab: int) -> set:
    """The ids HF sets to -inf, from finite scores."""
    out = hf_scores(bans, ids, prompt_len, eos, torch.zeros(vocab))
    return set(torch.nonzero(torch.isinf(out) & (out < 0)).flatten().tolist())
