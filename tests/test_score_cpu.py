"""CPU-only: the host side of teacher-forced scoring (video_llava_amd/scoring.py, the bit-pattern collation of eval/score_answers.py)."""
import os
import re

import numpy as np
import pytest
import torch

from video_llava_amd import _lib, parallel
from video_llava_amd.eval import score_answers
from video_llava_amd.scoring import ScoreOutput, continuation_labels, shift_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shift_labels_on_ragged_batches():
    seqs = [[1, 5, 6, 7], [1, 9], [4], [1, 2, 3]]
    labels = [[-100, -100, 6, 7], [-100, -100], [4], [-100, -100, 3]]        # a tail span; all ignored; one token; only the last position
    t = shift_labels(seqs, labels)
    assert t.dtype == np.int32 and t.tolist() == [-1, 6, 7, -1, -1, -1, -1, -1, 3, -1]
    # HF's rule: row p is scored iff p + 1 < len and labels[p + 1] != -100 -- the first label never counts, the last row never scores
    assert shift_labels([[1, 2, 3]], [[9, -100, -100]]).tolist() == [-1, -1, -1]
    assert shift_labels(torch.tensor([[1, 2, 3], [4, 5, 6]]), torch.tensor([[1, 2, 3], [-100, 5, -100]])).tolist() == [2, 3, -1, 5, -1, -1]
    with pytest.raises(ValueError, match="labels for"):
        shift_labels([[1, 2, 3]], [[1, 2]])
    with pytest.raises(ValueError, match="label rows"):
        shift_labels([[1, 2, 3]], [[1, 2, 3], [1]])
    with pytest.raises(ValueError, match="negative labels"):
        shift_labels([[1, 2, 3]], [[1, -1, 3]])


def test_continuation_labels():
    assert continuation_labels([1, 5, 6], [1, 5, 6, 7, 8]) == [-100, -100, -100, 7, 8]
    assert continuation_labels([1, 5], [1, 5]) == [-100, -100]
    assert shift_labels([[1, 5, 6, 7, 8]], [continuation_labels([1, 5, 6], [1, 5, 6, 7, 8])]).tolist() == [-1, -1, 7, 8, -1]
    with pytest.raises(ValueError, match="not a prefix"):
        continuation_labels([1, 5, 6], [1, 5, 9, 7])                 # the tokenizer merged across the boundary
    with pytest.raises(ValueError, match="not a prefix"):
        continuation_labels([1, 5, 6], [1, 5])


def test_score_output_loss_is_cross_entropy_on_the_reference_logits():
    """ScoreOutput.loss (-sum / count over the batch) against torch's CrossEntropyLoss in fp64 on the REFERENCE's own logits
    (tests/golden/llama_tiny.npz: lin_prefill_logits [42, 515], |logit| <= 8.1, log-probs in -12.7 .. -3.3) with labels = lin_ids.  The
    per-token values are rounded to fp32 as the device returns them: each is off by at most 2^-24 * 16, and so is their mean."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "llama_tiny.npz"))
    logits = torch.from_numpy(g["lin_prefill_logits"]).double()
    ids = g["lin_ids"].tolist()
    assert logits.shape == (42, 515) and float(logits.abs().max()) <= 8.1
    targets = shift_labels([ids], [ids])
    lsm = torch.log_softmax(logits, dim=1)
    lp = np.array([float(lsm[r, t]) if t >= 0 else 7.0 for r, t in enumerate(targets)], dtype=np.float32)    # 7: garbage on the unscored row
    assert -12.7 <= lp[:-1].min() and lp[:-1].max() <= -3.3
    out = ScoreOutput.from_rows([42], targets, lp, lsm.argmax(1).numpy())
    ce = torch.nn.functional.cross_entropy(logits[:-1], torch.tensor(ids[1:]))
    assert abs(out.loss - float(ce)) <= 2.0 ** -24 * 16
    assert int(out.counts[0]) == 41 and out.scored[0].tolist() == [False] + [True] * 41
    assert float(out.token_logprobs[0][0]) == 0.0 and int(out.argmax[0][0]) == -1
    assert out.sequence_logprob.dtype == torch.float64 and float(out.sequence_logprob[0]) == float(torch.from_numpy(lp[:-1]).double().sum())
    # a ragged batch with -100 labels: the mean runs over the scored tokens of the whole batch
    lab2 = [-100] * 30 + ids[30:40]
    t2 = shift_labels([ids, ids[:40]], [ids, lab2])
    lp2 = np.concatenate([lp, np.where(t2[42:] >= 0, lp[:40], np.float32(3.0))]).astype(np.float32)
    out2 = ScoreOutput.from_rows([42, 40], t2, lp2, np.zeros(82, dtype=np.int32))
    ce2 = torch.nn.functional.cross_entropy(torch.cat([logits[:-1], logits[:39]]), torch.tensor(ids[1:] + lab2[1:]), ignore_index=-100)
    assert out2.counts.tolist() == [41, 10] and abs(out2.loss - float(ce2)) <= 2.0 ** -24 * 16
    assert bool((out2.token_logprobs[1][:30] == 0).all())
    assert np.isnan(ScoreOutput.from_rows([3], np.array([-1, -1, -1]), np.zeros(3), np.zeros(3)).loss)


def test_logprob_bit_patterns_round_trip_through_gather_answers():
    """eval/score_answers.py: fp32 log-probabilities travel through parallel.gather_answers (world 1) as int32 bit patterns, losslessly."""
    lps = [torch.tensor([-0.0, -1.5e-7, -3.25, -12.7, float("-inf")]), torch.tensor([]), None, torch.tensor([-88.125])]
    width = 5
    toks = torch.zeros(4, width, dtype=torch.int32)
    lens = torch.zeros(4, dtype=torch.int32)
    for j, lp in enumerate(lps):
        if lp is not None:
            toks[j, :lp.numel()] = score_answers.pack_logprobs(lp)
            lens[j] = lp.numel() + 1
    back = parallel.gather_answers(toks, lens, 4, 0, 1, length_offset=1)
    assert back[2] is None and back[1] == []
    for j in (0, 1, 3):
        got = score_answers.unpack_logprobs(back[j])
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), lps[j].view(torch.int32))
    samples = [{"id": i, "question": "q", "answer": "a"} for i in range(4)]
    out = score_answers.build_output(samples, [back[3], None, back[1], back[0]])
    assert [o["id"] for o in out] == [0, 2, 3]
    assert out[0] == {"id": 0, "question": "q", "answer": "a", "answer_logprob": -88.125, "answer_tokens": 1, "answer_ppl": float(np.exp(88.125))}
    assert out[1]["answer_tokens"] == 0 and np.isnan(out[1]["answer_ppl"])


def test_score_chunk_rows_matches_the_header():
    header = open(os.path.join(ROOT, "include", "pgv.h")).read()
    assert int(re.search(r"#define PGV_SCORE_CHUNK_ROWS (\d+)", header).group(1)) == _lib.SCORE_CHUNK_ROWS
    assert "pgv_llm_score" in _lib.PROTOTYPES and "pgv_logprob_rows" in _lib.PROTOTYPES and _lib.ABI_VERSION >= 325
    assert "video_chatgpt/model/video_chatgpt.py:228-239" in header
