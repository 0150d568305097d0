"""Score the dataset's own gold answers: for every ActivityNet-QA sample the log-likelihood of its `answer` under the model, teacher-forced
behind the prompt `video_chatgpt_infer` would build -- a quality number that needs nothing but this decoder (the reference's quantitative
evaluation needs a served judge LLM), e.g. to compare the fp8 weight path or bf16 against fp16 beyond token agreement.

CLI: ActivityNet-QA's (run_inference_qa_activitynet: `load_samples`, `find_video`) plus `_sharded.add_runtime_arguments`; of the latter only
--batch and --feature-cache matter here (nothing is generated: --max_new_tokens, --do_sample, --schedule, --seed, --top_p,
--repetition_penalty and --timings are accepted and ignored).  Writes `[{"id", "question", "answer", "answer_logprob", "answer_tokens",
"answer_ppl"}, ...]` to `{output_dir}/{output_name}.json`; a sample whose video is missing or fails is reported and left out, as in the
other runners.

The loop is `_sharded._Runner`'s: samples sharded over the ranks, groups of --batch clips with the host half one group ahead, one tower pass
per group, the feature cache -- and ONE `model.score` call per group.  Collation goes through the unchanged `parallel.run_sharded`: the
per-token fp32 log-probabilities travel as their int32 bit patterns in the token buffer (width = the longest gold answer in tokens,
length_offset = 1), so it stays one fixed-shape all-gather and every rank ends with the same numbers.
"""
from __future__ import annotations

import math
import os

import torch

from . import _sharded
from .run_inference_qa_activitynet import find_video, load_samples, parse_args  # noqa: F401  (parse_args: this runner's CLI is that runner's)


def pack_logprobs(lp: torch.Tensor) -> torch.Tensor:
    """fp32 log-probabilities -> their int32 bit patterns (what the token buffer of parallel.run_sharded carries)."""
    return lp.detach().to(device="cpu", dtype=torch.float32).contiguous().view(torch.int32)


def unpack_logprobs(ids) -> torch.Tensor:
    """The inverse, from the list of ints parallel.gather_answers hands back."""
    return torch.tensor(list(ids), dtype=torch.int32).view(torch.float32)


class _ScoreRunner(_sharded._Runner):
    """`_Runner` with one schedule of its own: a group is one score() call."""

    def __init__(self, args, tasks, components, load_frames, rank, width):
        super().__init__(args, tasks, components, load_frames, rank, None)
        self.width = width

    def sequence(self, idx, clips, feat_of):
        """Task idx -> (ids of prompt + answer + stop string, labels, pooled features); None after the print-and-continue of `inputs`."""
        from ..inference import build_prompt
        from ..scoring import continuation_labels
        inp = self.inputs(idx, clips, feat_of)
        if inp is None:
            return None
        prompt_ids, feat, stop = inp
        try:
            prompt, _ = build_prompt(self.tasks[idx]["question"], self.args.conv_mode, self.video_token_len, self.use_se)
            full = list(self.tokenizer([prompt + self.tasks[idx]["answer"] + stop]).input_ids[0])
            return full, continuation_labels(prompt_ids, full), feat
        except Exception as e:                                         # noqa: BLE001
            return self.failed(idx, e)

    def infer_score(self, indices, clips=None):
        """-> (int32 bit patterns of the per-token log-probabilities [n, width], lengths: 0 = failed, k + 1 = k scored tokens)."""
        feat_of, host = self.group_features(self.prepare(indices) if clips is None else clips)
        toks, lens = torch.zeros(len(indices), self.width, dtype=torch.int32), [0] * len(indices)
        keep = []
        for j, idx in enumerate(indices):
            seq = self.sequence(idx, host["clips"], feat_of)
            if seq is not None:
                keep.append((j,) + seq)

        def run(part):
            out = self.model.score([f for _, f, _, _ in part], [l for _, _, l, _ in part],
                                   video_spatio_temporal_features=torch.stack([x for _, _, _, x in part]))
            for b, (j, _, _, _) in enumerate(part):
                lp = pack_logprobs(out.token_logprobs[b][out.scored[b]])[:self.width]
                toks[j, :lp.numel()] = lp
                lens[j] = lp.numel() + 1

        if keep:
            try:
                run(keep)
            except Exception as e:                                     # noqa: BLE001 -- one bad sample must not take the group down
                print(f"batched scoring failed ({type(e).__name__}: {e}); retrying the {len(keep)} samples one by one")
                for item in keep:
                    try:
                        run([item])
                    except Exception as e1:                            # noqa: BLE001
                        self.failed(indices[item[0]], e1)
        self.group_no += 1
        return toks, lens


def answer_width(samples, tokenizer, conv_mode, video_token_len, use_se) -> int:
    """The longest gold answer in scored tokens (answer + stop string behind the prompt): the width of the collation buffer, the same on every
    rank.  A sample that cannot be tokenised counts 0 here and fails in its group."""
    from ..inference import build_prompt
    width = 1
    for s in samples:
        try:
            prompt, stop = build_prompt(s["question"], conv_mode, video_token_len, use_se)
            width = max(width, len(tokenizer([prompt + s["answer"] + stop]).input_ids[0]) - len(tokenizer([prompt]).input_ids[0]))
        except Exception:                                              # noqa: BLE001
            pass
    return width


def build_output(samples, scored):
    out = []
    for s, ids in zip(samples, scored):
        if ids is None:
            continue
        lp = unpack_logprobs(ids)
        n = int(lp.numel())
        total = float(lp.double().sum())
        out.append({"id": s["id"], "question": s["question"], "answer": s["answer"], "answer_logprob": total, "answer_tokens": n,
                    "answer_ppl": math.exp(-total / n) if n else float("nan")})
    return out


def run_inference(args, components=None, load_frames=None):
    """components = (model, vision_tower, tokenizer, image_processor, video_token_len) may be injected (tests)."""
    from .. import parallel
    from ..feature_extraction import load_video

    rank, world, components = _sharded.setup(args, components)
    model, vision_tower, tokenizer, image_processor, video_token_len = components
    frame_size = (image_processor.crop_size["height"], image_processor.crop_size["width"])
    load_frames = load_frames or (lambda path: load_video(path, shape=frame_size, device_resize=True))
    samples = load_samples(args.gt_file_question, args.gt_file_answers)
    os.makedirs(args.output_dir, exist_ok=True)
    tasks = [{"path": find_video(args.video_dir, s["video_name"]), "name": s["video_name"], "question": s["question"], "answer": s["answer"]}
             for s in samples]
    width = answer_width(samples, tokenizer, args.conv_mode, video_token_len, model.get_model().vision_config.use_vid_start_end)
    device = vision_tower.device if hasattr(vision_tower, "device") else torch.device("cpu")
    if getattr(args, "batch", "auto") == "auto":
        # results do not depend on the group size (score() is batch invariant), so every rank may pick its own
        free_b = torch.cuda.mem_get_info(device)[0] if device.type == "cuda" else 0
        args.batch = _sharded.pick_batch(model.config, vision_tower.config.image_size, width, free_b) if free_b else 8
    run = _ScoreRunner(args, tasks, components, load_frames, rank, width)
    scored = parallel.run_sharded(len(tasks), run.infer_score, width, rank, world, device, per_gpu_batch=args.batch, length_offset=1,
                                  prepare=run.prepare, spill_path=os.path.join(args.output_dir, args.output_name))
    return _sharded.write_output(args, build_output(samples, scored), rank)


if __name__ == "__main__":
    run_inference(parse_args())
