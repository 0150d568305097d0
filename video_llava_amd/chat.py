"""Interactive chat entry point with the reference's class, methods and CLI
(video_chatgpt/chat.py:15-222 `VideoChatGPTInterface`, :336-367 `parse_args` / `__main__`).

Same conversation state machine (add_text -> answer), same prompt assembly (`<video>` replaced by the placeholder run once, :129-130),
same stop-string handling and post-processing.  Device work runs in libpgv.  Two deliberate differences:
  * the reference re-runs the CLIP tower on the whole clip for EVERY turn (:137-144); here the pooled features of the uploaded clip
    are computed once in `upload_video` and reused by every `answer()` of the conversation;
  * the reference re-runs the decoder over the WHOLE conversation every turn (:129-154); here a later turn prefills only the tokens behind the
    prefix the KV cache already holds (`generate(kv_reuse_key=...)` -> pgv_llm_prefill_append) -- same tokens, `last_timings["reused_tokens"]`;
  * `PGVideoLLaVA` (grounding: GroundingDINO / SAM / DEVA / RAM / OpenAI entity matching, :225-333) and the WhisperX transcript model are
    side stacks outside the hot path: `--with_grounding` and `--use_asr` raise NotImplementedError.
"""
from __future__ import annotations

import argparse

import torch

from .constants import DEFAULT_TRANSCRIPT_START, DEFAULT_VID_END_TOKEN, DEFAULT_VID_START_TOKEN, DEFAULT_VIDEO_PATCH_TOKEN
from .generation import check_lookup, given
from .model.utils import KeywordsStoppingCriteria
from .video_conversation import SeparatorStyle, conv_templates, default_conversation


class VideoChatGPTInterface:
    def __init__(self, args_model_name, args_projection_path, use_asr=False, conv_mode="pg-video-llava", temperature=0.2,
                 max_output_tokens=1024, components=None, do_sample=True, reuse_kv=True, top_p=None, repetition_penalty=None, lookup=0,
                 lookup_ngram=2, lookup_sample=False, guidance_scale=None, guidance_negative="no_video", answer_choices=None) -> None:
        if use_asr:
            raise NotImplementedError("--use_asr needs the WhisperX transcript stack, which is outside this package's hot path")
        self.use_asr = use_asr
        self.conv_mode = conv_mode
        if components is None:
            from .eval.model_utils import initialize_model
            components = initialize_model(args_model_name, args_projection_path)
        model, vision_tower, tokenizer, image_processor, video_token_len = components
        self.tokenizer, self.image_processor, self.vision_tower, self.model = tokenizer, image_processor, vision_tower, model
        self.temperature = temperature
        self.top_p, self.repetition_penalty = top_p, repetition_penalty      # None: the checkpoint's generation_config.json, else HF's default
        self.max_new_tokens = max_output_tokens
        self.do_sample = do_sample
        # prompt-lookup speculative decoding (generate(lookup=D, lookup_ngram=n)): greedy, or with lookup_sample the sampled run's own answer;
        # refused here as generate() would refuse it
        self.lookup = check_lookup(lookup, lookup_ngram, 1, bool(do_sample), who="VideoChatGPTInterface", lookup_sample=bool(lookup_sample))
        self.lookup_sample = bool(lookup_sample)
        # classifier-free guidance (generate(guidance=)): every turn runs the conversation a second time without the clip ("no_video") or from
        # its last token (HF's default negative) as B more rows of the decode steps; such a turn keeps no KV cache for the next one
        self.guidance_scale = guidance_from_flags(guidance_scale, guidance_negative, lookup=self.lookup[0], who="VideoChatGPTInterface")
        self.guidance_negative = guidance_negative
        self.reuse_kv = reuse_kv and self.guidance_scale is None
        # constrained decoding (generate(allowed=)): every answer is one of `answer_choices` (a list of strings), followed on the device as a token
        # automaton compiled once here; such a turn runs the full prefill (generate's own fall-back under `kv_reuse_key`)
        if answer_choices and self.lookup[0]:
            raise ValueError(f"VideoChatGPTInterface: answer_choices cannot be combined with lookup={self.lookup[0]} (the drafts are verified against the "
                             f"unconstrained pick)")
        self.allowed = allowed_from_choices(tokenizer, answer_choices)
        self.frame_size = (image_processor.crop_size["height"], image_processor.crop_size["width"])
        if self.model.get_model().vision_config.use_vid_start_end:
            self.replace_token = DEFAULT_VID_START_TOKEN + DEFAULT_VIDEO_PATCH_TOKEN * video_token_len + DEFAULT_VID_END_TOKEN
        else:
            self.replace_token = DEFAULT_VIDEO_PATCH_TOKEN * video_token_len
        self.clear_history()

    def clear_history(self):
        self.state = default_conversation.copy()
        self.video_features = None          # pooled [100 + P, 1024] features of the uploaded clip (computed once per clip)
        self.kv_key = None                  # names the uploaded clip: later turns of the same clip continue the KV cache of the earlier ones
        self.last_timings = {}
        self.video_path = None
        self.video_frames = None
        self.transcript_text = None
        self.first_run = True

    def upload_video(self, video_path):
        """Decode + sample + resize the clip (reference :62-75) and run the vision stage ONCE for the whole conversation."""
        from .feature_extraction import load_video
        from .inference import video_features
        if isinstance(video_path, str):
            frames = load_video(video_path, shape=self.frame_size, device_resize=True)
        elif hasattr(video_path, "shape"):                 # uint8 [T, H, W, 3] frames handed over directly
            frames = video_path
        else:
            raise NotImplementedError
        self.video_path = video_path if isinstance(video_path, str) else None
        self.video_frames = frames
        self.video_features = video_features(frames, self.vision_tower, self.image_processor)
        self.kv_key = object() if self.reuse_kv else None
        self.transcript_text = None

    def add_text(self, text, video_path):
        """Queue one user turn (reference :90-104): empty input without a clip is skipped; a turn is cut at 1536 characters, the first turn of a
        clip at 1200 and carries the `<video>` (and, with ASR, `<audio_transcript>`) markers and the clip path."""
        self.state.skip_next = (not text) and video_path is None      # (overwritten below exactly like the reference: the turn is queued either way)
        limit = 1200 if self.first_run else 1536
        turn = text[:limit]
        if self.first_run:
            if "<video>" not in turn:
                turn += "\n<video>"
            if self.use_asr:
                turn += "\n<audio_transcript>"
            turn = (turn, video_path)
            self.state = default_conversation.copy()
        user, assistant = self.state.roles[0], self.state.roles[1]
        self.state.append_message(user, turn)
        self.state.append_message(assistant, None)
        self.state.skip_next = False

    def answer(self):
        if self.state.skip_next:
            return
        if self.video_features is None:
            raise RuntimeError("upload_video() first")
        if self.first_run:                                   # re-root the first turn on the chosen template (:113-120)
            first_user_turn = self.state.messages[-2][1]
            self.state = conv_templates[self.conv_mode].copy()
            self.state.append_message(self.state.roles[0], first_user_turn)
            self.state.append_message(self.state.roles[1], None)
            self.first_run = False
        raw = self.state.get_prompt()
        prompt = raw.replace("<video>", self.replace_token, 1)
        prompt = prompt.replace("<audio_transcript>", f'{DEFAULT_TRANSCRIPT_START}\n"{self.transcript_text}"', 1)
        inputs = self.tokenizer([prompt])
        guide = {}
        if self.guidance_scale is not None:
            from .guidance import Guidance
            negative = "last_token"
            if self.guidance_negative == "no_video":        # the same conversation without the video tokens
                no_video = raw.replace("<video>", "", 1).replace("<audio_transcript>", f'{DEFAULT_TRANSCRIPT_START}\n"{self.transcript_text}"', 1)
                negative = [list(self.tokenizer([no_video]).input_ids[0])]
            guide = {"guidance": Guidance(self.guidance_scale, negative)}
        input_ids = torch.as_tensor(inputs.input_ids)
        stop_str = self.state.sep if self.state.sep_style != SeparatorStyle.TWO else self.state.sep2
        stopping_criteria = KeywordsStoppingCriteria([stop_str], self.tokenizer, input_ids)
        self.state.messages[-1][-1] = ""
        with torch.inference_mode():
            output_ids = self.model.generate(input_ids, video_spatio_temporal_features=self.video_features.unsqueeze(0),
                                             do_sample=self.do_sample, temperature=float(self.temperature),
                                             max_new_tokens=min(int(self.max_new_tokens), 1536), stopping_criteria=[stopping_criteria],
                                             kv_reuse_key=self.kv_key, timings=self.last_timings, top_p=self.top_p,
                                             repetition_penalty=self.repetition_penalty,
                                             **given(lookup=self.lookup[0], lookup_ngram=self.lookup[1], lookup_sample=self.lookup_sample, allowed=self.allowed),
                                             **guide)
        n_in = input_ids.shape[1]
        n_diff = int((input_ids.to(output_ids.device) != output_ids[:, :n_in]).sum())
        if n_diff > 0:
            print(f"[Warning] {n_diff} output_ids are not the same as the input_ids")
        outputs = self.tokenizer.batch_decode(output_ids[:, n_in:], skip_special_tokens=True)[0].strip()
        if outputs.endswith(stop_str):
            outputs = outputs[:-len(stop_str)]
        output = self._post_process_code(outputs.strip())
        self.state.messages[-1][-1] += output
        return output

    def interact(self):
        """Terminal loop (reference :173-199): ask for a clip, then turns until an empty line (new conversation) or Ctrl-C (quit)."""
        print("Welcome to PG-Video-LLaVA !")
        clip = None
        try:
            while True:
                if clip is None:
                    clip = input("Please enter the video file path:   ")
                    self.upload_video(clip)
                text = input("USER>>")
                if text:
                    self.add_text(text, clip)
                    print("ASSISTANT>>", self.answer())
                else:                                        # empty line: drop the conversation and ask for the next clip
                    print("----------\n\n")
                    self.clear_history()
                    clip = None
        except KeyboardInterrupt:
            print("----------\nQUITTING...")

    def print_state(self):
        lines = [f"SYSTEM: {self.state.system}"]
        lines += [f"{role}: {msg[0] if type(msg) is tuple else msg}" for role, msg in self.state.messages]
        print("\n".join(lines) + "\n")

    @staticmethod
    def _post_process_code(code):
        """Undo the `\\_` escapes inside fenced code blocks when the fences pair up (reference :212-222)."""
        fence = "\n```"
        parts = code.split(fence)
        if len(parts) > 1 and len(parts) % 2 == 1:
            parts[1::2] = [inner.replace("\\_", "_") for inner in parts[1::2]]
        return fence.join(parts)


def guidance_from_flags(scale, negative, lookup=0, beams=1, samples_per_prompt=1, schedule="group", who="--guidance_scale"):
    """--guidance_scale S / --guidance_negative of a command line -> the scale as a float, or None when nothing is asked (no flag, or 1);
    ValueError names the flag guidance cannot run with, as generate() would refuse it."""
    import math
    if negative not in ("no_video", "last_token"):
        raise ValueError(f"{who}: --guidance_negative has to be no_video or last_token, but is {negative!r}")
    if scale is None:
        return None
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"{who}: --guidance_scale has to be a finite float, but is {scale!r}")
    if scale == 1.0:
        return None
    for flag, bad, why in (("--schedule refill", schedule == "refill", "a refill would separate the twins from their prompts"),
                           (f"--beams {beams}", int(beams or 1) > 1, "a beam step already runs K rows per prompt and applies no logits processor"),
                           (f"--lookup {lookup}", int(lookup or 0) > 0, "the drafts are verified against the unguided pick"),
                           (f"--samples_per_prompt {samples_per_prompt}", int(samples_per_prompt or 1) > 1, "a fork would separate the twins from their prompts")):
        if bad:
            raise ValueError(f"--guidance_scale {scale:g} cannot be combined with {flag} ({why})")
    return scale


def answer_choices_from_flags(choices, choices_file, lookup=0, beams=1):
    """--answer_choices "yes,no" / --answer_choices_file F (one answer per line) of a command line -> the answers as a list of strings, or None when
    neither flag is given; ValueError names what is wrong, or the flag constrained decoding cannot run with, as generate() would refuse it."""
    if choices is None and choices_file is None:
        return None
    if choices is not None and choices_file is not None:
        raise ValueError("--answer_choices and --answer_choices_file are two ways to give the same list: pass one of them")
    if choices is not None:
        texts = [t.strip() for t in str(choices).split(",")]
    else:
        with open(choices_file, encoding="utf-8") as fh:
            texts = [line.strip() for line in fh]
    texts = [t for t in texts if t]
    if not texts:
        raise ValueError("--answer_choices / --answer_choices_file: no answer given")
    if int(beams or 1) > 1:
        raise ValueError(f"--answer_choices cannot be combined with --beams {beams} (the beam pick applies no logits processor)")
    if int(lookup or 0) > 0:
        raise ValueError(f"--answer_choices cannot be combined with --lookup {lookup} (the drafts are verified against the unconstrained pick)")
    return texts


def allowed_from_choices(tokenizer, texts):
    """The answers of answer_choices_from_flags as generate()'s `allowed`: allowed.TokenAutomaton.from_texts (None: no constraint).  The tokenizer
    is asked for each answer on its own, without special tokens.  ASSUMPTION, not checked against a real tokenizer or checkpoint: that these ids are
    the ones the model produces behind its prompt -- for LLaMA's sentencepiece the answer with its leading-space piece -- and that the model writes the
    answer as it is spelled here ("Yes" and "yes" are different tokens: list both where either may come).  Where that does not hold, build the
    automaton from id lists (TokenAutomaton.from_sequences) or give from_texts a `prefix`."""
    if not texts:
        return None
    from .allowed import TokenAutomaton
    return TokenAutomaton.from_texts(tokenizer, list(texts))


def add_answer_choice_flags(parser):
    parser.add_argument("--answer_choices", default=None, metavar="A,B,...",
                        help="constrained decoding (generate(allowed=); HF: prefix_allowed_tokens_fn): every answer is one of these comma-separated "
                             "strings, e.g. \"yes,no\" or \"A,B,C,D\" -- compiled once into a token automaton that the device follows; not with --beams "
                             "or --lookup")
    parser.add_argument("--answer_choices_file", default=None, metavar="F", help="--answer_choices from a file, one answer per line")


def add_guidance_flags(parser):
    parser.add_argument("--guidance_scale", type=float, default=None, metavar="S",
                        help="classifier-free guidance (generate(guidance=); HF: guidance_scale): every pick reads S * (log_softmax(cond) - "
                             "log_softmax(uncond)) + log_softmax(uncond), uncond the logits of the negative prompt, which runs as one more row per clip of "
                             "every decode step; 1 (default): off; not with --schedule refill, --beams, --lookup or --samples_per_prompt")
    parser.add_argument("--guidance_negative", choices=("no_video", "last_token"), default="no_video",
                        help="--guidance_scale: the negative prompt -- no_video (default): the same conversation without the video tokens, i.e. contrast "
                             "decoding against the language prior; last_token: HF's default, the prompt's last token")


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Demo")
    parser.add_argument("--model-name", type=str, required=True)
    parser.add_argument("--projection_path", type=str, required=True)
    parser.add_argument("--use_asr", action="store_true", help="Whether to use audio transcripts or not")
    parser.add_argument("--conv_mode", type=str, required=False, default="pg-video-llava")
    parser.add_argument("--with_grounding", action="store_true", help="Run with grounding module")
    parser.add_argument("--do_sample", action="store_true", help="the reference's temperature-0.2 sampling (the default unless --lookup is given)")
    parser.add_argument("--lookup", type=int, default=0, metavar="D",
                        help="greedy decoding as prompt-lookup speculative decoding with D <= 15 drafts per step (generate(lookup=D)): the greedy answer, "
                             "bit for bit, in fewer passes over the weights; not with --do_sample unless --lookup_sample is given")
    parser.add_argument("--lookup_ngram", type=int, default=2, metavar="N", help="--lookup: the largest n-gram matched, 1 .. 4 (HF: max_matching_ngram_size)")
    parser.add_argument("--lookup_sample", action="store_true",
                        help="--lookup D --do_sample: lookup steps for the sampled run (generate(lookup_sample=True)): bit for bit the answer of --do_sample alone")
    add_guidance_flags(parser)
    add_answer_choice_flags(parser)
    args = parser.parse_args(argv)
    if args.lookup_sample and not args.do_sample:
        parser.error("--lookup_sample needs --do_sample (greedy lookup is --lookup D alone)")
    if args.lookup_sample and not args.lookup:
        parser.error("--lookup_sample needs --lookup D with D >= 1 drafts per step")
    if args.lookup and args.do_sample and not args.lookup_sample:
        parser.error(f"--lookup {args.lookup} cannot be combined with --do_sample (a sampled token has no draft to verify)")
    try:
        check_lookup(args.lookup, args.lookup_ngram, 1, who="chat.py")
        guidance_from_flags(args.guidance_scale, args.guidance_negative, lookup=args.lookup)
        args.answer_choice_list = answer_choices_from_flags(args.answer_choices, args.answer_choices_file, lookup=args.lookup)
    except (ValueError, OSError) as e:
        parser.error(str(e))
    return args


if __name__ == "__main__":
    args = parse_args()
    if args.with_grounding:
        raise NotImplementedError("the grounding stack (GroundingDINO / SAM / DEVA / RAM) is outside this package's hot path")
    VideoChatGPTInterface(args_model_name=args.model_name, args_projection_path=args.projection_path, use_asr=args.use_asr,
                          conv_mode=args.conv_mode, do_sample=args.lookup_sample or not args.lookup, lookup=args.lookup, lookup_ngram=args.lookup_ngram,
                          lookup_sample=args.lookup_sample, guidance_scale=args.guidance_scale, guidance_negative=args.guidance_negative,
                          answer_choices=args.answer_choice_list).interact()
