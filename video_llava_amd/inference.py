"""Single-video QA entry points with the reference's names and signatures
(video_chatgpt/inference.py:13-44 `get_spatio_temporal_features_torch`, :47-124 `video_chatgpt_infer`).

Device work -- CLIP tower, pooling, projector, decoder -- runs in libpgv (HIP, gfx950); this module is the host
orchestration: prompt assembly, tokenisation, preprocessing, stop handling, detokenisation.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .constants import (DEFAULT_TRANSCRIPT_START, DEFAULT_VID_END_TOKEN, DEFAULT_VID_START_TOKEN, DEFAULT_VIDEO_PATCH_TOKEN,
                        DEFAULT_VIDEO_TOKEN, NUM_TEMPORAL_TOKENS)
from .generation import given
from .model.utils import KeywordsStoppingCriteria
from .scoring import continuation_labels
from .video_conversation import SeparatorStyle, conv_templates


def get_spatio_temporal_features_torch(features: torch.Tensor) -> torch.Tensor:
    """[T, P, C] frame features -> [100 + P, C] fp16: per-frame means (zero padded to 100 rows) followed by per-patch
    means over time (reference video_chatgpt/inference.py:13-44).  One HIP pass; the `[:, 1:]` view of the hidden
    state is consumed in place."""
    if not features.is_cuda:
        raise RuntimeError("get_spatio_temporal_features_torch: features must live on the GPU (no CPU fallback in this package)")
    if features.stride(2) != 1 or features.stride(1) != features.shape[2]:
        features = features.contiguous()
    if features.dtype not in (torch.float16, torch.bfloat16):
        features = features.half()
    return _lib.Context.get(features.device).st_pool(features, NUM_TEMPORAL_TOKENS, torch.float16)


def build_prompt(question: str, conv_mode: str, video_token_len: int, use_vid_start_end: bool, transcript=None, video: bool = True):
    """Prompt string + stop string exactly as video_chatgpt_infer assembles them (inference.py:66-80,101).  video=False: the same conversation
    without the video tokens -- the "no_video" negative prompt of classifier-free guidance (guidance_for)."""
    if not video:
        qs = question + "\n"
    elif use_vid_start_end:
        qs = question + "\n" + DEFAULT_VID_START_TOKEN + DEFAULT_VIDEO_PATCH_TOKEN * video_token_len + DEFAULT_VID_END_TOKEN
    else:
        qs = question + "\n" + DEFAULT_VIDEO_PATCH_TOKEN * video_token_len
    if transcript:
        qs = f'{qs}\n{DEFAULT_TRANSCRIPT_START}\n"{transcript}"'
    conv = conv_templates[conv_mode].copy()
    conv.append_message(conv.roles[0], qs)
    conv.append_message(conv.roles[1], None)
    stop_str = conv.sep if conv.sep_style != SeparatorStyle.TWO else conv.sep2
    return conv.get_prompt(), stop_str


def guidance_for(guidance_scale, guidance_negative, question: str, conv_mode: str, tokenizer, video_token_len: int, use_vid_start_end: bool,
                 transcript=None):
    """`guidance_scale` / `guidance_negative` of the single-clip entry points as the `guidance` argument of model.generate (None: off -- no scale,
    or scale 1).  guidance_negative: "no_video" (default) -- the same conversation prompt built without the video tokens, i.e. contrast decoding
    against what the language model would say without the clip; "last_token" -- HF's default, the prompt's last id; any other string -- a
    negative prompt text, tokenised as it is."""
    from .guidance import Guidance
    if guidance_scale is None or float(guidance_scale) == 1.0:
        return None
    if not isinstance(guidance_negative, str):
        raise ValueError(f"`guidance_negative` has to be \"no_video\", \"last_token\" or a negative prompt text, but is {guidance_negative!r}")
    if guidance_negative == "last_token":
        return Guidance(float(guidance_scale), "last_token")
    if guidance_negative == "no_video":
        text, _ = build_prompt(question, conv_mode, video_token_len, use_vid_start_end, transcript, video=False)
    else:
        text = guidance_negative
    return Guidance(float(guidance_scale), [list(tokenizer([text]).input_ids[0])])


def frames_to_pixels(video_frames, image_processor, vision_tower) -> torch.Tensor:
    """Frames -> normalised NCHW tensor on the tower's device.  uint8 arrays already at the crop size take the fused
    HIP path (pgv_preprocess_u8 == CLIPImageProcessor for crop-sized frames); anything else goes through
    the caller's image_processor exactly like the reference (inference.py:86-89)."""
    S = vision_tower.config.image_size
    from .feature_extraction import NativeFrames
    if isinstance(video_frames, NativeFrames):
        # frames at the decoder's resolution: load_video's nearest resize + CLIPImageProcessor in one HIP pass (pgv_ingest_u8)
        if video_frames.shape == (S, S):
            dev = vision_tower.device
            return _lib.Context.get(dev).ingest_u8(torch.from_numpy(video_frames.array).to(dev), S, vision_tower.dtype)
        video_frames = video_frames.resized()                # not the tower's crop size: host resize, then the caller's image_processor
        video_frames = [video_frames[i] for i in range(video_frames.shape[0])]
    if isinstance(video_frames, np.ndarray) and video_frames.dtype == np.uint8 and video_frames.shape[1:] == (S, S, 3):
        dev = vision_tower.device
        return _lib.Context.get(dev).preprocess_u8(torch.from_numpy(video_frames).to(dev), vision_tower.dtype)
    if torch.is_tensor(video_frames) and video_frames.dtype == torch.uint8 and tuple(video_frames.shape[1:]) == (S, S, 3):
        dev = vision_tower.device
        return _lib.Context.get(dev).preprocess_u8(video_frames.to(dev).contiguous(), vision_tower.dtype)
    px = image_processor.preprocess(video_frames, return_tensors="pt")["pixel_values"]
    return px.to(vision_tower.dtype).to(vision_tower.device)


def video_features(video_frames, vision_tower, image_processor) -> torch.Tensor:
    """frames -> [100 + P, 1024] fp16 pooled CLIP features (inference.py:86-95)."""
    image_tensor = frames_to_pixels(video_frames, image_processor, vision_tower)
    with torch.no_grad():
        out = vision_tower(image_tensor, output_hidden_states=True)
        frame_features = out.hidden_states[-2][:, 1:]          # second-to-last layer, CLS dropped
    return get_spatio_temporal_features_torch(frame_features)


GROUP_UPLOAD_MAX_BYTES = 512 << 20      # native-resolution bytes uploaded and ingested together (a run of same-sized clips is cut at this budget)


def video_features_batch(clips, vision_tower, image_processor, timings=None):
    """Several clips (ragged frame counts) -> list of [100 + P, 1024] fp16 pooled features with ONE tower pass over the concatenated frames.
    The tower is bitwise batch-split invariant (tests/test_gpu_vision.py::test_vit_100_frames_properties), so every entry equals
    `video_features(clip)` bit for bit; what changes is the launch shape: 8 clips x 100 frames fill the persistent GEMM's 256 CUs with
    3216 + tiles per launch instead of 404, and there is one launch sequence instead of eight.  Clips that share a native resolution are
    uploaded and ingested (nearest resize + CLIP normalisation, pgv_ingest_u8) together, in runs of at most GROUP_UPLOAD_MAX_BYTES
    native bytes copied into ONE destination buffer (no per-clip device tensors + torch.cat: the transient device memory of a group is the
    run's bytes once, not twice -- the per-clip DEVICE_RESIZE_MAX_BYTES bound of load_video is not undone by grouping).
    `timings` (a dict) receives upload_ingest_s / tower_pool_s from events on the launch stream (one synchronisation at the end)."""
    from .feature_extraction import NativeFrames
    S = vision_tower.config.image_size
    dev = vision_tower.device
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timings is not None else None
    if ev:
        ev[0].record()
    px_parts, counts = [], []
    i = 0
    while i < len(clips):
        c = clips[i]
        j = i + 1
        if isinstance(c, NativeFrames) and c.shape == (S, S):
            # run of clips decoded at the same native resolution: one destination buffer, one ingest launch
            run_bytes = c.array.nbytes
            while (j < len(clips) and isinstance(clips[j], NativeFrames) and clips[j].shape == (S, S) and clips[j].array.shape[1:] == c.array.shape[1:]
                   and run_bytes + clips[j].array.nbytes <= GROUP_UPLOAD_MAX_BYTES):
                run_bytes += clips[j].array.nbytes
                j += 1
            host = [torch.as_tensor(x.array) for x in clips[i:j]]
            if len(host) == 1:
                up = host[0].to(dev, non_blocking=True)
            else:
                up = torch.empty((sum(int(h.shape[0]) for h in host),) + tuple(host[0].shape[1:]), dtype=torch.uint8, device=dev)
                o = 0
                for h in host:
                    up[o:o + h.shape[0]].copy_(h, non_blocking=True)
                    o += int(h.shape[0])
            px_parts.append(_lib.Context.get(dev).ingest_u8(up.contiguous(), S, vision_tower.dtype))
            del up
            counts.extend(int(h.shape[0]) for h in host)
        else:
            px = frames_to_pixels(c, image_processor, vision_tower)
            px_parts.append(px)
            counts.append(int(px.shape[0]))
        i = j
    px = torch.cat(px_parts) if len(px_parts) > 1 else px_parts[0]
    del px_parts
    if ev:
        ev[1].record()
    with torch.no_grad():
        hid = vision_tower(px, output_hidden_states=True).hidden_states[-2]
    out, off = [], 0
    for t in counts:
        out.append(get_spatio_temporal_features_torch(hid[off:off + t, 1:]))
        off += t
    if ev:
        ev[2].record()
        ev[2].synchronize()
        timings.update(upload_ingest_s=ev[0].elapsed_time(ev[1]) * 1e-3, tower_pool_s=ev[1].elapsed_time(ev[2]) * 1e-3, frames=int(sum(counts)))
    return out


def _infer_generate(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len, transcript, do_sample,
                    temperature, max_new_tokens, features, generate_kwargs):
    """The generate() call of `video_chatgpt_infer` -> (what generate returned, its sequences, prompt length, stop string).  The keywords
    `guidance_scale` / `guidance_negative` among generate_kwargs become generate's `guidance` (guidance_for)."""
    use_se = model.get_model().vision_config.use_vid_start_end
    prompt, stop_str = build_prompt(question, conv_mode, video_token_len, use_se, transcript)
    generate_kwargs = dict(generate_kwargs)
    scale, negative = generate_kwargs.pop("guidance_scale", None), generate_kwargs.pop("guidance_negative", "no_video")
    guide = guidance_for(scale, negative, question, conv_mode, tokenizer, video_token_len, use_se, transcript)
    if guide is not None:
        generate_kwargs["guidance"] = guide
    inputs = tokenizer([prompt])
    feats = features if features is not None else video_features(video_frames, vision_tower, image_processor)
    input_ids = torch.as_tensor(inputs.input_ids)
    stopping_criteria = KeywordsStoppingCriteria([stop_str], tokenizer, input_ids)
    with torch.inference_mode():
        out = model.generate(input_ids, video_spatio_temporal_features=feats.unsqueeze(0), do_sample=do_sample,
                             temperature=temperature, max_new_tokens=max_new_tokens, stopping_criteria=[stopping_criteria], **generate_kwargs)
    output_ids = out if torch.is_tensor(out) else out.sequences
    n_in = input_ids.shape[1]
    n_diff = int((input_ids.to(output_ids.device) != output_ids[:, :n_in]).sum())
    if n_diff > 0:
        print(f"[Warning] {n_diff} output_ids are not the same as the input_ids")
    return out, output_ids, n_in, stop_str


def video_chatgpt_infer_ids(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len,
                            transcript=None, do_sample=True, temperature=0.2, max_new_tokens=1024, features=None, **generate_kwargs):
    """`video_chatgpt_infer` up to (not including) the detokenisation: -> (generated token ids [n] as a list, stop string).  The runners'
    sampling path collates these ids through the same fixed-shape all-gather as the greedy path (parallel.gather_answers) and decodes them
    on every rank.  `features`: pooled [100 + P, 1024] features computed earlier for this clip (skips the tower).  `generate_kwargs`
    (top_p, repetition_penalty, ...) go to model.generate as they are."""
    _out, output_ids, n_in, stop_str = _infer_generate(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len,
                                                       transcript, do_sample, temperature, max_new_tokens, features, generate_kwargs)
    return output_ids[0, n_in:].tolist(), stop_str


def guidance_kwargs(guidance_scale, guidance_negative) -> dict:
    """The two guidance keywords as _infer_generate takes them: {} when no scale asks anything, so that a plain call stays the call it has always been."""
    if guidance_scale is None or float(guidance_scale) == 1.0:
        return {}
    return {"guidance_scale": guidance_scale, "guidance_negative": guidance_negative}


def video_chatgpt_infer(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len,
                        transcript=None, do_sample=True, temperature=0.2, max_new_tokens=1024, features=None, bans=None, filters=None, lookup=0,
                        lookup_ngram=2, lookup_sample=False, guidance_scale=None, guidance_negative="no_video", allowed=None):
    """Answer `question` about one clip.  Same positional signature and defaults as the reference
    (video_chatgpt/inference.py:47; do_sample=True, temperature=0.2, max_new_tokens=1024 at :109-111); pass
    do_sample=False for deterministic greedy decoding.  `features`: pooled features computed earlier (skips the tower).  `bans`
    (logit_bans.LogitBans or a dict of its fields): HF's -inf processors -- no_repeat_ngram, bad_words, suppress, begin_suppress, min_length,
    min_new_tokens -- passed to model.generate(bans=) as it is.  `filters` (sample_filters.SampleFilters or a dict of its fields): HF's sampling warpers
    behind top_p -- min_p, typical_p, epsilon_cutoff, eta_cutoff -- passed to model.generate(filters=) as it is.  `lookup` = D > 0 (needs
    do_sample=False): prompt-lookup speculative decoding, model.generate(lookup=D, lookup_ngram=n) -- the same answer in fewer passes over the weights.
    `lookup_sample=True` (with lookup = D > 0 and do_sample=True): the sampled form, model.generate(lookup_sample=True) -- bit for bit the sampled
    answer of the call without the two keywords for the same generator state.  `guidance_scale` = s (None or 1: off): classifier-free guidance,
    model.generate(guidance=) -- every pick reads s * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond), `uncond` the logits of
    `guidance_negative`: "no_video" (the same conversation prompt without the video tokens: contrast decoding against the language prior),
    "last_token" (HF's default negative) or a negative prompt text.  `allowed` (allowed.TokenAutomaton): constrained decoding,
    model.generate(allowed=) -- the answer is a path of the automaton, e.g. TokenAutomaton.from_texts(tokenizer, ["yes", "no"])."""
    new_ids, stop_str = video_chatgpt_infer_ids(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len,
                                                transcript, do_sample, temperature, max_new_tokens, features,
                                                **given(bans=bans, filters=filters, lookup=lookup, lookup_ngram=lookup_ngram, lookup_sample=lookup_sample, allowed=allowed),
                                                **guidance_kwargs(guidance_scale, guidance_negative))
    outputs = tokenizer.batch_decode([new_ids], skip_special_tokens=True)[0]
    return outputs.strip().rstrip(stop_str).strip()


def video_chatgpt_infer_logprobs(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len,
                                 transcript=None, do_sample=True, temperature=0.2, max_new_tokens=1024, features=None, bans=None, filters=None, lookup=0,
                                 lookup_ngram=2, lookup_sample=False, guidance_scale=None, guidance_negative="no_video", allowed=None, **generate_kwargs):
    """`video_chatgpt_infer` that also says how probable the answer it produced was (model.generate(output_logprobs=True): recorded on the device
    at pick time, no second prefill).  Returns a dict: "text" (what video_chatgpt_infer returns), "ids" (the generated token ids),
    "token_logprobs" (per id, the model's own log-probability: HF's compute_transition_scores on the raw logits -- what video_chatgpt_score
    gives for the same ids), "transition_scores" (per id, the log of the probability the pick used, after repetition penalty / temperature /
    top-k / top-p) and "logprob" (the fp64 sum of token_logprobs).  `lookup` / `lookup_sample` keep the signature of
    video_chatgpt_infer; lookup steps record no log-probabilities, so anything but 0 / False is refused by generate().  `guidance_scale` /
    `guidance_negative` likewise: a guided pick records none, so a scale other than None / 1 is refused by generate().  `allowed`
    (allowed.TokenAutomaton): constrained decoding, as in video_chatgpt_infer -- "transition_scores" are then normalised over the allowed tokens."""
    asked = dict(given(bans=bans, filters=filters, lookup=lookup, lookup_ngram=lookup_ngram, lookup_sample=lookup_sample, allowed=allowed),
                 **guidance_kwargs(guidance_scale, guidance_negative))
    out, output_ids, n_in, stop_str = _infer_generate(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len,
                                                      transcript, do_sample, temperature, max_new_tokens, features,
                                                      dict(generate_kwargs, output_logprobs=True, **asked))
    new_ids = output_ids[0, n_in:].tolist()
    text = tokenizer.batch_decode([new_ids], skip_special_tokens=True)[0].strip().rstrip(stop_str).strip()
    n = len(new_ids)
    return {"text": text, "ids": new_ids, "token_logprobs": out.token_logprobs[0, :n].tolist(), "transition_scores": out.transition_scores[0, :n].tolist(),
            "logprob": float(out.sequence_logprob[0])}


def video_chatgpt_infer_samples(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len, n,
                                transcript=None, temperature=0.2, max_new_tokens=1024, features=None, **generate_kwargs):
    """n sampled answers to one question about one clip for the price of ONE CLIP pass and ONE prefill (model.generate(samples_per_prompt=n):
    the prompt's KV-cache slot is forked n ways on the device, pgv_kv_fork) -- the raw material of best-of-N ranking and self-consistency voting.
    Always samples (do_sample=True; greedy decoding has one answer).  The stop string ends each answer on its own (generate's `stop_strings`, the
    batched form of the reference's KeywordsStoppingCriteria).  Returns a list of n dicts shaped like video_chatgpt_infer_logprobs', in sample
    order: "text", "ids", "token_logprobs", "transition_scores", "logprob".  `features`: pooled features computed earlier (skips the tower);
    `generate_kwargs` (top_p, repetition_penalty, generator, ...) go to model.generate as they are."""
    prompt, stop_str = build_prompt(question, conv_mode, video_token_len, model.get_model().vision_config.use_vid_start_end, transcript)
    input_ids = torch.as_tensor(tokenizer([prompt]).input_ids)
    feats = features if features is not None else video_features(video_frames, vision_tower, image_processor)
    with torch.inference_mode():
        out = model.generate(input_ids, video_spatio_temporal_features=feats.unsqueeze(0), do_sample=True, temperature=temperature,
                             max_new_tokens=max_new_tokens, stop_strings=[stop_str], tokenizer=tokenizer, samples_per_prompt=n,
                             **dict(generate_kwargs, output_logprobs=True))
    n_in = input_ids.shape[1]
    res = []
    for j in range(int(n)):
        k = int(out.new_lengths[j])                 # the rows of a batch are padded to the longest answer: cut each at its own length
        new_ids = out.sequences[j, n_in:n_in + k].tolist()
        text = tokenizer.batch_decode([new_ids], skip_special_tokens=True)[0].strip().rstrip(stop_str).strip()
        res.append({"text": text, "ids": new_ids, "token_logprobs": out.token_logprobs[j, :k].tolist(),
                    "transition_scores": out.transition_scores[j, :k].tolist(), "logprob": float(out.sequence_logprob[j])})
    return res


def video_chatgpt_infer_beams(video_frames, question, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len, beams,
                              transcript=None, length_penalty=None, early_stopping=None, max_new_tokens=1024, features=None, **generate_kwargs):
    """The beam-search answer to one question about one clip (model.generate(beams=K): HF's generate(num_beams=K) on the device, K beams from ONE
    CLIP pass and ONE prefill).  A beam ends on EOS or the budget; a stop string that is ordinary text is cut afterwards, as the reference's own
    post-processing does (inference.py:119-123).  Returns a dict: "text", "ids" (the generated token ids of the best hypothesis, up to the cut)
    and "score" (HF's sequences_scores of the uncut hypothesis: its summed token log-probabilities over length ** length_penalty).
    `length_penalty` / `early_stopping`: None = the model's generation config, else HF's defaults; `features`: pooled features computed
    earlier (skips the tower); `generate_kwargs` go to model.generate as they are."""
    from .model.utils import first_stop_length
    prompt, stop_str = build_prompt(question, conv_mode, video_token_len, model.get_model().vision_config.use_vid_start_end, transcript)
    input_ids = torch.as_tensor(tokenizer([prompt]).input_ids)
    feats = features if features is not None else video_features(video_frames, vision_tower, image_processor)
    with torch.inference_mode():
        out = model.generate(input_ids, video_spatio_temporal_features=feats.unsqueeze(0), do_sample=False, max_new_tokens=max_new_tokens, beams=beams,
                             length_penalty=length_penalty, early_stopping=early_stopping, **dict(generate_kwargs, output_beam_scores=int(beams) > 1))
    n_in = input_ids.shape[1]
    if torch.is_tensor(out):                        # beams == 1: greedy decoding has no beam score
        new_ids, score = out[0, n_in:].tolist(), None
    else:
        new_ids, score = out.sequences[0, n_in:n_in + int(out.new_lengths[0])].tolist(), float(out.sequences_scores[0])
    n = first_stop_length(new_ids, tokenizer, [stop_str]) if stop_str else None
    if n is not None:
        new_ids = new_ids[:n]
    text = tokenizer.batch_decode([new_ids], skip_special_tokens=True)[0].strip()
    return {"text": text.rstrip(stop_str).strip() if stop_str else text, "ids": new_ids, "score": score}


def best_sample(samples) -> int:
    """Index of the sample with the largest "logprob" (video_chatgpt_infer_samples' dicts); ties go to the first."""
    if not samples:
        raise ValueError("best_sample: no samples")
    best = 0
    for i, s_ in enumerate(samples):
        if s_["logprob"] > samples[best]["logprob"]:
            best = i
    return best


def majority_sample(samples) -> int:
    """Self-consistency vote over video_chatgpt_infer_samples' dicts: index of the first sample carrying the most frequent "text"; among equally
    frequent texts the one whose samples' "logprob" values sum highest wins, then the one seen first."""
    if not samples:
        raise ValueError("majority_sample: no samples")
    votes = {}                  # text -> [count, summed logprob, first index]; dicts keep insertion order
    for i, s_ in enumerate(samples):
        v = votes.setdefault(s_["text"], [0, 0.0, i])
        v[0] += 1
        v[1] += float(s_["logprob"])
    best = None
    for v in votes.values():
        if best is None or (v[0], v[1]) > (best[0], best[1]):
            best = v
    return best[2]


def video_chatgpt_score(video_frames, question, answers, conv_mode, model, vision_tower, tokenizer, image_processor, video_token_len,
                        transcript=None, features=None):
    """How likely is each of `answers` (a list of candidate strings) as the reply to `question` about one clip: the prompt of
    `video_chatgpt_infer`, each candidate teacher-forced behind it.  CLIP runs once (`features`: pooled features computed earlier skip it) and
    all candidates go through ONE model.score call as B sequences.  A candidate's ids are tokenizer(prompt + answer + stop_str) cut at the
    prompt's length (the usual context / continuation split; a tokenizer that merges across the boundary raises in continuation_labels), so
    the scored span includes the stop token(s).  Returns one dict per candidate, in order: "logprob" (sum over the span), "tokens" (its
    length), "mean_logprob", "greedy" (every scored position's argmax is its target: greedy decoding would have produced this candidate)."""
    prompt, stop_str = build_prompt(question, conv_mode, video_token_len, model.get_model().vision_config.use_vid_start_end, transcript)
    prompt_ids = tokenizer([prompt]).input_ids[0]
    feats = features if features is not None else video_features(video_frames, vision_tower, image_processor)
    full = [list(tokenizer([prompt + a + stop_str]).input_ids[0]) for a in answers]
    labels = [continuation_labels(prompt_ids, f) for f in full]
    with torch.inference_mode():
        out = model.score(full, labels, video_spatio_temporal_features=feats.unsqueeze(0))
    res = []
    for b in range(len(full)):
        m = out.scored[b]
        n = int(out.counts[b])
        lp = float(out.sequence_logprob[b])
        greedy = bool((out.argmax[b][m].long() == torch.tensor(labels[b], dtype=torch.long)[m]).all())
        res.append({"logprob": lp, "tokens": n, "mean_logprob": lp / n if n else float("nan"), "greedy": greedy})
    return res
