"""Shared core of the eval runners: answer a list of (video, question) tasks data-parallel over the ranks of a
`torch.distributed.run` launch and hand every rank the same list of prediction strings.

The reference's runners (video_chatgpt/eval/run_inference_*.py) all share one loop -- load the video, call
`video_chatgpt_infer`, append the sample with its prediction, print and skip on any exception -- and differ only in how a
sample names its video file and which keys the output record carries.  Here that loop is one function: tasks are sharded over
the ranks (one process per GPU), each rank answers its shard in groups of `--batch` clips: ONE ViT pass over all frames of the group
(the launch shape bench.py measures), batched prefill + KV-cached greedy decode in libpgv, while a background thread decodes the next
group's frames into pinned memory; the only collective is the final all-gather of the answer token ids (video_llava_amd/parallel.py).
A task whose video is missing or fails yields None (the reference prints and leaves the sample out).
`--schedule refill` keeps the groups for the host half and the tower pass, but decodes through continuous.generate_continuous: a slot whose
answer has ended takes the next task at once.  `--do_sample` restores the reference's temperature-0.2 sampling: through `video_chatgpt_infer`
one task at a time, or batched with `--schedule refill`, every task drawing from its own seeded stream.  `_Runner` holds what the schedules share.
"""
from __future__ import annotations

import torch


MAX_BATCH = 64      # pgv_kv_create: the decode GEMVs tile the batch over up to 4 MFMA column tiles of 16 sequences (weights streamed once)


def add_runtime_arguments(parser):
    """Flags this package adds to every runner on top of the reference's."""
    parser.add_argument("--batch", type=_batch_arg, default="auto", metavar=f"[auto|1-{MAX_BATCH}]",
                        help=f"clips answered together per GPU (greedy decoding; the decode kernels tile at most {MAX_BATCH} sequences; the weight stream of a "
                             "token step is shared by the whole group, so larger groups raise videos/s: 8.9 / 13.4 / 16.2 / 18.9 at 8 / 16 / 32 / 64 on MI355X). "
                             "auto (default): the largest of 8 / 16 / 32 / 64 whose KV cache + tower workspace fit the GPU's free memory (pick_batch)")
    parser.add_argument("--max_new_tokens", type=int, default=1024)
    parser.add_argument("--do_sample", action="store_true", help="reference decoding: temperature-0.2 sampling, one clip at a time (with --schedule refill: "
                                                                 "batched, every task drawing from its own seeded stream)")
    parser.add_argument("--top_p", type=float, default=None,
                        help="nucleus filter of --do_sample (HF TopPLogitsWarper); default: the checkpoint's generation_config.json, else 1.0")
    parser.add_argument("--repetition_penalty", type=float, default=None,
                        help="HF RepetitionPenaltyLogitsProcessor over prompt + answer, greedy and sampled; default: the checkpoint's "
                             "generation_config.json, else 1.0")
    parser.add_argument("--min_p", type=float, default=None, metavar="P",
                        help="--do_sample: HF MinPLogitsWarper behind --top_p, on the device (generate(filters=)): keeps the tokens whose probability is at "
                             "least P x the most likely token's; default: the checkpoint's generation_config.json when another of these four flags is "
                             "given, else off")
    parser.add_argument("--typical_p", type=float, default=None, metavar="P", help="--do_sample: HF TypicalLogitsWarper (locally typical mass P); 1: off")
    parser.add_argument("--epsilon_cutoff", type=float, default=None, metavar="E", help="--do_sample: HF EpsilonLogitsWarper (probability floor E); 0: off")
    parser.add_argument("--eta_cutoff", type=float, default=None, metavar="E", help="--do_sample: HF EtaLogitsWarper (entropy-dependent floor); 0: off")
    parser.add_argument("--no_repeat_ngram", type=int, default=0, metavar="N",
                        help="HF NoRepeatNGramLogitsProcessor (no_repeat_ngram_size=N) over prompt + answer, on the device (generate(bans=)): no n-gram of "
                             "N tokens occurs twice -- the remedy for greedy answers that loop; 0 (default): off")
    parser.add_argument("--min_new_tokens", type=int, default=0, metavar="N",
                        help="HF MinNewTokensLengthLogitsProcessor: the end-of-sequence token is banned until the answer has N tokens; 0 (default): off")
    parser.add_argument("--suppress_tokens", type=_id_list_arg, default=(), metavar="ID[,ID...]",
                        help="HF SuppressTokensLogitsProcessor: token ids that are never generated; default: none")
    parser.add_argument("--schedule", choices=("group", "refill"), default="group",
                        help="group (default): answer the shard in static groups of --batch clips, each decoding until its longest answer ends; refill: keep "
                             "--batch decode slots busy and refill a slot with the next task as soon as its answer ends (continuous batching, "
                             "video_llava_amd/continuous.py) -- the same answers, fewer wasted decode steps when answer lengths differ")
    parser.add_argument("--seed", type=int, default=0,
                        help="--schedule refill --do_sample: task i samples from torch.Generator seeded with seed * 1000003 + i, so its answer does "
                             "not depend on --batch or on the slot it lands in")
    parser.add_argument("--samples_per_prompt", type=int, default=1, metavar="N",
                        help="--schedule refill --do_sample: N sampled answers per task from ONE prefill of its prompt (sample j seeded "
                             "continuous.sample_seed(task seed, j)); --sample_pick chooses the one that is recorded")
    parser.add_argument("--sample_pick", choices=("best", "majority"), default="best",
                        help="best (default): the sample with the largest summed log-probability (inference.best_sample); majority: the most frequent "
                             "answer string, ties to the larger summed log-probability, then to the first (inference.majority_sample)")
    parser.add_argument("--samples_out", default=None, metavar="FILE.jsonl",
                        help="--samples_per_prompt: append one JSON line per task with all its samples (text, ids, logprob) and the index picked "
                             "(rank-local file `FILE.jsonl.rank<r>` when world > 1)")
    parser.add_argument("--beams", type=int, default=1, metavar="K",
                        help=f"beam search with K <= {MAX_BEAMS} beams per clip as HF's generate(num_beams=K) computes it, on the device (generate(beams=K)); "
                             "--schedule group only, not with --do_sample or --samples_per_prompt; a group holds --batch clips x K sequences "
                             "(--batch auto counts K decode slots per clip)")
    parser.add_argument("--length_penalty", type=float, default=None, help="--beams: HF's length_penalty; default: the checkpoint's generation_config.json, else 1.0")
    parser.add_argument("--early_stopping", choices=("false", "true", "never"), default=None,
                        help="--beams: HF's early_stopping; default: the checkpoint's generation_config.json, else false")
    parser.add_argument("--lookup", type=int, default=0, metavar="D",
                        help=f"greedy decoding as prompt-lookup speculative decoding with D <= {MAX_LOOKUP} drafts per sequence and step (generate(lookup=D)): the "
                             "greedy answers, bit for bit, in fewer passes over the weights when answers repeat themselves or quote the prompt; --schedule group "
                             "only, not with --do_sample (unless --lookup_sample), --beams, --samples_per_prompt, --repetition_penalty or the ban flags; a group holds --batch clips x "
                             "(1 + D) rows (--batch auto counts 1 + D rows per clip); --timings lines gain lookup_steps_group / lookup_emitted_group")
    parser.add_argument("--lookup_ngram", type=int, default=2, metavar="N", help="--lookup: the largest n-gram matched, 1 .. 4 (HF: max_matching_ngram_size)")
    parser.add_argument("--lookup_sample", action="store_true",
                        help="--lookup D --do_sample: lookup steps for the sampled run (generate(lookup_sample=True)) -- every draft is verified against the "
                             "pick from the uniform the plain run draws for that token, so the answers are bit for bit those of --do_sample alone; lifts "
                             "only the --do_sample refusal of --lookup")
    from ..chat import add_answer_choice_flags, add_guidance_flags
    add_answer_choice_flags(parser)     # --answer_choices "yes,no" / --answer_choices_file F: generate(allowed=), every schedule
    add_guidance_flags(parser)          # --guidance_scale S / --guidance_negative: --batch and --batch auto count two rows per clip
    parser.add_argument("--timings", default=None, metavar="OUT.jsonl",
                        help="append one JSON line per answered task (rank-local file `OUT.jsonl.rank<r>` when world > 1): frame load, upload + ingest, "
                             "tower + pool, prefill, decode seconds, generated tokens, group size, feature-cache hit (SURVEY 5: per-clip stage timings)")
    parser.add_argument("--feature-cache", type=int, default=FEATURE_CACHE_CLIPS, metavar="N",
                        help="pooled video features of the last N distinct clips stay on the device and are reused by later questions about the same "
                             "video (ActivityNet-QA asks several per clip; the reference recomputes them, chat.py:137-144); 0 disables")
    # flags that only mean something together are checked once all of them are parsed
    inner = parser.parse_known_args

    def parse_known_args(args=None, namespace=None):
        ns, rest = inner(args, namespace)
        if ns.samples_per_prompt < 1 or ns.samples_per_prompt > MAX_BATCH:
            parser.error(f"--samples_per_prompt {ns.samples_per_prompt} outside [1, {MAX_BATCH}]")
        if ns.samples_per_prompt > 1 and not (ns.schedule == "refill" and ns.do_sample):
            parser.error(f"--samples_per_prompt {ns.samples_per_prompt} needs --schedule refill --do_sample")
        if ns.batch != "auto" and ns.samples_per_prompt > ns.batch:
            parser.error(f"--samples_per_prompt {ns.samples_per_prompt} exceeds the --batch {ns.batch} decode slots")
        try:
            if filters_from_args(ns) and not ns.do_sample:        # validates the four flags, HF's wording
                raise ValueError("--min_p / --typical_p / --epsilon_cutoff / --eta_cutoff need --do_sample (they filter a sampled pick)")
            K, _, _ = check_beam_args(ns)
            lookup_from_args(ns)
            guidance_scale_from_args(ns)
            answer_choices_from_args(ns)
            if bans_from_args(ns) and K > 1:        # validates the three flags, HF's wording
                raise ValueError(f"--beams {K} cannot be combined with --no_repeat_ngram / --min_new_tokens / --suppress_tokens (the beam pick applies "
                                 f"no logits processor)")
        except (ValueError, OSError) as e:
            parser.error(str(e))
        return ns, rest

    parser.parse_known_args = parse_known_args
    return parser


MAX_BEAMS = 8       # generation.MAX_BEAMS
MAX_LOOKUP = 15     # generation.MAX_LOOKUP


def lookup_from_args(ns) -> dict:
    """--lookup / --lookup_ngram / --lookup_sample of a parsed command line as generate() arguments ({}: off); ValueError names the flag lookup cannot run with."""
    from ..generation import check_lookup
    D = int(getattr(ns, "lookup", 0) or 0)
    sampled = bool(getattr(ns, "lookup_sample", False))
    if sampled and not getattr(ns, "do_sample", False):
        raise ValueError("--lookup_sample needs --do_sample (greedy lookup is --lookup D alone)")
    if sampled and D == 0:
        raise ValueError("--lookup_sample needs --lookup D with D >= 1 drafts per step")
    if D == 0:
        return {}
    D, n = check_lookup(D, getattr(ns, "lookup_ngram", 2), who="--lookup")
    if getattr(ns, "do_sample", False) and not sampled:
        raise ValueError(f"--lookup {D} cannot be combined with --do_sample (a sampled token has no draft to verify)")
    if int(getattr(ns, "beams", 1)) > 1:
        raise ValueError(f"--lookup {D} cannot be combined with --beams {ns.beams} (a beam step already runs K rows per prompt)")
    if getattr(ns, "schedule", "group") == "refill":
        raise ValueError(f"--lookup {D} cannot be combined with --schedule refill (refill needs per-slot lengths on the host between chunks)")
    if int(getattr(ns, "samples_per_prompt", 1)) > 1:
        raise ValueError(f"--lookup {D} cannot be combined with --samples_per_prompt {ns.samples_per_prompt}")
    rp = getattr(ns, "repetition_penalty", None)
    if rp is not None and float(rp) != 1.0:
        raise ValueError(f"--lookup {D} cannot be combined with --repetition_penalty {rp} (the drafts are verified against the plain arg-max)")
    if bans_from_args(ns):
        raise ValueError(f"--lookup {D} cannot be combined with --no_repeat_ngram / --min_new_tokens / --suppress_tokens (the drafts are verified against "
                         f"the plain arg-max)")
    batch = getattr(ns, "batch", "auto")
    if batch != "auto" and batch * (1 + D) > MAX_BATCH:
        raise ValueError(f"--batch {batch} clips x (1 + --lookup {D}) rows exceed the {MAX_BATCH} rows of a decode step")
    return {"lookup": D, "lookup_ngram": n, **({"lookup_sample": True} if sampled else {})}


def answer_choices_from_args(ns):
    """--answer_choices / --answer_choices_file of a parsed command line -> the answers as a list of strings (None: no constraint); ValueError names
    the flag constrained decoding cannot run with."""
    from ..chat import answer_choices_from_flags
    return answer_choices_from_flags(getattr(ns, "answer_choices", None), getattr(ns, "answer_choices_file", None), getattr(ns, "lookup", 0),
                                     getattr(ns, "beams", 1))


def allowed_from_args(ns, tokenizer) -> dict:
    """The same two flags as generate() / generate_continuous() keywords: {} when neither is given, else {"allowed": TokenAutomaton} -- ONE automaton
    for every question of the run, compiled once per call site from the run's tokenizer (TokenAutomaton.from_texts)."""
    from ..chat import allowed_from_choices
    texts = answer_choices_from_args(ns)
    return {} if texts is None else {"allowed": allowed_from_choices(tokenizer, texts)}


def guidance_scale_from_args(ns):
    """--guidance_scale / --guidance_negative of a parsed command line -> the scale (None: off); ValueError names the flag guidance cannot run
    with.  A group holds --batch clips x 2 rows: the clip's prompt and its negative."""
    from ..chat import guidance_from_flags
    scale = guidance_from_flags(getattr(ns, "guidance_scale", None), getattr(ns, "guidance_negative", "no_video"), getattr(ns, "lookup", 0),
                                getattr(ns, "beams", 1), getattr(ns, "samples_per_prompt", 1), getattr(ns, "schedule", "group"))
    batch = getattr(ns, "batch", "auto")
    if scale is not None and batch != "auto" and 2 * batch > MAX_BATCH:
        raise ValueError(f"--batch {batch} clips x 2 rows under --guidance_scale exceed the {MAX_BATCH} rows of a decode step")
    return scale


def check_beam_args(ns):
    """--beams / --length_penalty / --early_stopping of a parsed command line -> (K, length_penalty or None, early_stopping or None) as generate()
    takes them (None: the generation config decides); ValueError names the flag a beam search cannot run with."""
    K = int(getattr(ns, "beams", 1))
    if not 1 <= K <= MAX_BEAMS:
        raise ValueError(f"--beams {K} outside [1, {MAX_BEAMS}]")
    early = {None: None, "false": False, "true": True, "never": "never"}[getattr(ns, "early_stopping", None)]
    lp = getattr(ns, "length_penalty", None)
    if K == 1:
        return K, lp, early
    if getattr(ns, "do_sample", False):
        raise ValueError(f"--beams {K} cannot be combined with --do_sample (beam search picks by score)")
    if getattr(ns, "schedule", "group") == "refill":
        raise ValueError(f"--beams {K} cannot be combined with --schedule refill (the beams of a clip are a fixed group of decode slots)")
    if int(getattr(ns, "samples_per_prompt", 1)) > 1:
        raise ValueError(f"--beams {K} cannot be combined with --samples_per_prompt {ns.samples_per_prompt}")
    batch = getattr(ns, "batch", "auto")
    if batch != "auto" and batch * K > MAX_BATCH:
        raise ValueError(f"--batch {batch} clips x --beams {K} exceed the {MAX_BATCH} decode slots of a group")
    return K, lp, early


def _id_list_arg(text):
    try:
        ids = tuple(int(t) for t in text.split(",") if t.strip() != "")
    except ValueError:
        ids = None
    if ids is None or any(t < 0 for t in ids):
        import argparse
        raise argparse.ArgumentTypeError(f"--suppress_tokens {text!r} is not a comma-separated list of non-negative token ids")
    return ids


def bans_from_args(ns) -> dict:
    """--no_repeat_ngram / --min_new_tokens / --suppress_tokens of a parsed command line as generate() / generate_continuous() keywords: {} when all
    are off, else {"bans": LogitBans}.  (Bad words are not a flag: tokenising them, with the prefix-space pitfalls, belongs to the caller.)"""
    from ..logit_bans import LogitBans
    b = LogitBans(no_repeat_ngram=getattr(ns, "no_repeat_ngram", 0), min_new_tokens=getattr(ns, "min_new_tokens", 0),
                  suppress=tuple(getattr(ns, "suppress_tokens", ()) or ()))
    b.check(1 << 31)            # HF's wording for a negative value; the vocabulary is checked by generate()
    return {} if b.neutral else {"bans": b}


def filters_from_args(ns) -> dict:
    """--min_p / --typical_p / --epsilon_cutoff / --eta_cutoff of a parsed command line as generate() / generate_continuous() keywords: {} when none
    is given, else {"filters": {flag: value}} with the flags given only -- the rest comes from the model's generation config."""
    from ..sample_filters import HF_ARGUMENTS, SampleFilters
    given = {name: getattr(ns, name, None) for name in HF_ARGUMENTS}
    given = {k: v for k, v in given.items() if v is not None}
    SampleFilters.coerce(given).check()
    return {"filters": given} if given else {}


def _batch_arg(text):
    if text == "auto":
        return text
    n = int(text)
    if not 1 <= n <= MAX_BATCH:
        import argparse
        raise argparse.ArgumentTypeError(f"--batch {n} outside [1, {MAX_BATCH}]")
    return n


def batch_bytes(batch: int, model_config, image_size: int, max_new_tokens: int, frames_per_clip: int = 100, prompt_tokens: int | None = None) -> int:
    """Device bytes a group of `batch` clips needs beyond the weights: the decoder's KV cache + decode buffers for `batch` sequences of
    prompt + max_new_tokens positions, and the tower's per-pass workspace for batch x frames_per_clip frames (fp32 residual,
    16-bit operand / qkv / attention / MLP buffers of both lanes)."""
    c = model_config
    patches = (image_size // 14) ** 2
    prompt = prompt_tokens if prompt_tokens is not None else 100 + patches + 128
    seq = min((prompt + max_new_tokens + 63) // 64 * 64, int(getattr(c, "max_position_embeddings", 4096)))
    kv = 2 * c.num_hidden_layers * c.hidden_size * seq * 2 * batch
    logits = batch * (c.vocab_size + 64) * 4 * 3
    rows = batch * frames_per_clip * (patches + 1)
    vit = rows * (1024 * 4 + 1024 * 2 + 3072 * 2 + 1024 * 2 + 4096 * 2 + 16 * 8) + batch * frames_per_clip * image_size * image_size * 3 * (1 + 2)
    prefill = batch * prompt * (c.hidden_size * (4 + 2 + 6 + 2) + c.intermediate_size * 2)
    return int(kv + logits + max(vit, prefill))


def pick_batch(model_config, image_size: int, max_new_tokens: int, free_bytes: int, frames_per_clip: int = 100) -> int:
    """Largest group size in (64, 32, 16, 8) that fits 70 % of the free device memory (a real ActivityNet queue should run in
    the wide-batch regime the decode kernels support, not at a fixed 8); never below 8 -- smaller GPUs fail loudly in the allocation instead."""
    for b in (64, 32, 16):
        if batch_bytes(b, model_config, image_size, max_new_tokens, frames_per_clip) <= 0.7 * free_bytes:
            return b
    return 8


def setup(args, components=None):
    """-> (rank, world, components).  components = (model, vision_tower, tokenizer, image_processor, video_token_len) may be injected."""
    import os
    from .. import parallel
    if components is None and int(os.environ.get("WORLD_SIZE", "1")) > 1 and torch.cuda.is_available():
        # host placement FIRST: threads the process-group backend starts below inherit the mask
        parallel.pin_rank_to_numa_node(int(os.environ.get("LOCAL_RANK", "0")))
    rank, world, local = parallel.init_distributed()
    if components is None:
        from .model_utils import initialize_model
        if torch.cuda.is_available():
            torch.cuda.set_device(local)
        components = initialize_model(args.model_name, args.projection_path)
    if getattr(args, "use_asr", False):
        raise NotImplementedError("--use_asr needs the WhisperX transcript stack, which is outside this package's hot path")
    return rank, world, components


FEATURE_CACHE_CLIPS = 64      # x 0.73 MB ([356, 1024] fp16) at 224 px, 1.4 MB at 336 px


class FeatureCache:
    """LRU of pooled video features keyed by video path.  The prefetch thread only READS (`get`, which also refreshes recency and hands out a
    reference, so an entry evicted before its group runs stays alive for that group); the device thread inserts."""

    def __init__(self, capacity: int):
        import collections
        import threading
        self.capacity, self._d, self._lock = max(int(capacity), 0), collections.OrderedDict(), threading.Lock()
        self.hits = self.misses = 0

    def get(self, path):
        with self._lock:
            f = self._d.get(path)
            if f is not None:
                self._d.move_to_end(path)
                self.hits += 1
            else:
                self.misses += 1
            return f

    def put(self, path, feat):
        if self.capacity <= 0:
            return
        with self._lock:
            self._d[path] = feat
            self._d.move_to_end(path)
            while len(self._d) > self.capacity:
                self._d.popitem(last=False)


class _Cached:
    """Marker the prefetch thread returns for a clip whose pooled features are in the cache (no frames were read)."""

    def __init__(self, feat):
        self.feat = feat


class _Runner:
    """What the schedules of `answer_tasks` share on one rank: the host half of a group (`prepare`), its pooled features, a task's inputs,
    the answer collation (`toks`, `lens`) and the --timings lines; `infer_batch` / `infer_refill` / `infer_sampled` are the schedules.
    Length encoding: lens[j] = 0 = the task failed (no prediction), k + 1 = an answer of k tokens (k = 0 is a legitimate empty answer: the
    reference writes pred = '' when the first token is EOS)."""

    def __init__(self, args, tasks, components, load_frames, rank, tfile, sfile=None):
        from ..feature_extraction import PinnedRing
        self.args, self.tasks, self.load_frames, self.rank, self.tfile, self.sfile = args, tasks, load_frames, rank, tfile, sfile
        self.model, self.vision_tower, self.tokenizer, self.image_processor, self.video_token_len = components
        self.use_se = self.model.get_model().vision_config.use_vid_start_end
        self.allowed_kw = allowed_from_args(args, self.tokenizer)      # --answer_choices: one automaton for the run, compiled once ({}: off)
        self.cache = FeatureCache(getattr(args, "feature_cache", FEATURE_CACHE_CLIPS))
        self.ring = PinnedRing()
        self.stop_strs = {}             # task -> the stop string of its prompt
        self.group_no = 0

    def prepare(self, indices):
        """HOST half of a group, run one group ahead on the prefetch thread (parallel.run_sharded): decode / sample the frames of the group's
        distinct clips into pinned memory -- except clips whose pooled features are still cached from an earlier group.
        -> {path: frames | _Cached | Exception} (+ "__load_s__": {path: seconds})"""
        import time
        from ..feature_extraction import pin_frames
        self.ring.new_group()
        clips, load_s = {}, {}
        for idx in indices:
            path = self.tasks[idx]["path"]
            if path is None or path in clips:
                continue
            hit = self.cache.get(path)
            if hit is not None:
                clips[path] = _Cached(hit)
                continue
            t0 = time.perf_counter()
            try:
                clips[path] = pin_frames(self.load_frames(path), self.ring)
            except Exception as e:                                     # noqa: BLE001 -- reported per task below, like the reference's except
                clips[path] = e
            load_s[path] = time.perf_counter() - t0
        clips["__load_s__"] = load_s
        return clips

    def features_for(self, clips, tm):
        """{path: pooled features} for every usable clip of a group: cached ones as they are, the others through ONE tower pass
        (inference.video_features_batch; bitwise equal to per-clip passes)."""
        from .. import inference
        feat_of = {p: f.feat for p, f in clips.items() if isinstance(f, _Cached)}
        good = []
        for p, f in clips.items():
            if isinstance(f, (Exception, _Cached)):
                continue
            hit = self.cache.get(p)          # the prefetch thread runs one group ahead: a clip it loaded may have been pooled by the group in between
            if hit is not None:
                feat_of[p] = hit
                clips[p] = _Cached(hit)
            else:
                good.append(p)
        if good:
            try:
                fresh = dict(zip(good, inference.video_features_batch([clips[p] for p in good], self.vision_tower, self.image_processor, timings=tm)))
            except Exception as e:                                     # noqa: BLE001 -- one bad clip must not take the group down
                print(f"batched feature extraction failed ({e}); retrying the {len(good)} clips one by one")
                fresh = {}
                for p in good:
                    try:
                        fresh[p] = inference.video_features(clips[p], self.vision_tower, self.image_processor)
                    except Exception as e1:                            # noqa: BLE001
                        clips[p] = e1
            for p, f in fresh.items():
                self.cache.put(p, f)
            feat_of.update(fresh)
        return feat_of

    def group_features(self, clips):
        """Device half of a group, first part.  -> (feat_of, host): host is what the group's --timings lines say about that half."""
        load_s = clips.pop("__load_s__", {})
        tm_v = {} if self.tfile else None
        feat_of = self.features_for(clips, tm_v)
        n_fresh = sum(1 for f in clips.values() if not isinstance(f, (Exception, _Cached)))
        return feat_of, {"clips": clips, "load_s": load_s, "tm_v": tm_v or {}, "n_fresh": n_fresh}

    def failed(self, idx, why):
        print(f"Error processing video file '{self.tasks[idx]['name']}': {why}")

    def inputs(self, idx, clips, feat_of):
        """Task idx -> (prompt ids, pooled features, stop string); None after the reference's print-and-continue for a missing video, a clip
        that failed to load or pool, or a prompt that cannot be built."""
        from ..inference import build_prompt
        t = self.tasks[idx]
        if t["path"] is None:
            return self.failed(idx, "not found")
        try:
            if t["path"] not in feat_of:
                raise clips[t["path"]]
            prompt, stop = build_prompt(t["question"], self.args.conv_mode, self.video_token_len, self.use_se)
            ids = self.tokenizer([prompt]).input_ids[0]
            self.stop_strs[idx] = stop
            return ids, feat_of[t["path"]], stop
        except Exception as e:                                         # noqa: BLE001 -- the reference's print-and-continue
            return self.failed(idx, e)

    def record(self, toks, lens, j, new, strip_eos=True):
        """Answer `new` (ids) of row j: stripped from its EOS on, cut at --max_new_tokens."""
        eos = self.model.config.eos_token_id
        if strip_eos and eos is not None and eos in new:
            new = new[:new.index(eos)]
        new = new[:self.args.max_new_tokens]
        toks[j, :len(new)] = torch.tensor(new, dtype=torch.int32)
        lens[j] = len(new) + 1

    def write_timing(self, idx, length, group, host, tm_g, group_size):
        """One --timings line.  host: group_features' second result; tm_g: prefill_s / decode_s / steps of the generation the task was in."""
        import json
        t = self.tasks[idx]
        self.tfile.write(json.dumps({"task": idx, "video": t["name"], "rank": self.rank, "group": group, "group_size": group_size, "ok": length > 0,
                                     "tokens": max(length - 1, 0), "feature_cache_hit": isinstance(host["clips"].get(t["path"]), _Cached),
                                     "load_s": host["load_s"].get(t["path"], 0.0), "upload_ingest_s_group": host["tm_v"].get("upload_ingest_s", 0.0),
                                     "tower_pool_s_group": host["tm_v"].get("tower_pool_s", 0.0), "clips_in_tower_pass": host["n_fresh"],
                                     "prefill_s_group": tm_g.get("prefill_s"), "decode_s_group": tm_g.get("decode_s"),
                                     "decode_steps_group": tm_g.get("steps"),
                                     **({"lookup_steps_group": tm_g["lookup_steps"], "lookup_emitted_group": tm_g["lookup_emitted"]} if "lookup_steps" in tm_g else {})})
                         + "\n")

    def warpers(self):
        """--top_p / --repetition_penalty as generate() arguments: only the ones given, so the rest comes from the model's generation config."""
        given = {"top_p": getattr(self.args, "top_p", None), "repetition_penalty": getattr(self.args, "repetition_penalty", None)}
        return {k: v for k, v in given.items() if v is not None}

    def guidance(self, idxs) -> dict:
        """--guidance_scale / --guidance_negative as generate()'s `guidance` for the tasks idxs ({}: off): the "no_video" negative of a task is its
        conversation prompt built without the video tokens."""
        from ..guidance import Guidance
        from ..inference import build_prompt
        scale = guidance_scale_from_args(self.args)
        if scale is None:
            return {}
        if getattr(self.args, "guidance_negative", "no_video") == "last_token":
            return {"guidance": Guidance(scale, "last_token")}
        texts = [build_prompt(self.tasks[i]["question"], self.args.conv_mode, self.video_token_len, self.use_se, video=False)[0] for i in idxs]
        return {"guidance": Guidance(scale, [list(self.tokenizer([t]).input_ids[0]) for t in texts])}

    def infer_batch(self, indices, clips=None):
        """--schedule group -> (tokens [n, <= max_new] int32, lengths).  DEVICE half of a group: ONE tower pass over the frames of all distinct
        uncached clips of the group, then batched prefill + decode with the per-chunk stop-string check."""
        from ..continuous import split_refused
        feat_of, host = self.group_features(self.prepare(indices) if clips is None else clips)
        tm_g = {} if self.tfile else None
        toks, lens = torch.zeros(len(indices), self.args.max_new_tokens, dtype=torch.int32), [0] * len(indices)
        keep = []                                                      # (row, prompt ids, features, stop string) of the tasks that can run
        for j, idx in enumerate(indices):
            inp = self.inputs(idx, host["clips"], feat_of)
            if inp is not None:
                keep.append((j,) + inp)

        def generate(part, timings=None):
            # a stop string that IS the EOS piece (pg-video-llava: "</s>") is already handled on the device by the EOS flag; the host check
            # is for conv modes whose stop is ordinary text (default: "###") -- without it every group decodes max_new_tokens steps
            K, lp, early = check_beam_args(self.args)
            if K > 1:
                # a beam search ends on EOS or the budget; answer_tasks cuts a stop string that is ordinary text afterwards, as for any generate()
                return self.model.generate([ids for _, ids, _, _ in part], video_spatio_temporal_features=torch.stack([f for _, _, f, _ in part]),
                                           do_sample=False, max_new_tokens=self.args.max_new_tokens, timings=timings, beams=K, length_penalty=lp,
                                           early_stopping=early, **self.warpers()).cpu()
            return self.model.generate([ids for _, ids, _, _ in part], video_spatio_temporal_features=torch.stack([f for _, _, f, _ in part]),
                                       do_sample=False, max_new_tokens=self.args.max_new_tokens, stop_strings=[s for _, _, _, s in part],
                                       tokenizer=self.tokenizer, timings=timings, **self.warpers(), **bans_from_args(self.args), **self.allowed_kw,
                                       **lookup_from_args(self.args), **self.guidance([indices[j] for j, _, _, _ in part])).cpu()

        def record(part, out):
            for row, (j, ids, _, _) in zip(out, part):
                self.record(toks, lens, j, row[len(ids):].tolist())

        if keep:
            try:
                record(keep, generate(keep, tm_g))
            except Exception as e:                                     # noqa: BLE001
                # one bad sample (e.g. an over-long prompt) must not take the whole group down: the reference loses only that sample.  Out of
                # memory (the KV cache of the group did not fit next to whatever else lives on the device: ADVICE r5) is not a sample's fault:
                # halve the group until it fits, one by one only for everything else
                oom = isinstance(e, (MemoryError, torch.cuda.OutOfMemoryError))
                size = max(1, len(keep) // 2) if oom and len(keep) > 1 else 1
                print(f"batched generation failed ({type(e).__name__}: {e}); retrying the {len(keep)} samples in groups of {size}")
                for part, out, e1 in split_refused([keep[i:i + size] for i in range(0, len(keep), size)], generate):
                    if e1 is None:
                        record(part, out)
                    else:
                        self.failed(indices[part[0][0]], e1)
        if self.tfile:
            for j, idx in enumerate(indices):
                self.write_timing(idx, lens[j], self.group_no, host, tm_g, len(indices))
            self.tfile.flush()
        self.group_no += 1
        return toks, lens

    def infer_refill(self, indices, clips=None):
        """--schedule refill: the whole shard through generate_continuous.  The groups of --batch tasks still drive the host half -- prepare()
        one group ahead on a background thread, one tower pass per group, the feature cache -- but decode slots are refilled task by task."""
        from concurrent.futures import ThreadPoolExecutor
        from ..continuous import Task, generate_continuous
        args = self.args
        W = max(1, int(args.batch))
        groups = [indices[g0:g0 + W] for g0 in range(0, len(indices), W)]
        toks, lens = torch.zeros(len(indices), args.max_new_tokens, dtype=torch.int32), [0] * len(indices)
        row = {idx: j for j, idx in enumerate(indices)}
        info = {}                                                      # task -> (its group, the group's host half)
        n_samples = int(getattr(args, "samples_per_prompt", 1))
        many = {"samples": n_samples} if n_samples > 1 else {}

        def stream():
            pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="pgv-prefetch")
            try:
                fut = pool.submit(self.prepare, groups[0]) if groups else None
                for gi, group in enumerate(groups):
                    try:
                        clips_g = fut.result()
                    except Exception as e:                             # noqa: BLE001 -- the group's tasks fail, the others go on
                        clips_g = {self.tasks[i]["path"]: e for i in group}
                    fut = pool.submit(self.prepare, groups[gi + 1]) if gi + 1 < len(groups) else None
                    feat_of, host = self.group_features(clips_g)
                    for idx in group:
                        info[idx] = (gi, host)
                        inp = self.inputs(idx, clips_g, feat_of)
                        if inp is not None:
                            yield Task(idx, inp[0], inp[1], stop=inp[2], seed=int(getattr(args, "seed", 0)) * 1000003 + idx, **many)
            finally:
                pool.shutdown(wait=True, cancel_futures=True)

        tm = {} if self.tfile else None
        # temperature 0.2, top_k 50: the reference's call (inference.py:106-112 + HF's default); the two warpers by generate()'s precedence
        from ..generation import resolve_sampling, step_kwargs
        warp, _ = step_kwargs(*resolve_sampling(0.2, 50, generation_config=getattr(self.model, "generation_config", None), **self.warpers())[2:])
        lps = {} if many else None                                    # the samples are ranked by their log-probabilities
        for idx, new in generate_continuous(self.model, stream(), W, args.max_new_tokens, do_sample=args.do_sample, temperature=0.2, top_k=50,
                                            tokenizer=self.tokenizer, on_error=self.failed, timings=tm, **warp, **({"logprobs": lps} if many else {}),
                                            **bans_from_args(args), **filters_from_args(args), **self.allowed_kw):
            if new is not None and many:
                new = self.pick_sample(idx, new, lps.pop(idx))
            if new is not None:
                self.record(toks, lens, row[idx], new)
        if self.tfile:
            for j, idx in enumerate(indices):
                g = tm.get(idx, {})
                if isinstance(g, list):                                # one entry per sample: the task's prefill, its samples' decode chunks together
                    g = {"prefill_s": g[0]["prefill_s"], "decode_s": max(x["decode_s"] for x in g), "steps": max(x["steps"] for x in g),
                         "group_size": g[0]["group_size"]}
                self.write_timing(idx, lens[j], info[idx][0], info[idx][1], g, g.get("group_size"))
            self.tfile.flush()
        return toks, lens

    def pick_sample(self, idx, news, lps):
        """--samples_per_prompt: the ids of the sample of task idx that --sample_pick chooses; every sample goes to --samples_out."""
        import json
        from ..inference import best_sample, majority_sample
        stop = self.stop_strs.get(idx)
        eos = self.model.config.eos_token_id
        samples = []
        for new, lp in zip(news, lps):
            ids = new[:new.index(eos)] if eos is not None and eos in new else new
            text = self.tokenizer.batch_decode([ids[:self.args.max_new_tokens]], skip_special_tokens=True)[0].strip()       # as answer_tasks cleans the recorded one
            samples.append({"text": text.rstrip(stop).strip() if stop else text, "ids": new, "logprob": float(sum(lp["token_logprobs"]))})
        k = majority_sample(samples) if getattr(self.args, "sample_pick", "best") == "majority" else best_sample(samples)
        if self.sfile:
            self.sfile.write(json.dumps({"task": idx, "video": self.tasks[idx]["name"], "rank": self.rank, "picked": k, "samples": samples}) + "\n")
            self.sfile.flush()
        return news[k]

    def infer_sampled(self, indices, clips=None):
        """--do_sample (--schedule group): the reference's temperature-0.2 sampling with its stopping criterion, one task at a time
        (video_chatgpt_infer's path up to the detokenisation); the ids travel through the same fixed-shape collation as the greedy answers."""
        from ..inference import guidance_kwargs, video_chatgpt_infer_ids
        if clips is None:
            clips = self.prepare(indices)
        clips.pop("__load_s__", None)
        feat_of = self.features_for(clips, None)
        toks, lens = torch.zeros(len(indices), self.args.max_new_tokens, dtype=torch.int32), [0] * len(indices)
        for j, idx in enumerate(indices):
            t = self.tasks[idx]
            try:
                if t["path"] is None:
                    raise FileNotFoundError(t["name"])
                if t["path"] not in feat_of:
                    raise clips[t["path"]]
                new, stop = video_chatgpt_infer_ids(None, t["question"], self.args.conv_mode, self.model, self.vision_tower, self.tokenizer,
                                                    self.image_processor, self.video_token_len, None, max_new_tokens=self.args.max_new_tokens,
                                                    features=feat_of[t["path"]], **self.warpers(), **bans_from_args(self.args), **filters_from_args(self.args), **self.allowed_kw,
                                                    **lookup_from_args(self.args),      # --lookup D --lookup_sample: the same ids in fewer passes
                                                    **guidance_kwargs(guidance_scale_from_args(self.args), getattr(self.args, "guidance_negative", "no_video")))
                self.stop_strs[idx] = stop
                self.record(toks, lens, j, new, strip_eos=False)       # the ids end where the reference's criterion stopped them
            except Exception as e:                                     # noqa: BLE001
                self.failed(idx, e)
        return toks, lens


def answer_tasks(args, tasks, components, load_frames, rank, world):
    """tasks: [{"path": str | None, "name": str, "question": str}] -> [str | None] in task order, identical on every rank."""
    import os
    from .. import parallel
    from ..inference import build_prompt

    model, vision_tower, tokenizer = components[:3]
    timings_path = getattr(args, "timings", None)
    if timings_path and world > 1:
        timings_path = f"{timings_path}.rank{rank}"
    tfile = open(timings_path, "a") if timings_path else None
    samples_path = getattr(args, "samples_out", None)
    if samples_path and world > 1:
        samples_path = f"{samples_path}.rank{rank}"
    sfile = open(samples_path, "a") if samples_path else None
    run = _Runner(args, tasks, components, load_frames, rank, tfile, sfile)
    device = vision_tower.device if hasattr(vision_tower, "device") else torch.device("cpu")
    if getattr(args, "batch", "auto") == "auto":
        free_b = torch.cuda.mem_get_info(device)[0] if device.type == "cuda" else 0
        # processes that share this device see the same free pool and would each claim 70 % of it: PGV_DEVICE_SHARERS (or, in a
        # shared-device control-flow run, the world size) divides it
        sharers = int(os.environ.get("PGV_DEVICE_SHARERS", world if os.environ.get("PGV_BENCH_SHARE_DEVICE") else 1))
        args.batch = pick_batch(model.config, vision_tower.config.image_size, args.max_new_tokens, free_b // max(sharers, 1)) if free_b else 8
        if world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
            # one group size for the whole job: the smallest any rank can afford (ranks with different free memory would otherwise run
            # different launch shapes -- same answers, since results do not depend on the batch, but skewed finish times)
            t = torch.tensor([args.batch], dtype=torch.int32, device=device if torch.distributed.get_backend() == "nccl" else "cpu")
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MIN)
            args.batch = int(t[0])
        beams = int(getattr(args, "beams", 1))
        if beams > 1:
            args.batch = max(1, args.batch // beams)                   # a clip holds K decode slots: the same number of sequences per group
        if int(getattr(args, "lookup", 0) or 0) > 0:
            args.batch = max(1, min(args.batch, MAX_BATCH // (1 + int(args.lookup))))      # a clip holds 1 + D rows of a lookup step
        if guidance_scale_from_args(args) is not None:
            args.batch = max(1, args.batch // 2)                       # a clip holds two decode slots: its prompt and its negative
        if rank == 0:
            print(f"[pgv] --batch auto: {args.batch} clips per group ({free_b / 2 ** 30:.0f} GiB free on {device}, shared by {sharers})", flush=True)
    spill = os.path.join(args.output_dir, args.output_name) if getattr(args, "output_dir", None) and getattr(args, "output_name", None) else None
    if spill:
        os.makedirs(args.output_dir, exist_ok=True)
    try:
        if getattr(args, "schedule", "group") == "refill":
            # one infer call over the whole shard (it prefetches its own groups); the answers collate like the static groups'
            answers = parallel.run_sharded(len(tasks), run.infer_refill, args.max_new_tokens, rank, world, device, per_gpu_batch=max(1, len(tasks)),
                                           length_offset=1, spill_path=spill)
        elif args.do_sample:
            answers = parallel.run_sharded(len(tasks), run.infer_sampled, args.max_new_tokens, rank, world, device, per_gpu_batch=1, length_offset=1, prepare=run.prepare,
                                           spill_path=spill)
        else:
            answers = parallel.run_sharded(len(tasks), run.infer_batch, args.max_new_tokens, rank, world, device, per_gpu_batch=args.batch,
                                           length_offset=1, prepare=run.prepare, spill_path=spill)
    finally:
        if tfile:
            tfile.close()
        if sfile:
            sfile.close()
    from ..model.utils import first_stop_length
    preds = []
    for idx, ids in enumerate(answers):
        if ids is None:
            preds.append(None)                                         # failed / missing: left out of the output like the reference's except
            continue
        stop = run.stop_strs.get(idx) or build_prompt("", args.conv_mode, 1, run.use_se)[1]
        if args.do_sample:
            # the ids already end where the reference's criterion stopped them; its own post-processing (inference.py:119-123)
            text = tokenizer.batch_decode([ids], skip_special_tokens=True)[0]
            preds.append(text.strip().rstrip(stop).strip())
            continue
        # The batched greedy loop stops a sequence at most one chunk late and cuts it where the reference's per-sample loop would have stopped
        # (KeywordsStoppingCriteria); ids gathered from OTHER ranks went through the same cut.  Re-applying the cut here is idempotent and
        # keeps this function correct for a generate() without stop support; then clean like the reference does.
        n = first_stop_length(ids, tokenizer, [stop]) if stop else None
        if n is not None:
            ids = ids[:n]
        text = tokenizer.batch_decode([ids], skip_special_tokens=True)[0].strip()
        preds.append(text.rstrip(stop).strip() if stop else text)     # the reference's own stop handling (inference.py:123)
    return preds


DECORD_FREE_FORMATS = (".npy", "")      # a uint8 [T,H,W,3] array, or a directory of frame images named like the video (no extension)


def first_existing(video_dir, stem, formats):
    """First existing `{stem}{ext}` in the given extension order; None when absent."""
    import os
    for fmt in formats:
        path = os.path.join(video_dir, f"{stem}{fmt}")
        if os.path.exists(path):
            return path
    return None


def write_output(args, output_list, rank):
    import json
    import os
    if rank == 0:
        with open(os.path.join(args.output_dir, f"{args.output_name}.json"), "w") as f:
            json.dump(output_list, f)
    return output_list
