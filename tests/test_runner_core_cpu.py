"""The eval runners' answering core (video_llava_amd.eval._sharded.answer_tasks) on the CPU: the real function -- and below it the real
`generate`, `generate_continuous`, `run_sharded` -- over a scripted backend, a character tokenizer and a stand-in for the tower.  Every schedule
(--schedule group, --schedule refill, --do_sample, and refill with --do_sample) has to hand back the same predictions for the same tasks:
failed tasks, the feature cache, the three ways an answer ends, the retry / isolation of a refused call and the --timings file."""
import json
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from video_llava_amd.eval import _sharded
from video_llava_amd.inference import build_prompt
from video_llava_amd.model.video_chatgpt import VideoChatGPTConfig, VideoChatGPTLlamaForCausalLM, VisionConfig

EOS, V, NEW = 2, 4, 40                  # EOS id, video rows per clip, --max_new_tokens
FILLER, POISON = "x", "~"               # what the backend emits once a script has run out; a prompt holding POISON is refused by the backend
STOPS = {"default": "###", "video-chatgpt_v1": "</s>"}      # conv mode -> its stop string (ordinary text for the character tokenizer)
TIMING_KEYS = {"task", "video", "rank", "group", "group_size", "ok", "tokens", "feature_cache_hit", "load_s", "upload_ingest_s_group",
               "tower_pool_s_group", "clips_in_tower_pass", "prefill_s_group", "decode_s_group", "decode_steps_group"}


class CharTok:
    """One id per character (its code point); 1 = BOS, ids <= 2 are special."""

    @staticmethod
    def _encode(s):
        assert all(2 < ord(c) < 256 for c in s), s
        return [1] + [ord(c) for c in s]

    def __call__(self, x):
        return types.SimpleNamespace(input_ids=[self._encode(t) for t in x] if isinstance(x, (list, tuple)) else self._encode(x))

    def batch_decode(self, ids, skip_special_tokens=True):
        return ["".join(chr(int(t)) for t in row if int(t) > 2) for row in ids]


def _script(ids, feat):
    """The answer the backend gives to a prompt: the text between the prompt's last braces, `$` = EOS, `@` = the letter the clip's
    features carry (so an answer shows WHICH clip's features reached the decoder); FILLER for ever once that has run out."""
    text = "".join(chr(t) for t in ids[1:])
    body = text[text.rindex("{") + 1:text.rindex("}")]
    return [EOS if c == "$" else ord(c) for c in body.replace("@", chr(int(feat[0, 0])))]


class _KV:
    def __init__(self, n, max_seq):
        self.max_seq, self.script, self.g, self.done, self.len = max_seq, [None] * n, [0] * n, [False] * n, [0] * n


class ScriptedLM(VideoChatGPTLlamaForCausalLM):
    """The real host logic of the model class (generate) over scripted device calls: the surface generate and generate_continuous drive.
    A sequence's tokens depend on its own prompt, features and step only; EOS is sticky, as on the device."""
    vocab_size = 256

    def __init__(self, max_pos, max_group=None):
        nn.Module.__init__(self)
        self.config = VideoChatGPTConfig(vocab_size=256, eos_token_id=EOS, max_position_embeddings=max_pos)
        self.device_ = torch.device("cpu")
        vc = VisionConfig()
        vc.use_vid_start_end = True
        self.model = types.SimpleNamespace(vision_config=vc)
        self.max_group = max_group          # a prefill over more sequences runs out of memory
        self.calls = []                     # ("prefill" | "prefill_slots", number of sequences) of every call, refused ones included
        self._reuse = None

    def _video_positions(self, seqs, num_video_rows):
        return [-1] * len(seqs)

    def _start(self, kv, s, ids, feat):
        kv.script[s], kv.g[s], kv.done[s], kv.len[s] = _script(ids, feat), 0, False, len(ids)
        return self._emit(kv, s, EOS)

    @staticmethod
    def _emit(kv, s, eos_id):
        sc, g = kv.script[s], kv.g[s]
        t = eos_id if kv.done[s] else (sc[g] if g < len(sc) else ord(FILLER))
        kv.done[s] = kv.done[s] or t == eos_id
        kv.g[s] += 1
        return t

    def _refuse(self, seqs):
        if any(ord(POISON) in p for p in seqs):
            raise ValueError("refused: poison token")

    def prefill(self, seqs, feats, max_seq, want_logits=False, want_all_logits=False, append_to=None):
        self.calls.append(("prefill", len(seqs)))
        if self.max_group is not None and len(seqs) > self.max_group:
            raise MemoryError(f"no room for {len(seqs)} sequences")
        self._refuse(seqs)
        assert feats.shape == (len(seqs), V, 8)
        kv = _KV(len(seqs), max_seq)
        return kv, torch.tensor([self._start(kv, s, p, feats[s]) for s, p in enumerate(seqs)], dtype=torch.int32), None

    def prefill_slots(self, kv, slots, seqs, feats, want_logits=False, u=None, temperature=1.0, top_k=50):
        self.calls.append(("prefill_slots", len(seqs)))
        self._refuse(seqs)
        assert len(set(slots)) == len(slots) and all(0 <= s < len(kv.g) for s in slots) and feats.shape == (len(seqs), V, 8)
        return torch.tensor([self._start(kv, s, p, feats[i]) for i, (s, p) in enumerate(zip(slots, seqs))], dtype=torch.int32), None

    def decode_greedy(self, kv, first, n, eos_id=-1):
        out = torch.zeros(len(kv.g), n, dtype=torch.int32)
        for s in range(len(kv.g)):
            assert kv.len[s] + n <= kv.max_seq, f"slot {s} would grow to {kv.len[s] + n} of {kv.max_seq}"
            for i in range(n):
                out[s, i] = self._emit(kv, s, eos_id)
            kv.len[s] += n
        return out

    def sample_last(self, kv, u, temperature, top_k=50):         # the scripted distribution is a point mass: sampling picks the same token
        assert u.shape == (len(kv.g),) and temperature == 0.2 and top_k == 50
        return torch.tensor([kv.script[s][0] if kv.script[s] else ord(FILLER) for s in range(len(kv.g))], dtype=torch.int32)

    def decode_sample(self, kv, first, n, eos_id, temperature, top_k, u):
        assert u.shape == (n, len(kv.g)) and temperature == 0.2 and top_k == 50
        return self.decode_greedy(kv, first, n, eos_id)

    def kv_len(self, kv, s):
        return kv.len[s]

    def kv_truncate(self, kv, s, length):
        kv.len[s] = length


def _frames(letter):
    return np.full((2, 4, 4, 3), ord(letter), dtype=np.uint8)


def _load_frames(path):
    if path == "B":
        raise RuntimeError("cannot decode B")
    return _frames(path)


def _features(clip):
    return torch.full((V, 8), float(clip.flat[0]), dtype=torch.float16)


@pytest.fixture
def tower(monkeypatch):
    """Stand-in for the tower: pooled features that carry the clip's letter; `passes` lists the clips of every batched pass."""
    passes = []

    def video_features_batch(clips, vision_tower, image_processor, timings=None):
        passes.append("".join(chr(int(c.flat[0])) for c in clips))
        if timings is not None:
            timings.update(upload_ingest_s=0.25, tower_pool_s=0.5, frames=sum(len(c) for c in clips))
        return [_features(c) for c in clips]

    monkeypatch.setattr("video_llava_amd.inference.video_features_batch", video_features_batch)
    monkeypatch.setattr("video_llava_amd.inference.video_features", lambda clip, vision_tower, image_processor: _features(clip))
    return passes


LONG_ANSWER = "a man walks a dog in a sunny park"          # 33 tokens + EOS: past generate's chunk of 32 and two of the refill loop's 16


def _tasks(stop):
    """(path, name, question, prediction).  Clip letters are the video paths; with --batch 2 the static groups are the rows in pairs."""
    rows = [("A", "vA", "what is there? {a dog$}", "a dog"),                          # ends by EOS
            (None, "gone", "where? {lost$}", None),                                   # missing video
            ("B", "vB", "who? {lost$}", None),                                        # the loader raises
            ("C", "vC", f"which colour? {{red {stop} blue$}}", "red"),                # a stop string ahead of the EOS of the same chunk
            ("A", "vA", "anything else? {$}", ""),                                    # first token EOS: an empty answer, not a failure; cache hit
            ("D", "vD", "and on? {}", FILLER * NEW),                                  # runs into --max_new_tokens
            ("E", "vE", "which clip? {clip @ first$}", "clip E first"),               # two questions about one clip inside one group
            ("E", "vE", "what happens? {" + LONG_ANSWER + "$}", LONG_ANSWER),
            ("F", "vF", "far too long? " + "and then " * 30 + "{lost$}", None),       # prompt + budget past the context window
            ("G", "vG", "after the long one? {seen @$}", "seen G"),
            ("H", "vH", "refused " + POISON + " {lost$}", None),                      # the backend refuses any call that holds it
            ("I", "vI", "and the last? {last @$}", "last I")]
    return [{"path": p, "name": n, "question": q} for p, n, q, _ in rows], [a for _, _, _, a in rows]


def _prompt_len(question, conv_mode):
    return len(CharTok()([build_prompt(question, conv_mode, V, True)[0]]).input_ids[0])


def _run(tmp_path, tasks, conv_mode, schedule, do_sample, batch=2, max_group=None):
    lens = [_prompt_len(t["question"], conv_mode) for t in tasks]
    normal = max(n for n in lens if n < min(lens) + 128)
    model = ScriptedLM(max_pos=normal + NEW + 16 + 4, max_group=max_group)       # room for every prompt but the over-long one (+ budget + a chunk)
    tpath = tmp_path / f"t_{schedule}_{int(do_sample)}.jsonl"
    args = types.SimpleNamespace(conv_mode=conv_mode, max_new_tokens=NEW, batch=batch, do_sample=do_sample, schedule=schedule, seed=3,
                                 timings=str(tpath), feature_cache=64, output_dir=None, output_name=None)
    components = (model, types.SimpleNamespace(device=torch.device("cpu"), config=types.SimpleNamespace(image_size=224)), CharTok(), None, V)
    preds = _sharded.answer_tasks(args, tasks, components, _load_frames, 0, 1)
    lines = [json.loads(x) for x in open(tpath)]
    assert all(set(x) == TIMING_KEYS for x in lines)
    return preds, lines, model


def _errors(out):
    return [x for x in out.splitlines() if x.startswith(("Error processing", "batched generation failed"))]


@pytest.mark.parametrize("conv_mode", sorted(STOPS))
def test_every_schedule_gives_the_same_predictions(tmp_path, capsys, tower, conv_mode):
    stop = STOPS[conv_mode]
    assert build_prompt("q", conv_mode, V, True)[1] == stop
    tasks, want = _tasks(stop)
    n_long, n_pos = _prompt_len(tasks[8]["question"], conv_mode), None
    got = {}
    for schedule, do_sample in (("group", False), ("refill", False), ("group", True), ("refill", True)):
        del tower[:]
        preds, lines, model = _run(tmp_path, tasks, conv_mode, schedule, do_sample)
        n_pos = model.config.max_position_embeddings
        errors = _errors(capsys.readouterr().out)
        assert preds == want, (schedule, do_sample)
        got[schedule, do_sample] = preds
        # the tower ran once per distinct clip: A's second question (two groups later) and E's (same group) reuse the pooled features
        assert sorted("".join(tower)) == list("ACDEFGHI") and all(len(p) <= 2 for p in tower)
        too_long = f"prompt + max_new_tokens = {n_long + NEW} exceeds max_position_embeddings {n_pos}"
        no_room = f"prompt of {n_long} tokens + {NEW} new tokens does not fit the group's {n_pos} cache positions"
        if schedule == "refill":
            assert errors == ["Error processing video file 'gone': not found", "Error processing video file 'vB': cannot decode B",
                              f"Error processing video file 'vF': {no_room}", "Error processing video file 'vH': refused: poison token"]
            assert ("prefill", 2) == model.calls[0] and all(c[0] == "prefill_slots" for c in model.calls[1:])
            assert [x["task"] for x in lines] == list(range(12))
            assert [x["group"] for x in lines] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
            # slots a task's prefill call filled: the opening pair, then one or two freed slots at a time; None = never reached a slot
            assert [x["group_size"] for x in lines][:4] == [2, None, None, 2]
            assert all(x["group_size"] in (1, 2) for i, x in enumerate(lines) if want[i] is not None)
            assert all(x["group_size"] is None and x["prefill_s_group"] is None for i, x in enumerate(lines) if want[i] is None)
        elif do_sample:
            assert errors == ["Error processing video file 'gone': gone", "Error processing video file 'vB': cannot decode B",
                              f"Error processing video file 'vF': {too_long}", "Error processing video file 'vH': refused: poison token"]
            assert all(c == ("prefill", 1) for c in model.calls) and lines == []       # one task at a time; this path writes no timing lines
        else:
            assert errors == ["Error processing video file 'gone': not found", "Error processing video file 'vB': cannot decode B",
                              f"batched generation failed (ValueError: {too_long}); retrying the 2 samples in groups of 1",
                              f"Error processing video file 'vF': {too_long}",
                              "batched generation failed (ValueError: refused: poison token); retrying the 2 samples in groups of 1",
                              "Error processing video file 'vH': refused: poison token"]
            # groups of one (a task of the pair failed on the host), of two, and the one-by-one retries of the two refused pairs
            assert [n for _, n in model.calls] == [1, 1, 2, 2, 1, 2, 1, 1]
            assert [(x["task"], x["group"], x["group_size"]) for x in lines] == [(i, i // 2, 2) for i in range(12)]
            assert [x["clips_in_tower_pass"] for x in lines] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2]
            # generate's `steps`: tokens up to the EOS of the group's last sequence ("a dog$"; "red <stop> blue$": the stop cut does not
            # shorten the chunk that was already decoded; the cap; LONG_ANSWER + EOS)
            n_c = len(f"red {stop} blue") + 1
            assert [x["decode_steps_group"] for x in lines] == [6, 6, n_c, n_c, NEW, NEW, 34, 34, None, None, None, None]
            assert all((x["prefill_s_group"] is None) == (x["task"] >= 8) for x in lines)      # a refused call leaves no stage times
        if lines:
            assert [x["video"] for x in lines] == [t["name"] for t in tasks] and all(x["rank"] == 0 for x in lines)
            assert [x["ok"] for x in lines] == [a is not None for a in want]
            assert [x["tokens"] for x in lines] == [5, 0, 0, len(f"red {stop}"), 0, NEW, 12, len(LONG_ANSWER), 0, 6, 0, 6]
            assert [x["feature_cache_hit"] for x in lines] == [False] * 4 + [True] + [False] * 7
            assert all(x["upload_ingest_s_group"] == 0.25 and x["tower_pool_s_group"] == 0.5 and x["load_s"] >= 0.0 for x in lines)
    assert got["group", False] == got["refill", False] == got["group", True] == got["refill", True]


@pytest.mark.parametrize("max_group, calls", [(2, [4, 2, 2]), (1, [4, 2, 1, 1, 2, 1, 1])])
def test_group_that_runs_out_of_memory_is_halved(tmp_path, capsys, tower, max_group, calls):
    tasks, want = _tasks("###")
    keep = [0, 3, 6, 9]
    tasks, want = [tasks[i] for i in keep], [want[i] for i in keep]
    preds, lines, model = _run(tmp_path, tasks, "default", "group", False, batch=4, max_group=max_group)
    assert preds == want
    assert _errors(capsys.readouterr().out) == ["batched generation failed (MemoryError: no room for 4 sequences); retrying the 4 samples in groups of 2"]
    assert [n for _, n in model.calls] == calls
    assert [(x["ok"], x["group_size"], x["prefill_s_group"]) for x in lines] == [(True, 4, None)] * 4
