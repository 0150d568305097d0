"""`VideoChatGPTLlamaForCausalLM` drop-in: the object `initialize_model` returns in slot 1 and
`video_chatgpt_infer` drives through `model.get_model().vision_config`, `model.get_model().mm_projector` and
`model.generate(input_ids, video_spatio_temporal_features=..., do_sample, temperature, max_new_tokens,
stopping_criteria)` (reference: video_chatgpt/model/video_chatgpt.py:16-325; call sites
video_chatgpt/inference.py:67,105-112, chat.py:148-154, eval/model_utils.py:104-144).

The decoder stack, the video splice, lm_head and greedy picking run in libpgv (hand-written gfx950 kernels);
this file is host orchestration only: placeholder validation (same ValueErrors as the reference) and the
step methods; generate()'s checks are generation.plan_generate, its token loop is generate_loop.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, generate_loop
from ..constants import CLIP_WIDTH
from ..beam_reference import early_code
from ..generation import MAX_GROUP, CacheSettings, fork_sources, load_generation_config, plan_generate
from ..logit_bans import LogitBans
from ..sample_filters import SampleFilters
from ..scoring import ScoreOutput, id_rows, shift_labels
from .multimodal_projector.builder import HipLinear, IdentityMap, build_vision_projector

DEFAULT_VIDEO_TOKEN = "<video>"
DEFAULT_VIDEO_PATCH_TOKEN = "<vid_patch>"
DEFAULT_VID_START_TOKEN = "<vid_start>"
DEFAULT_VID_END_TOKEN = "<vid_end>"


class VisionConfig:
    """Same fields as the reference's VisionConfig (model/video_chatgpt.py:16-30)."""

    def __init__(self, frame_size=224, patch_size=14, hidden_size=1024):
        self.frame_size = frame_size
        self.patch_size = patch_size
        self.hidden_size = hidden_size
        self.use_vid_start_end = None
        self.vid_start_token = None
        self.vid_end_token = None
        self.vid_patch_token = None


class VideoChatGPTConfig:
    """The LlamaConfig fields the path reads + the multimodal keys of config.json
    (`mm_vision_tower`, `use_mm_proj`, `mm_hidden_size`, `mm_projector_type`; model/video_chatgpt.py:43-55)."""
    model_type = "VideoChatGPT"

    def __init__(self, vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32,
                 num_attention_heads=32, num_key_value_heads=None, max_position_embeddings=4096, rms_norm_eps=1e-5,
                 rope_theta=10000.0, mm_vision_tower=None, use_mm_proj=True, mm_hidden_size=1024,
                 mm_projector_type="linear", eos_token_id=2, bos_token_id=1, pad_token_id=None, **extra):
        if num_key_value_heads not in (None, num_attention_heads):
            raise ValueError("grouped-query checkpoints are outside the PG-Video-LLaVA path (7B/13B are MHA)")
        self.vocab_size, self.hidden_size, self.intermediate_size = vocab_size, hidden_size, intermediate_size
        self.num_hidden_layers, self.num_attention_heads = num_hidden_layers, num_attention_heads
        self.max_position_embeddings, self.rms_norm_eps, self.rope_theta = max_position_embeddings, rms_norm_eps, rope_theta
        self.mm_vision_tower, self.use_mm_proj, self.mm_hidden_size = mm_vision_tower, use_mm_proj, mm_hidden_size
        self.mm_projector_type = mm_projector_type
        self.eos_token_id, self.bos_token_id, self.pad_token_id = eos_token_id, bos_token_id, pad_token_id
        self.extra = extra

    @classmethod
    def from_pretrained(cls, path: str) -> "VideoChatGPTConfig":
        with open(os.path.join(path, "config.json")) as f:
            return cls(**json.load(f))


class VideoChatGPTLlamaModel(nn.Module):
    """`model.get_model()`: carries vision_config and mm_projector like the reference's inner LlamaModel subclass."""

    def __init__(self, config: VideoChatGPTConfig, vision_config: VisionConfig, dtype, device):
        super().__init__()
        self.config = config
        self.vision_config = vision_config
        if config.use_mm_proj:
            if vision_config.frame_size == 224:      # LLaVA-Lightning style bare Linear (model/video_chatgpt.py:52-53)
                self.mm_projector = HipLinear(config.mm_hidden_size, config.hidden_size, dtype, device)
            else:                                     # LLaVA-1.5: by config.mm_projector_type (:54-55)
                self.mm_projector = build_vision_projector(config, dtype=dtype, device=device)


class PastKeyValues:
    """What forward() hands back as `past_key_values`: the library's KV-cache handle (the cache lives in HBM inside libpgv; HF's tuple of
    tensors / DynamicCache has no counterpart).  Truthy once it holds tokens, like the tuple the reference tests at model/video_chatgpt.py:256."""

    def __init__(self, owner, kv, batch: int, seq_len: int, max_seq: int, epoch: int):
        self.owner, self.kv, self.batch, self.seq_len = owner, kv, batch, seq_len
        self.max_seq = max_seq          # capacity of the cache behind `kv`
        self.epoch = epoch              # the model's cache epoch when this object was handed out: any later prefill / generate makes it stale

    def get_seq_length(self, layer_idx: int = 0) -> int:
        return self.seq_len

    def __bool__(self):
        return self.seq_len > 0

    def __len__(self):
        return self.owner.config.num_hidden_layers


class CausalLMOutputWithPast:
    """`.logits` / `.past_key_values`, also indexable like HF's ModelOutput ([0] = logits, [1] = past_key_values)."""

    def __init__(self, logits, past_key_values):
        self.logits, self.past_key_values = logits, past_key_values
        self.loss = self.hidden_states = self.attentions = None

    def __getitem__(self, i):
        return (self.logits, self.past_key_values)[i]


class VideoChatGPTLlamaForCausalLM(nn.Module):
    generation_config = None        # the checkpoint's generation_config.json (from_pretrained; generation.GenerationDefaults): HF's per-model generate() defaults

    def __init__(self, config: VideoChatGPTConfig, vision_config: Optional[VisionConfig] = None,
                 torch_dtype: torch.dtype = torch.float16, device=None):
        super().__init__()
        self.config = config
        self.dtype_ = torch_dtype
        self.ctx = _lib.Context.get(device)
        self.device_ = torch.device("cuda", self.ctx.device)
        if vision_config is None:
            vision_config = _vision_config_from(config.mm_vision_tower)
        if vision_config.hidden_size != CLIP_WIDTH:
            raise ValueError(f"CLIP width must be {CLIP_WIDTH} (the reference hard-codes it at model/video_chatgpt.py:106)")
        self.model = VideoChatGPTLlamaModel(config, vision_config, torch_dtype, self.device_)
        lc = _lib.LlmConfig(config.vocab_size, config.hidden_size, config.intermediate_size, config.num_hidden_layers,
                            config.num_attention_heads, config.rms_norm_eps, config.rope_theta)
        h = C.c_void_p()
        _lib.check(self.ctx.lib.pgv_llm_create(self.ctx.handle, C.byref(lc), _lib.dtype_code(torch_dtype), C.byref(h)), "pgv_llm_create")
        self.handle = h
        self._kv: dict = {}
        self._kv_epoch = 0              # bumped by every call that (re)fills a cache from position 0: what PastKeyValues objects are checked against
        self._reuse = None              # generate(kv_reuse_key=...): (key, kv handle, max_seq, ids whose keys / values sit in the cache)

    def __del__(self):
        try:
            for kv in getattr(self, "_kv", {}).values():
                self.ctx.lib.pgv_kv_destroy(kv)
            if getattr(self, "handle", None):
                self.ctx.lib.pgv_llm_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ---- HF-module surface the reference touches ----------------------------------------------------
    def get_model(self) -> VideoChatGPTLlamaModel:
        return self.model

    def eval(self):
        return self

    def cuda(self, *a, **k):
        return self

    def half(self):
        return self

    @property
    def device(self):
        return self.device_

    @property
    def vocab_size(self) -> int:
        return self.ctx.lib.pgv_llm_vocab(self.handle)

    # ---- fp8 weight path (BASELINE config 5) ------------------------------------------------------------
    def quantize_weights_fp8(self):
        """Quantise every decoder matrix and lm_head to e4m3 with per-row power-of-two scales (pgv_llm_quantize_fp8): decode then
        streams half the weight bytes per token; prefill and decode both compute with the dequantised values, which
        `get_weight(key)` returns for a checkpoint writer or a parity oracle.  Call after load_state_dict."""
        _lib.check(self.ctx.lib.pgv_llm_quantize_fp8(self.ctx.handle, self.handle, _lib.stream_ptr(self.device_)), "pgv_llm_quantize_fp8")
        return self

    @property
    def is_fp8(self) -> bool:
        return bool(self.ctx.lib.pgv_llm_is_fp8(self.handle))

    def get_weight(self, key: str) -> torch.Tensor:
        """fp32 [out, in] copy of a decoder matrix / lm_head under its HF key, as the kernels see it (dequantised after fp8)."""
        shape = self._expected_shape(key) or (1,)       # not a decoder key: the library rejects it (as it does the norm vectors and embed_tokens)
        out = torch.empty(shape, dtype=torch.float32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_llm_get_weight(self.ctx.handle, self.handle, key.encode(), out.data_ptr(), _lib.stream_ptr(self.device_)),
                   "pgv_llm_get_weight")
        return out

    def resize_token_embeddings(self, new_num_tokens: int):
        """eval/model_utils.py:119: grow embed_tokens / lm_head for the three video tokens (new rows are zero until a checkpoint fills
        them; HF initialises them from the old rows' statistics -- neither is ever a trained value)."""
        _lib.check(self.ctx.lib.pgv_llm_resize_vocab(self.handle, int(new_num_tokens), _lib.stream_ptr(self.device_)),
                   "resize_token_embeddings")
        self.config.vocab_size = int(new_num_tokens)
        for kv in self._kv.values():                    # logits buffers / captured decode graphs carry the old vocabulary size
            self.ctx.lib.pgv_kv_destroy(kv)
        self._kv.clear()
        self._kv_epoch += 1
        self._reuse = None

    # ---- weights ----------------------------------------------------------------------------------------
    def _expected_shape(self, key: str):
        """Shape HF's LlamaForCausalLM holds under `key` for this config and the CURRENT vocabulary (None: not a decoder key)."""
        c = self.config
        H, I, V = c.hidden_size, c.intermediate_size, self.vocab_size
        if key in ("model.embed_tokens.weight", "lm_head.weight"):
            return (V, H)
        if key == "model.norm.weight":
            return (H,)
        if not key.startswith("model.layers."):
            return None
        rest = key.split(".", 3)[-1]
        return {"self_attn.q_proj.weight": (H, H), "self_attn.k_proj.weight": (H, H), "self_attn.v_proj.weight": (H, H),
                "self_attn.o_proj.weight": (H, H), "mlp.gate_proj.weight": (I, H), "mlp.up_proj.weight": (I, H),
                "mlp.down_proj.weight": (H, I), "input_layernorm.weight": (H,), "post_attention_layernorm.weight": (H,)}.get(rest)

    def load_state_dict(self, sd: dict, strict: bool = True):
        """Routes `model.mm_projector.*` to the projector module and every other key to the packed device weights.
        Returns an object with `.missing_keys` / `.unexpected_keys` like torch (eval/model_utils.py:124-126); a tensor whose shape
        disagrees with the config (or, for the vocabulary matrices, with the current vocabulary size) raises torch's "size mismatch"
        RuntimeError -- also under strict=False, as torch does."""
        lib = self.ctx.lib
        unexpected: List[str] = []
        proj_sd = {}
        for k, v in sd.items():
            if isinstance(v, np.ndarray):
                v = torch.from_numpy(v)
            if k.startswith("model.mm_projector."):
                proj_sd[k[len("model.mm_projector."):]] = v
                continue
            if "rotary_emb.inv_freq" in k:
                continue
            v = v.detach()
            if v.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                v = v.float()
            v = v.contiguous()
            exp = self._expected_shape(k)
            if exp is not None and tuple(v.shape) != exp:
                raise RuntimeError(f"Error(s) in loading state_dict for VideoChatGPTLlamaForCausalLM:\n\tsize mismatch for {k}: copying a param "
                                   f"with shape {tuple(v.shape)} from checkpoint, the shape in current model is {exp}.")
            if v.is_cuda:
                torch.cuda.current_stream(v.device).synchronize()
            dev = 1 if v.is_cuda else 0
            if k in ("model.embed_tokens.weight", "lm_head.weight"):
                rc = lib.pgv_llm_load_rows(self.handle, k.encode(), v.data_ptr(), _lib.dtype_code(v.dtype), dev, 0, v.shape[0], v.numel(),
                                           _lib.stream_ptr(self.device_))
            else:
                rc = lib.pgv_llm_load_tensor(self.handle, k.encode(), v.data_ptr(), _lib.dtype_code(v.dtype), dev, v.numel(),
                                             _lib.stream_ptr(self.device_))
            if rc == _lib.PGV_ENAME:
                unexpected.append(k)
                continue
            _lib.check(rc, f"load {k}")
        if proj_sd:
            mp = self.model.mm_projector
            res = mp.load_state_dict({k: v.to(self.dtype_) for k, v in proj_sd.items()}, strict=False)
            unexpected += ["model.mm_projector." + k for k in res.unexpected_keys]
        torch.cuda.synchronize(self.device_)
        missing = lib.pgv_llm_missing(self.handle)
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: {missing} decoder tensors missing, unexpected keys {unexpected}")

        class _Status:
            pass
        st = _Status()
        st.missing_keys = [f"<{missing} decoder tensors>"] if missing else []
        st.unexpected_keys = unexpected
        return st

    @classmethod
    def from_pretrained(cls, path: str, low_cpu_mem_usage: bool = True, torch_dtype: torch.dtype = torch.float16,
                        use_cache: bool = True, device=None, vision_config: Optional[VisionConfig] = None):
        """Load a local HF checkpoint directory (config.json + *.safetensors or pytorch_model*.bin shards)."""
        cfg = VideoChatGPTConfig.from_pretrained(path)
        model = cls(cfg, vision_config, torch_dtype, device)
        files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
        if files:
            from safetensors.torch import load_file
            for f in files:
                model.load_state_dict(load_file(os.path.join(path, f)), strict=False)
        else:
            for f in sorted(f for f in os.listdir(path) if f.startswith("pytorch_model") and f.endswith(".bin")):
                model.load_state_dict(torch.load(os.path.join(path, f), map_location="cpu"), strict=False)
        if model.ctx.lib.pgv_llm_missing(model.handle):
            raise RuntimeError(f"{path}: decoder checkpoint is incomplete")
        model.generation_config = load_generation_config(path)     # HF's from_pretrained reads it the same way; absent: None
        return model

    # ---- prompt validation (host): same checks and messages as model/video_chatgpt.py:113-128,150-157 ----
    def _video_positions(self, seqs: Sequence[Sequence[int]], num_video_rows: int) -> List[int]:
        vc = self.model.vision_config
        out = []
        for ids in seqs:
            a = np.asarray(ids)
            if int((a == vc.vid_patch_token).sum()) == 0:
                out.append(-1)                          # text-only sample (:113-118)
                continue
            if vc.use_vid_start_end:
                starts = np.nonzero(a == vc.vid_start_token)[0]
                if len(starts) != int((a == vc.vid_end_token).sum()):
                    raise ValueError("The number of video start tokens and video end tokens should be the same.")
                pos = -1
                for p in starts.tolist():
                    if p + num_video_rows + 1 >= len(a) or a[p + num_video_rows + 1] != vc.vid_end_token:
                        raise ValueError("The video end token should follow the video start token.")
                    pos = p                              # with several runs the reference keeps the last splice (:123-146)
                out.append(pos)
            else:
                idx = np.nonzero(a == vc.vid_patch_token)[0]
                if len(idx) != num_video_rows:
                    raise ValueError("The number of video patch tokens should be the same as the number of video patches.")
                if (idx != np.arange(idx[0], idx[0] + num_video_rows)).any():
                    raise ValueError("The video patch tokens should be consecutive.")
                out.append(int(idx[0]) - 1)              # rows (pos, pos+V] are replaced
        return out

    # ---- KV cache handles --------------------------------------------------------------------------------
    def _get_kv(self, batch: int, max_seq: int):
        key = (batch, max_seq)
        if key not in self._kv:
            for old in self._kv.values():               # keep one cache alive (they are GBs)
                self.ctx.lib.pgv_kv_destroy(old)
            self._kv.clear()
            self._reuse = None
            h = C.c_void_p()
            _lib.check(self.ctx.lib.pgv_kv_create(self.ctx.handle, self.handle, batch, max_seq, C.byref(h)), "pgv_kv_create")
            self._kv[key] = h
        return self._kv[key]

    def _reusable_prefix(self, key, ids: Sequence[int], max_new_tokens: int) -> int:
        """Positions of the cache kept by the last generate(kv_reuse_key=key) that the prompt `ids` can start from (0: none -- full prefill)."""
        r = self._reuse
        if r is None or r[0] != key or self._kv.get((1, r[2])) is not r[1] or len(ids) + max_new_tokens > r[2]:
            return 0
        cached = r[3]
        n = min(len(cached), len(ids) - 1)                 # at least one new token has to run: its logits pick the first answer token
        a, b = np.asarray(cached[:n]), np.asarray(ids[:n])
        diff = np.flatnonzero(a != b)
        L = int(diff[0]) if diff.size else n
        vc = self.model.vision_config
        video_ids = [t for t in (vc.vid_patch_token, vc.vid_start_token, vc.vid_end_token) if t is not None]
        if L < 1 or np.isin(np.asarray(ids[L:]), video_ids).any():
            return 0                                       # the placeholder run is (partly) in the new tokens: it needs the splice of a full prefill
        return L

    # ---- low-level steps (used by generate and by the parity tests) -------------------------------------
    def _project_video(self, feats: torch.Tensor, seqs, broadcast: bool = False):
        """Pooled features [n, V, C] (or [V, C]) of the prompts `seqs` -> (mm_projector output [n, V, hidden] contiguous (:105), V, the
        placeholder positions).  broadcast: one feature set stands for all prompts (projected once)."""
        n = len(seqs)
        if feats.dim() == 2:
            feats = feats.unsqueeze(0)
        proj = self.model.mm_projector(feats.to(self.device_))
        if isinstance(self.model.mm_projector, IdentityMap):
            proj = proj.to(self.dtype_)
        if broadcast and proj.shape[0] == 1 and n > 1:
            proj = proj.expand(n, -1, -1)
        if proj.shape[0] != n:
            raise ValueError(f"{proj.shape[0]} video feature sets for {n} prompts")
        proj = proj.contiguous()
        return proj, proj.shape[1], self._video_positions(seqs, proj.shape[1])

    def prefill(self, seqs: Sequence[Sequence[int]], video_spatio_temporal_features: Optional[torch.Tensor], max_seq: int,
                want_logits: bool = False, want_all_logits: bool = False, append_to=None, logprobs: Optional[bool] = None,
                capacity: Optional[int] = None, bans=None, eos_id: int = -1, lookup=None, allowed=None):
        """Run the prompt(s); returns (kv handle, next-token ids [B] int32 on device, logits [B, vocab] or None) -- with want_all_logits a fourth
        entry: the logits of EVERY position, [sum of lengths, vocab] fp32 (what the reference's forward returns, model/video_chatgpt.py:225-226).
        `append_to` = a kv handle this model filled before: the rows continue its sequences (pgv_llm_prefill_append; `max_seq` is ignored).
        `logprobs` (True / False): set the cache's log-probability switch (set_logprobs) before the prompt runs, so that the greedy first token is
        recorded too; None leaves the switch as it is.
        `capacity`: the cache is created for max(B, capacity) sequences, so that fork() has slots to grow into (ignored with `append_to`).
        `bans` (logit_bans.LogitBans, checked) with `eos_id`: set the cache's logit bans (set_bans) before the prompt runs, so that the slots' id
        record holds it -- on the `append_to` path too; None leaves the cache's configuration as it is.
        `lookup` (D, n): set_lookup before the prompt runs, for the same reason; None leaves the setting as it is.
        `allowed` (allowed.Allowed, checked: an automaton and one root per prompt) with `eos_id`: set_allowed before the prompt runs, so that the
        slots' prompt lengths are recorded; None leaves the cache's automaton as it is."""
        B = len(seqs)
        lens = [len(s) for s in seqs]
        feats = video_spatio_temporal_features
        proj = None
        V = 0
        vid_pos = [-1] * B
        if feats is not None and not (max(lens) == 1):     # the reference skips the splice when input_ids.shape[1]==1 (:103)
            proj, V, vid_pos = self._project_video(feats, seqs)
        if append_to is None:
            kv = self._get_kv(max(B, 1, int(capacity or 0)), max_seq)
            self._kv_epoch += 1
            self._reuse = None
        else:
            kv = append_to
        on = CacheSettings(logprobs, bans, eos_id, lookup=lookup, allowed=allowed)
        on.apply(self, kv)
        flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs])
        h_lens = (C.c_int32 * B)(*lens)
        h_pos = (C.c_int32 * B)(*vid_pos)
        nxt = torch.empty(B, dtype=torch.int32, device=self.device_)
        logits = torch.empty(B, self.vocab_size, dtype=torch.float32, device=self.device_) if want_logits else None
        ld_all = (self.vocab_size + 15) // 16 * 16
        all_logits = torch.empty(int(flat.size), ld_all, dtype=torch.float32, device=self.device_) if want_all_logits else None
        fn, who = (self.ctx.lib.pgv_llm_prefill, "pgv_llm_prefill") if append_to is None else (self.ctx.lib.pgv_llm_prefill_append, "pgv_llm_prefill_append")
        try:
            _lib.check(fn(self.ctx.handle, self.handle, kv, flat.ctypes.data_as(C.c_void_p), h_lens, B,
                          proj.data_ptr() if proj is not None else None, V, h_pos,
                          logits.data_ptr() if logits is not None else None, nxt.data_ptr(),
                          all_logits.data_ptr() if all_logits is not None else None, ld_all,
                          _lib.stream_ptr(self.device_)), who)
        except Exception:
            on.clear(self, kv)                             # a refused prompt never reaches the caller who would turn the switches off again
            raise
        if want_all_logits:
            return kv, nxt, logits, all_logits[:, :self.vocab_size]
        return kv, nxt, logits

    # ---- score: the per-token terms of the reference's forward(labels=...) loss (model/video_chatgpt.py:228-239) ------------------------
    @torch.no_grad()
    def score(self, input_ids, labels, video_spatio_temporal_features: Optional[torch.Tensor] = None) -> ScoreOutput:
        """Teacher-forced log-probabilities of given tokens: one prefill of `input_ids` ([B, S] tensor or a ragged list of id lists) and, for every
        position p whose `labels[p]` is not -100, log P(labels[p] | ids[:p]) from the logits of row p - 1 (HF's shift) -- computed on the device
        row by row (pgv_llm_score), never as a [rows, vocab] tensor.  `labels` has the shape of `input_ids`; scoring.continuation_labels builds the
        usual prompt / answer split.  `video_spatio_temporal_features`: [B, V, C], or one clip ([V, C] / [1, V, C]) for all B sequences (projected
        once).  Returns scoring.ScoreOutput; `.loss` is the number the reference's forward(labels=) returns as `loss` (forward(labels=) itself
        stays refused).  The KV cache (capacity: the longest sequence rounded up to 64) is refilled as by any prefill: earlier past_key_values
        go stale, and `.kv` is a live group that decode_step / decode_greedy continue from."""
        seqs = id_rows(input_ids)
        B = len(seqs)
        lens = [len(s_) for s_ in seqs]
        if B < 1 or min(lens) < 1:
            raise ValueError("score(): needs at least one non-empty sequence")
        targets = shift_labels(seqs, labels)
        limit = min(int(self.config.max_position_embeddings), 4096)
        if max(lens) > limit:
            raise ValueError(f"sequence of {max(lens)} tokens exceeds max_position_embeddings {limit}")
        max_seq = min(limit, (max(lens) + 63) // 64 * 64)
        feats = video_spatio_temporal_features
        proj, V, vid_pos = None, 0, [-1] * B
        if feats is not None:
            proj, V, vid_pos = self._project_video(feats, seqs, broadcast=True)
        kv = self._get_kv(B, max_seq)
        self._kv_epoch += 1
        self._reuse = None
        flat = np.concatenate([np.asarray(s_, dtype=np.int32) for s_ in seqs])
        M = int(flat.size)
        out = torch.empty(3, M, dtype=torch.float32, device=self.device_)         # logprob | lse | argmax (int32 bits)
        _lib.check(self.ctx.lib.pgv_llm_score(self.ctx.handle, self.handle, kv, flat.ctypes.data_as(C.c_void_p), (C.c_int32 * B)(*lens), B,
                                              proj.data_ptr() if proj is not None else None, V, (C.c_int32 * B)(*vid_pos),
                                              targets.ctypes.data_as(C.c_void_p), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                              _lib.stream_ptr(self.device_)), "pgv_llm_score")
        host = out.cpu()
        return ScoreOutput.from_rows(lens, targets, host[0].numpy(), host[2].view(torch.int32).numpy(), kv=kv)

    def prefill_slots(self, kv, slots: Sequence[int], seqs: Sequence[Sequence[int]], video_spatio_temporal_features: Optional[torch.Tensor],
                      want_logits: bool = False, u: Optional[torch.Tensor] = None, temperature: float = 1.0, top_k: int = 50,
                      top_p: float = 1.0, repetition_penalty: float = 1.0, counts: Optional[Sequence[int]] = None, filters=None):
        """Prefill NEW prompts `seqs` into cache slots `slots` of the live group `kv` (a handle prefill() returned) while the other slots keep
        their state (pgv_llm_prefill_slots: continuous batching).  `video_spatio_temporal_features` [n, V, C] (None: text only; a text-only
        prompt next to video ones takes any [V, C] block, it is not read).  u [n] (optional): draw each first token as sample_last does,
        else greedy.  top_p / repetition_penalty: the cache's warpers from this call on (set_warpers); the refilled slots start from a seen-set
        of their own prompt only.  Returns (first tokens [n] int32 on device, logits [n, vocab] or None).
        `counts` (pgv_llm_prefill_slots_n): prompt i gets counts[i] >= 1 sampled answers from ONE prefill -- `slots` and `u` then have
        S = sum(counts) entries, prompt 0's first, and S first tokens / logits rows come back; bit for bit the call with prompt i repeated
        counts[i] times.
        `filters` (sample_filters.SampleFilters or a dict of its fields): the cache's filter tail from this call on (set_filters); None leaves the
        cache's values as they are."""
        n = len(seqs)
        self.set_warpers(kv, top_p, repetition_penalty)
        if filters is not None:
            self.set_filters(kv, filters)
        if counts is not None and len(counts) != n:
            raise ValueError(f"{len(counts)} counts for {n} prompts")
        S = n if counts is None else sum(int(c) for c in counts)
        if len(slots) != S:
            raise ValueError(f"{len(slots)} slots for {n} prompts" + ("" if counts is None else f" with {S} samples"))
        lens = [len(s) for s in seqs]
        feats = video_spatio_temporal_features
        proj, V, vid_pos = None, 0, [-1] * n
        if feats is not None:
            proj, V, vid_pos = self._project_video(feats, seqs)
        flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs])
        nxt = torch.empty(S, dtype=torch.int32, device=self.device_)
        logits = torch.empty(S, self.vocab_size, dtype=torch.float32, device=self.device_) if want_logits else None
        if u is not None:
            u = u.to(device=self.device_, dtype=torch.float32).contiguous()
            assert u.numel() == S
        h_slots = (C.c_int32 * S)(*[int(s) for s in slots])
        tail = (flat.ctypes.data_as(C.c_void_p), (C.c_int32 * n)(*lens), proj.data_ptr() if proj is not None else None, V, (C.c_int32 * n)(*vid_pos),
                float(temperature), int(top_k), u.data_ptr() if u is not None else None, logits.data_ptr() if logits is not None else None,
                nxt.data_ptr(), _lib.stream_ptr(self.device_))
        if counts is None:
            _lib.check(self.ctx.lib.pgv_llm_prefill_slots(self.ctx.handle, self.handle, kv, h_slots, n, *tail), "pgv_llm_prefill_slots")
        else:
            _lib.check(self.ctx.lib.pgv_llm_prefill_slots_n(self.ctx.handle, self.handle, kv, h_slots, (C.c_int32 * n)(*[int(c) for c in counts]), n, *tail),
                       "pgv_llm_prefill_slots_n")
        return nxt, logits

    def set_warpers(self, kv, top_p: float = 1.0, repetition_penalty: float = 1.0):
        """pgv_kv_set_warpers: HF's TopPLogitsWarper / RepetitionPenaltyLogitsProcessor values for every later pick on this cache."""
        _lib.check(self.ctx.lib.pgv_kv_set_warpers(kv, float(top_p), float(repetition_penalty)), "pgv_kv_set_warpers")

    def set_filters(self, kv, filters=None):
        """pgv_kv_set_filters: HF's min_p / typical_p / epsilon_cutoff / eta_cutoff warpers (sample_filters.SampleFilters or a dict of its fields;
        None or a neutral record: off) for every later SAMPLED pick on this cache; set_warpers leaves them alone, greedy picks ignore them."""
        f = SampleFilters.coerce(filters).check()
        if f.neutral:
            _lib.check(self.ctx.lib.pgv_kv_set_filters(kv, None), "pgv_kv_set_filters")
            return
        cfg = _lib.FilterConfig.from_filters(f)
        _lib.check(self.ctx.lib.pgv_kv_set_filters(kv, C.byref(cfg)), "pgv_kv_set_filters")

    def set_bans(self, kv, bans=None, eos_id: int = -1):
        """pgv_kv_set_bans: HF's -inf processors (logit_bans.LogitBans; None or a neutral record: off) for every later covered pick on this cache.
        Set them before the prefill of the sequences they are meant for (prefill(..., bans=) does).  `eos_id`: the id the two length rules ban."""
        bans = LogitBans.coerce(bans).check(self.vocab_size, eos_id)
        if bans.effective_neutral(eos_id):
            _lib.check(self.ctx.lib.pgv_kv_set_bans(kv, None), "pgv_kv_set_bans")
            return
        cfg = _lib.BanConfig.from_bans(bans, -1 if eos_id is None else int(eos_id))
        _lib.check(self.ctx.lib.pgv_kv_set_bans(kv, C.byref(cfg)), "pgv_kv_set_bans")

    def set_allowed(self, kv, automaton=None, roots=None, eos_id: int = -1):
        """pgv_kv_set_allowed: constrained decoding by a token automaton (allowed.TokenAutomaton; None: off) for every later covered pick on this
        cache.  `roots`: the start state of every slot (None: all 0; a shorter list is padded with 0).  `eos_id`: the token that ends an answer --
        the rule needs one.  Set it before the prefill of the sequences it is meant for (prefill(..., allowed=) does)."""
        if automaton is None:
            _lib.check(self.ctx.lib.pgv_kv_set_allowed(kv, None), "pgv_kv_set_allowed")
            return
        full = np.zeros(MAX_GROUP, dtype=np.int32)
        if roots is not None:
            full[:len(roots)] = np.asarray(roots, dtype=np.int32)
        cfg = _lib.AllowConfig.from_automaton(automaton, full, -1 if eos_id is None else int(eos_id))
        _lib.check(self.ctx.lib.pgv_kv_set_allowed(kv, C.byref(cfg)), "pgv_kv_set_allowed")

    def allow_peek(self, kv, slot: int, n: int):
        """pgv_kv_allow_peek (test read-back): (the first n entries of the slot's state record as a list, the slot's root)."""
        out = torch.empty(int(n) + 1, dtype=torch.int32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_kv_allow_peek(kv, int(slot), int(n), out.data_ptr(), out[int(n):].data_ptr(), _lib.stream_ptr(self.device_)),
                   "pgv_kv_allow_peek")
        h = out.cpu().tolist()
        return h[:int(n)], h[int(n)]

    def set_guidance(self, kv, scale: float = 1.0, pairs: int = 0):
        """pgv_kv_set_guidance: classifier-free guidance for every later covered pick on this cache -- slots [0, pairs) of a live group of 2 * pairs are
        the conditional sequences, slot pairs + p the unconditional twin of p (prefill prompts + negatives as one batch).  scale 1 or pairs 0: off."""
        _lib.check(self.ctx.lib.pgv_kv_set_guidance(kv, float(scale), int(pairs)), "pgv_kv_set_guidance")

    def guidance_logits(self, cond: torch.Tensor, uncond: torch.Tensor, scale: float) -> torch.Tensor:
        """pgv_guidance_logits: scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond) on fp32 logits [P, vocab] -> [P, vocab], the
        kernel a guided pick reads its rows from (guidance.guided_scores is the rule in fp64)."""
        return self.ctx.guidance_logits(cond.to(device=self.device_, dtype=torch.float32), uncond.to(device=self.device_, dtype=torch.float32), scale)

    def ids_peek(self, kv, slot: int, n: int):
        """pgv_kv_ids_peek (test read-back): (the first n ids of the slot's record as a list, the slot's prompt length)."""
        out = torch.empty(int(n) + 1, dtype=torch.int32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_kv_ids_peek(kv, int(slot), int(n), out.data_ptr(), out[int(n):].data_ptr(), _lib.stream_ptr(self.device_)),
                   "pgv_kv_ids_peek")
        h = out.cpu().tolist()
        return h[:int(n)], h[int(n)]

    def set_logprobs(self, kv, on: bool = True):
        """pgv_kv_set_logprobs: record the two log-probabilities (`model`, `pick`: include/pgv.h) of every later pick on this cache."""
        _lib.check(self.ctx.lib.pgv_kv_set_logprobs(kv, 1 if on else 0), "pgv_kv_set_logprobs")

    def logprobs_last(self, kv, width: int) -> torch.Tensor:
        """pgv_kv_logprobs_last: fp32 [2, width] on the device -- row 0 `model`, row 1 `pick` of each slot's most recent pick."""
        out = torch.empty(2, int(width), dtype=torch.float32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_kv_logprobs_last(kv, out[0].data_ptr(), out[1].data_ptr(), _lib.stream_ptr(self.device_)), "pgv_kv_logprobs_last")
        return out

    def logprobs_steps(self, kv, width: int, n: int) -> torch.Tensor:
        """pgv_kv_logprobs_steps: fp32 [2, width, n] on the device -- the `model` / `pick` values of the n steps of the last decode_greedy /
        decode_sample call, laid out like its tokens."""
        out = torch.empty(2, int(width), int(n), dtype=torch.float32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_kv_logprobs_steps(kv, int(n), out[0].data_ptr(), out[1].data_ptr(), _lib.stream_ptr(self.device_)), "pgv_kv_logprobs_steps")
        return out

    def greedy_last(self, kv, width: int, repetition_penalty: float = 1.0) -> torch.Tensor:
        """The greedy pick of every sequence from the logits of the last prefill / decode call, under the repetition penalty
        (pgv_llm_pick_greedy): what the prefill's own argmax, which knows no penalty, has to be replaced with."""
        self.set_warpers(kv, 1.0, repetition_penalty)
        nxt = torch.empty(int(width), dtype=torch.int32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_llm_pick_greedy(self.ctx.handle, self.handle, kv, nxt.data_ptr(), _lib.stream_ptr(self.device_)), "pgv_llm_pick_greedy")
        return nxt

    def fork(self, kv, counts: Sequence[int]) -> int:
        """pgv_kv_fork: sequence p of the live group of `kv` becomes counts[p] consecutive slots (new slot i copies old slot
        generation.fork_sources(counts)[i]: cache rows, length, current token, done flag, seen-set, logits row, latest log-probabilities).
        The cache must have been created for at least sum(counts) sequences (prefill(..., capacity=)).  Returns the new width."""
        src = fork_sources(counts)
        P = len(counts)
        _lib.check(self.ctx.lib.pgv_kv_fork(self.ctx.handle, self.handle, kv, (C.c_int32 * P)(*[int(c) for c in counts]), P,
                                            _lib.stream_ptr(self.device_)), "pgv_kv_fork")
        self._kv_epoch += 1                 # a PastKeyValues object handed out earlier describes another group width
        return len(src)

    def kv_gather(self, kv, K: int, src: Sequence[int], row0: Sequence[int]):
        """pgv_kv_gather: inside every group of K consecutive slots of the live group, slot g * K + i receives the cache rows [row0[g], len) and the
        current token of slot g * K + src[g * K + i] (the cache reorder of a beam step; rows below row0[g] are shared by the group and stay)."""
        W, P = len(src), len(row0)
        _lib.check(self.ctx.lib.pgv_kv_gather(self.ctx.handle, self.handle, kv, int(K), (C.c_int32 * W)(*[int(v) for v in src]),
                                              (C.c_int32 * P)(*[int(v) for v in row0]), _lib.stream_ptr(self.device_)), "pgv_kv_gather")

    def beam_begin(self, kv, beams: int, max_new_tokens: int, eos_id: int = -1, length_penalty: float = 1.0, early_stopping=False):
        """pgv_beam_begin: start a beam search on the live group of `kv` (a prefill with capacity >= prompts x beams): every prompt is forked to
        `beams` consecutive slots and the first pick runs on the prefill's logits."""
        cfg = _lib.BeamConfig(int(beams), int(max_new_tokens), int(eos_id), float(length_penalty), early_code(early_stopping))
        _lib.check(self.ctx.lib.pgv_beam_begin(self.ctx.handle, self.handle, kv, C.byref(cfg), _lib.stream_ptr(self.device_)), "pgv_beam_begin")
        self._kv_epoch += 1                 # a PastKeyValues object handed out earlier describes another group width

    def decode_beam(self, kv, n: int):
        """pgv_llm_decode_beam: n beam steps on the device (trunk, lm_head, beam pick, in-group cache gather), no host round trip."""
        _lib.check(self.ctx.lib.pgv_llm_decode_beam(self.ctx.handle, self.handle, kv, int(n), _lib.stream_ptr(self.device_)), "pgv_llm_decode_beam")

    def beam_open(self, kv, prompts: int) -> List[bool]:
        """pgv_beam_open: which prompts of the beam run can still improve (synchronises)."""
        h = (C.c_int32 * int(prompts))()
        _lib.check(self.ctx.lib.pgv_beam_open(kv, h, _lib.stream_ptr(self.device_)), "pgv_beam_open")
        return [bool(v) for v in h]

    def beam_result(self, kv, p: int, rank: int = 0):
        """pgv_beam_result: (tokens, score, finished) of finished entry `rank` (0 = best) of prompt p; score is HF's sequences_scores."""
        n, score, fin = C.c_int32(), C.c_float(), C.c_int32()
        s = _lib.stream_ptr(self.device_)
        _lib.check(self.ctx.lib.pgv_beam_result(kv, int(p), int(rank), None, 0, C.byref(n), C.byref(score), C.byref(fin), s), "pgv_beam_result")
        toks = (C.c_int32 * max(1, n.value))()
        if n.value:
            _lib.check(self.ctx.lib.pgv_beam_result(kv, int(p), int(rank), toks, n.value, C.byref(n), C.byref(score), C.byref(fin), s), "pgv_beam_result")
        return [int(toks[i]) for i in range(n.value)], float(score.value), bool(fin.value)

    def kv_peek(self, kv, layer: int, which: int, slot: int, row0: int, nrows: int) -> torch.Tensor:
        """pgv_kv_peek (tests / debugging): cache rows [row0, row0 + nrows) of `slot` in `layer`, which = 0 keys / 1 values ->
        [heads, nrows, 128] in the model's dtype."""
        out = torch.empty(self.config.num_attention_heads, int(nrows), 128, dtype=self.dtype_, device=self.device_)
        _lib.check(self.ctx.lib.pgv_kv_peek(kv, int(layer), int(which), int(slot), int(row0), int(nrows), out.data_ptr(),
                                            _lib.stream_ptr(self.device_)), "pgv_kv_peek")
        return out

    def kv_len(self, kv, b: int) -> int:
        return int(self.ctx.lib.pgv_kv_len(kv, int(b)))

    def kv_truncate(self, kv, b: int, length: int):
        _lib.check(self.ctx.lib.pgv_kv_truncate(kv, int(b), int(length), _lib.stream_ptr(self.device_)), "pgv_kv_truncate")

    def decode_step(self, kv, last: torch.Tensor, want_logits: bool = False):
        B = last.shape[0]
        nxt = torch.empty(B, dtype=torch.int32, device=self.device_)
        logits = torch.empty(B, self.vocab_size, dtype=torch.float32, device=self.device_) if want_logits else None
        _lib.check(self.ctx.lib.pgv_llm_decode(self.ctx.handle, self.handle, kv, last.data_ptr(),
                                               logits.data_ptr() if logits is not None else None, nxt.data_ptr(),
                                               _lib.stream_ptr(self.device_)), "pgv_llm_decode")
        return nxt, logits

    def set_lookup(self, kv, D: int, n: int = 2):
        """pgv_kv_set_lookup: D drafts per sequence and step by n-gram lookup (`decode_lookup`), up to 1 + D rows per sequence in `decode_rows`; 0
        turns it off.  Set it before the prompt runs (`prefill(lookup=(D, n))`), so that the cache's id record holds the prompt."""
        _lib.check(self.ctx.lib.pgv_kv_set_lookup(kv, int(D), int(n)), "pgv_kv_set_lookup")

    def decode_lookup(self, kv, first: Optional[torch.Tensor], steps: int, eos_id: int, budget: Sequence[int]):
        """pgv_llm_decode_lookup: `steps` prompt-lookup steps from `first` [B] (None: from the cache's current tokens, where the last call
        stopped); budget [B]: tokens each sequence may still emit.  Returns (tokens int32 [B, steps * (1 + D)] on the device, each row's emitted
        tokens packed from column 0; counts int32 [steps, B] on the HOST: tokens emitted per step).  The tokens are those of decode_greedy, in
        fewer passes over the weights."""
        B = len(budget)
        D = max(0, int(self.ctx.lib.pgv_kv_lookup(kv)))
        toks = torch.zeros(B, int(steps) * (1 + D), dtype=torch.int32, device=self.device_)
        counts = torch.zeros(int(steps), B, dtype=torch.int32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_llm_decode_lookup(self.ctx.handle, self.handle, kv, first.data_ptr() if first is not None else None, int(steps), int(eos_id),
                                                      (C.c_int32 * B)(*[int(x) for x in budget]), toks.data_ptr(), counts.data_ptr(),
                                                      _lib.stream_ptr(self.device_)), "pgv_llm_decode_lookup")
        return toks, counts.cpu().numpy()

    def decode_lookup_sample(self, kv, first: Optional[torch.Tensor], steps: int, eos_id: int, budget: Sequence[int], u_base: Sequence[int],
                             temperature: float, top_k: int, u: torch.Tensor):
        """pgv_llm_decode_lookup_sample: `decode_lookup` for a sampled run.  u [rows, B]: the uniforms of the whole run, row i those of its i-th new
        token; u_base [B]: tokens each sequence has emitted before this call.  Row (b, j) of a step is picked with u[u_base[b] + e + j][b], e = tokens
        b has emitted in this call, by the pick of `decode_sample` (the cache's top_p and filters included; `set_warpers` / `set_filters` beforehand).
        Returns what decode_lookup returns; the tokens are bit for bit those of decode_sample from the same uniforms."""
        B = len(budget)
        assert len(u_base) == B, "one uniform base per sequence"
        D = max(0, int(self.ctx.lib.pgv_kv_lookup(kv)))
        u = u.to(device=self.device_, dtype=torch.float32).contiguous()
        assert u.dim() == 2 and u.shape[1] == B, "u is [rows, B]"
        toks = torch.zeros(B, int(steps) * (1 + D), dtype=torch.int32, device=self.device_)
        counts = torch.zeros(int(steps), B, dtype=torch.int32, device=self.device_)
        ints = lambda xs: (C.c_int32 * B)(*[int(x) for x in xs])      # noqa: E731
        _lib.check(self.ctx.lib.pgv_llm_decode_lookup_sample(self.ctx.handle, self.handle, kv, first.data_ptr() if first is not None else None, int(steps),
                                                             int(eos_id), ints(budget), ints(u_base), float(temperature), int(top_k), u.data_ptr(),
                                                             int(u.shape[0]), toks.data_ptr(), counts.data_ptr(), _lib.stream_ptr(self.device_)),
                   "pgv_llm_decode_lookup_sample")
        return toks, counts.cpu().numpy()

    def decode_rows(self, kv, slots, tokens: torch.Tensor) -> torch.Tensor:
        """pgv_llm_decode_rows: one pass over the weights for several consecutive positions per sequence.  `slots` lists the sequence of every row
        (a sequence's rows consecutively), `tokens` [R] int32 the token each row consumes; row j of a sequence runs at position kv_len + j.  Returns
        the fp32 logits [R, vocab], bit for bit those of consecutive `decode_step` calls fed the same tokens.  Nothing advances."""
        slots = [int(b) for b in slots]
        tokens = tokens.to(device=self.device_, dtype=torch.int32).contiguous()
        assert tokens.numel() == len(slots), "one token per row"
        logits = torch.empty(len(slots), self.vocab_size, dtype=torch.float32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_llm_decode_rows(self.ctx.handle, self.handle, kv, (C.c_int32 * len(slots))(*slots), tokens.data_ptr(), len(slots),
                                                    logits.data_ptr(), _lib.stream_ptr(self.device_)), "pgv_llm_decode_rows")
        return logits

    def decode_greedy(self, kv, first: torch.Tensor, n: int, eos_id: int = -1, repetition_penalty: float = 1.0) -> torch.Tensor:
        """n greedy steps on the device; repetition_penalty != 1: the argmax of the penalised logits (the cache's seen-set)."""
        B = first.shape[0]
        self.set_warpers(kv, 1.0, repetition_penalty)
        toks = torch.empty(B, n, dtype=torch.int32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_llm_decode_greedy(self.ctx.handle, self.handle, kv, first.data_ptr(), n, eos_id, toks.data_ptr(),
                                                      _lib.stream_ptr(self.device_)), "pgv_llm_decode_greedy")
        return toks

    def sample_last(self, kv, u: torch.Tensor, temperature: float, top_k: int = 50, top_p: float = 1.0, repetition_penalty: float = 1.0) -> torch.Tensor:
        """Draw the next token of every sequence from the logits of the last prefill / decode call (pgv_llm_sample): u [B] uniforms."""
        self.set_warpers(kv, top_p, repetition_penalty)
        u = u.to(device=self.device_, dtype=torch.float32).contiguous()
        nxt = torch.empty(u.numel(), dtype=torch.int32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_llm_sample(self.ctx.handle, self.handle, kv, float(temperature), int(top_k), u.data_ptr(), nxt.data_ptr(),
                                               _lib.stream_ptr(self.device_)), "pgv_llm_sample")
        return nxt

    def decode_sample(self, kv, first: torch.Tensor, n: int, eos_id: int, temperature: float, top_k: int, u: torch.Tensor, top_p: float = 1.0,
                      repetition_penalty: float = 1.0) -> torch.Tensor:
        """n sampled steps on the device (pgv_llm_decode_sample): u [n, B] uniforms, step i draws with u[i]."""
        B = first.shape[0]
        self.set_warpers(kv, top_p, repetition_penalty)
        u = u.to(device=self.device_, dtype=torch.float32).contiguous()
        assert u.shape == (n, B)
        toks = torch.empty(B, n, dtype=torch.int32, device=self.device_)
        _lib.check(self.ctx.lib.pgv_llm_decode_sample(self.ctx.handle, self.handle, kv, first.data_ptr(), n, eos_id, float(temperature), int(top_k),
                                                      u.data_ptr(), toks.data_ptr(), _lib.stream_ptr(self.device_)), "pgv_llm_decode_sample")
        return toks

    # ---- forward: the reference's own public entry (model/video_chatgpt.py:193-251) --------------------------------
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, past_key_values=None, inputs_embeds=None, labels=None, use_cache=None,
                output_attentions=None, output_hidden_states=None, video_spatio_temporal_features: Optional[torch.Tensor] = None,
                return_dict=None, max_length: Optional[int] = None, **_unused):
        """`model(input_ids=ids, video_spatio_temporal_features=f, use_cache=True)` -> object with `.logits` [B, S, vocab] and `.past_key_values`;
        `model(input_ids=tok [B, 1], past_key_values=out.past_key_values, ...)` -> the next step (`input_ids.shape[1] == 1` skips the splice,
        :103); `input_ids [B, S > 1]` next to a cache appends S tokens per sequence (a later chat turn) and returns their S logit rows.
        `max_length` (first call): positions the cache is allocated for (default: prompt + 256).
        This is the recipe SURVEY.md 8c drives the reference with (prefill + cached single-token steps); `generate()` is the fast path
        and what the reference's own callers use.  Inference only: `labels`, `inputs_embeds`, attention / hidden-state outputs and a padded
        `attention_mask` have no counterpart in the eval path and raise; logits are fp32 (HF up-casts them for the loss the same way)."""
        if labels is not None or inputs_embeds is not None or output_attentions or output_hidden_states:
            raise NotImplementedError("forward(): labels / inputs_embeds / output_attentions / output_hidden_states belong to the training path, "
                                      "which is outside this package (SURVEY.md 2 OUT-OF-SCOPE)")
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        ids = torch.as_tensor(input_ids)
        if ids.dim() == 1:
            ids = ids[None]
        B, S = ids.shape
        if attention_mask is not None and not bool(torch.as_tensor(attention_mask).to(torch.bool).all()):
            raise NotImplementedError("forward(): padded batches are not supported; pass equal-length prompts or use generate() with a list of prompts")
        limit = min(int(self.config.max_position_embeddings), 4096)
        if past_key_values is None:
            # cache capacity: the prompt + `max_length` headroom (default 256 further positions, rounded up to 64) -- NOT the whole context window
            # (2 GiB per 7B sequence at 4096 positions, and a second cache shape evicts the one generate() was using)
            max_seq = min(limit, (int(max_length) if max_length is not None else S + 256) + 63 & ~63)
            if S > max_seq:
                raise ValueError(f"prompt of {S} tokens exceeds {'max_length' if max_length is not None and S <= limit else 'max_position_embeddings'} {max_seq}")
            kv, _nxt, _lg, all_lg = self.prefill([row.tolist() for row in ids.cpu()], video_spatio_temporal_features, max_seq, want_all_logits=True)
            return CausalLMOutputWithPast(all_lg.reshape(B, S, -1), PastKeyValues(self, kv, B, S, max_seq, self._kv_epoch))
        if not isinstance(past_key_values, PastKeyValues) or past_key_values.owner is not self:
            raise ValueError("past_key_values must be the object a previous forward() of this model returned")
        if past_key_values.batch != B:
            raise ValueError(f"{B} sequences for a cache of {past_key_values.batch}")
        # one KV cache is kept alive per model and a later prefill of the SAME shape refills it in place: the epoch, not the handle, tells
        # whether this object still describes what the cache holds
        if past_key_values.epoch != self._kv_epoch or self._kv.get((past_key_values.batch, past_key_values.max_seq)) is not past_key_values.kv:
            raise RuntimeError("past_key_values is stale: the model has run another prefill / generate since (one KV cache is kept alive per model)")
        if past_key_values.seq_len + S > past_key_values.max_seq:
            raise ValueError(f"{past_key_values.seq_len} cached + {S} new tokens exceed the cache's {past_key_values.max_seq} positions "
                             f"(pass max_length= to the first forward(); the model's limit is {limit})")
        if S != 1:
            # any number of new tokens next to a cache (model/video_chatgpt.py:193-251; a later chat turn): prefill them behind the cached ones
            _kv, _nxt, _lg, all_lg = self.prefill([row.tolist() for row in ids.cpu()], video_spatio_temporal_features, 0, want_all_logits=True,
                                                  append_to=past_key_values.kv)
            past_key_values.seq_len += S
            return CausalLMOutputWithPast(all_lg.reshape(B, S, -1), past_key_values)
        _nxt, lg = self.decode_step(past_key_values.kv, ids[:, 0].to(device=self.device_, dtype=torch.int32).contiguous(), want_logits=True)
        past_key_values.seq_len += 1
        return CausalLMOutputWithPast(lg[:, None, :], past_key_values)

    # ---- generate ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, input_ids, video_spatio_temporal_features: Optional[torch.Tensor] = None, do_sample: bool = False,
                 temperature: Optional[float] = None, max_new_tokens: int = 1024, stopping_criteria=None, eos_token_id="config",
                 chunk: int = 32, generator: Optional[torch.Generator] = None, top_k: Optional[int] = None,
                 stop_strings: Optional[Sequence[Optional[str]]] = None, tokenizer=None, timings: Optional[dict] = None,
                 kv_reuse_key=None, top_p: Optional[float] = None, repetition_penalty: Optional[float] = None, output_logprobs: bool = False,
                 samples_per_prompt: int = 1, beams: int = 1, length_penalty: Optional[float] = None, early_stopping=None,
                 output_beam_scores: bool = False, bans=None, filters=None, lookup: int = 0, lookup_ngram: int = 2, lookup_sample: bool = False,
                 guidance=None, allowed=None, **_unused):
        """Returns LongTensor [B, S + n_new] on the device, prompt echoed (checked by inference.py:115-117).
        `output_logprobs=True` (a keyword of this package): returns generation.GenerateLogprobsOutput instead -- `.sequences` is that tensor,
        `.token_logprobs` / `.transition_scores` [B, n_new] fp32 on the host are each new token's log-probability under the model's own
        distribution / under the distribution the pick used (HF's compute_transition_scores on `logits` / `scores`, normalize_logits=True), cut
        where the ids are cut and 0 beyond a sequence's end; `.sequence_logprob` [B] fp64 sums the former.  The values are recorded on the device
        by the pick kernels inside the decode chunks (pgv_kv_set_logprobs); the ids are those of the call without the keyword, whatever `chunk`.

        input_ids: LongTensor [B, S] (equal-length prompts, the reference's case) or a list of id lists (ragged batch).
        Tokens never leave the device inside a chunk of `chunk` steps, in both modes:
          * greedy: pgv_llm_decode_greedy;
          * do_sample=True (the reference's default, temperature 0.2, inference.py:109-110): HF's sample loop is logits / temperature ->
            top-k mask (top_k = 50 is HF's default GenerationConfig value, which the reference inherits) -> softmax -> multinomial.  The
            multinomial draw is an inverse-CDF pick in a HIP kernel (pgv_llm_decode_sample) fed with uniforms drawn up front from
            `generator` (a device torch.Generator; one uniform per sequence and step, so a run is reproducible from the seed and
            independent of the chunk size).
        `temperature`, `top_k`, `top_p`, `repetition_penalty`: each from the call if given, else from `self.generation_config` (the checkpoint's
        generation_config.json), else HF's default (1.0, 50, 1.0, 1.0) -- HF's own precedence (generation.resolve_sampling).  top_p and the
        repetition penalty are HF's TopPLogitsWarper / RepetitionPenaltyLogitsProcessor inside the same device pick (pgv.h: pgv_kv_set_warpers);
        the penalty sees the prompt ids as given plus every generated token and also applies to greedy decoding, top_p to sampling only.
        Any other argument that would change HF's result (num_beams > 1, min_p, typical_p < 1, no_repeat_ngram_size > 0, ...:
        generation.REFUSED), in the call or in the generation config, raises ValueError naming it; inert ones stay ignored.
        Stopping criteria (B == 1, as in the reference) are evaluated on the host after each chunk, token by token in generation
        order, and the output is cut at the first hit: the same ids as a per-token loop, the surplus steps of the chunk are discarded.
        `stop_strings` (one per sequence, None = no stop string; needs `tokenizer`): the BATCHED form of the reference's
        KeywordsStoppingCriteria (model/utils.py:6-26, passed at inference.py:101-102 with batch size 1): after every chunk each live
        sequence's new ids are checked with `first_stop_length` (the exact per-token criterion, scanned incrementally); a sequence that
        fired is cut there and finished, and the loop ends when every sequence has finished -- at most one chunk past the last stop.
        `timings` (a dict) receives prefill_s / decode_s / steps of this call (host clock; the chunk boundaries are D2H syncs anyway).
        `kv_reuse_key` (B == 1; any hashable naming the conversation's video, None = off): keep the KV cache of this call for the next one with
        the same key -- a later chat turn whose prompt extends what the cache holds prefills only the NEW tokens behind the common prefix
        (pgv_kv_truncate + pgv_llm_prefill_append; the reference re-runs the whole conversation every turn, chat.py:108-160).  The video run
        must lie inside the common prefix (it was spliced when the cache was filled); otherwise the call falls back to a full prefill.  The
        appended rows are bitwise what one prefill over the same cache contents computes; cache entries that DECODE steps wrote (the previous
        answer) carry the decode path's 16-bit rounding instead of the prefill path's -- as with any KV cache that is kept across calls.
        `timings["reused_tokens"]` reports the prefix.
        `samples_per_prompt=n` (a keyword of this package; HF's `num_return_sequences` stays refused): n sampled answers per prompt from ONE
        prefill.  The B prompts run once in a cache created for B * n sequences, pgv_kv_fork copies every prompt's cache rows and slot state to n
        consecutive slots, and the loop above runs at width B * n -- the result is what generate() returns for the prompts repeated n times each
        (repeat_interleave: row b * n + j is sample j of prompt b) with the same generator, minus n - 1 prefills per prompt.  Uniforms are
        torch.rand(max_new_tokens, B * n); `stop_strings` and `video_spatio_temporal_features` stay per PROMPT.  Needs do_sample=True and
        B * n <= 64; not combinable with `stopping_criteria` or `kv_reuse_key`.  n = 1 is the path above, unchanged.
        `beams=K` (a keyword of this package; HF's `num_beams` stays refused): beam search as HF's generate(num_beams=K) computes it, K <= 8 beams per
        prompt from ONE prefill, every step on the device (pgv.h: pgv_beam_begin states the rules; equal scores, which torch.topk leaves open, go to
        the lower index).  `length_penalty` / `early_stopping` (False, True, "never"): from the call, else the generation config, else HF's defaults
        (1.0, False); without `beams` they stay inert.  Returns the best hypothesis of every prompt in the shape above; `output_beam_scores=True`
        returns generation.GenerateBeamsOutput with HF's `sequences_scores`.  The result does not depend on `chunk` (the steps between two looks at the
        prompts' open flags).  B * K <= 64; not combinable with do_sample, samples_per_prompt > 1, a repetition penalty, output_logprobs,
        stopping_criteria, stop_strings or kv_reuse_key (generation.check_beams).  K = 1 is greedy decoding, the path above, unchanged.
        `bans` (a keyword of this package: logit_bans.LogitBans, a dict of its fields, or None; HF's argument names stay refused): HF's processors
        that set scores to -inf -- no_repeat_ngram (HF: no_repeat_ngram_size), bad_words (bad_words_ids), suppress (suppress_tokens), begin_suppress
        (begin_suppress_tokens), min_length, min_new_tokens -- applied on the device between the lm_head and the pick (pgv.h: pgv_kv_set_bans), at
        HF's place in the chain: after the repetition penalty, before temperature / top-k / top-p.  They see the prompt ids as given plus every
        generated token; the prompt length of min_new_tokens / begin_suppress is the length of the prompt.  Validated on the host before any device
        work, with HF's wording; a bad word equal to [eos] is dropped, as HF does.  Greedy decoding under bans takes the route of greedy under a
        repetition penalty.  With `output_logprobs`, token_logprobs stay the raw model's and transition_scores are normalised over what survives
        (HF's `scores`).  Works with samples_per_prompt; `kv_reuse_key` falls back to the full prefill; `beams` > 1 is refused.  None or a record
        that asks nothing is the call without the keyword; the cache's configuration is cleared when the call ends.
        `filters` (a keyword of this package: sample_filters.SampleFilters, a dict of its fields, or None; HF's four argument names stay refused):
        HF's sampling warpers behind top-p -- min_p, typical_p, epsilon_cutoff, eta_cutoff -- inside the device pick, in HF's order (pgv.h:
        pgv_kv_set_filters).  Each field comes from the call if given (a key of the dict / a field that differs from its neutral value), else from
        `self.generation_config` under the same name, else it is neutral; a checkpoint whose generation_config.json carries one of them runs when
        the call passes `filters` (an empty dict takes the file's values) and is refused without it.  Validated on the host before any device
        work, with HF's wording.  Inert with do_sample=False, as top_p is; `beams` > 1 is refused.  With `output_logprobs`, transition_scores are
        normalised over the final survivors.  None or a neutral record is the call without the keyword, bit for bit.
        `lookup=D`, `lookup_ngram=n` (keywords of this package; HF's `prompt_lookup_num_tokens` / `max_matching_ngram_size` name the same two
        numbers and stay ignored, being inert for a greedy result): prompt-lookup speculative decoding.  Every step drafts up to D tokens per
        sequence by n-gram lookup in prompt + answer (HF's PromptLookupCandidateGenerator rule, on the device), verifies them in ONE pass over the
        weights and keeps the longest prefix the model agrees with -- the returned tensor is bit for bit the one of the call without the keyword,
        in fewer passes when the answer repeats itself or quotes the prompt.  `chunk` counts lookup steps.  Any B with B * (1 + D) <= 64; ragged
        prompts, `eos_token_id`, `max_new_tokens`, `stopping_criteria`, `stop_strings` and `timings` (which gains `lookup_steps` and
        `lookup_emitted`: tokens per pass = their quotient) work as without it; `kv_reuse_key` falls back to the full prefill.  Refused with
        do_sample, beams > 1, samples_per_prompt > 1, a repetition penalty, bans and output_logprobs (generation.check_lookup).
        `lookup_sample=True` (with `lookup=D` and do_sample=True): the same steps for a sampled run.  The uniforms are drawn as without it, one
        torch.rand(max_new_tokens, B) from `generator`; every row of a step is picked by the device pick from the uniform the plain run uses for that
        token (pgv.h: pgv_llm_decode_lookup_sample), and a draft is kept exactly when it equals that pick.  The returned tensor is therefore bit for
        bit the one of generate(do_sample=True) with the same generator -- not merely equal in distribution -- under any temperature, top_k, top_p
        and `filters`.  A draft x is kept with the probability p(x) the pick gives it, which is HF's speculative acceptance min(1, p / q) for a
        one-hot draft distribution q; how often that happens on real answers is unmeasured.  The other refusals of `lookup` stay.
        `guidance` (a keyword of this package: guidance.Guidance, a scale, a dict of its fields, or None; HF's `guidance_scale` /
        `negative_prompt_ids` name the same two things and are not arguments here): classifier-free guidance, HF's
        UnbatchedClassifierFreeGuidanceLogitsProcessor -- every pick reads scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond),
        `uncond` the logits of a negative prompt ("last_token" / None: HF's default, each prompt's last id; or one id list per prompt, e.g. the same
        question without the video: contrast decoding against the language prior).  The negatives are prefilled with the prompts as one ragged
        batch and run as B more rows of every token step; the mix is a kernel between the lm_head and the pick (pgv.h: pgv_kv_set_guidance), at
        HF's place in the chain: in front of the repetition penalty, the bans and the warpers, which all see the guided scores.  Combines with
        sampling, temperature, top_k, top_p, `filters`, repetition_penalty, `bans`, `stop_strings` and `stopping_criteria`; the uniforms stay
        torch.rand(max_new_tokens, B).  Refused with beams > 1, lookup, samples_per_prompt > 1, kv_reuse_key, output_logprobs and B > 32
        (guidance.check_guidance).  None or scale 1 is the call without the keyword, bit for bit.
        `allowed` (a keyword of this package: allowed.TokenAutomaton for all prompts, a list with one per prompt, or None; HF's
        `prefix_allowed_tokens_fn` is refused -- a callback cannot run on the device): constrained decoding, HF's PrefixConstrainedLogitsProcessor
        with the callback compiled into a token automaton (TokenAutomaton.from_sequences / from_texts: a closed set of answers; from_edges: the
        general form) that the device follows inside the captured decode graphs (pgv.h: pgv_kv_set_allowed), at the bans' place in the chain.  Only
        the tokens of the reached state's edges may come next, plus EOS where the state accepts; a walk that leaves the automaton, or a state
        without edges, allows EOS alone (allowed.allowed_ids is the rule).  Needs an EOS token.  Greedy decoding takes the route of greedy under a
        repetition penalty.  Combines with sampling, temperature, top_k, top_p, `filters`, repetition_penalty, `bans`, `guidance`,
        samples_per_prompt (a sample starts at its prompt's root), output_logprobs (token_logprobs stay the raw model's, transition_scores are
        normalised over what survives), stop_strings and stopping_criteria; `kv_reuse_key` falls back to the full prefill; `beams` > 1 and `lookup`
        are refused.  None is the call without the keyword, bit for bit; the cache's automaton is cleared when the call ends."""
        seqs = [row.tolist() for row in input_ids.cpu()] if torch.is_tensor(input_ids) else [list(s) for s in input_ids]
        plan = plan_generate(self, seqs, do_sample, temperature, max_new_tokens, stopping_criteria, eos_token_id, chunk, top_k, stop_strings, tokenizer,
                             kv_reuse_key, top_p, repetition_penalty, output_logprobs, samples_per_prompt, beams, length_penalty, early_stopping,
                             output_beam_scores, bans, filters, lookup, lookup_ngram, lookup_sample, unused=_unused, guidance=guidance, allowed=allowed)
        if plan.beams > 1:
            return generate_loop.generate_beams(self, plan, seqs, video_spatio_temporal_features, timings)
        return generate_loop.generate_chunks(self, plan, seqs, video_spatio_temporal_features, generator, tokenizer, timings, kv_reuse_key)


def _vision_config_from(mm_vision_tower) -> VisionConfig:
    """VisionConfig from the CLIP config the checkpoint names (model/video_chatgpt.py:43-49).  Accepts a local
    directory with a CLIP config.json, a CLIPVisionTowerConfig-like object, or the two published hub names."""
    if mm_vision_tower is None:
        return VisionConfig()
    if hasattr(mm_vision_tower, "image_size"):
        c = mm_vision_tower
        return VisionConfig(frame_size=c.image_size, patch_size=c.patch_size, hidden_size=c.hidden_size)
    if isinstance(mm_vision_tower, str) and os.path.isdir(mm_vision_tower):
        from ..vision_tower import CLIPVisionTowerConfig
        c = CLIPVisionTowerConfig.from_pretrained(mm_vision_tower)
        return VisionConfig(frame_size=c.image_size, patch_size=c.patch_size, hidden_size=c.hidden_size)
    known = {"openai/clip-vit-large-patch14": 224, "openai/clip-vit-large-patch14-336": 336}
    if mm_vision_tower in known:
        return VisionConfig(frame_size=known[mm_vision_tower], patch_size=14, hidden_size=1024)
    raise ValueError(f"cannot resolve mm_vision_tower={mm_vision_tower!r} offline: pass a local CLIP directory")
