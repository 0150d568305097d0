"""ctypes binding of libpgv.so (include/pgv.h).

There is NO fallback: if the HIP library cannot be built/loaded, or there is no gfx950 device when a
context is requested, this module raises.  Nothing here (or anywhere under video_llava_amd/) imports the
CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpgv.so")

ABI_VERSION = 328          # PGV_VERSION of include/pgv.h this table was written against
PGV_OK, PGV_EINVAL, PGV_EHIP, PGV_ENOMEM, PGV_ESTATE, PGV_ENAME = 0, 1, 2, 3, 4, 5
PGV_F16, PGV_BF16, PGV_F32 = 0, 1, 2
EPI_NONE, EPI_BIAS, EPI_BIAS_QGELU, EPI_BIAS_GELU, EPI_RESID, EPI_BIAS_RESID, EPI_SWIGLU, EPI_F32 = range(8)
EPI_LN_BIAS, EPI_LN_BIAS_QGELU, EPI_BIAS_RESID_LNOUT = 8, 9, 10      # folded LayerNorm (pgv_gemm_ex only)
SCORE_CHUNK_ROWS = 1024    # PGV_SCORE_CHUNK_ROWS: scored rows pgv_llm_score sends through lm_head at a time
FAMILIES = ("gemm", "vit_attn", "llm_prefill_attn", "decode_gemv", "decode_attn", "other", "decode_small")


class VitConfig(C.Structure):
    _fields_ = [("hidden", C.c_int), ("inter", C.c_int), ("layers", C.c_int), ("heads", C.c_int),
                ("image", C.c_int), ("patch", C.c_int), ("eps", C.c_float)]


class LlmConfig(C.Structure):
    _fields_ = [("vocab", C.c_int), ("hidden", C.c_int), ("inter", C.c_int), ("layers", C.c_int), ("heads", C.c_int),
                ("eps", C.c_float), ("rope_theta", C.c_float)]


_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float


class BeamConfig(C.Structure):
    """pgv_beam_config of include/pgv.h.  early_stopping: 0 False, 1 True, 2 "never"."""
    _fields_ = [("beams", _i), ("max_new_tokens", _i), ("eos_id", _i), ("length_penalty", _f), ("early_stopping", _i)]


BAN_MAX_IDS, BAN_MAX_WORDS, BAN_MAX_WORD_LEN = 1024, 256, 16      # PGV_BAN_MAX_* of include/pgv.h


class BanConfig(C.Structure):
    """pgv_ban_config of include/pgv.h (pgv_kv_set_bans, pgv_ban_logits).  `from_bans` keeps the host arrays alive as attributes."""
    _fields_ = [("no_repeat_ngram", _i), ("h_bad_words", C.POINTER(C.c_int32)), ("h_bad_word_lens", C.POINTER(C.c_int32)), ("n_bad_words", _i),
                ("h_suppress", C.POINTER(C.c_int32)), ("n_suppress", _i), ("h_begin_suppress", C.POINTER(C.c_int32)), ("n_begin_suppress", _i),
                ("min_length", _i), ("min_new_tokens", _i), ("eos_id", _i)]

    @classmethod
    def from_bans(cls, bans, eos_id: int = -1) -> "BanConfig":
        """`bans`: logit_bans.LogitBans (already checked: the EOS filter of its bad words is the caller's)."""
        flat = [int(t) for w in bans.bad_words for t in w]
        lens = [len(w) for w in bans.bad_words]
        arrs = [(C.c_int32 * max(1, len(v)))(*v) for v in (flat, lens, [int(t) for t in bans.suppress], [int(t) for t in bans.begin_suppress])]
        cfg = cls(int(bans.no_repeat_ngram), arrs[0], arrs[1], len(lens), arrs[2], len(bans.suppress), arrs[3], len(bans.begin_suppress),
                  int(bans.min_length), int(bans.min_new_tokens), int(eos_id))
        cfg._keep = arrs
        return cfg


class FilterConfig(C.Structure):
    """pgv_filter_config of include/pgv.h (pgv_kv_set_filters, pgv_sample_logits_filtered)."""
    _fields_ = [("min_p", _f), ("typical_p", _f), ("epsilon_cutoff", _f), ("eta_cutoff", _f)]

    @classmethod
    def from_filters(cls, f) -> "FilterConfig":
        """`f`: sample_filters.SampleFilters (min_p None: 0, the neutral value of the C layer)."""
        return cls(0.0 if f.min_p is None else float(f.min_p), float(f.typical_p), float(f.epsilon_cutoff), float(f.eta_cutoff))


ALLOW_MAX_STATES, ALLOW_MAX_EDGES = 1 << 20, 1 << 22      # PGV_ALLOW_MAX_* of include/pgv.h


class AllowConfig(C.Structure):
    """pgv_allow_config of include/pgv.h (pgv_kv_set_allowed, pgv_allow_logits).  `from_automaton` keeps the host arrays alive as attributes."""
    _fields_ = [("h_row_ptr", C.POINTER(C.c_int32)), ("h_edge_token", C.POINTER(C.c_int32)), ("h_edge_next", C.POINTER(C.c_int32)),
                ("h_accept", C.POINTER(C.c_uint8)), ("n_states", _i), ("n_edges", _i), ("h_roots", C.POINTER(C.c_int32)), ("eos_id", _i)]

    @classmethod
    def from_automaton(cls, automaton, roots=None, eos_id: int = -1) -> "AllowConfig":
        """`automaton`: allowed.TokenAutomaton; `roots`: one state per slot of the cache (None: all 0)."""
        import numpy as np
        arrs = [np.ascontiguousarray(automaton.row_ptr, dtype=np.int32), np.ascontiguousarray(automaton.edge_token, dtype=np.int32),
                np.ascontiguousarray(automaton.edge_next, dtype=np.int32), np.ascontiguousarray(automaton.accept, dtype=np.uint8)]
        if roots is not None:
            arrs.append(np.ascontiguousarray(roots, dtype=np.int32))
        ptr = [a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_int32)) if a.size else None for a in arrs]
        cfg = cls(ptr[0], ptr[1], ptr[2], ptr[3], int(automaton.n_states), int(automaton.n_edges), ptr[4] if roots is not None else None, int(eos_id))
        cfg._keep = arrs
        return cfg


def beam_state_words(K: int) -> int:
    """PGV_BEAM_STATE_WORDS(K): 32-bit words of one prompt's beam state."""
    return 6 * int(K) + 2


class GemmDesc(C.Structure):
    """pgv_gemm_desc of include/pgv.h (pgv_gemm_ex)."""
    _fields_ = [("d_A", _vp), ("lda", _i), ("d_W", _vp), ("ldw", _i), ("w_blocked", _i), ("d_bias", _vp), ("d_C", _vp), ("ldc", _i),
                ("M", _i), ("N", _i), ("K", _i), ("epi", _i), ("d_rowstat", _vp), ("d_colsum", _vp), ("d_gnext", _vp), ("d_x16", _vp),
                ("ldx16", _i), ("d_stats_part", _vp), ("d_rowmean", _vp), ("d_cshift", _vp)]


class GemvShape(C.Structure):
    """pgv_gemv_shape of include/pgv.h: the launch shape pgv_gemv_ex ran."""
    _fields_ = [("tl", _i), ("ct", _i), ("x2", _i), ("k8", _i), ("nwb", _i), ("wfmt", _i)]


class GemvDesc(C.Structure):
    """pgv_gemv_desc of include/pgv.h (pgv_gemv_ex)."""
    _fields_ = [("mode", _i), ("d_W", _vp), ("d_wscale", _vp), ("d_W12", _vp), ("d_x", _vp), ("ldx", _i), ("d_out", _vp), ("ldo", _i),
                ("N", _i), ("K", _i), ("B", _i), ("d_ssq_in", _vp), ("nparts_in", _i), ("hidden", _i), ("eps", _f),
                ("d_gamma", _vp), ("d_xg", _vp), ("d_ssq_out", _vp), ("d_amax_val", _vp), ("d_amax_idx", _vp), ("ssq_ts", _i), ("amax_ts", _i),
                ("d_k8_part", _vp), ("k8_part_bytes", C.c_size_t), ("x_blocked", _i), ("shape", C.POINTER(GemvShape))]


# name -> (restype, argtypes); every symbol declared in include/pgv.h
PROTOTYPES = {
    "pgv_version": (_i, []),
    "pgv_last_error": (C.c_char_p, []),
    "pgv_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "pgv_ctx_destroy": (None, [_vp]),
    "pgv_ctx_workspace_bytes": (C.c_size_t, [_vp]),
    "pgv_prof_enable": (_i, [_vp, _i]),
    "pgv_prof_reset": (_i, [_vp]),
    "pgv_prof_get": (_i, [_vp, _i, C.POINTER(_i64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pgv_prof_calibrate": (_i, [_vp, _vp, _i, C.POINTER(C.c_double)]),
    "pgv_vit_create": (_i, [_vp, C.POINTER(VitConfig), _i, C.POINTER(_vp)]),
    "pgv_vit_destroy": (None, [_vp]),
    "pgv_vit_load_tensor": (_i, [_vp, C.c_char_p, _vp, _i, _i, _i64, _vp]),
    "pgv_vit_missing": (_i, [_vp]),
    "pgv_preprocess_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pgv_vit_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "pgv_st_pool": (_i, [_vp, _vp, _i, _i, _i, _i, _i64, _i, _vp, _i, _vp]),
    "pgv_projector": (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _i, _i, _vp, _i, _vp, _vp]),
    "pgv_llm_create": (_i, [_vp, C.POINTER(LlmConfig), _i, C.POINTER(_vp)]),
    "pgv_llm_destroy": (None, [_vp]),
    "pgv_llm_load_tensor": (_i, [_vp, C.c_char_p, _vp, _i, _i, _i64, _vp]),
    "pgv_llm_missing": (_i, [_vp]),
    "pgv_llm_load_rows": (_i, [_vp, C.c_char_p, _vp, _i, _i, _i, _i, _i64, _vp]),
    "pgv_llm_resize_vocab": (_i, [_vp, _i, _vp]),
    "pgv_llm_vocab": (_i, [_vp]),
    "pgv_kv_create": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "pgv_kv_destroy": (None, [_vp]),
    "pgv_kv_len": (_i, [_vp, _i]),
    "pgv_llm_prefill": (_i, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _i, _vp, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _i, _vp]),
    "pgv_llm_prefill_append": (_i, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _i, _vp, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _i, _vp]),
    "pgv_llm_prefill_slots": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), _i, _vp, C.POINTER(C.c_int32), _vp, _i, C.POINTER(C.c_int32), _f, _i, _vp, _vp,
                                   _vp, _vp]),
    "pgv_llm_prefill_slots_n": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _vp, C.POINTER(C.c_int32), _vp, _i, C.POINTER(C.c_int32),
                                     _f, _i, _vp, _vp, _vp, _vp]),
    "pgv_logprob_rows": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pgv_llm_score": (_i, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _i, _vp, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp]),
    "pgv_kv_truncate": (_i, [_vp, _i, _i, _vp]),
    "pgv_kv_fork": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), _i, _vp]),
    "pgv_kv_peek": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pgv_kv_gather": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp]),
    "pgv_beam_begin": (_i, [_vp, _vp, _vp, C.POINTER(BeamConfig), _vp]),
    "pgv_llm_decode_beam": (_i, [_vp, _vp, _vp, _i, _vp]),
    "pgv_beam_open": (_i, [_vp, C.POINTER(C.c_int32), _vp]),
    "pgv_beam_result": (_i, [_vp, _i, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(_f), C.POINTER(C.c_int32), _vp]),
    "pgv_beam_pick_logits": (_i, [_vp, _vp, _i, _i, C.POINTER(BeamConfig), _i, _vp, _vp, _vp, _vp]),
    "pgv_llm_decode": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pgv_kv_set_lookup": (_i, [_vp, _i, _i]),
    "pgv_kv_lookup": (_i, [_vp]),
    "pgv_llm_decode_lookup": (_i, [_vp, _vp, _vp, _vp, _i, _i, C.POINTER(C.c_int32), _vp, _vp, _vp]),
    "pgv_llm_decode_lookup_sample": (_i, [_vp, _vp, _vp, _vp, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _f, _i, _vp, _i, _vp, _vp, _vp]),
    "pgv_llm_decode_rows": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), _vp, _i, _vp, _vp]),
    "pgv_llm_decode_greedy": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "pgv_llm_sample": (_i, [_vp, _vp, _vp, _f, _i, _vp, _vp, _vp]),
    "pgv_llm_decode_sample": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp]),
    "pgv_sample_logits": (_i, [_vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp]),
    "pgv_sample_logits_ex": (_i, [_vp, _vp, _i, _i, _f, _i, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "pgv_kv_set_warpers": (_i, [_vp, _f, _f]),
    "pgv_kv_set_logprobs": (_i, [_vp, _i]),
    "pgv_kv_logprobs_last": (_i, [_vp, _vp, _vp, _vp]),
    "pgv_kv_logprobs_steps": (_i, [_vp, _i, _vp, _vp, _vp]),
    "pgv_llm_pick_greedy": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "pgv_sample_logits_lp": (_i, [_vp, _vp, _i, _i, _f, _i, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "pgv_kv_set_filters": (_i, [_vp, C.POINTER(FilterConfig)]),
    "pgv_sample_logits_filtered": (_i, [_vp, _vp, _i, _i, _f, _i, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, C.POINTER(FilterConfig), _vp, _vp]),
    "pgv_kv_set_bans": (_i, [_vp, C.POINTER(BanConfig)]),
    "pgv_ban_logits": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i, C.POINTER(BanConfig), _vp]),
    "pgv_kv_ids_peek": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "pgv_kv_set_allowed": (_i, [_vp, C.POINTER(AllowConfig)]),
    "pgv_allow_logits": (_i, [_vp, _vp, _i, _i, _vp, _i, C.POINTER(AllowConfig), _vp]),
    "pgv_allow_logits_copy": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, C.POINTER(AllowConfig), _vp]),
    "pgv_kv_allow_peek": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "pgv_guidance_logits": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _i, _vp]),
    "pgv_kv_set_guidance": (_i, [_vp, _f, _i]),
    "pgv_kv_guidance": (_i, [_vp]),
    "pgv_ingest_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pgv_gemm": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pgv_gemm_ex": (_i, [_vp, _i, C.POINTER(GemmDesc), _vp]),
    "pgv_ln_stats": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "pgv_vit_attention": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pgv_gemv": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "pgv_pack_blocked": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp]),
    "pgv_unpack_blocked": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp]),
    "pgv_quantize_fp8_blocked": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "pgv_gemv_fp8": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "pgv_llm_quantize_fp8": (_i, [_vp, _vp, _vp]),
    "pgv_llm_is_fp8": (_i, [_vp]),
    "pgv_llm_set_weight_stream": (_i, [_vp, _i]),
    "pgv_llm_weight_stream_bytes": (_i64, [_vp, _i]),
    "pgv_w12_bytes": (C.c_size_t, [_i, _i]),
    "pgv_encode_w12_blocked": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "pgv_gemv_w12": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "pgv_gemv_ex": (_i, [_vp, _i, C.POINTER(GemvDesc), _vp]),
    "pgv_gemv_prep": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "pgv_llm_get_weight": (_i, [_vp, _vp, C.c_char_p, _vp, _vp]),
    "pgv_decode_attention": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "pgv_decode_attention_rows": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "pgv_prefill_attention": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp, _i, _i, _vp]),
    "pgv_layernorm": (_i, [_vp, _i, _vp, _vp, _vp, _f, _vp, _i, _i, _vp]),
    "pgv_rmsnorm": (_i, [_vp, _i, _vp, _vp, _f, _vp, _i, _i, _vp]),
}

_lib = None
_lock = threading.Lock()


def use_lab_build() -> None:
    """Lab scripts only (scripts/microbench.py ablate): bind the -DPGV_LAB library, which carries the timing-ablation switches.  Must be called
    before the first load(); nothing in the product calls it and no environment variable selects it."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("libpgv is already loaded")
    from . import build as _build
    LIB_PATH = _build.build(lab=True)


def load(build_if_missing: bool = True) -> C.CDLL:
    """Load libpgv.so (building it with hipcc first if it is not there).  Raises on any failure."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            if not build_if_missing:
                raise RuntimeError(f"{LIB_PATH} is missing; run `python -m video_llava_amd.build`")
            from . import build as _build
            _build.build()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)          # AttributeError = header/library mismatch: fail loudly
            fn.restype = res
            fn.argtypes = args
        if lib.pgv_version() != ABI_VERSION:
            raise RuntimeError(f"libpgv version {lib.pgv_version()} does not match the binding ({ABI_VERSION}); rebuild with "
                               "`python -m video_llava_amd.build --force`")
        _lib = lib
        return lib


def check(rc: int, what: str = "") -> None:
    if rc == PGV_OK:
        return
    msg = load().pgv_last_error().decode("utf-8", "replace")
    text = f"{what}: {msg}" if what else msg
    if rc == PGV_EINVAL or rc == PGV_ENAME:
        raise ValueError(text)
    if rc == PGV_ENOMEM:
        raise MemoryError(text)
    raise RuntimeError(text)


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float16:
        return PGV_F16
    if dt == torch.bfloat16:
        return PGV_BF16
    if dt == torch.float32:
        return PGV_F32
    raise ValueError(f"unsupported dtype {dt}")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class Context:
    """One pgv_ctx per GPU (per rank).  Use Context.get(device)."""
    _cache: dict[int, "Context"] = {}

    def __init__(self, device: int):
        if not torch.cuda.is_available():
            raise RuntimeError("video_llava_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                               "and there is no CPU fallback")
        self.lib = load()
        self.device = int(device)
        h = _vp()
        check(self.lib.pgv_ctx_create(self.device, C.byref(h)), "pgv_ctx_create")
        self.handle = h

    @classmethod
    def get(cls, device=None) -> "Context":
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        if isinstance(device, torch.device):
            device = device.index if device.index is not None else torch.cuda.current_device()
        device = int(device)
        if device not in cls._cache:
            cls._cache[device] = Context(device)
        return cls._cache[device]

    # ---- profiling -----------------------------------------------------------------------
    def prof_enable(self, on: bool = True):
        check(self.lib.pgv_prof_enable(self.handle, 1 if on else 0))

    def prof_reset(self):
        check(self.lib.pgv_prof_reset(self.handle))

    def prof_get(self) -> dict[str, dict]:
        out = {}
        for i, name in enumerate(FAMILIES):
            n, ms, fl, by = _i64(), C.c_double(), C.c_double(), C.c_double()
            check(self.lib.pgv_prof_get(self.handle, i, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
            out[name] = {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}
        return out

    def prof_calibrate(self, n: int = 512) -> float:
        """Mean elapsed ms of an empty event pair on the current stream (the fixed cost inside every per-launch measurement)."""
        ms = C.c_double()
        check(self.lib.pgv_prof_calibrate(self.handle, stream_ptr(), n, C.byref(ms)), "pgv_prof_calibrate")
        return ms.value

    # ---- thin op wrappers used by tests and by the Python mirrors ------------------------------
    def gemm(self, a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None, epi: int = EPI_NONE,
             out: torch.Tensor | None = None) -> torch.Tensor:
        """out = a @ w.T with the fused epilogue `epi` (see include/pgv.h enum pgv_epi)."""
        assert a.is_cuda and w.is_cuda and a.dtype == w.dtype and a.dim() == 2 and w.dim() == 2
        assert a.stride(1) == 1 and w.stride(1) == 1
        M, K = a.shape
        N = w.shape[0]
        if bias is not None:
            assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N
        if out is None:
            if epi == EPI_F32:
                out = torch.empty(M, N, dtype=torch.float32, device=a.device)
            elif epi == EPI_SWIGLU:
                out = torch.empty(M, N // 2, dtype=a.dtype, device=a.device)
            elif epi in (EPI_RESID, EPI_BIAS_RESID):
                raise ValueError("residual epilogues accumulate into `out`; pass it")
            else:
                out = torch.empty(M, N, dtype=a.dtype, device=a.device)
        check(self.lib.pgv_gemm(self.handle, dtype_code(a.dtype), epi, a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0),
                                bias.data_ptr() if bias is not None else None, out.data_ptr(), out.stride(0),
                                M, N, K, stream_ptr(a.device)), "pgv_gemm")
        return out

    def layernorm(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, dtype: torch.dtype) -> torch.Tensor:
        assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
        y = torch.empty(x.shape, dtype=dtype, device=x.device)
        check(self.lib.pgv_layernorm(self.handle, dtype_code(dtype), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps,
                                     y.data_ptr(), x.shape[0], x.shape[1], stream_ptr(x.device)), "pgv_layernorm")
        return y

    def rmsnorm(self, x: torch.Tensor, gamma: torch.Tensor, eps: float, dtype: torch.dtype) -> torch.Tensor:
        assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
        y = torch.empty(x.shape, dtype=dtype, device=x.device)
        check(self.lib.pgv_rmsnorm(self.handle, dtype_code(dtype), x.data_ptr(), gamma.data_ptr(), eps,
                                   y.data_ptr(), x.shape[0], x.shape[1], stream_ptr(x.device)), "pgv_rmsnorm")
        return y

    def st_pool(self, feats: torch.Tensor, n_temporal: int = 100, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
        """[T, P, C] (any frame stride, unit channel stride) -> [n_temporal + P, C]."""
        assert feats.is_cuda and feats.dim() == 3 and feats.stride(2) == 1 and feats.stride(1) == feats.shape[2]
        T, P, Cc = feats.shape
        out = torch.empty(n_temporal + P, Cc, dtype=out_dtype, device=feats.device)
        check(self.lib.pgv_st_pool(self.handle, feats.data_ptr(), dtype_code(feats.dtype), T, P, Cc, feats.stride(0), n_temporal,
                                   out.data_ptr(), dtype_code(out_dtype), stream_ptr(feats.device)), "pgv_st_pool")
        return out

    def ingest_u8(self, frames: torch.Tensor, size: int, dtype: torch.dtype) -> torch.Tensor:
        """uint8 [T, H, W, 3] on the device at native resolution -> nearest resize (load_video's rule) + CLIP normalisation -> [T, 3, size, size]."""
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 4 and frames.shape[-1] == 3
        T, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        out = torch.empty(T, 3, size, size, dtype=dtype, device=frames.device)
        check(self.lib.pgv_ingest_u8(self.handle, frames.data_ptr(), T, H, W, size, dtype_code(dtype), out.data_ptr(),
                                     stream_ptr(frames.device)), "pgv_ingest_u8")
        return out

    def sample_logits(self, logits: torch.Tensor, u: torch.Tensor, temperature: float, top_k: int = 50, top_p: float = 1.0,
                      repetition_penalty: float = 1.0, seen_ids: "torch.Tensor | None" = None) -> torch.Tensor:
        """Inverse-CDF pick from softmax(logits / temperature) restricted to the top_k logits (<= 0: all) with uniforms u [B] -> int32 [B].
        top_p / repetition_penalty (over seen_ids [B, n] int32) other than 1: sample_logits_ex."""
        if float(top_p) != 1.0 or float(repetition_penalty) != 1.0:
            return self.sample_logits_ex(logits, u, temperature, top_k, top_p, repetition_penalty, seen_ids)
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
        assert u.is_cuda and u.dtype == torch.float32 and u.is_contiguous() and u.numel() == logits.shape[0]
        out = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
        check(self.lib.pgv_sample_logits(self.handle, logits.data_ptr(), logits.shape[1], logits.shape[0], float(temperature), int(top_k),
                                         u.data_ptr(), out.data_ptr(), stream_ptr(logits.device)), "pgv_sample_logits")
        return out

    def sample_logits_ex(self, logits: torch.Tensor, u: torch.Tensor, temperature: float, top_k: int = 50, top_p: float = 1.0,
                         repetition_penalty: float = 1.0, seen_ids: "torch.Tensor | None" = None, seen_lens: "torch.Tensor | None" = None,
                         want_kept: bool = False):
        """pgv_sample_logits_ex: the pick with HF's repetition penalty (over seen_ids [B, n] int32, the first seen_lens[b] of each row; None:
        nothing seen) and nucleus filter.  Returns tokens int32 [B], or (tokens, kept [B]) with want_kept: the entries left with non-zero
        probability per row."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
        assert u.is_cuda and u.dtype == torch.float32 and u.is_contiguous() and u.numel() == logits.shape[0]
        B = logits.shape[0]
        stride = 0
        if seen_ids is not None:
            assert seen_ids.is_cuda and seen_ids.dtype == torch.int32 and seen_ids.is_contiguous() and seen_ids.dim() == 2 and seen_ids.shape[0] == B
            stride = seen_ids.shape[1]
            if seen_lens is None:
                seen_lens = torch.full((B,), stride, dtype=torch.int32, device=logits.device)
            assert seen_lens.is_cuda and seen_lens.dtype == torch.int32 and seen_lens.numel() == B and int(seen_lens.max()) <= stride
        out = torch.empty(B, dtype=torch.int32, device=logits.device)
        kept = torch.empty(B, dtype=torch.int32, device=logits.device) if want_kept else None
        check(self.lib.pgv_sample_logits_ex(self.handle, logits.data_ptr(), logits.shape[1], B, float(temperature), int(top_k), float(top_p),
                                            float(repetition_penalty), seen_ids.data_ptr() if seen_ids is not None else None, stride,
                                            seen_lens.data_ptr() if seen_ids is not None else None, u.data_ptr(), out.data_ptr(),
                                            kept.data_ptr() if kept is not None else None, stream_ptr(logits.device)), "pgv_sample_logits_ex")
        return (out, kept) if want_kept else out

    def ban_logits(self, logits: torch.Tensor, ids: torch.Tensor, lens: torch.Tensor, prompt_lens: torch.Tensor, bans, eos_id: int = -1) -> torch.Tensor:
        """pgv_ban_logits: HF's -inf processors (`bans`: logit_bans.LogitBans; the [eos] filter of its bad words is the caller's) on `logits`
        [B, V] fp32 IN PLACE.  Row b's sequence: the first lens[b] entries of ids[b] (int32 [B, stride]); prompt_lens [B].  Returns `logits`."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
        B = logits.shape[0]
        assert ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous() and ids.dim() == 2 and ids.shape[0] == B
        for t in (lens, prompt_lens):
            assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B
        assert B == 0 or int(lens.max()) <= ids.shape[1]
        cfg = BanConfig.from_bans(bans, int(eos_id))
        check(self.lib.pgv_ban_logits(self.handle, logits.data_ptr(), logits.shape[1], B, ids.data_ptr(), ids.shape[1], lens.data_ptr(),
                                      prompt_lens.data_ptr(), int(eos_id), C.byref(cfg), stream_ptr(logits.device)), "pgv_ban_logits")
        return logits

    def guidance_logits(self, cond: torch.Tensor, uncond: torch.Tensor, scale: float, V: "int | None" = None, out: "torch.Tensor | None" = None) -> torch.Tensor:
        """pgv_guidance_logits: HF's classifier-free guidance rule on fp32 rows cond / uncond [P, ld] (unit column stride, any row stride >= V, one
        stride for both; they may be the same tensor) over columns [0, V) (default: all) -> fp32 [P, V] (or `out`, any row stride >= V)."""
        for t in (cond, uncond):
            assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1
        assert cond.shape == uncond.shape
        P = cond.shape[0]
        V = cond.shape[1] if V is None else int(V)
        ld = max(cond.stride(0), cond.shape[1]) if P > 1 else cond.shape[1]
        assert P <= 1 or uncond.stride(0) == cond.stride(0), "cond and uncond need one row stride"
        if out is None:
            out = torch.empty(P, V, dtype=torch.float32, device=cond.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == P and out.shape[1] >= V
        check(self.lib.pgv_guidance_logits(self.handle, cond.data_ptr(), uncond.data_ptr(), ld, V, P, float(scale), out.data_ptr(),
                                           max(out.stride(0), out.shape[1]) if P > 1 else out.shape[1], stream_ptr(cond.device)), "pgv_guidance_logits")
        return out

    def allow_logits(self, logits: torch.Tensor, states: torch.Tensor, automaton, eos_id: int, out: "torch.Tensor | None" = None) -> torch.Tensor:
        """pgv_allow_logits: the token automaton's mask (allowed.TokenAutomaton) on `logits` [B, V] fp32 IN PLACE, row b in state states[b]
        (int32 [B]; -1: DEAD).  Returns `logits`.  `out` [B, V] fp32: pgv_allow_logits_copy -- the masked rows go there, `logits` stays as it is (the
        launch a pick on a cache makes); returns `out`."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
        B = logits.shape[0]
        assert states.is_cuda and states.dtype == torch.int32 and states.is_contiguous() and states.numel() == B
        cfg = AllowConfig.from_automaton(automaton, None, int(eos_id))
        if out is not None:
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == logits.shape
            check(self.lib.pgv_allow_logits_copy(self.handle, logits.data_ptr(), out.data_ptr(), logits.shape[1], B, states.data_ptr(), int(eos_id),
                                                 C.byref(cfg), stream_ptr(logits.device)), "pgv_allow_logits_copy")
            return out
        check(self.lib.pgv_allow_logits(self.handle, logits.data_ptr(), logits.shape[1], B, states.data_ptr(), int(eos_id), C.byref(cfg),
                                        stream_ptr(logits.device)), "pgv_allow_logits")
        return logits

    def sample_logits_lp(self, logits: torch.Tensor, u: "torch.Tensor | None", temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                         repetition_penalty: float = 1.0, seen_ids: "torch.Tensor | None" = None, seen_lens: "torch.Tensor | None" = None,
                         greedy: bool = False):
        """pgv_sample_logits_lp: sample_logits_ex plus the two log-probabilities of the returned token.  greedy: the arg-max of the penalised
        logits (temperature / top_k / top_p / u ignored).  Returns (tokens int32 [B], kept int32 [B], model fp32 [B], pick fp32 [B])."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
        B = logits.shape[0]
        if not greedy:
            assert u is not None and u.is_cuda and u.dtype == torch.float32 and u.is_contiguous() and u.numel() == B
        stride = 0
        if seen_ids is not None:
            assert seen_ids.is_cuda and seen_ids.dtype == torch.int32 and seen_ids.is_contiguous() and seen_ids.dim() == 2 and seen_ids.shape[0] == B
            stride = seen_ids.shape[1]
            if seen_lens is None:
                seen_lens = torch.full((B,), stride, dtype=torch.int32, device=logits.device)
            assert seen_lens.is_cuda and seen_lens.dtype == torch.int32 and seen_lens.numel() == B and int(seen_lens.max()) <= stride
        out = torch.empty(B, dtype=torch.int32, device=logits.device)
        kept = torch.empty(B, dtype=torch.int32, device=logits.device)
        lp = torch.empty(2, B, dtype=torch.float32, device=logits.device)
        check(self.lib.pgv_sample_logits_lp(self.handle, logits.data_ptr(), logits.shape[1], B, float(temperature), int(top_k), float(top_p),
                                            float(repetition_penalty), seen_ids.data_ptr() if seen_ids is not None else None, stride,
                                            seen_lens.data_ptr() if seen_ids is not None else None, u.data_ptr() if u is not None else None,
                                            out.data_ptr(), kept.data_ptr(), 1 if greedy else 0, lp[0].data_ptr(), lp[1].data_ptr(),
                                            stream_ptr(logits.device)), "pgv_sample_logits_lp")
        return out, kept, lp[0], lp[1]

    def sample_logits_filtered(self, logits: torch.Tensor, u: "torch.Tensor | None", temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                               repetition_penalty: float = 1.0, seen_ids: "torch.Tensor | None" = None, seen_lens: "torch.Tensor | None" = None,
                               greedy: bool = False, filters=None, want_range: bool = True):
        """pgv_sample_logits_filtered: sample_logits_lp behind HF's filter tail (`filters`: sample_filters.SampleFilters, a dict of its fields, or
        None -- passed to the C layer unchecked, so that its refusals can be seen).  Returns (tokens, kept, model, pick, kept_range fp32 [B, 2] or
        None): kept_range is the smallest / largest kept (penalised) logit of each row."""
        from .sample_filters import SampleFilters
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
        B = logits.shape[0]
        if not greedy:
            assert u is not None and u.is_cuda and u.dtype == torch.float32 and u.is_contiguous() and u.numel() == B
        stride = 0
        if seen_ids is not None:
            assert seen_ids.is_cuda and seen_ids.dtype == torch.int32 and seen_ids.is_contiguous() and seen_ids.dim() == 2 and seen_ids.shape[0] == B
            stride = seen_ids.shape[1]
            if seen_lens is None:
                seen_lens = torch.full((B,), stride, dtype=torch.int32, device=logits.device)
            assert seen_lens.is_cuda and seen_lens.dtype == torch.int32 and seen_lens.numel() == B and int(seen_lens.max()) <= stride
        out = torch.empty(B, dtype=torch.int32, device=logits.device)
        kept = torch.empty(B, dtype=torch.int32, device=logits.device)
        lp = torch.empty(2, B, dtype=torch.float32, device=logits.device)
        rng = torch.empty(B, 2, dtype=torch.float32, device=logits.device) if want_range else None
        cfg = None if filters is None else FilterConfig.from_filters(SampleFilters.coerce(filters))
        check(self.lib.pgv_sample_logits_filtered(self.handle, logits.data_ptr(), logits.shape[1], B, float(temperature), int(top_k), float(top_p),
                                                  float(repetition_penalty), seen_ids.data_ptr() if seen_ids is not None else None, stride,
                                                  seen_lens.data_ptr() if seen_ids is not None else None, u.data_ptr() if u is not None else None,
                                                  out.data_ptr(), kept.data_ptr(), 1 if greedy else 0, lp[0].data_ptr(), lp[1].data_ptr(),
                                                  C.byref(cfg) if cfg is not None else None, rng.data_ptr() if rng is not None else None,
                                                  stream_ptr(logits.device)), "pgv_sample_logits_filtered")
        return out, kept, lp[0], lp[1], rng

    def beam_pick_logits(self, logits: torch.Tensor, state: torch.Tensor, beams: int, t: int, max_new_tokens: int, eos_id: int = -1,
                         length_penalty: float = 1.0, early_stopping: int = 0):
        """pgv_beam_pick_logits: step t of the beam-search rules (include/pgv.h) on logits [P * beams, V] fp32 and the state words
        int32 [P, beam_state_words(beams)], updated in place.  early_stopping: 0 False, 1 True, 2 "never".  Returns (tokens, parents), int32 [P * beams]."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
        K = int(beams)
        assert state.is_cuda and state.dtype == torch.int32 and state.is_contiguous() and state.dim() == 2 and state.shape[1] == beam_state_words(K)
        P = state.shape[0]
        assert logits.shape[0] == P * K
        cfg = BeamConfig(K, int(max_new_tokens), int(eos_id), float(length_penalty), int(early_stopping))
        tok = torch.empty(P * K, dtype=torch.int32, device=logits.device)
        par = torch.empty(P * K, dtype=torch.int32, device=logits.device)
        check(self.lib.pgv_beam_pick_logits(self.handle, logits.data_ptr(), logits.shape[1], P, C.byref(cfg), int(t), state.data_ptr(), tok.data_ptr(),
                                            par.data_ptr(), stream_ptr(logits.device)), "pgv_beam_pick_logits")
        return tok, par

    def logprob_rows(self, logits: torch.Tensor, targets: torch.Tensor, V: "int | None" = None):
        """pgv_logprob_rows on fp32 logits [R, ld] (unit column stride, ld % 4 == 0) over columns [0, V) (default: all): -> (logprob [R] fp32,
        logsumexp [R] fp32, argmax [R] int32).  targets int32 [R]; a negative target gives logprob 0."""
        assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
        assert targets.is_cuda and targets.dtype == torch.int32 and targets.is_contiguous() and targets.numel() == logits.shape[0]
        R, ld = logits.shape[0], max(logits.stride(0), logits.shape[1])       # a [:, :V] view of a wider buffer keeps the buffer's row stride
        V = logits.shape[1] if V is None else int(V)
        lp = torch.empty(R, dtype=torch.float32, device=logits.device)
        lse = torch.empty(R, dtype=torch.float32, device=logits.device)
        am = torch.empty(R, dtype=torch.int32, device=logits.device)
        check(self.lib.pgv_logprob_rows(self.handle, logits.data_ptr(), ld, V, R, targets.data_ptr(), lp.data_ptr(), lse.data_ptr(), am.data_ptr(),
                                        stream_ptr(logits.device)), "pgv_logprob_rows")
        return lp, lse, am

    def preprocess_u8(self, frames: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """uint8 [T, S, S, 3] on the device -> normalised [T, 3, S, S]."""
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.shape[-1] == 3
        T, S = frames.shape[0], frames.shape[1]
        assert frames.shape[2] == S
        out = torch.empty(T, 3, S, S, dtype=dtype, device=frames.device)
        check(self.lib.pgv_preprocess_u8(self.handle, frames.data_ptr(), T, S, dtype_code(dtype), out.data_ptr(),
                                         stream_ptr(frames.device)), "pgv_preprocess_u8")
        return out
