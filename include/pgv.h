/*
 * pgv.h -- C ABI of libpgv.so: the MI355X (gfx950) hot path of PG-Video-LLaVA.
 *
 * The reference (mbzuai-oryx/Video-LLaVA, package `video_chatgpt`) has no FFI layer: its
 * boundary is Python objects handed between `initialize_model` and `video_chatgpt_infer`
 * (SURVEY.md 8b).  This header is the C boundary placed *under* those Python contracts; each
 * entry point cites the reference call site (path:line under /root/reference) it replaces.
 * The Python mirror in video_llava_amd/ binds these symbols with ctypes.
 *
 * Conventions
 *  - plain C, no C++/torch types; every pointer named `d_*` is a DEVICE pointer owned by the
 *    caller (the library never frees caller memory); `h_*` is a HOST pointer.
 *  - every compute call is enqueued on the caller's `stream` (a hipStream_t passed as void*,
 *    e.g. torch.cuda.current_stream().cuda_stream) and returns without synchronising.
 *  - return value: 0 = ok, otherwise a PGV_E* code; pgv_last_error() gives the message for the
 *    calling thread.  No exceptions cross the ABI.
 *  - one pgv_ctx per GPU/rank; a ctx is not thread-safe (one host thread per rank).
 *  - activations/weights are 16-bit (PGV_F16 or PGV_BF16, chosen per model handle), all
 *    accumulation, normalisation statistics, softmax and the residual stream are fp32.
 */
#ifndef PGV_H
#define PGV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGV_VERSION 328

enum { PGV_OK = 0, PGV_EINVAL = 1, PGV_EHIP = 2, PGV_ENOMEM = 3, PGV_ESTATE = 4, PGV_ENAME = 5 };
enum { PGV_F16 = 0, PGV_BF16 = 1, PGV_F32 = 2 };

typedef struct pgv_ctx pgv_ctx;   /* device + workspace arena                         */
typedef struct pgv_vit pgv_vit;   /* packed CLIP vision tower weights                 */
typedef struct pgv_llm pgv_llm;   /* packed mm_projector + LLaMA decoder weights      */
typedef struct pgv_kv pgv_kv;     /* KV cache + decode state for a batch of sequences */

int pgv_version(void);
const char *pgv_last_error(void);

/* ---- context -------------------------------------------------------------------------------- */
int pgv_ctx_create(int device, pgv_ctx **out);
void pgv_ctx_destroy(pgv_ctx *ctx);
/* bytes currently held by the workspace arena (grows on demand, never inside a captured region) */
size_t pgv_ctx_workspace_bytes(const pgv_ctx *ctx);

/* Per-kernel-family device timers (hipEvent pairs around every launch of the family on the
 * caller's stream).  family: 0 = MFMA GEMM, 1 = ViT attention, 2 = LLM prefill attention,
 * 3 = decode GEMV, 4 = decode attention, 5 = pooling and the cache gather of a beam step, 6 = the short decode kernels (residual+RMSNorm, embedding,
 * argmax, the beam pick with its row statistics) and logprob_rows.
 * Off by default. */
#define PGV_NFAMILY 7
int pgv_prof_enable(pgv_ctx *ctx, int on);
int pgv_prof_reset(pgv_ctx *ctx);
/* synchronises the recorded events; fills launches / total ms / algorithmic flops / algorithmic bytes */
int pgv_prof_get(pgv_ctx *ctx, int family, int64_t *launches, double *ms, double *flops, double *bytes);
/* mean elapsed ms of an EMPTY event pair on `stream`: the fixed per-launch cost included in pgv_prof_get's totals */
int pgv_prof_calibrate(pgv_ctx *ctx, void *stream, int n, double *ms_per_pair);

/* ---- CLIP vision tower ------------------------------------------------------------------------
 * Replaces `vision_tower(image_tensor, output_hidden_states=True)` -- video_chatgpt/inference.py:93,
 * video_chatgpt/chat.py:140, scripts/save_spatio_temporal_clip_features.py:116 (HF CLIPVisionModel). */
typedef struct {
    int hidden;      /* 1024 */
    int inter;       /* 4096 */
    int layers;      /* 24   */
    int heads;       /* 16 (head_dim must be 64) */
    int image;       /* 224 or 336 */
    int patch;       /* 14 */
    float eps;       /* 1e-5 */
} pgv_vit_config;

int pgv_vit_create(pgv_ctx *ctx, const pgv_vit_config *cfg, int dtype, pgv_vit **out);
void pgv_vit_destroy(pgv_vit *vit);
/* Load one tensor by its HF state-dict name ("vision_model.encoder.layers.3.mlp.fc1.weight" ...;
 * the "vision_model." prefix is optional).  `data` is contiguous in `src_dtype`, on the device if
 * `on_device` else on the host.  The library converts/re-lays it out into its packed storage
 * (fused qkv, K-padded patch filter, fp32 biases and norm parameters).  `numel` is the element count of `data`: a tensor whose size
 * disagrees with the shape the config implies is rejected with PGV_EINVAL (torch's "size mismatch"), never read past its end.  Replaces
 * CLIPVisionModel.from_pretrained(...) at video_chatgpt/eval/model_utils.py:134-136. */
int pgv_vit_load_tensor(pgv_vit *vit, const char *name, const void *data, int src_dtype, int on_device, int64_t numel, void *stream);
/* number of tensors still missing (0 = ready) */
int pgv_vit_missing(const pgv_vit *vit);

/* Frame preprocessing fused for the GPU: uint8 RGB frames [T, image, image, 3] (already at the crop
 * size) -> (x/255 - mean)/std in NCHW 16-bit, i.e. CLIPImageProcessor.preprocess(...).half()
 * (video_chatgpt/inference.py:86-89) for crop-sized input. */
int pgv_preprocess_u8(pgv_ctx *ctx, const uint8_t *d_frames, int T, int image, int dtype, void *d_pixels, void *stream);
/* Frame ingest at native resolution: uint8 RGB frames [T, H, W, 3] as the video decoder delivers them -> nearest
 * resize to image x image exactly as load_video does it (video_chatgpt/eval/model_utils.py:38-43: permute, .float(),
 * F.interpolate(size) with the default mode 'nearest' -> source index min(floorf(dst * (float)in / out), in - 1) per axis, cast back
 * to uint8) -> CLIPImageProcessor normalisation -> NCHW 16-bit, in one pass.  H == W == image reduces to pgv_preprocess_u8. */
int pgv_ingest_u8(pgv_ctx *ctx, const uint8_t *d_frames, int T, int H, int W, int image, int dtype, void *d_pixels, void *stream);

/* hidden_states[k] of the tower for k = n_layers (k=0: pre-LayerNorm'ed embeddings):
 * d_pixels [T,3,image,image] 16-bit NCHW -> d_hidden [T, patches+1, hidden] 16-bit.
 * The reference selects hidden_states[-2] => n_layers = layers-1 (inference.py:94); only the
 * layers that feed the selected state are executed. */
int pgv_vit_forward(pgv_ctx *ctx, pgv_vit *vit, const void *d_pixels, int T, int n_layers, void *d_hidden, void *stream);

/* ---- spatio-temporal pooling -------------------------------------------------------------------
 * Replaces get_spatio_temporal_features_torch (video_chatgpt/inference.py:13-44; chat.py:77-87) and
 * the numpy twin get_spatio_temporal_features (scripts/save_spatio_temporal_clip_features.py:46-57).
 * d_feats: T frames of P patch rows x C channels, 16-bit, row stride C, frame stride
 * `frame_stride` elements (so the `[:, 1:]` view of a [T,P+1,C] tensor is consumed without a copy).
 * d_out [n_temporal + P, C]: rows [0,T) = per-frame mean over patches, rows [T,n_temporal) = 0,
 * rows [n_temporal, n_temporal+P) = per-patch mean over frames.  fp32 accumulation, one rounding.
 * T > n_temporal is rejected (the reference never truncates; its callers cap T at 100). */
int pgv_st_pool(pgv_ctx *ctx, const void *d_feats, int in_dtype, int T, int P, int C, int64_t frame_stride,
                int n_temporal, void *d_out, int out_dtype, void *stream);

/* ---- mm_projector ------------------------------------------------------------------------------
 * Replaces `self.mm_projector(video_spatio_temporal_features)` (video_chatgpt/model/video_chatgpt.py:105):
 * a bare nn.Linear(mm_hidden, hidden) for 224-px towers (:52-53) or build_vision_projector's
 * Linear + (depth-1) x [GELU(erf), Linear] (multimodal_projector/builder.py:33-50).  The parameters stay
 * owned by the caller's nn.Module (so `mm_projector.bin` loads by name, eval/model_utils.py:122-127):
 * d_weights[i] is layer i's [out, in] 16-bit row-major weight, d_biases[i] its fp32 bias.
 * d_x [rows, mm_hidden] -> d_y [rows, hidden]; depth 0 (identity) is rejected (nothing to run). */
int pgv_projector(pgv_ctx *ctx, int dtype, int depth, const void *const *d_weights, const float *const *d_biases,
                  int mm_hidden, int hidden, const void *d_x, int rows, void *d_y, void *stream);

/* ---- LLaMA decoder --------------------------------------------------------------------------------
 * Replaces VideoChatGPTLlamaForCausalLM (video_chatgpt/model/video_chatgpt.py:178-325) as driven by
 * model.generate at video_chatgpt/inference.py:105-112 / chat.py:148-154. */
typedef struct {
    int vocab;            /* 32003 */
    int hidden;           /* 4096 / 5120 */
    int inter;            /* 11008 / 13824 */
    int layers;           /* 32 / 40 */
    int heads;            /* 32 / 40 (MHA; head_dim must be 128) */
    float eps;            /* rms_norm_eps */
    float rope_theta;     /* 10000 */
} pgv_llm_config;

int pgv_llm_create(pgv_ctx *ctx, const pgv_llm_config *cfg, int dtype, pgv_llm **out);
void pgv_llm_destroy(pgv_llm *llm);
/* HF names: "model.embed_tokens.weight", "model.layers.N.self_attn.q_proj.weight", ...,
 * "model.norm.weight", "lm_head.weight".  `model.embed_tokens.weight` may be re-loaded later (the
 * projector checkpoint carries the rows of the added video tokens, train/llava_trainer.py:34). */
int pgv_llm_load_tensor(pgv_llm *llm, const char *name, const void *data, int src_dtype, int on_device, int64_t numel, void *stream);
int pgv_llm_missing(const pgv_llm *llm);
/* Load `nrows` rows starting at `row0` of "model.embed_tokens.weight" or "lm_head.weight" (checkpoints whose
 * vocabulary is smaller than the resized model, eval/model_utils.py:119-127). */
int pgv_llm_load_rows(pgv_llm *llm, const char *name, const void *data, int src_dtype, int on_device, int row0, int nrows, int64_t numel, void *stream);
/* model.resize_token_embeddings(n) (eval/model_utils.py:119): the handle is allocated with 64 spare vocabulary
 * rows; growing within them zero-fills the new embed / lm_head rows (the projector checkpoint then overwrites them). */
int pgv_llm_resize_vocab(pgv_llm *llm, int new_vocab, void *stream);
int pgv_llm_vocab(const pgv_llm *llm);
/* fp8 weight path (BASELINE config 5, "13B, fp8 weight path"): after every tensor is loaded, quantise all decoder matrices and
 * lm_head to OCP e4m3 with one power-of-two scale per output row.  The decode GEMVs then stream the fp8 copies (half the
 * bytes per token); the 16-bit copies are overwritten with the dequantised values (exactly representable), so prefill, decode
 * and a CPU oracle fed with pgv_llm_get_weight() all compute with the same weights.  Replaces nothing in the reference (it
 * has no quantised path); idempotent. */
int pgv_llm_quantize_fp8(pgv_ctx *ctx, pgv_llm *llm, void *stream);
int pgv_llm_is_fp8(const pgv_llm *llm);
/* bf16 models: once every tensor is loaded, the decode GEMVs stream a lossless 12-bit copy of every decoder matrix and lm_head at batches of
 * up to 16 sequences (pgv_encode_w12_blocked; a matrix whose exceptions do not fit keeps its 16-bit stream).  Every weight load or
 * vocabulary resize rebuilds the copy; pgv_llm_quantize_fp8 drops it.  Tokens and logits are bitwise those of the 16-bit stream.
 * pgv_llm_set_weight_stream(llm, 0) streams the 16-bit matrices, 1 (the default) the 12-bit copies where they exist.
 * pgv_llm_weight_stream_bytes: the weight bytes one decode token step streams at `batch` sequences (matrices + lm_head + side data). */
int pgv_llm_set_weight_stream(pgv_llm *llm, int use12);
int64_t pgv_llm_weight_stream_bytes(const pgv_llm *llm, int batch);
/* Read a decoder matrix ("model.layers.N.{self_attn.{q,k,v,o}_proj,mlp.{gate,up,down}_proj}.weight", "lm_head.weight") back as
 * row-major fp32 [rows, cols] in its HF orientation: the values the path computes with (after quantisation: dequantised). */
int pgv_llm_get_weight(pgv_ctx *ctx, pgv_llm *llm, const char *name, float *d_out, void *stream);

int pgv_kv_create(pgv_ctx *ctx, pgv_llm *llm, int batch, int max_seq, pgv_kv **out);
void pgv_kv_destroy(pgv_kv *kv);

/* Prefill (the `input_ids.shape[1] != 1` branch, video_chatgpt/model/video_chatgpt.py:100-175 and
 * :225-226): embed + splice projected video rows + decoder stack + lm_head on the LAST position of
 * each sequence.  Sequences are ragged: h_seq_lens[b] tokens each, concatenated in h_ids (host: the
 * tokenizer output never lives on the device, and the row map of the splice is built from it).
 * d_video [B, V, hidden] = mm_projector output, 16-bit (or NULL); h_vid_pos[b] = index of <vid_start>
 * in sequence b, or -1 for a text-only sample (rows (pos, pos+V] are replaced -- the caller has already
 * validated the placeholder run on the host, raising the reference's ValueErrors).
 * Outputs (any may be NULL): d_logits [B, vocab] fp32, d_next [B] int32 greedy argmax, and -- what
 * VideoChatGPTLlamaForCausalLM.forward returns (:225-226, `logits = self.lm_head(hidden_states)` over ALL positions) --
 * d_all_logits [sum of h_seq_lens, ld_all] fp32 with ld_all >= vocab rounded up to a multiple of 16 (row r = token r of the
 * concatenated batch; columns >= vocab hold the zero spare rows of lm_head). */
int pgv_llm_prefill(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *h_ids, const int32_t *h_seq_lens, int B,
                    const void *d_video, int V, const int32_t *h_vid_pos, float *d_logits, int32_t *d_next, float *d_all_logits,
                    int ld_all, void *stream);

/* Prefill of NEW tokens behind the ones already in the cache: VideoChatGPTLlamaForCausalLM.forward called with `past_key_values` and
 * input_ids.shape[1] > 1 (video_chatgpt/model/video_chatgpt.py:193-251 accepts any input_ids next to a cache; :103 still splices when the new
 * ids carry a placeholder run) -- what a second chat turn is (video_chatgpt/chat.py:108-160 re-tokenises and re-runs the WHOLE conversation
 * every turn although the prefix is unchanged).  Same arguments as pgv_llm_prefill; B must equal the batch of the prefill that filled `kv`;
 * row p of sequence b takes position pgv_kv_len(kv, b) + p, attends to the cached prefix and the new rows before it, and is appended.
 * h_vid_pos is relative to the NEW rows.  Outputs as pgv_llm_prefill (d_all_logits: the new rows only).  Given the same cache contents an
 * appended row is bitwise the row of one full prefill over prefix + new tokens (a prefix that pgv_llm_prefill wrote reproduces the one-call
 * result exactly; entries written by decode steps carry that path's rounding). */
int pgv_llm_prefill_append(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *h_ids, const int32_t *h_seq_lens, int B,
                           const void *d_video, int V, const int32_t *h_vid_pos, float *d_logits, int32_t *d_next, float *d_all_logits,
                           int ld_all, void *stream);
/* Continuous batching: prefill n NEW prompts into slots h_slots[0..n) of a cache that holds a live group (the last pgv_llm_prefill of `kv`),
 * while the other slots keep their state.  1 <= n, every slot < the width of that prefill, slots distinct.  h_ids / h_seq_lens / d_video [n, V, hidden]
 * / h_vid_pos as pgv_llm_prefill, in slot-list order.  d_u == NULL: greedy first token; otherwise it is drawn exactly as pgv_llm_sample does, with
 * d_u[i], `temperature` (> 0) and `top_k`.  d_logits [n, vocab] / d_next [n] (either may be NULL) receive the refilled sequences' logits / first tokens.
 * A listed slot s: cache rows [0, len) hold the new prompt, pgv_kv_len(kv, s) == len, its current token is the pick, its done flag and step
 * counter are cleared.  An unlisted slot: cache rows, length, current token and done flag are untouched; the group's width does not change and
 * captured decode graphs stay valid (they read positions and tokens from device memory).  A refilled sequence's later tokens and logits are
 * bitwise those of the same prompt run alone through pgv_llm_prefill + decode.  Refused (cache unchanged): no live group or a slot outside it
 * (PGV_ESTATE / PGV_EINVAL), a duplicate slot, a prompt longer than the cache, a bad video run or token id (PGV_EINVAL).
 * A slot with no task left is not released: rewind it with pgv_kv_truncate(kv, s, 1) before every decode chunk so that it neither outgrows
 * max_seq nor keeps reading a long cache; its tokens are then meaningless and ignored by the caller. */
int pgv_llm_prefill_slots(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *h_slots, int n, const int32_t *h_ids, const int32_t *h_seq_lens,
                          const void *d_video, int V, const int32_t *h_vid_pos, float temperature, int top_k, const float *d_u, float *d_logits,
                          int32_t *d_next, void *stream);
/* pgv_llm_prefill_slots with h_counts[i] >= 1 sampled answers of prompt i (best-of-N / self-consistency voting inside a live group): h_slots lists
 * S = sum of h_counts distinct slots of the live group, prompt 0's first, then prompt 1's, ..., in any order inside the group.  h_ids / h_seq_lens /
 * d_video [n, V, hidden] / h_vid_pos describe the n PROMPTS; d_u (NULL: greedy first tokens, also under a repetition penalty), d_next and d_logits
 * have S entries / rows, in slot-list order.
 *  - Result: bit for bit what pgv_llm_prefill_slots leaves when prompt i is repeated h_counts[i] times in that slot order with the same d_u -- cache
 *    rows [0, len) of every layer, K and V, of every listed slot, pgv_kv_len, device position, current token, done flag, step counter, seen-set
 *    bitmap, both pgv_kv_logprobs_last values, d_next and d_logits.  Unlisted slots and rows [len, max_seq) of the listed ones are untouched;
 *    the width and the captured decode graphs stay valid.
 *  - Cost: the decoder trunk runs over the n prompts' rows once.  The cache rows of the first slot of a run are copied to the run's other slots
 *    (one launch per prompt with more than one sample); last-row gather, final norm, lm_head, pick and the seen-set (built per slot from the
 *    prompt's ids alone -- a pick adds its token to its own slot's set only) run per sample.
 *  - Refused, cache and state unchanged, the message names the offending value: no live group (PGV_ESTATE); a count < 1, S beyond the live width,
 *    a duplicate slot, a slot outside the group, and whatever pgv_llm_prefill_slots refuses (PGV_EINVAL). */
int pgv_llm_prefill_slots_n(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *h_slots, const int32_t *h_counts, int n, const int32_t *h_ids,
                            const int32_t *h_seq_lens, const void *d_video, int V, const int32_t *h_vid_pos, float temperature, int top_k,
                            const float *d_u, float *d_logits, int32_t *d_next, void *stream);
/* Teacher-forced scoring: the log-probability of GIVEN tokens -- the per-token terms of the loss the reference's forward(labels=...) computes
 * (video_chatgpt/model/video_chatgpt.py:228-239: shift logits and labels by one, flatten, CrossEntropyLoss) -- without materialising the
 * logits of every position.
 * pgv_logprob_rows (building block, caller buffers): d_logits [R, ld] fp32 (16-byte aligned, ld % 4 == 0, ld >= V), d_targets [R].  Per row
 * (each output pointer may be NULL): d_logprob[r] = x[t] - logsumexp(x[0:V]), d_lse[r] = logsumexp(x[0:V]), d_argmax[r] = the first index
 * of the largest entry (the greedy pick's tie rule).  The reduction covers exactly columns [0, V) -- never the spare columns [V, ld) that the
 * lm_head GEMM fills with logit 0.  d_targets[r] < 0: d_logprob[r] = 0, the other two are still written; a target at or beyond V (it cannot be
 * checked on the host) gives NaN.  -inf entries contribute 0, a target on -inf gives -inf.  Every reduction has a fixed order: a row's result
 * does not depend on R, on the row's index or on the launch.
 * pgv_llm_score = pgv_llm_prefill + score: h_targets[r] (r = row of the concatenated batch) is the id whose probability row r's logits are
 * asked for (the caller has done the shift of :234-235: usually the id of row r + 1), or < 0 = row not scored.  d_logprob / d_lse / d_argmax
 * (each may be NULL): [sum of h_seq_lens], unscored rows 0 / 0 / -1.  The scored rows take the final norm and lm_head in chunks of at most
 * PGV_SCORE_CHUNK_ROWS rows through a workspace buffer; their logits are bit for bit those of d_all_logits.  The cache is left a live group
 * exactly as pgv_llm_prefill leaves it.  A target >= the vocabulary is refused with PGV_EINVAL like a bad token id, the cache unchanged. */
#define PGV_SCORE_CHUNK_ROWS 1024
int pgv_logprob_rows(pgv_ctx *ctx, const float *d_logits, int ld, int V, int R, const int32_t *d_targets, float *d_logprob, float *d_lse,
                     int32_t *d_argmax, void *stream);
int pgv_llm_score(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *h_ids, const int32_t *h_seq_lens, int B, const void *d_video, int V,
                  const int32_t *h_vid_pos, const int32_t *h_targets, float *d_logprob, float *d_lse, int32_t *d_argmax, void *stream);

/* Forget the cache entries of sequence b from position `len` on (1 <= len <= pgv_kv_len): the next append / decode call continues there.
 * Used when a new chat turn shares only a prefix with what the cache holds (surplus decode steps past a stop string,
 * video_chatgpt/model/utils.py:6-26). */
int pgv_kv_truncate(pgv_kv *kv, int b, int len, void *stream);

/* Fork the live group: slot p of the P = active sequences becomes h_counts[p] >= 1 consecutive slots, in order (HF's
 * _expand_inputs_for_generation: input_ids.repeat_interleave(n) -- what num_return_sequences does to a batch): new slot i is a copy of old
 * slot src(i), src = [0]*c0 + [1]*c1 + ...  New width W = sum of counts <= the batch the cache was created with.  One prefill, then N sampled
 * answers per prompt; the same primitive is the cache side of a beam search.
 *  - Result: as if every read preceded every write (the copy runs in place: a slot may be a source and another source's destination).  New
 *    slot i holds old slot src(i)'s cache rows [0, len) in every layer, K and V, its pgv_kv_len, device position, current token, done flag,
 *    seen-set bitmap (repetition penalty), row of the logits of the last prefill / decode call (pgv_llm_sample draws the first token from it) and
 *    both pgv_kv_logprobs_last values.  The per-call step counter is cleared, as every stepping call does.  The group's width becomes W.
 *    Rows [len, max_seq) of a destination are neither read nor written.  Everything else a slot has (residual, norms, greedy candidates) is
 *    rebuilt by the next decode step from the current token and position: a forked slot's later tokens and logits are bitwise those of the
 *    same prompt prefilled W times.
 *  - Valid on any live group between calls: right after pgv_llm_prefill / _append / _slots / pgv_llm_score, and after decode steps.
 *  - Enqueued on the caller's stream, no host synchronisation (lengths are host bookkeeping).  One launch per source whose slot moves or
 *    multiplies; with all counts 1 nothing is launched.  Not attributed to a pgv_prof family.
 *  - No decode kernel or graph changes: the captured decode graphs are keyed on the group's width and rebuild themselves at the next step.
 *  - Refused, cache and state unchanged: no live group (PGV_ESTATE); P != the group's width, a count < 1, W > the cache's batch (PGV_EINVAL);
 *    the message names the offending value.
 *  - The sampling state of pgv_kv_set_warpers / pgv_kv_set_logprobs belongs to the cache, not to a slot, and is untouched.
 * Not provided: sharing the prompt's K / V between the copies inside decode attention.  (The non-monotone slot gather a beam search needs on top of
 * the fork is pgv_kv_gather, below; pgv_llm_prefill_slots_n copies a fresh prompt to listed slots, not live state.) */
int pgv_kv_fork(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *h_counts, int P, void *stream);
/* In-place slot gather inside groups of K consecutive slots of the live group (the cache reorder of a beam step): with W = the group's width (a
 * multiple of K) and P = W / K groups, slot g * K + i receives the cache rows [h_row0[g], len) of slot g * K + h_src[g * K + i] in every layer, K and V,
 * and its current token.  Rows [0, h_row0[g]) are NOT moved: the caller states that the K slots of group g agree on them -- they do, bit for bit,
 * when h_row0[g] is the length the group had when pgv_kv_fork made it, which is why a beam step moves only the rows generated since the fork.
 *  - Result: as if every read preceded every write (any map: broadcasts, swaps, cycles).  A destination whose source is itself is not written; a
 *    group whose map is the identity costs the read of its map.  Rows [len, max_seq) are neither read nor written.  Lengths, done flags, seen-sets,
 *    logits rows and log-probabilities stay with their slots (a beam run uses none of them); the lengths inside a group must be equal.
 *  - One launch whose grid does not depend on the lengths; enqueued on the caller's stream after one synchronising upload of the two lists.
 *  - Refused, cache unchanged: no live group (PGV_ESTATE); K outside [1, 8], W no multiple of K, an entry of h_src outside [0, K), unequal lengths
 *    inside a group, h_row0[g] outside [1, len] (PGV_EINVAL). */
int pgv_kv_gather(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, int K, const int32_t *h_src, const int32_t *h_row0, void *stream);
/* Test / debug read-back: rows [row0, row0 + nrows) of every head of `slot` (< the cache's batch, live or not) of layer `layer`,
 * which = 0 K / 1 V  ->  d_out [heads][nrows][128] 16-bit.  row0 + nrows <= max_seq. */
int pgv_kv_peek(pgv_kv *kv, int layer, int which, int slot, int row0, int nrows, void *d_out, void *stream);

/* One decode step for all B sequences (the `input_ids.shape[1] == 1` branch, :103): consumes
 * d_last [B] token ids, appends to the KV cache, writes d_logits [B, vocab] and/or d_next [B]. */
int pgv_llm_decode(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *d_last, float *d_logits, int32_t *d_next, void *stream);
/* Prompt-lookup speculative decoding (token-exact; greedy and sampled) and its building block, the row-wise decode step: several consecutive positions of a
 * sequence in ONE pass over the weights.  A row is bit for bit the plain step at its position (the decode GEMVs are batch-invariant, the row form
 * of the attention keeps the plain kernels' key order), so a lookup run emits exactly the tokens pgv_llm_decode_greedy emits.
 * pgv_kv_set_lookup(kv, D, n): D drafts per sequence and step, 0 <= D <= 15 (0: off, the default; n is ignored then), ngram size 1 <= n <= 4
 *   (the stepping calls need sequences x (1 + D) <= 64).  The first call with D > 0 allocates the cache's row scratch (a second set of the per-row decode buffers, for
 *   min(64, 16 x batch) rows) and, unless pgv_kv_set_bans has, the id record.  Set it BEFORE pgv_llm_prefill: while it is on, the prefill writes
 *   each slot's ids to the record, as under bans.  A call that is refused changes nothing.
 * pgv_llm_decode_rows: h_slots [R] lists the sequence of every row, the rows of one sequence consecutively (at most 1 + D of them).  Row j of a
 *   sequence's run consumes d_tokens[r] at position pgv_kv_len + j: its K / V go to that cache row and d_logits [R, vocab] receives its logits --
 *   those of the j-th of consecutive pgv_llm_decode calls fed the same tokens.  Lengths, current tokens and step counters do NOT advance: the
 *   caller keeps a prefix of the rows by stepping on.  Runs eagerly.  PGV_ESTATE without lookup set or prefilled sequences; PGV_EINVAL for a slot
 *   outside the live group, a sequence listed twice, too many rows, or a row past max_seq; nothing is launched then.
 * pgv_llm_decode_lookup: `steps` lookup steps from d_first [B] (as pgv_llm_decode_greedy takes it).  A step drafts up to D tokens per sequence by
 *   HF's prompt-lookup rule (PromptLookupCandidateGenerator.get_candidates with num_output_tokens = D, max_matching_ngram_size = n, on the slot's ids
 *   as given plus everything emitted; cut before eos_id), runs current token + drafts as rows, and emits the model's token behind the current one
 *   plus one per leading draft the model agrees with: between 1 and 1 + D tokens.  eos_id (< 0: none) ends a sequence behind the token that emits
 *   it; h_budget [B] bounds what each sequence may emit in this call (pgv_kv_len + h_budget <= max_seq).  A finished sequence emits nothing more.
 *   d_tokens [B, steps x (1 + D)]: each sequence's emitted tokens, packed from column 0; d_counts [steps, B]: tokens emitted per step.  On return
 *   pgv_kv_len is true again (one blocking copy) and the cache's current tokens are the last emitted ones (d_first NULL continues from them); cache rows at or beyond pgv_kv_len are
 *   stale: never read, overwritten later.  Eager the first time, then captured graphs of 1 and 8 steps keyed by (D, n).  Refused with PGV_ESTATE and
 *   nothing launched: lookup off, a cache whose record does not cover its sequences (prefilled before pgv_kv_set_lookup, or stepped / forked /
 *   refilled since), a repetition penalty, bans, log-probabilities on, a beam run in flight.
 * pgv_llm_decode_lookup_sample: the same steps for a sampled run, bit for bit the tokens pgv_llm_decode_sample emits from the same uniforms.  d_u is
 *   fp32 [u_rows][B], B the active width, row i holding the uniforms of the run's i-th new token (copied into the cache's, so u_rows <= max_seq);
 *   h_u_base [B]: tokens sequence b has emitted before this call in the current generation.  The uniform indexing rule: the row for (sequence b,
 *   offset j) of a step is picked with u[h_u_base[b] + e + j][b], e = tokens b has emitted so far in this call -- the uniform the plain run picks
 *   that token with.  The pick is pgv_llm_decode_sample's (temperature, top_k, the cache's top_p and pgv_kv_set_filters values) on the row's logits,
 *   and a draft is accepted exactly when it equals the pick behind the row in front of it.  Everything else is pgv_llm_decode_lookup's, the
 *   refusals included; also PGV_EINVAL for temperature <= 0, a null d_u / h_u_base, h_u_base[b] < 0 or h_u_base[b] + h_budget[b] > u_rows.
 *   Captured graphs are keyed by the pick parameters besides (D, n). */
int pgv_kv_set_lookup(pgv_kv *kv, int D, int n);
int pgv_kv_lookup(const pgv_kv *kv);        /* the D in force (0: off) */
int pgv_llm_decode_rows(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *h_slots, const int32_t *d_tokens, int R, float *d_logits, void *stream);
int pgv_llm_decode_lookup(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *d_first, int steps, int eos_id, const int32_t *h_budget,
                          int32_t *d_tokens, int32_t *d_counts, void *stream);
int pgv_llm_decode_lookup_sample(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *d_first, int steps, int eos_id, const int32_t *h_budget,
                                 const int32_t *h_u_base, float temperature, int top_k, const float *d_u, int u_rows, int32_t *d_tokens,
                                 int32_t *d_counts, void *stream);

/* n greedy steps without host round trips: step i consumes the previous argmax (step 0 consumes
 * d_first [B]); token of step i of sequence b is written to d_tokens[b * n + i].  A sequence that
 * emits eos_id (>= 0) keeps emitting eos_id.  Replaces the per-token loop of GenerationMixin for
 * do_sample=False. */
int pgv_llm_decode_greedy(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *d_first, int n, int eos_id,
                          int32_t *d_tokens, void *stream);

/* Sampling (the reference's DEFAULT decode mode: model.generate(do_sample=True, temperature=0.2), video_chatgpt/inference.py:106-112;
 * HF's sample loop = TemperatureLogitsWarper, TopKLogitsWarper(top_k=50 from the default GenerationConfig), softmax, multinomial).
 * The multinomial draw is an inverse-CDF pick with a caller-supplied uniform u in [0,1): token = the first vocabulary index whose
 * cumulative probability exceeds u; probabilities = softmax(logits / temperature) over the top_k largest logits (top_k <= 0: all of
 * them; ties at the k-th value are kept, as HF's `scores < kth` mask does).  The token stays on the device.
 * pgv_llm_sample: pick from the logits of the last prefill / decode call of `kv` with d_u [B]; the result replaces the greedy pick
 * as the cache's current token and is written to d_next [B] (may be NULL). */
int pgv_llm_sample(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, float temperature, int top_k, const float *d_u, int32_t *d_next, void *stream);
/* n sampled steps without host round trips (twin of pgv_llm_decode_greedy): step i draws with d_u[i * B + b]. */
int pgv_llm_decode_sample(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const int32_t *d_first, int n, int eos_id, float temperature, int top_k,
                          const float *d_u, int32_t *d_tokens, void *stream);
/* building block: the same pick on caller logits [B, V] fp32 (row stride V) */
int pgv_sample_logits(pgv_ctx *ctx, const float *d_logits, int V, int B, float temperature, int top_k, const float *d_u, int32_t *d_next,
                      void *stream);

/* The two further HF processors of a sampled run (HF generation/logits_process.py; HF's order, as GenerationMixin._get_logits_processor /
 * _get_logits_warper build it: repetition penalty on the raw logits, then temperature, top-k, top-p, softmax, multinomial):
 *  - RepetitionPenaltyLogitsProcessor(penalty) (`score = torch.where(score < 0, score * penalty, score / penalty)` gathered / scattered at
 *    input_ids): for every token id in the sequence's seen-set, x = x < 0 ? x * penalty : x / penalty.
 *  - TopPLogitsWarper(top_p, min_tokens_to_keep = 1) (`sorted_indices_to_remove = cumulative_probs <= (1 - top_p)` over the ASCENDING sort of
 *    the softmax of what top-k left): a token stays iff the probability mass of the tokens ranked above it is < top_p; the largest always stays.
 *    TIE RULE (HF's torch.sort leaves the order of equal logits unspecified): equal logits share one rank -- a value stays iff the mass of the
 *    values STRICTLY greater is < top_p -- so equal logits are kept or removed together, exactly as the top-k mask `scores < kth` treats them.
 * The sums that decide the nucleus are integer (64-bit fixed point, 2^-40 of the largest weight per entry) and every other reduction has a
 * fixed order: same logits, same seen-set, same u -> same token on any launch, batch slot and group width.  top_p == 1 and
 * repetition_penalty == 1 run the pick without the two processors: bit for bit the tokens of the calls above.
 * Refused with PGV_EINVAL, in HF's words: top_p outside (0, 1] ("`top_p` has to be a float > 0 and <= 1"), repetition_penalty <= 0
 * ("`penalty` has to be a strictly positive float").
 *
 * pgv_sample_logits_ex: pgv_sample_logits with both processors on caller buffers.  Seen-set of row b: the d_seen_lens[b] ids at
 * d_seen_ids + b * seen_stride (both NULL: empty; ids outside [0, V) are ignored).  d_kept [B] (may be NULL) receives the number of
 * vocabulary entries left with non-zero probability. */
int pgv_sample_logits_ex(pgv_ctx *ctx, const float *d_logits, int V, int B, float temperature, int top_k, float top_p, float repetition_penalty,
                         const int32_t *d_seen_ids, int seen_stride, const int32_t *d_seen_lens, const float *d_u, int32_t *d_next, int32_t *d_kept,
                         void *stream);
/* Sampling state of a cache, default (1, 1): every later pick on it -- pgv_llm_sample, pgv_llm_decode_sample, the first-token draw of
 * pgv_llm_prefill_slots, and with repetition_penalty != 1 also pgv_llm_decode_greedy and the greedy first token of pgv_llm_prefill_slots (the
 * largest PENALISED logit, first index on ties; top_p plays no part in a greedy pick, as in HF) -- runs with these values.  The captured
 * decode graph is rebuilt when they change.  A slot's seen-set (HF's `input_ids`): the ids of its prompt as handed to pgv_llm_prefill /
 * _slots (placeholder ids included; a refill starts from an empty set, pgv_llm_prefill_append adds to it) plus every token one of those picks
 * returned while a value differed from (1, 1).  Set the values before the prefill of the sequences they are meant for.  Not covered: the
 * greedy d_next of pgv_llm_prefill / _append and plain pgv_llm_decode steps, which neither apply the penalty nor record a token -- a caller
 * who wants the penalised first token draws it with pgv_llm_pick_greedy (the token of pgv_llm_sample(temperature 1, top_k 1, u = 0)). */
int pgv_kv_set_warpers(pgv_kv *kv, float top_p, float repetition_penalty);

/* Log-probabilities of the tokens the picks RETURN (the mirror image of pgv_llm_score, which scores GIVEN tokens): two floats per pick, recorded
 * on the device next to the token, inside the captured decode graphs -- no logits leave the device.  For the token t a pick returns for a
 * sequence at one step, x the fp32 logits of that step over columns [0, vocab):
 *  - `model` = x[t] - logsumexp(x): the model's own distribution, no processor.  HF: compute_transition_scores(sequences, logits,
 *    normalize_logits=True) on output_logits=True.  Same reduction order as pgv_logprob_rows: for the same row and token it is the same float, and
 *    its NaN / -inf rules hold (a NaN in the row poisons the sum; a token on -inf gives -inf).
 *  - `pick` = the log of the probability the pick used.  HF: compute_transition_scores(sequences, scores, normalize_logits=True), `scores` the
 *    processed scores of output_scores=True.  Sampling: log-softmax over the scores after repetition penalty -> temperature -> top-k -> top-p
 *    (HF's order, the tie rules above), computed as (x'[t] - M) / T - ln sum_kept exp((x' - M) / T) from the logit itself; a NaN logit has
 *    weight 0, as in the pick.  Greedy without a penalty: `model`, the same float bit for bit -- hence NaN, like `model`, on a row that holds a NaN
 *    (the penalty-free greedy value IS the model's; the weight-0 rule applies wherever a processor is at work).  Greedy under a penalty (pgv_kv_set_warpers with
 *    repetition_penalty != 1): the log-softmax of the PENALISED logits over the whole vocabulary at temperature 1, as HF's greedy loop has it
 *    -- not the degenerate top-1 value 0.  The seen-set is the one the pick itself read (the returned token joins it afterwards).
 *  - finished sequences: the step that emits eos_id carries its real values, the sticky steps after it 0.0 for both -- a row sum over the
 *    history is the answer's log-probability.
 * pgv_kv_set_logprobs(kv, on), default off: off, every launch, captured graph and token is exactly what it is without this switch; on, every
 * pick that sets the cache's current token also stores the two values of its slot -- the greedy d_next of pgv_llm_prefill / _append, the first
 * token of pgv_llm_prefill_slots (at the SLOT, not at the scratch row the pick ran in), pgv_llm_sample, pgv_llm_pick_greedy, pgv_llm_decode, and
 * every step of pgv_llm_decode_greedy / _sample, which also append them to a per-slot history parallel to the token history (same index, same
 * per-call reset).  The tokens do not change.  The captured decode graphs are rebuilt when the switch changes.
 * pgv_kv_logprobs_last: d_model / d_pick [width of the live group] (either may be NULL), by slot: the values of each slot's most recent pick.
 * pgv_kv_logprobs_steps: d_model / d_pick [B, n] (either may be NULL), laid out like d_tokens: the first n steps of the last
 * pgv_llm_decode_greedy / _sample call.  PGV_ESTATE when the switch was off during that call (both calls: when it is off now).
 * pgv_llm_pick_greedy: the greedy pick from the logits of the last prefill / decode call under the cache's repetition penalty -- the token of
 * pgv_llm_sample(temperature 1, top_k 1, u = 0), recorded with the GREEDY `pick` value (pgv_llm_sample with top_k = 1 records a sampled pick: 0).
 * It replaces the cache's current token and is written to d_next [B] (may be NULL).
 * pgv_sample_logits_lp (building block, same kernels): pgv_sample_logits_ex plus d_lp_model / d_lp_pick [B] (either may be NULL).  greedy != 0:
 * the arg-max of the penalised logits; temperature, top_k, top_p and d_u (may be NULL) are ignored.  Tokens and d_kept are bit for bit those of
 * pgv_sample_logits_ex (greedy: of temperature 1, top_k 1, top_p 1, u = 0). */
int pgv_kv_set_logprobs(pgv_kv *kv, int on);
int pgv_kv_logprobs_last(pgv_kv *kv, float *d_model, float *d_pick, void *stream);
int pgv_kv_logprobs_steps(pgv_kv *kv, int n, float *d_model, float *d_pick, void *stream);
int pgv_llm_pick_greedy(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, int32_t *d_next, void *stream);
int pgv_sample_logits_lp(pgv_ctx *ctx, const float *d_logits, int V, int B, float temperature, int top_k, float top_p, float repetition_penalty,
                         const int32_t *d_seen_ids, int seen_stride, const int32_t *d_seen_lens, const float *d_u, int32_t *d_next, int32_t *d_kept,
                         int greedy, float *d_lp_model, float *d_lp_pick, void *stream);

/* The filter tail of a sampled pick: HF's four remaining sampling warpers (generation/logits_process.py: MinPLogitsWarper, TypicalLogitsWarper,
 * EpsilonLogitsWarper, EtaLogitsWarper), in HF's order behind top-p:
 *   repetition penalty -> temperature -> top-k -> top-p -> min_p -> typical_p -> epsilon_cutoff -> eta_cutoff -> softmax -> multinomial.
 * y = the scores after penalty / temperature / top-k / top-p, -inf where removed.  Each stage works on the CURRENT survivors: p = their softmax,
 * H = -sum p ln p their entropy, "top" = the largest current survivor.  Every stage keeps the top (HF's min_tokens_to_keep = 1).
 *   min_p           on when > 0       keeps i iff p_i >= min_p * p_max
 *   typical_p       on when < 1       d_i = |(-ln p_i) - H|; sorted ascending by d, last = min(#(cumulative p < typical_p), n - 1),
 *                                     d* = d_sorted[last]; keeps i iff d_i <= d*.  TIE RULE: entries of equal d are kept or removed together (HF
 *                                     removes `sorted_scores > threshold`), the entry that crosses the mass is kept, the smallest d always stays.
 *                                     The survivors are a BAND in the logit, not a threshold: the row's largest logit is routinely removed, and
 *                                     "the top" of the two stages behind it is the largest logit that is still there.
 *   epsilon_cutoff  on when > 0       keeps i iff p_i >= epsilon, or i is the top
 *   eta_cutoff      on when > 0       keeps i iff p_i >= min(eta, sqrt(eta) * exp(-H)), or i is the top
 * On the device the mass of the typical stage is summed in 2^40 fixed point (order-free), every other sum in a fixed order: same logits, same
 * seen-set, same u -> same token.  Entries whose weights are the same float are kept or removed together in every stage.
 * Refused with PGV_EINVAL, in HF's words and with the value: min_p outside [0, 1] ("`min_p` has to be a float in the [0, 1] interval"), typical_p
 * outside (0, 1] ("`typical_p` has to be a float > 0 and < 1"; 1 is this library's neutral value), epsilon_cutoff / eta_cutoff outside [0, 1)
 * ("`epsilon_cutoff` / `eta_cutoff` has to be a float > 0 and < 1"; 0 is off).
 *
 * pgv_kv_set_filters: the values of every later SAMPLED pick on this cache -- pgv_llm_sample, pgv_llm_decode_sample, the first-token draw of
 * pgv_llm_prefill_slots / _slots_n; NULL or the neutral record (0, 1, 0, 0) turns them off, and every launch is then what it is without this call.
 * Greedy picks ignore them, as they ignore top_p.  pgv_kv_set_warpers leaves them alone.  With pgv_kv_set_logprobs the `pick` value is normalised
 * over the FINAL survivors (HF: compute_transition_scores on `scores`).  The captured decode graphs are rebuilt when a value changes.
 * pgv_sample_logits_filtered (building block, same kernels): pgv_sample_logits_lp plus the record (NULL: neutral) and d_kept_range [B, 2] (may be
 * NULL): the smallest and the largest kept (penalised) logit of each row, (+inf, -inf) for a row that keeps nothing.  With d_kept it pins the kept
 * SET: the survivors are the entries in that logit interval that passed top-k / top-p.  A neutral record gives the tokens, d_kept and both
 * log-probabilities of pgv_sample_logits_lp bit for bit. */
typedef struct pgv_filter_config { float min_p, typical_p, epsilon_cutoff, eta_cutoff; } pgv_filter_config;
int pgv_kv_set_filters(pgv_kv *kv, const pgv_filter_config *cfg);
int pgv_sample_logits_filtered(pgv_ctx *ctx, const float *d_logits, int V, int B, float temperature, int top_k, float top_p, float repetition_penalty,
                               const int32_t *d_seen_ids, int seen_stride, const int32_t *d_seen_lens, const float *d_u, int32_t *d_next,
                               int32_t *d_kept, int greedy, float *d_lp_model, float *d_lp_pick, const pgv_filter_config *cfg, float *d_kept_range,
                               void *stream);

/* Beam search (HF: generate(num_beams = K); GenerationMixin._beam_search of transformers 5, steps b-g), K beams per prompt from ONE prefill, every
 * step on the device.  Per prompt, with t = tokens generated so far, N = max_new_tokens, all arithmetic fp32, NEG = -1e9f:
 *   start  running scores [0, NEG, ...]; finished scores all NEG, finished flags all 0; unsat = 1; open = 1.
 *   b.     logp[k][v] = (x[k][v] - max_k) - ln sum_v exp(x[k][v] - max_k) (the row statistics of pgv_logprob_rows); acc[k * V + v] = logp[k][v] + run[k].
 *   c.     the top 2K of acc.  TIE RULE (torch.topk leaves it open): higher score first, then the lower flat index; a NaN ranks as -inf.
 *          parent = index / V, token = index % V.
 *   d.     hit[j] = token[j] == eos_id || t + 1 >= N   (eos_id < 0: only the budget ends a beam).
 *   e.     r[j] = top[j] + (hit[j] ? NEG : 0); the next running beams are the top K of r (ties: lower j) with those r as scores.
 *   f.     s[j] = top[j] / (t + 1)^length_penalty, + NEG if all K finished flags are set and early_stopping is True, + NEG if !unsat, + NEG unless
 *          (hit[j] && j < K); the K old finished entries followed by the 2K new ones, the top K by score kept (ties: earlier in that list).
 *   g.     best = run'[0] / len^length_penalty with len = N if early_stopping is "never" and length_penalty > 0, else t + 1;
 *          unsat &= any_i (best > (flag'[i] ? min(finished scores') : NEG));  open &= unsat && !(all flags' && early_stopping True) && !all_j hit[j].
 *   A prompt that is no longer open keeps stepping with its group; its finished set, unsat and open stand.
 * (t + 1)^length_penalty is (float)pow((double)(t + 1), (double)length_penalty), computed on the host.
 * State words of one prompt (32-bit, PGV_BEAM_STATE_WORDS(K) of them): run [K] f32 | finished score [K] f32, best first | finished length [K] (tokens;
 * 0: none) | finished parent [K] (the beam the last token continued) | finished last token [K] | finished flag [K] | unsat | open.
 *
 * pgv_beam_begin: on a live group of P prompts (right after pgv_llm_prefill / _append / pgv_llm_score), P * beams <= the batch the cache was created
 *   with.  Forks every prompt to `beams` consecutive slots (pgv_kv_fork), allocates the run's device state on first use (a cache that never runs
 *   beams allocates nothing), and runs the first pick on the prefill's logits.  Refused: no live group (PGV_ESTATE); beams outside [1, 8],
 *   max_new_tokens < 1 or beyond what the cache holds, early_stopping outside 0 (False) / 1 (True) / 2 ("never"), eos_id >= the vocabulary (PGV_EINVAL).
 * pgv_llm_decode_beam: n further steps, each the decode trunk + lm_head of pgv_llm_decode on the current tokens, the row statistics, the beam pick
 *   (token -> current token, parent -> the gather map, both appended to a per-step history, position + 1) and pgv_kv_gather's kernel over the rows
 *   generated since the fork, with map, lengths and every run parameter other than K read from device memory: steps replay from captured graphs
 *   like those of pgv_llm_decode_greedy.  Host-checked before anything is enqueued: a beam run is live (PGV_ESTATE: any other call that moves the
 *   slots -- prefill, fork, gather, truncate, the other decode / pick calls -- ends it), the cache has room, picks done + n <= max_new_tokens.
 * pgv_beam_open: h_open [P] = the open flags (a caller stops stepping when none is set).  Synchronises the stream.
 * pgv_beam_result: finished entry `rank` (0 = best) of prompt p: *n tokens (0: the entry is empty) written to h_tokens [cap >= *n], traced back
 *   through the parent history; *score = HF's sequences_scores; *finished = its flag.  Each output may be NULL.  Synchronises the stream.
 * pgv_beam_pick_logits (building block, same kernels): step t (0 <= t < max_new_tokens) of the rules on caller logits [P * beams, V] fp32 (row
 *   stride V; rows p * beams + k) and caller state d_state [P][PGV_BEAM_STATE_WORDS(beams)], updated in place; d_tokens / d_parents [P * beams]
 *   receive the new running beams.  Every reduction has a fixed order: same logits, same state -> same result on any launch and group width. */
#define PGV_BEAM_STATE_WORDS(K) (6 * (K) + 2)
typedef struct {
    int beams;             /* K, 1..8 */
    int max_new_tokens;    /* N */
    int eos_id;            /* < 0: none */
    float length_penalty;
    int early_stopping;    /* 0 False, 1 True, 2 "never" */
} pgv_beam_config;
int pgv_beam_begin(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, const pgv_beam_config *cfg, void *stream);
int pgv_llm_decode_beam(pgv_ctx *ctx, pgv_llm *llm, pgv_kv *kv, int n, void *stream);
int pgv_beam_open(pgv_kv *kv, int32_t *h_open, void *stream);
int pgv_beam_result(pgv_kv *kv, int p, int rank, int32_t *h_tokens, int cap, int32_t *n, float *score, int32_t *finished, void *stream);
int pgv_beam_pick_logits(pgv_ctx *ctx, const float *d_logits, int V, int P, const pgv_beam_config *cfg, int t, uint32_t *d_state, int32_t *d_tokens,
                         int32_t *d_parents, void *stream);

/* Logit bans: HF's processors that set scores to -inf (HF generation/logits_process.py; built by GenerationMixin._get_logits_processor between
 * the repetition penalty and the warpers).  Each writes -inf or nothing, so their order among themselves and against the penalty (-inf * p and
 * -inf / p are -inf for p > 0) does not change the result.  With ids [0, L) the sequence of a slot -- its prompt as handed to the prefill, placeholder
 * ids included, plus every token a covered pick returned and a later step consumed -- and P its prompt length (the length after the last prefill of the
 * slot; for pgv_llm_prefill_append the total after the append: HF sees the whole conversation as the prompt):
 *  - no_repeat_ngram = n > 0 (NoRepeatNGramLogitsProcessor.__call__ / _get_generated_ngrams): nothing while L < n; else every window ids[j : j + n),
 *    0 <= j <= L - n, whose first n - 1 ids equal the suffix ids[L - n + 1 : L) bans ids[j + n - 1].  n = 1 bans every id of the sequence.
 *  - bad word w of m ids (NoBadWordsLogitsProcessor = SequenceBiasLogitsProcessor.__call__, bias -inf): m = 1 always banned; m > 1: skipped while
 *    m > L, else w[m - 1] is banned iff ids[L - m + 1 : L) == w[0 : m - 1).  (HF's constructor drops a word equal to [eos]: that filter is the
 *    caller's, video_llava_amd/logit_bans.py applies it.)
 *  - suppress (SuppressTokensLogitsProcessor): always banned.  begin_suppress (SuppressTokensAtBeginLogitsProcessor): banned iff L == P.
 *  - min_length (MinLengthLogitsProcessor): eos_id is banned while L < min_length.  min_new_tokens (MinNewTokensLengthLogitsProcessor): eos_id is
 *    banned while L - P < min_new_tokens.  eos_id < 0 makes both rules empty.  The eos_id of the configuration is the one banned; the eos_id argument
 *    of the stepping calls keeps its own meaning (the sticky end of a sequence).
 * Limits (refused with PGV_EINVAL, the message names the value): at most PGV_BAN_MAX_WORDS bad words of at most PGV_BAN_MAX_WORD_LEN ids each, at
 * most PGV_BAN_MAX_IDS listed ids in total (suppress + begin_suppress + all bad-word ids), every listed id in [0, vocab)
 * (SequenceBiasLogitsProcessor._prepare_bias_variables), no negative count; a vocabulary beyond 65536 (the ban set is an LDS bitmap).
 *
 * pgv_kv_set_bans (modelled on pgv_kv_set_warpers): the configuration of every later COVERED pick on this cache; NULL or a configuration that asks
 *   nothing turns the feature off.  Set it before the prefill of the sequences it is meant for: while it is on, the prefill calls (pgv_llm_prefill,
 *   _append, _slots, _slots_n, pgv_llm_score) write each slot's ids and prompt length to a per-cache record int32 [batch][max_seq], indexed by cache
 *   position (so pgv_kv_truncate needs no action), and the ban kernel of a decode step appends the token the step consumes at the slot's position.
 *   The record, a second logits buffer and the device copy of the lists are allocated by the first configuration that asks something; a cache that
 *   never asks allocates nothing and launches nothing.  Synchronises the device (the lists may be read by work in flight); the captured decode graphs
 *   are rebuilt when the configuration changes.
 *   Covered picks: pgv_llm_sample, pgv_llm_pick_greedy, every step of pgv_llm_decode_greedy / _sample, and the first token of
 *   pgv_llm_prefill_slots / _slots_n.  Greedy picks then take the route of a greedy pick under a repetition penalty (the lm_head's arg-max candidates
 *   know no ban).  NOT covered, exactly as for the penalty: the greedy d_next of pgv_llm_prefill / _append (re-pick with pgv_llm_pick_greedy) and plain
 *   pgv_llm_decode steps, which neither ban nor record the token they consume.  Beam runs: pgv_beam_begin on a cache with bans set returns PGV_ESTATE.
 *   pgv_kv_fork copies a source's record rows [0, len) and prompt length to its destinations; pgv_llm_prefill_slots_n writes the prompt's ids to every
 *   sample's slot.
 *   RE-PICKED ROWS: the bans are written to a COPY of the logits row, which the pick reads; the cache's own logits (what d_logits returns, what
 *   pgv_kv_fork copies, what a second pgv_llm_sample reads) are never modified and the row statistics of pgv_kv_set_logprobs are always taken from
 *   them.  Log-probabilities under bans: `model` stays the raw logits' log-softmax (HF's `logits`); `pick` is normalised over what survives the bans
 *   and the warpers (HF's `scores`) -- for a greedy pick the whole-vocabulary log-softmax of the banned (and penalised) logits at temperature 1.
 *   Measured on one MI355X at 7B shapes, 8 sequences, 461-token prompt, 256 steps, no_repeat_ngram 3 + min_new_tokens 8 (scripts/bench_bans.py; LAB.md):
 *   sampled 2.504 -> 2.517 ms per token step (+0.013 ms: the ban kernel); greedy 2.427 -> 2.508 ms (+0.082 ms, of which 0.072 ms is the pick route
 *   that greedy under a repetition penalty already pays).  Off: the steps of the commit before, within run-to-run spread.
 * pgv_ban_logits: the same kernel on caller buffers, in place: d_logits [B, V] fp32 (row stride V), row b's sequence = the d_lens[b] ids at
 *   d_ids + b * ids_stride, its prompt length d_prompt_lens[b]; eos_id as an argument (cfg->eos_id is not read).  Entries outside the ban set keep their
 *   bits (NaN and -inf included); a configuration that asks nothing launches nothing.  Every entry is written by at most one thread: the result does not
 *   depend on B or on the row's index.  Synchronises the stream.
 * pgv_kv_ids_peek (test read-back): the first n <= max_seq entries of slot's record -> d_out [n] int32 (may be NULL), the slot's prompt length ->
 *   d_prompt_len [1] (may be NULL).  PGV_ESTATE while the cache has no record. */
#define PGV_BAN_MAX_IDS 1024
#define PGV_BAN_MAX_WORDS 256
#define PGV_BAN_MAX_WORD_LEN 16
typedef struct {
    int no_repeat_ngram;                 /* n; 0: off */
    const int32_t *h_bad_words;          /* the ids of all bad words, concatenated */
    const int32_t *h_bad_word_lens;      /* [n_bad_words] ids per word */
    int n_bad_words;
    const int32_t *h_suppress; int n_suppress;
    const int32_t *h_begin_suppress; int n_begin_suppress;
    int min_length, min_new_tokens;      /* 0: off */
    int eos_id;                          /* the id the two length rules ban; < 0: none */
} pgv_ban_config;
int pgv_kv_set_bans(pgv_kv *kv, const pgv_ban_config *cfg);
int pgv_ban_logits(pgv_ctx *ctx, float *d_logits, int V, int B, const int32_t *d_ids, int ids_stride, const int32_t *d_lens,
                   const int32_t *d_prompt_lens, int eos_id, const pgv_ban_config *cfg, void *stream);
int pgv_kv_ids_peek(pgv_kv *kv, int slot, int n, int32_t *d_out, int32_t *d_prompt_len, void *stream);

/* Classifier-free guidance: HF's UnbatchedClassifierFreeGuidanceLogitsProcessor (generation/logits_process.py; generate(guidance_scale = s,
 * negative_prompt_ids = ...), the FIRST processor GenerationMixin._get_logits_processor builds).  HF runs the model a second time on the negative
 * prompt and hands the rest of the chain
 *     guided = s * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond).
 * Here the unconditional stream is P more rows of the same decode step: a live group of width 2P whose slots [0, P) are the conditional sequences
 * and whose slot P + p is the unconditional twin of p (the caller prefills prompts + negatives as ONE ragged pgv_llm_prefill of 2P rows).  The trunk
 * and the lm_head run over all 2P rows, unchanged; between the lm_head and the pick, per pair p and vocabulary index v, in fp32 and in this order:
 *     lc = (xc[v] - Mc) - lsc,   lu = (xu[v] - Mu) - lsu,   out[v] = s * (lc - lu) + lu,
 * M the row's maximum and ls = ln sum exp(x - M), the row statistics of pgv_logprob_rows in its reduction order ((x[v] - M) - ls is bit for bit its
 * log-probability of target v).  A pair's result depends on its two rows alone: not on P, the pair's index or the launch.  IEEE results stand: a -inf
 * in the conditional row gives -inf under s > 0; what is NaN in HF's tensor arithmetic (0 * inf, inf - inf) is NaN here.
 *
 * pgv_guidance_logits (building block, the same kernel on caller buffers): rows p of d_cond / d_uncond [P, ld] -> d_out [P, ld_out], columns [0, V).
 *   Any ld, ld_out >= V; 4-byte alignment is all that is required (the decode logits are `vocab` floats apart: 32003 is odd).  d_uncond may equal
 *   d_cond: the output is then the row's log-softmax.  PGV_EINVAL for a stride below V or a scale that is not finite.
 * pgv_kv_set_guidance(kv, scale, pairs): the state of every later COVERED pick on this cache; pairs == 0 or scale == 1 is off, the default, and
 *   every launch, captured graph and token is then what it is without this call.  The guided rows go to a buffer [batch / 2, vocab] that the first
 *   call that switches guidance on allocates; the cache's own logits (d_logits of pgv_llm_decode, what a second pick reads) stay raw.  Refused, and
 *   nothing changes: a scale that is not finite, 2 * pairs beyond the cache's batch (PGV_EINVAL); log-probabilities or lookup on, a beam run in flight
 *   (PGV_ESTATE).  pgv_kv_guidance: the pairs in force (0: off).
 *   Covered picks: pgv_llm_sample, pgv_llm_pick_greedy and every step of pgv_llm_decode_greedy / _sample.  They need a live group of exactly
 *   2 * pairs sequences, else PGV_ESTATE.  The pick runs over P rows reading the guided buffer, with the conditional slot's seen-set (repetition
 *   penalty: HF applies it to the guided scores, as here) and, under pgv_kv_set_bans, the ban copy made from the guided row with the conditional
 *   slot's id record; greedy takes the route of greedy under a penalty.  d_u keeps the group's width 2P as its row length, only columns [0, P) are
 *   read.  Behind the pick the twin follows: current token and done flag of slot P + p become those of slot p and its device position advances
 *   exactly when slot p's does, so rows [P, 2P) of d_next / d_tokens repeat rows [0, P); EOS ends both.  A guided step adds two launches (mix,
 *   follow), inside the captured decode graphs, whose key carries (pairs, scale).
 *   NOT covered, as for the penalty and bans: the greedy d_next of pgv_llm_prefill / _append and plain pgv_llm_decode steps (all 2P rows, unguided).
 *   Refused with PGV_ESTATE while guidance is on: pgv_kv_fork, pgv_llm_prefill_slots / _slots_n, pgv_beam_begin, pgv_kv_set_lookup (D > 0) and the
 *   lookup calls, pgv_kv_set_logprobs(on). */
int pgv_guidance_logits(pgv_ctx *ctx, const float *d_cond, const float *d_uncond, int ld, int V, int P, float scale, float *d_out, int ld_out,
                        void *stream);
int pgv_kv_set_guidance(pgv_kv *kv, float scale, int pairs);
int pgv_kv_guidance(const pgv_kv *kv);

/* Constrained decoding: HF's PrefixConstrainedLogitsProcessor (generation/logits_process.py; generate(prefix_allowed_tokens_fn = fn), built by
 * GenerationMixin._get_logits_processor behind the bans and in front of the warpers), with the Python callback replaced by a deterministic token
 * AUTOMATON that the device follows.  It writes -inf or nothing, like every ban, so its order against the bans and the repetition penalty does not
 * change the result: it runs at the bans' place, between the lm_head and the pick.
 * The automaton: states 0 .. S - 1; the edges of state s are entries [row_ptr[s], row_ptr[s + 1]) of edge_token / edge_next, their tokens in
 * [0, vocab), strictly rising within a state (sorted, distinct), their targets states; accept[s] != 0 marks a state in which the answer may end.
 * DEAD is the state -1.  With P the prompt length of a slot (the length after its last prefill; for pgv_llm_prefill_append the total after the
 * append, so the next answer starts at the root again), r its root and g the ids at cache positions [P, L) -- every token a covered pick returned
 * and a later step consumed:
 *  - the walk: q = r; for every t of g: q = the target of t's edge in q, DEAD when q has none; DEAD stays DEAD.
 *  - the allowed set of the pick at length L: the tokens of q's edges, plus eos_id when q accepts; when q is DEAD or has no edge: {eos_id} alone
 *    (the answer ends; HF raises for an empty list instead).  Every score outside the set becomes -inf; a score inside it keeps its bits, NaN
 *    and -inf included.
 * Limits (PGV_EINVAL, the message names the value): 1 <= S <= PGV_ALLOW_MAX_STATES, 0 <= E <= PGV_ALLOW_MAX_EDGES, eos_id in [0, vocab) -- the rule
 * needs it --, every root in [0, S), a vocabulary of at most 65536 (the allowed set is an LDS bitmap), and the shape above (row_ptr rising from 0 to
 * E, tokens sorted and distinct, targets in range): the kernel then reads inside the arrays whatever the record holds.
 *
 * pgv_kv_set_allowed (modelled on pgv_kv_set_bans): the automaton of every later COVERED pick on this cache; NULL turns the feature off, and every
 *   launch, captured graph and token is then what it is without this call.  h_roots [batch]: the root of every slot (NULL: all 0), written when
 *   the call is made.  Set it before the prefill of the sequences it is meant for: while it is on, the prefill calls write each slot's prompt length
 *   (and ids) to the record of pgv_kv_set_bans, which it shares.  The state record int32 [batch][max_seq], indexed by cache position like the id record
 *   (entry pos >= P: the state after the ids at [P, pos]; so pgv_kv_truncate needs no action), the roots [batch] and the device copy of the automaton
 *   are allocated by the first configuration that asks; the copy grows with the automaton.  The kernel of a decode step does ONE edge lookup: it reads
 *   the state before the step's position (the root at P), follows the edge of the token the step consumes and stores the new state at the position;
 *   a pick that advances nothing (pgv_llm_sample, pgv_llm_pick_greedy, the first token of a refill) reads the state and stores nothing.  No walk from
 *   the root, no host round trip; inside the captured decode graphs, whose key carries a generation counter that moves when the uploaded automaton
 *   changes.  Synchronises the device.
 *   pgv_kv_fork copies a source's state rows [0, len) and root to its destinations; pgv_llm_prefill_slots / _slots_n give every slot they fill
 *   root 0 (one automaton for every task of a refill run).
 *   Covered picks: pgv_llm_sample, pgv_llm_pick_greedy, every step of pgv_llm_decode_greedy / _sample, and the first token of
 *   pgv_llm_prefill_slots / _slots_n.  Greedy picks then take the route of a greedy pick under a repetition penalty (the lm_head's arg-max candidates
 *   know no constraint).  NOT covered, exactly as for the penalty and the bans: the greedy d_next of pgv_llm_prefill / _append (re-pick with
 *   pgv_llm_pick_greedy) and plain pgv_llm_decode steps, which neither mask nor record the state of the token they consume.
 *   With pgv_kv_set_bans also on, the result is the union of the two -inf sets: this kernel writes the pick's copy of the row, logit_ban_kernel runs
 *   in place behind it.  Under guidance the input is the guided row and the record is the conditional slot's.
 *   PGV_ESTATE, and nothing changes: a beam run in flight or pgv_kv_set_lookup on; in turn pgv_beam_begin, pgv_kv_set_lookup (D > 0) and the lookup
 *   calls are refused while it is on.
 *   RE-PICKED ROWS: as under bans, the pick reads a COPY of the row; the cache's own logits (d_logits, what pgv_kv_fork copies, what a second pick
 *   reads) stay raw, `model` log-probabilities are the raw row's, `pick` is normalised over what survives.
 *   Measured on one MI355X at 7B shapes, 8 sequences, 461-token prompt, 256 steps (scripts/bench_allowed.py; LAB.md): the kernel takes 6 - 7 us for
 *   a narrow state and 20 us for a cyclic state of 30000 edges (the ban kernel: 13 us): sampled 2.500 -> 2.520 ms per token step with the latter
 *   (+0.020 ms).  A state with fewer edges than top_k costs more in the PICK: sample_kernel at top_k 50 takes 153 us instead of 83 us over a row with
 *   fewer than 50 finite entries, so sampled 2.500 -> 2.577 ms (+0.077 ms) with a live 10-edge state or behind the end of a 1000-answer trie.  Greedy
 *   2.422 -> 2.512 - 2.518 ms (+0.089 - 0.096 ms, of which 0.072 ms is the pick route that greedy under a repetition penalty already pays).  Off: the
 *   steps of the commit before, within the process-to-process spread.
 * pgv_allow_logits: the same kernel on caller buffers, in place: d_logits [B, V] fp32 (row stride V), row b in state d_states[b] (-1, or anything
 *   outside [0, S): DEAD); eos_id as an argument (cfg->eos_id and cfg->h_roots are not read).  Every entry is written by at most one thread: the
 *   result does not depend on B or on the row's index.  Synchronises the stream.
 * pgv_allow_logits_copy: its out-of-place form, the launch kv_pick makes: rows of d_src [B, V] -> d_dst [B, V], d_src unchanged; d_dst == d_src is
 *   pgv_allow_logits, any other overlap is refused.
 * pgv_kv_allow_peek (test read-back): the first n <= max_seq entries of slot's state record -> d_out [n] int32 (may be NULL), the slot's root ->
 *   d_root [1] (may be NULL).  PGV_ESTATE while the cache has no record. */
#define PGV_ALLOW_MAX_STATES (1 << 20)
#define PGV_ALLOW_MAX_EDGES (1 << 22)
typedef struct {
    const int32_t *h_row_ptr;            /* [n_states + 1] */
    const int32_t *h_edge_token;         /* [n_edges] sorted and distinct within a state */
    const int32_t *h_edge_next;          /* [n_edges] */
    const uint8_t *h_accept;             /* [n_states] */
    int n_states, n_edges;
    const int32_t *h_roots;              /* [batch] or NULL = all 0 */
    int eos_id;
} pgv_allow_config;
int pgv_kv_set_allowed(pgv_kv *kv, const pgv_allow_config *cfg);
int pgv_allow_logits(pgv_ctx *ctx, float *d_logits, int V, int B, const int32_t *d_states, int eos_id, const pgv_allow_config *cfg, void *stream);
int pgv_allow_logits_copy(pgv_ctx *ctx, const float *d_src, float *d_dst, int V, int B, const int32_t *d_states, int eos_id,
                          const pgv_allow_config *cfg, void *stream);
int pgv_kv_allow_peek(pgv_kv *kv, int slot, int n, int32_t *d_out, int32_t *d_root, void *stream);

/* current length (tokens in cache) of sequence b, host-side bookkeeping */
int pgv_kv_len(const pgv_kv *kv, int b);

/* ---- building blocks exported for unit parity tests (same kernels the calls above use) -------- */
/* C[M,N] = A[M,K] * W[N,K]^T (+bias) with epilogue `epi` (see pgv_epi); 16-bit in, fp32 accumulate. */
enum pgv_epi {
    PGV_EPI_NONE = 0,        /* C16 = acc                        */
    PGV_EPI_BIAS = 1,        /* C16 = acc + bias                 */
    PGV_EPI_BIAS_QGELU = 2,  /* C16 = quick_gelu(acc + bias)     */
    PGV_EPI_BIAS_GELU = 3,   /* C16 = gelu_erf(acc + bias)       */
    PGV_EPI_RESID = 4,       /* R32 += acc                       */
    PGV_EPI_BIAS_RESID = 5,  /* R32 += acc + bias                */
    PGV_EPI_SWIGLU = 6,      /* C16[:, n/2] = silu(gate)*up, W rows interleaved gate/up in blocks of 32 */
    PGV_EPI_F32 = 7          /* C32 = acc (+bias if given)       */
};
int pgv_gemm(pgv_ctx *ctx, int dtype, int epi, const void *d_A, int lda, const void *d_W, int ldw, const float *d_bias,
             void *d_C, int ldc, int M, int N, int K, void *stream);
/* pgv_gemm with every argument of the internal launcher, as the CLIP tower and the decoder fill it: W in the pgv_pack_blocked layout
 * (w_blocked != 0: N % 16 == 0, ldw ignored; every prefill GEMM of the decoder) and the three epilogues of the folded LayerNorm, which the
 * public enum does not list.  Same kernels, same host checks; unused pointers are NULL.
 *  consumer  (PGV_EPI_LN_BIAS, PGV_EPI_LN_BIAS_QGELU): C16 = [quick_gelu] (rstd_m (acc - mean_m colsum_n) + bias_n) with d_rowstat [M][2] =
 *            (mean, rstd) per row, d_colsum [N], d_bias [N] (all required).
 *  producer  (PGV_EPI_BIAS_RESID_LNOUT): R32 = d_C += acc + bias (read-modify-write, fp32, ldc); d_x16 [M][ldx16] = round16((R32 - c_m) gnext_n)
 *            with the centre c_m = d_rowmean[m] + *d_cshift (d_rowmean NULL: c = 0 and d_cshift is ignored; d_cshift NULL: 0);
 *            d_stats_part [N / 64][M][2] = (sum, sum of squares) of R32 - c_m over each 64-column piece.  N % 64 == 0, ldx16 % 4 == 0.
 * All three need row-major W and K >= 128. */
enum { PGV_EPI_LN_BIAS = 8, PGV_EPI_LN_BIAS_QGELU = 9, PGV_EPI_BIAS_RESID_LNOUT = 10 };
typedef struct {
    const void *d_A; int lda;
    const void *d_W; int ldw; int w_blocked;
    const float *d_bias;
    void *d_C; int ldc;
    int M, N, K;
    int epi;
    const float *d_rowstat, *d_colsum;                                    /* consumer */
    const float *d_gnext; void *d_x16; int ldx16; float *d_stats_part;    /* producer */
    const float *d_rowmean, *d_cshift;
} pgv_gemm_desc;
int pgv_gemm_ex(pgv_ctx *ctx, int dtype, const pgv_gemm_desc *desc, void *stream);
/* The kernel between producer and consumer: d_part [np][rows][2] -> d_rowstat [rows][2] = (delta, rsqrt(var + eps)) with delta = sum / cols,
 * var = max(sumsq / cols - delta^2, 0), and d_rowmean[row] += delta + *d_cshift (d_cshift NULL: 0). */
int pgv_ln_stats(pgv_ctx *ctx, const float *d_part, float *d_rowstat, float *d_rowmean, const float *d_cshift, int rows, int np, int cols,
                 float eps, void *stream);
/* CLIP self-attention on a fused qkv buffer [T*N, 3C] (q | k | v column blocks) -> [T*N, C]; head_dim 64, no mask
 * (HF CLIPAttention eager math, HF:clip/modeling_clip.py:259-277). */
int pgv_vit_attention(pgv_ctx *ctx, int dtype, const void *d_qkv, void *d_out, int T, int N, int C, int heads, void *stream);
/* Decode-time projection y[B,N] = x[B,K] W[N,K]^T for B <= 64 (weights streamed once; 16 sequences per MFMA column tile).  mode: 0 = 16-bit out,
 * 1 = fp32 residual accumulate, 2 = SwiGLU (W rows interleaved [32 gate | 32 up], out [B, N/2]), 3 = fp32 out.
 * d_W is in the fragment-blocked layout produced by pgv_pack_blocked (rows padded to a multiple of 16). */
int pgv_gemv(pgv_ctx *ctx, int dtype, int mode, const void *d_W, const void *d_x, int ldx, void *d_out, int ldo, int N, int K,
             int B, void *stream);
/* Re-lay a row-major [rows, cols] 16-bit matrix (cols % 32 == 0) into the fragment-blocked layout
 * [rows/16][cols/32][4 k-groups][16 rows][8 elems]: each 1 KiB block is one v_mfma_f32_16x16x32 A fragment in lane order.
 * d_dst must hold ceil(rows/16)*16 * cols elements (zero it first when rows % 16 != 0). */
int pgv_pack_blocked(pgv_ctx *ctx, int dtype, const void *d_src, int rows, int cols, void *d_dst, void *stream);
/* Inverse of pgv_pack_blocked: blocked 16-bit [N, K] (N % 16 == 0, K % 32 == 0) -> row-major fp32. */
int pgv_unpack_blocked(pgv_ctx *ctx, int dtype, const void *d_src_blocked, float *d_dst, int N, int K, void *stream);
/* Quantise a blocked 16-bit matrix [N, K] (N % 16 == 0, K % 64 == 0) to e4m3 with per-row power-of-two scales: writes the fp8
 * blocked copy (N*K bytes: block (n/16, k/64) = 1 KiB, lane ((k%32)/8)*16 + n%16, byte ((k/32)%2)*8 + k%8), the scales [N], and
 * overwrites the 16-bit matrix with the dequantised values. */
int pgv_quantize_fp8_blocked(pgv_ctx *ctx, int dtype, void *d_w16_blocked, void *d_w8_blocked, float *d_scales, int N, int K, void *stream);
/* pgv_gemv on the fp8 copy: bit-identical to pgv_gemv on the dequantised 16-bit matrix, half the weight bytes.  modes 0..3. */
int pgv_gemv_fp8(pgv_ctx *ctx, int dtype, int mode, const void *d_W8, const float *d_scales, const void *d_x, int ldx, void *d_out, int ldo,
                 int N, int K, int B, void *stream);
/* Lossless 12-bit copy of a blocked bf16 matrix [N, K] (N % 16 == 0, K % 64 == 0) for the decode GEMVs: low byte of every weight kept, sign +
 * 3-bit exponent offset below a per-row base as a 4-bit code, the weights that do not fit listed per 16-row block (at most 64 each) and
 * patched back in registers.  d_w12 holds pgv_w12_bytes(N, K) bytes; d_counts [N / 16] receives the exception count of every row block --
 * the copy is usable iff none exceeds 64.  Layout: video_llava_amd/csrc/w12.h. */
size_t pgv_w12_bytes(int N, int K);
int pgv_encode_w12_blocked(pgv_ctx *ctx, int dtype, const void *d_w16_blocked, void *d_w12, int *d_counts, int N, int K, void *stream);
/* pgv_gemv on the 12-bit copy: bitwise equal to pgv_gemv on the bf16 matrix it was encoded from, 3/4 of the weight bytes.  modes 0..3, B <= 16;
 * N = the encoded row count (or fewer, mode 3). */
int pgv_gemv_w12(pgv_ctx *ctx, int dtype, int mode, const void *d_W12, const void *d_x, int ldx, void *d_out, int ldo, int N, int K, int B,
                 void *stream);
/* The decode GEMV with every argument of the internal launcher, as a decode step fills it (test entry: same kernels, the launch shape is chosen
 * exactly as in decode).  Unused pointers are NULL.
 *  mode      0..3 as pgv_gemv, or 5 = the residual + RMSNorm PRODUCER (o_proj, down_proj): d_out [B][ldo] fp32 residual += y (read-modify-write),
 *            d_xg = round16(residual * d_gamma[n]) (16-bit, row-major [B][ldo] or blocked, below), d_ssq_out [ct][n / 16][16] = the sum of the
 *            new residual's squares over each block of 16 rows per sequence (tile stride ssq_ts >= N; the slots of sequences >= B receive 0).
 *  weights   d_W = 16-bit blocked (pgv_pack_blocked), or the fp8 codes with d_wscale [ceil16(N)] (pgv_quantize_fp8_blocked); d_W12 = the 12-bit
 *            copy (pgv_encode_w12_blocked; bf16), streamed instead of d_W where the launch has one column tile (d_W may then be NULL).
 *  consumer  (modes 0, 2, 3 with d_ssq_in): out = (W x) * rsqrt(sum_parts ssq_in / hidden + eps), applied to the fp32 accumulators;
 *            d_ssq_in [ct][nparts_in][16] with tile stride ssq_ts >= 16 nparts_in, nparts_in <= 384.
 *  head      (mode 3 with d_amax_val / d_amax_idx [ct][ceil(N / 16)][16], tile stride amax_ts >= 16 ceil(N / 16)): per block of 16 rows and
 *            sequence the largest logit over rows < N and the smallest row index attaining it (NaN never wins; none: (-inf, 0x7fffffff)).
 *            Every tile of the launch is written, also those beyond B.
 *  strides   ssq_ts / amax_ts may be 0 only where the array they stride is NULL (the launcher is then handed the dense strides 16 and
 *            16 ceil(N / 16), which it requires at B > 16 but never uses); with the array given, the bounds above are checked.
 *  mode 1    (d_out fp32 += y, no norm field) is accepted for completeness; a decode step no longer runs it (the producer replaced it).
 *  tiles     ct = 1 / 2 / 4 column tiles of 16 sequences for B <= 16 / 32 / 64; sequence b is entry b % 16 of tile b / 16.
 *  x_blocked with B > 8 the 16-bit operand between producer and consumer (a consumer's d_x, a producer's d_xg) is in the fragment-blocked
 *            activation layout [K / 32][ct][4 k-groups][16 sequences][8 elements] (ct * 16 * K elements; ldx is ignored); B <= 8: row-major.
 *  d_k8_part scratch of the 8-phase form of a producer, (N / 16) * 8 * ct * 1024 bytes, k8_part_bytes = its size; NULL = 16-row kernel only.
 *  shape     (optional) receives the launch shape that ran: row blocks per workgroup, column tiles, merged x load, 8-phase form and its row
 *            blocks per workgroup, weight format streamed (0 = 16-bit, 1 = fp8, 2 = 12-bit). */
typedef struct { int tl, ct, x2, k8, nwb, wfmt; } pgv_gemv_shape;
typedef struct {
    int mode;
    const void *d_W; const float *d_wscale; const void *d_W12;
    const void *d_x; int ldx;
    void *d_out; int ldo;
    int N, K, B;
    const float *d_ssq_in; int nparts_in; int hidden; float eps;          /* consumer */
    const float *d_gamma; void *d_xg; float *d_ssq_out;                    /* producer */
    float *d_amax_val; int *d_amax_idx;                                    /* head */
    int ssq_ts, amax_ts;
    void *d_k8_part; size_t k8_part_bytes;
    int x_blocked;
    pgv_gemv_shape *shape;
} pgv_gemv_desc;
int pgv_gemv_ex(pgv_ctx *ctx, int dtype, const pgv_gemv_desc *desc, void *stream);
/* The two kernels that start a chain of folded GEMVs (test entry).  d_tok NULL: d_resid [B][H] fp32 is read (the final norm's prep); else
 * d_resid[b] = d_embed[d_tok[b]] (16-bit table [rows][H]; the ids are not checked) is written.  Both write d_xg = round16(resid * d_gamma)
 * (row-major [B][H], or blocked as above when x_blocked and B > 8) and d_ssq[(b / 16) * H + b % 16] = sum of resid[b]^2: one partial per
 * sequence, tile stride H.  H % 32 == 0, 1 <= B <= 64. */
int pgv_gemv_prep(pgv_ctx *ctx, int dtype, const int32_t *d_tok, const void *d_embed, float *d_resid, const float *d_gamma, void *d_xg,
                  float *d_ssq, int B, int H, int x_blocked, void *stream);
/* LLaMA decode attention of one token step on caller buffers: the kernels and launcher pgv_llm_decode runs (RoPE on q and k at h_pos[b], append of
 * the rotated k and of v at row h_pos[b], softmax over cache rows [0, h_pos[b]] with scale 128^-0.5).  `llm` supplies the dtype, head count and
 * RoPE table (no weights need to be loaded).  d_qkv [B, 3H] 16-bit (q | k | v), d_Kc / d_Vc [B, heads, max_seq, 128], d_out [B, H]; rows at
 * or past h_pos[b] are never read into the result.  Host-checked: 1 <= B <= 64, 1 <= max_seq <= 4096, 0 <= h_pos[b] < max_seq.  split: 0 = the
 * model's choice (as pgv_llm_decode), 1 / 2 / 4 / 8 = that many workgroups per (sequence, head).  d_part (B * heads * 8 * 130 floats) and
 * d_ticket (B * heads, zeroed by the caller; every launch leaves it zero) are the split merge's scratch.  Synchronises the stream once. */
int pgv_decode_attention(pgv_ctx *ctx, pgv_llm *llm, const void *d_qkv, const int32_t *h_pos, void *d_Kc, void *d_Vc, void *d_out, int B, int max_seq,
                         int split, float *d_part, uint32_t *d_ticket, void *stream);
/* Its row form, the kernels and launcher pgv_llm_decode_rows runs: row r of R is the pair (slot h_row_slot[r] of S, offset h_row_j[r]) and sits at
 * position p = h_pos[slot] + h_row_j[r].  The rotated k and the v of d_qkv[r] ([R, 3H]) are written to cache row p of the slot (by a launch in front
 * of the attention), the row attends to cache rows [0, p] and writes d_out[r] ([R, H]).  With the rows of a slot at offsets 0 .. n - 1, output and
 * cache rows are bit for bit those of n consecutive pgv_decode_attention calls at h_pos, h_pos + 1, ... on the same q / k / v (same `split`).
 * h_row_slot[r] == -1: no row -- nothing of it is read or written.  Host-checked: 1 <= S, R <= 64, every position below max_seq, no two rows at
 * one (slot, offset).  d_part (R * heads * 8 * 130 floats) and d_ticket (R * heads, zeroed by the caller; left zero).  Synchronises the stream once. */
int pgv_decode_attention_rows(pgv_ctx *ctx, pgv_llm *llm, const void *d_qkv, const int32_t *h_pos, int S, const int32_t *h_row_slot,
                              const int32_t *h_row_j, void *d_Kc, void *d_Vc, void *d_out, int R, int max_seq, int split, float *d_part,
                              uint32_t *d_ticket, void *stream);
/* LLaMA prefill attention on caller buffers: the kernels pgv_llm_prefill / pgv_llm_prefill_append run.  Sequence b has h_seq_lens[b] rows,
 * concatenated in d_qkv [M, 3H]; row i sits at position koff + i (h_koff[b], or 0 when h_koff is NULL).  q is rotated in place in d_qkv,
 * the rotated k and v are written to cache rows koff + i, and row i attends to keys [0, koff + i].  d_out [M, H].  Host-checked:
 * 1 <= B <= 64, 1 <= max_seq <= 4096, koff >= 0, koff + len <= max_seq.  Synchronises the stream once. */
int pgv_prefill_attention(pgv_ctx *ctx, pgv_llm *llm, void *d_qkv, const int32_t *h_seq_lens, const int32_t *h_koff, void *d_Kc, void *d_Vc,
                          void *d_out, int B, int max_seq, void *stream);
/* Row norms of an fp32 [rows, cols] matrix -> 16-bit d_y.  cols must be one of the instantiated widths 256, 512, 768, 1024, 2048, 4096, 5120; any
 * other width returns PGV_EINVAL before anything is launched. */
int pgv_layernorm(pgv_ctx *ctx, int dtype, const float *d_x, const float *d_gamma, const float *d_beta, float eps,
                  void *d_y, int rows, int cols, void *stream);
int pgv_rmsnorm(pgv_ctx *ctx, int dtype, const float *d_x, const float *d_gamma, float eps, void *d_y, int rows, int cols,
                void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PGV_H */
