// Internal interface of the LLaMA decoder translation units (llm.hip = host drivers; llm_prefill.hip, gemv.hip, decode_attn.hip, sampling.hip =
// kernels + launchers): launcher prototypes, mode enums and the few device helpers more than one of them uses.
#pragma once
#include "pgv_common.h"
#include "gemv_plan.h"     // GV_* epilogues, kMaxBatch, the decode GEMVs' launch plan
#include "pick_params.h"

constexpr int kHD = 128;             // LLaMA head_dim
constexpr int kDattnSplitMax = 8, kDattnPart = kHD + 2;                                 // w12.hip
int pgv_launch_encode_w12(const void* w16_blocked, void* w12, int* counts, long long N, long long K, hipStream_t s);
// decode_attn.hip: context splits, floats per partial state

// vit_attn.hip
int pgv_vit_attn_configure(pgv_ctx* ctx);  // per-device dynamic-LDS opt-in of the attention kernels: called once per context
// elementwise.hip
int pgv_launch_rmsnorm(int dtype, const float* x, const float* g, float eps, void* y, int rows, int cols, hipStream_t s);
// llm_prefill.hip
int pgv_launch_embed_splice(int dtype, const int* row_src, const void* embed, const void* video, float* resid, int M, int H, hipStream_t s);
int pgv_launch_gather_rows(const float* src, const int* rows, float* dst, int B, int H, hipStream_t s);
int pgv_launch_rope_kv_write(int dtype, void* qkv, const int* row_b, const int* row_pos, const void* rope, void* Kc, void* Vc, int M, int H,
                             int heads, int max_seq, hipStream_t s);
// slot [B]: cache slot of sequence b (null: b; pgv_llm_prefill_slots)
int pgv_launch_prefill_attn(pgv_ctx* ctx, int dtype, const void* qkv, void* out, const void* Kc, const void* Vc, const int* cu, const int* koff, int B, int max_len,
                            int H, int heads, int max_seq, double flops, hipStream_t s, const int* slot = nullptr);
// kv_fork.hip: slot `src` of a cache -> slots [d0, d0 + nd) except itself (pgv_kv_fork).  Cache rows: nrun = planes * heads runs of run_pieces
// 16-byte pieces each (rows [0, len) of one head are contiguous); plane = one layer's K or V, [slots][heads][max_seq][128] 16-bit, the planes a
// constant plane_stride bytes apart.  State: the slot's words of pos / cur / done, of lp_last [2][lp_stride], of seen [slots][seen_words] and
// of logits [slots][vocab].  The caller has checked every slot index against the cache's batch.
struct KvForkArgs {
    char* cache; size_t plane_stride, slot_stride, head_stride;
    int heads, nrun; unsigned run_pieces;
    int src, d0, nd;
    const int* dst = nullptr;   // pgv_launch_kv_fork_list: device list of the nd destination slots (d0 and the state pointers below are not read)
    int *pos, *cur, *done; float* lp_last; int lp_stride;
    unsigned* seen; int seen_words; float* logits; int vocab;
};
int pgv_launch_kv_fork(const KvForkArgs& a, hipStream_t s);
// the cache rows only, slot `src` -> slots dst[0 .. nd): distinct, none of them src (pgv_llm_prefill_slots_n)
int pgv_launch_kv_fork_list(const KvForkArgs& a, hipStream_t s);
// beam.hip: the two kernels of a beam-search step (pgv.h: pgv_beam_begin).
// kv_gather: inside every group of K consecutive slots, slot g0 + i receives rows [row0[g], len[g0]) of slot g0 + map[g0 + i], in every plane and
// head (the layout of KvForkArgs).  map / row0 / len are DEVICE arrays, read by the kernel: a captured launch stays valid at any position.  cur
// (optional): the slots' current tokens move with them.  The grid does not depend on len.
struct KvGatherArgs {
    char* cache; size_t plane_stride, slot_stride, head_stride;
    int heads, nrun, K, groups, max_seq;
    const int *map, *row0, *len;
    int* cur;
};
int pgv_launch_kv_gather(const KvGatherArgs& a, hipStream_t s);
// The run parameters of a beam search (HF's names); early: 0 False, 1 True, 2 "never"
struct BeamParams { int max_new, eos, early; float length_penalty; };
// beam_pick: one workgroup per prompt over the K logits rows of its group (rows p * K + k, stride ld, columns [0, V)), their statistics stat
// [P * K][2] (pgv_launch_row_lse) and the prompt's state words (pgv.h: PGV_BEAM_STATE_WORDS).  Writes, per new slot p * K + i, the token to cur and
// the parent to map, both also to hist_tok / hist_par [t][hist_stride] (null: no history; t < hist_steps), and with `advance` pos[slot] += 1.
// t and the parameters come from device memory (t_dev [P], advanced by the kernel; prm_dev; denom [n] = (float)pow(n + 1, length_penalty)) or, where
// those are null, by value (t_val, prm_val, den_t = the value for t, den_n = the value for max_new - 1).
struct BeamPickArgs {
    const float* logits; int ld, V, K;
    const float* stat;
    unsigned* state; int state_stride;
    int* t_dev; int t_val;
    const BeamParams* prm_dev; BeamParams prm_val;
    const float* denom; float den_t, den_n;
    int *cur, *map, *pos; int advance;
    int *hist_tok, *hist_par; int hist_stride, hist_steps;
};
int pgv_launch_beam_pick(const BeamPickArgs& a, int P, hipStream_t s);
// gemv.hip
// w12: the 12-bit copy of W (w12.h), streamed instead of W at batches of one column tile (B <= 16) -- bitwise the same result; W may be null
// only when B <= 16.  rows = the row count it was encoded with (>= N).
struct W12Ref { const void* buf = nullptr; long long rows = 0; };
// ran (optional): receives the launch shape chosen for this call (pgv_gemv_ex)
int pgv_launch_gemv(pgv_ctx* ctx, int dtype, int mode, const void* W, const void* x, int ldx, void* out, int ldo, int N, int K, int B, hipStream_t s,
                    const float* wscale = nullptr, const GemvNorm* norm = nullptr, const W12Ref* w12 = nullptr, pgv_gemv_shape* ran = nullptr);
int pgv_gemv_configure(pgv_ctx* ctx);      // per-device function attributes of the 8-phase producers: called once per context, outside graph capture
int pgv_launch_embed_tok_norm(int dtype, const int* tok, const void* embed, float* resid, const float* gamma, void* xg, float* ssq, int B, int H, hipStream_t s, bool x_blocked);
int pgv_launch_final_prep(int dtype, const float* resid, const float* gamma, void* xg, float* ssq, int B, int H, hipStream_t s, bool x_blocked);
int pgv_gemv_xblk_tiles(int B);            // column tiles of the blocked activation layout at B sequences (0: row-major)
// fp8.hip
int pgv_launch_quantize_fp8(int dtype, void* w16_blocked, void* w8_blocked, float* scales, long long N, long long K, hipStream_t s);
int pgv_launch_unpack_blocked(int dtype, const void* src, float* dst, long long N, long long K, long long row_blk, long long blk_stride, long long row_off,
                              long long rows, hipStream_t s);
// decode_attn.hip
int pgv_launch_decode_attn(pgv_ctx* ctx, int dtype, const void* qkv, const int* pos, const void* rope, void* Kc, void* Vc, void* out, int B, int H,
                           int heads, int max_seq, double bytes, hipStream_t s, float* part, unsigned* ticket, int split_force);
// the row form (decode_attn.hip): row r = (slot row_slot[r], offset row_j[r]) of R reads qkv[r], appends its k / v at cache row pos[slot] + row_j[r] (a
// launch of its own in front) and attends to rows [0, that]; row_slot[r] < 0: no row.  part / ticket: R * heads units.
int pgv_launch_decode_attn_rows(pgv_ctx* ctx, int dtype, const void* qkv, const int* pos, const int* row_slot, const int* row_j, const void* rope, void* Kc,
                                void* Vc, void* out, int R, int H, int heads, int max_seq, double bytes, hipStream_t s, float* part, unsigned* ticket,
                                int split_force);
// lookup.hip: the draft and accept kernels of a prompt-lookup step (pgv.h: pgv_llm_decode_lookup, pgv_llm_decode_lookup_sample).  Slot b owns rows b * (1 + D) + j, j = 0 .. D.
struct LookupArgs {
    int D = 0, n = 0, eos = -1, max_seq = 0;
    int *pos = nullptr, *cur = nullptr, *step = nullptr, *done = nullptr, *hist = nullptr; int hist_stride = 0;   // the cache's pick state (PickState)
    int* rec = nullptr;                       // id record [slots][max_seq], indexed by cache position
    const int* budget = nullptr;              // [slots] tokens the run may still emit per slot
    int *tok = nullptr, *row_slot = nullptr, *row_j = nullptr, *n_draft = nullptr;      // rows: token, slot (-1: no row), offset; drafts per slot
    const int* t = nullptr;                   // [rows] the arg-max behind every row
    int *counts = nullptr, counts_stride = 0, *k = nullptr;                            // emit counts [steps][counts_stride], the run's step counter
    // the sampled form (null u: the greedy form, which reads and writes none of these).  Row (b, j) is picked with the uniform the plain run uses for
    // that token, u[(u_base[b] + step[b] + j) * u_stride + b]: the draft kernel gathers it into u_row [rows] (0 for a row that is none).
    const float* u = nullptr; int u_stride = 0; const int* u_base = nullptr; float* u_row = nullptr;
    // seen-set bitmaps [slots][seen_words] (null: not kept): the accept kernel marks every emitted token below `vocab`, as a plain sampled pick does
    unsigned* seen = nullptr; int seen_words = 0, vocab = 0;
};
int pgv_launch_lookup_draft(const LookupArgs& a, int B, hipStream_t s);
int pgv_launch_lookup_accept(const LookupArgs& a, int B, hipStream_t s);
// sampling.hip
// Where a pick puts the token of row b and what it advances (the defaults: the caller's `next` only).  advance: AM_INC_POS does pos[b]++;
// AM_RECORD does hist[b * hist_stride + step[b]++] = token and keeps EOS sticky through done[b] (eos < 0: no EOS).
struct PickState {
    int* next = nullptr; int* pos = nullptr; int* step = nullptr; int* hist = nullptr; int hist_stride = 0; int* done = nullptr; int eos = -1, advance = 0;
};
// The seen-set a sampled pick's repetition penalty reads (top_p / penalty: pgv_launch_sample copies them in from its PickParams, a caller leaves
// them alone).  Row b: the bitmap of slot seen_slot[b] (null: b) in seen_bits [slots][seen_words] -- the pick then sets the bit of the token it returns --
// and / or the id list seen_ids[b * seen_stride .. + seen_lens[b]).  kept [B] (optional): vocabulary entries left with non-zero probability.
struct SampleWarp {
    float top_p = 1.f, penalty = 1.f;
    unsigned* seen_bits = nullptr; int seen_words = 0; const int* seen_slot = nullptr;
    const int* seen_ids = nullptr; int seen_stride = 0; const int* seen_lens = nullptr;
    int* kept = nullptr;
};
// Log-probabilities of the token a pick returns (pgv_kv_set_logprobs; null `stat`: none).  stat [B][2] = (maximum, ln of the sum of exp(x - maximum))
// of every raw logit row, written by pgv_launch_row_lse in front of the pick.  Row b's two values -- `model`: x[t] - logsumexp(x); `pick`: the log of
// the probability the pick used -- go to index slot[b] (null: b) of last_model / last_pick (each may be null) and, when the pick records
// (AM_RECORD), to hist_model / hist_pick [b * hist_stride + step[b]], next to the token history.  A sticky EOS step (the done flag was set before
// the pick) stores 0 for both.  greedy: PickParams::greedy, copied in by pgv_launch_sample (a caller leaves it alone) -- without a penalty the
// `pick` value of such a pick is `model`, the same float.
struct PickLp {
    const float* stat = nullptr;
    float *last_model = nullptr, *last_pick = nullptr;
    float *hist_model = nullptr, *hist_pick = nullptr; int hist_stride = 0;
    const int* slot = nullptr;
    int greedy = 0;
    int banned = 0;      // the logits the pick reads went through logit_ban_kernel: a greedy `pick` value is then their whole-vocabulary log-softmax, penalty or not
};
int pgv_check_warpers(const char* who, float top_p, float penalty);
// n zeros: the uniforms of a pick_greedy pick
inline int pgv_zero_uniforms(float* u, size_t n, hipStream_t s) { PGV_HIP(hipMemsetAsync(u, 0, n * 4, s)); return PGV_OK; }
int pgv_launch_sample(const float* logits, int V, int B, const PickParams& p, const float* u, int u_stride, int u_by_step, const PickState& st, hipStream_t s,
                      const SampleWarp* warp = nullptr, const PickLp* lp = nullptr, float* kept_range = nullptr);
// HF's constructor checks of the four filter warpers (pgv.h: pgv_kv_set_filters), their wording.  pgv_launch_sample runs the filter tail
// (sample_kernel<true, LP, true>) only when PickParams::filtered() or kept_range [B][2] (the smallest / largest kept logit) asks for it.
int pgv_check_filters(const char* who, float min_p, float typical_p, float epsilon, float eta);
// prefill: ids [M] of sequences with row ranges cu -> block b marks the ids of sequence seq[b] (null: b) in the bitmap of slot slots[b] (null: b);
// clear = start from an empty set
int pgv_launch_seen_mark(const int* ids, const int* cu, const int* slots, int B, int V, unsigned* bits, int words, int clear, hipStream_t s,
                         const int* seq = nullptr);
// logits [B, V] (row stride V) + lp: also store the log-probability of the pick (both values are `model`: a plain arg-max has no processor)
int pgv_launch_argmax_parts(const float* val, const int* idx, int nblk, int amax_ts, int V, int B, const PickState& st, hipStream_t s, const float* logits = nullptr,
                            const PickLp* lp = nullptr);
// pgv_llm_prefill_slots: sequence i of the call becomes slot slots[i] -- cur = pick[i], pos = lens[i], step = done = 0
int pgv_launch_slot_scatter(const int* slots, const int* pick, const int* lens, int n, int* cur, int* pos, int* step, int* done, hipStream_t s);

// logit_ban.hip: HF's processors that set scores to -inf (pgv.h: pgv_kv_set_bans).
// The lists of a configuration in DEVICE memory: suppress [n_sup], begin-suppress [n_beg], bad word w = word_ids[word_off[w] .. word_off[w + 1]).
struct BanLists {
    int ngram = 0, n_sup = 0, n_beg = 0, n_words = 0, min_length = 0, min_new = 0;
    const int *sup = nullptr, *beg = nullptr, *word_off = nullptr, *word_ids = nullptr;
};
// One workgroup per logits row b: dst[b] = src[b] with -inf at every id the rules ban (src == dst: only those entries are written).  The row's
// sequence is ids[slot * ids_stride .. + L) with slot = slot_map[b] (null: b) and L = lens[b]; with `inc` (the pick of a decode step, AM_INC_POS) the
// token the step consumed, cur[b], is first stored at rec[slot * ids_stride + lens[b]] and L = lens[b] + 1.  prompt_lens is indexed by slot.
// done (may be null): rows whose flag is set are copied without a ban.  eos < 0: the two length rules are empty.
struct BanArgs {
    const float* src = nullptr; float* dst = nullptr; int V = 0;
    const int* ids = nullptr; int ids_stride = 0;
    const int *slot_map = nullptr, *lens = nullptr, *prompt_lens = nullptr;
    int* rec = nullptr; const int* cur = nullptr; int inc = 0;
    const int* done = nullptr;
    int eos = -1;
    BanLists cfg;
};
int pgv_launch_logit_ban(const BanArgs& a, int B, hipStream_t s);
// prefill: workgroup t writes the ids of sequence seq[t] (null: t; rows cu[q] .. cu[q + 1] of `ids`) to rec[slot * stride + offs[q] ..) with slot =
// slots[t] (null: t), and prompt_lens[slot] = offs[q] + the row count -- the indirection of pgv_launch_seen_mark
int pgv_launch_ids_write(const int* ids, const int* cu, const int* offs, const int* slots, const int* seq, int T, int* rec, int stride, int* prompt_lens,
                         hipStream_t s);
// validate a pgv_ban_config against the limits of pgv.h and the vocabulary and pack its lists into `blob` (offsets into it: sup / beg / word_off /
// word_ids of `at`); ban_lists turns them into pointers behind a device copy of the blob
struct BanPacked { BanLists cfg; size_t sup = 0, beg = 0, word_off = 0, word_ids = 0; };
int pgv_ban_pack(const char* who, const pgv_ban_config* c, int V, std::vector<int>& blob, BanPacked& at);
bool pgv_ban_neutral(const pgv_ban_config* c, int eos);
inline BanLists ban_lists(const BanPacked& at, const int* d_blob) {
    BanLists l = at.cfg;
    l.sup = d_blob + at.sup; l.beg = d_blob + at.beg; l.word_off = d_blob + at.word_off; l.word_ids = d_blob + at.word_ids;
    return l;
}

// logit_allow.hip: constrained decoding by a token automaton (pgv.h: pgv_kv_set_allowed).
// The automaton in DEVICE memory, CSR: the edges of state s are [row_ptr[s], row_ptr[s + 1]), their tokens sorted and distinct.  One blob of
// allow_words(S, E) ints holds row_ptr [S + 1] | edge_token [E] | edge_next [E] | accept [S] bytes (allow_auto binds the pointers).
struct AllowAuto {
    const int *row_ptr = nullptr, *edge_token = nullptr, *edge_next = nullptr; const unsigned char* accept = nullptr;
    int n_states = 0, n_edges = 0;
};
inline size_t allow_words(int S, int E) { return (size_t)S + 1 + 2 * (size_t)E + ((size_t)S + 3) / 4; }
inline AllowAuto allow_auto(const int* d_blob, int S, int E) {
    AllowAuto a;
    a.row_ptr = d_blob; a.edge_token = d_blob + S + 1; a.edge_next = a.edge_token + E; a.accept = (const unsigned char*)(a.edge_next + E);
    a.n_states = S; a.n_edges = E;
    return a;
}
// One workgroup per logits row b: dst[b] = src[b] with -inf outside the tokens the row's state allows (src == dst: only those entries are written).
// The state: direct[b] (pgv_allow_logits; -1: DEAD), or that of the cache row -- slot = slot_map[b] (null: b), at = lens[b], and with
// prev = (at == prompt_lens[slot]) ? root[slot] : state[slot * state_stride + at - 1]: with `inc` (the pick of a decode step, AM_INC_POS) the target
// of cur[b]'s edge in prev (none: DEAD), which is first stored at state[slot * state_stride + at]; without it prev itself, nothing stored.
// done (may be null): rows whose flag is set are copied as they are.
struct AllowArgs {
    const float* src = nullptr; float* dst = nullptr; int V = 0;
    AllowAuto au;
    const int* direct = nullptr;
    int* state = nullptr; int state_stride = 0; const int* root = nullptr;
    const int *slot_map = nullptr, *lens = nullptr, *prompt_lens = nullptr, *cur = nullptr; int inc = 0;
    const int* done = nullptr;
    int eos = -1;
};
int pgv_launch_logit_allow(const AllowArgs& a, int B, hipStream_t s);
// root[slots[t]] = 0 for the n slots of a DEVICE list (a refill's slots start at the root of the shared automaton)
int pgv_launch_allow_root_zero(const int* slots, int n, int* root, hipStream_t s);
// validate a pgv_allow_config against the limits of pgv.h, the vocabulary and the shape of a CSR automaton (n_roots entries of h_roots, where given);
// pack its arrays into the blob layout above
int pgv_allow_check(const char* who, const pgv_allow_config* c, int V, int n_roots);
void pgv_allow_pack(const pgv_allow_config* c, std::vector<int>& blob);

// guidance.hip: classifier-free guidance (pgv.h: pgv_kv_set_guidance).
// mix: pair p of P reads cond[p * ld ..) and uncond[p * ld ..) over columns [0, V) and writes out[p * ld_out ..) = scale * (lc - lu) + lu with lc / lu
// the rows' log-softmax (row_lse_kernel's statistics, bit for bit).  Any strides >= V, 4-byte alignment.
int pgv_launch_guidance_mix(const float* cond, const float* uncond, int ld, int V, int P, float scale, float* out, int ld_out, hipStream_t s);
// follow: behind a pick on rows [0, P) with state `st` (the cache's own), slot P + p takes slot p's token and done flag and advances as st.advance says
int pgv_launch_guidance_follow(int P, const PickState& st, hipStream_t s);

// score.hip: per-row log-probability of targets[r] / logsumexp / argmax over columns [0, V) of fp32 logits [R, ld]; row r writes at index
// out_rows[r] (null: r).  Timed under family 6.
int pgv_launch_logprob_rows(pgv_ctx* ctx, const float* logits, int ld, int V, int R, const int* targets, const int* out_rows, float* logprob, float* lse,
                            int* argmax, hipStream_t s);
// its sibling in front of a pick (PickLp::stat): stat[r] = (maximum, ln sum exp(x - maximum)) over columns [0, V) of row r, in logprob_rows' reduction
// order -- (x[t] - stat[r][0]) - stat[r][1] is bit for bit its logprob.  Any ld >= V and any 4-byte alignment (the decode logits are vocab floats apart).
int pgv_launch_row_lse(const float* logits, int ld, int V, int R, float* stat, hipStream_t s);

#if defined(__HIPCC__)
// sum over each aligned group of 16 lanes with DPP (VALU latency) instead of ds_bpermute shuffles (LDS crossbar latency):
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_ror:4, row_ror:8 -> every lane of the row ends up with the row total.
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));
    return v;
}

// Buffer descriptor over `bytes` bytes at `base` from provably wave-uniform inputs (cdna_hip_programming.md T20): lanes whose voffset lies outside
// the range are dropped by the hardware -- no memory request, the result is 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gv_make_rsrc(const void* base, unsigned bytes) {
    const uintptr_t b = (uintptr_t)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)hi << 32) | lo), 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// Cross-row sums with gfx950's lane-swap instructions instead of ds_bpermute round trips.  Only the FIRST result of the swap is used (vdst:
// even rows / the low half keep their value, odd rows / the high half receive the partner's -- checked on hardware, scripts/lab/permlane_swap.hip):
// v + swap(v, v) is the pair sum in the odd rows / the high half, so after both steps the total of the four rows sits in ROW 3 (lanes 48..63).
// (The second result would give the sum everywhere, but with one value on both operands hipcc of ROCm 7.2 reads it from the wrong register.)
__device__ __forceinline__ float rows_sum_to_row3(float v) {
    const unsigned a = __builtin_bit_cast(unsigned, v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_permlane16_swap(a, a, false, false)[0]);          // rows 1, 3: v1 + v0, v3 + v2
    const unsigned b = __builtin_bit_cast(unsigned, v);
    return v + __builtin_bit_cast(float, __builtin_amdgcn_permlane32_swap(b, b, false, false)[0]);    // row 3: (v3 + v2) + (v1 + v0)
}
#endif
