// mm_projector + LLaMA decoder host side: packed weights, KV cache, prefill / decode drivers.
// Replaces VideoChatGPTLlamaForCausalLM.forward (video_chatgpt/model/video_chatgpt.py:193-251 -> :82-175 -> HF LlamaModel)
// as driven by model.generate (video_chatgpt/inference.py:105-112).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "kv_features.h"
#include "llm_internal.h"
#include "llm_weights.h"
#include "prefill_plan.h"
#include "w12.h"
#include "weights.h"

// One decoder matrix (shapes, HF keys and blob offsets: llm_weights.h) and its copies.
struct LlmMat {
    long long N, K;          // rows a GEMV computes / get_weight reads, columns.  lm_head: N = cfg.vocab, the live vocabulary (pgv_llm_resize_vocab)
    long long cap;           // allocated rows (LlmMatSlot::N): what the blobs, the 12-bit encoder and the fp8 quantiser cover (lm_head: vocab_cap, else N)
    void* w16;               // fragment-blocked 16-bit matrix: prefill reads it, decode streams it unless one of the copies below exists
    // fp8 decode copy (pgv_llm_quantize_fp8): e4m3 blocked matrix + per-row power-of-two scales; null until quantised
    void* w8 = nullptr; float* scale = nullptr;
    // lossless 12-bit decode copy of bf16 models (w12.h; buf null: none, or the matrix keeps its 16-bit stream)
    W12Ref z;
};
struct LlmLayer { float *in_g, *post_g; };

struct pgv_llm {
    pgv_ctx* ctx;
    pgv_llm_config cfg;
    int dtype;
    char* blob = nullptr;
    size_t blob_bytes = 0;
    void* embed;
    float* norm_g;
    float* rope;   // float2 [kMaxPos][64]
    std::vector<LlmLayer> layers;
    std::vector<LlmMat> mats;   // lm_head, then qkv, o, gate/up, down of every layer (llm_mat_index)
    LlmLayout lo;               // byte offset of every item in blob / blob8 / blob12
    std::set<std::string> loaded;
    int expected = 0;
    int vocab_cap = 0;   // allocated rows of embed / lm_head (cfg.vocab at creation + 64 spare)
    char* blob8 = nullptr;   // fp8 copies + scales (decode weight stream halves; the 16-bit copies hold the dequantised values)
    bool fp8 = false;
    char* blob12 = nullptr;  // 12-bit copies (bf16 models): built once every tensor is loaded, rebuilt by every later weight write
    bool use12 = true;       // pgv_llm_set_weight_stream
    int generation = 0;      // bumped by every call that changes what a captured decode graph baked in (vocabulary size, weight pointers)
};
static const LlmMat& layer_mat(const pgv_llm* m, int layer, int kind) { return m->mats[llm_mat_index(layer, kind)]; }

// The fixed-address buffers one decode step works in (so a step can be captured into a hipGraph), one entry per ROW of the step: the cache's own
// (pgv_kv::sc: row b is slot b) or the row scratch of pgv_kv_set_lookup, whose rows are (slot, offset) pairs.
struct DecodeScratch {
    float* resid = nullptr; void *xn = nullptr, *qkv = nullptr, *ao = nullptr, *act = nullptr; float* logits = nullptr;
    float* amax_val = nullptr; int* amax_idx = nullptr;     // greedy candidates of the lm_head GEMV, tile-major: [ceil(rows / 16)][vocab_cap / 16][16]
    float* ssq = nullptr;                                   // sum-of-squares partials of the folded RMSNorm, tile-major: [ceil(rows / 16)][hidden / 16][16] (see GemvArgs in gemv.hip)
    int ssq_ts = 0, amax_ts = 0;                            // their tile strides in elements: hidden, vocab_cap
    void* k8_part = nullptr;                                // 8-phase residual producers (gemv.hip gemv_k8_kernel): phase tiles [hidden / 16][8][column tiles][64] float4
    float* dattn_part = nullptr; unsigned* dattn_ticket = nullptr;   // context-split decode attention: partial states [rows * heads][8][130], arrival tickets [rows * heads] (zero between launches)
};

// A device block its owner allocates on first use and frees with itself.  unit: 10 reports KiB, 20 MiB.
struct DevBlock {
    char* p = nullptr;
    DevBlock() = default; DevBlock(const DevBlock&) = delete;
    ~DevBlock() { drop(); }
    void drop() { if (p) (void)hipFree(p); p = nullptr; }
    int alloc(const char* who, size_t bytes, int unit = 10) {
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) { p = nullptr; pgv_set_error("%s: hipMalloc(%zu %s): %s", who, bytes >> unit, unit == 10 ? "KiB" : "MiB", hipGetErrorString(e)); return PGV_ENOMEM; }
        return PGV_OK;
    }
};
// A configuration that lives in device memory, outside any capture: a captured decode step bakes in its addresses and sizes, and the graphs' key
// carries gen (config_upload).  host: the words the device copy holds; gen: bumped by every call that changes the device copy
struct DevConfig { std::vector<int> host; int eos = -1; bool on = false; int gen = 0; };
// The id record of a cache: each slot's ids at their cache positions [B][max_seq], its prompt length [B] and the copy of the logits that the -inf
// processors of a pick write to [B][vocab_cap].  Shared by the bans, lookup and the automaton; the first of them allocates it (kv_ids_alloc).
struct KvIds { DevBlock blob; int *ids = nullptr, *plen = nullptr; float* logits = nullptr; };
// logit bans (pgv_kv_set_bans): the lists of the configuration, in the id record's block
struct KvBan : DevConfig { int* lists = nullptr; BanLists cfg; };
// constrained decoding (pgv_kv_set_allowed): the state record [B][max_seq] (indexed by cache position) and the roots [B], one allocation by the
// first configuration that asks; the device copy of the automaton (au binds it; cap words allocated), which grows with the configuration
struct KvAllow : DevConfig { DevBlock blob, dev; int *state = nullptr, *root = nullptr; size_t cap = 0; AllowAuto au; };
// classifier-free guidance (pgv_kv_set_guidance): slots [0, pairs) of a live group of 2 * pairs are conditional, slot pairs + p is the unconditional
// twin of p.  logits [B / 2][vocab] (row stride vocab) holds the guided rows the pick reads; allocated when guidance is first switched on.  pairs 0: off
struct KvGuide { DevBlock logits; int pairs = 0; float scale = 1.f; };
// pgv_kv_set_logprobs: the two log-probabilities of every pick.  stat [B][2] row statistics (row_lse_kernel), last [2][B] the values of each
// slot's latest pick (model | pick), hist [2][B][max_seq] those of the stepping calls, parallel to d_hist
struct KvLogprobs {
    bool on = false; float *stat = nullptr, *last = nullptr, *hist = nullptr;
    int steps = -1;                     // steps of the last pgv_llm_decode_greedy / _sample call that ran with the switch on (-1: it was off)
};
// beam search (pgv_beam_begin): one allocation on first use, sized for the cache's batch -- state words [B][PGV_BEAM_STATE_WORDS(8)], gather map [B],
// prompt lengths row0 [B], step counters t [B], the run parameters, the length-penalty table denom [max_seq] and the per-step history of tokens
// and parents, hist [2][max_seq][B]
struct KvBeam {
    DevBlock blob; unsigned* state = nullptr; int *map = nullptr, *row0 = nullptr, *t = nullptr, *hist = nullptr; BeamParams* prm = nullptr; float* denom = nullptr;
    std::vector<unsigned> stage;        // host staging of the initial state (kept alive across the async copy)
    int K = 0, P = 0, N = 0, steps = 0; // the current run (K 0: none): width K, prompts, token budget, picks done
};
// row-wise steps (pgv_kv_set_lookup): one allocation by the first call that asks -- a second DecodeScratch for up to `rows` rows that are
// (slot, offset) pairs, and the row maps (slot [rows] | j [rows])
struct KvLookup {
    DevBlock blob; DecodeScratch sc;
    int *slot = nullptr, *j = nullptr, rows = 0, D = 0, n = 0;
    std::vector<int> stage;             // host staging of the row maps / the budgets (kept alive across the async copy)
    // prompt-lookup steps (pgv_llm_decode_lookup): row tokens and row arg-max [rows], drafts and budget per slot [B], the run's step counter and the
    // emit counts [max_seq][B]
    int *tok = nullptr, *t = nullptr, *ndraft = nullptr, *budget = nullptr, *k = nullptr, *counts = nullptr;
    // their sampled form (pgv_llm_decode_lookup_sample): the uniform of every row [rows], tokens emitted before the call per slot [B] (behind budget)
    float* u = nullptr; int* ubase = nullptr;
    bool valid = false;                 // the id record holds exactly the ids behind cache rows [0, len) of every live slot (a plain prefill wrote it, only lookup steps since)
};
enum StepKind { STEP_PLAIN, STEP_LOOKUP, STEP_LOOKUP_SAMPLED, STEP_KINDS };      // what run_steps runs: token steps, prompt-lookup steps, their sampled form

struct pgv_kv {
    pgv_llm* llm;
    int B, max_seq;
    DevBlock blob;
    std::vector<void*> Kc, Vc;          // per layer [B][heads][max_seq][128]
    size_t plane_bytes = 0;             // Kc[0], Vc[0], Kc[1], ... sit this far apart in the blob (pgv_kv_fork covers them in one launch)
    DecodeScratch sc;
    int *d_pos, *d_cur, *d_step, *d_done, *d_hist;
    std::vector<int> h_len;
    std::vector<int> h_meta;           // staging for prefill row maps (kept alive across the async copy)
    int active = 0;                     // sequences of the last prefill
    // one decode step captured as a hipGraph (all kernel arguments are fixed device addresses; positions, current
    // tokens and step counters live in device memory and are advanced by the argmax kernel)
    hipGraphExec_t gexec[2] = {nullptr, nullptr};      // [0]: one token step, [1]: kGraphSteps consecutive steps
    DecodeGraphKey gkey;                // what they baked in
    bool warmed[STEP_KINDS] = {};       // a step of the kind has run eagerly (code objects loaded) before the first capture
    float* d_u = nullptr;               // uniforms of a sampled decode run: [max_seq][B], indexed by the device-side step counter
    PickParams warpers;                 // pgv_kv_set_warpers: the top_p and penalty every later pick on this cache runs with (the other fields stay neutral)
    PickParams run;                     // the current stepping run (AM_SAMPLE)
    unsigned* d_seen = nullptr;         // seen-set of every slot (repetition penalty): [B][seen_words] bitmaps over the vocabulary
    int seen_words = 0;
    KvIds ids; KvBan ban; KvAllow allow; KvGuide guide; KvLogprobs lp; KvBeam beam; KvLookup lookup;
};
// THE place that reads the switches off a cache (kv_features.h): the graph key and every cross-feature refusal go through this snapshot
static KvFeatures kv_features(const pgv_kv* kv) {
    KvFeatures f;
    f.logprobs = kv->lp.on; f.bans = kv->ban.on ? kv->ban.gen : 0; f.allowed = kv->allow.on ? kv->allow.gen : 0; f.guide_pairs = kv->guide.pairs; f.guide_scale = kv->guide.scale;
    f.lookup_D = kv->lookup.D; f.lookup_n = kv->lookup.n; f.beams = kv->beam.K; f.penalty = kv->warpers.penalty;
    return f;
}
// PGV_OK, or the first refusal the rule table holds for the call in the cache's state (a null cache: the caller's own check reports it)
static int kv_allows(const pgv_kv* kv, KvOp op, const char* who, int phase = 0, const char* verifies = "") {
    char msg[384];
    if (!kv || !kv_refusal(op, phase, kv_features(kv), who, verifies, msg, sizeof(msg))) return PGV_OK;
    pgv_set_error("%s", msg); return PGV_ESTATE;
}
// every call that changes what the slots of the live group hold ends a beam run
static void beam_drop(pgv_kv* kv) { kv->beam.K = 0; }

extern "C" int pgv_llm_create(pgv_ctx* ctx, const pgv_llm_config* cfg, int dtype, pgv_llm** out) {
    PGV_CHECK(ctx && cfg && out, "pgv_llm_create: null argument");
    PGV_CHECK(dtype == PGV_F16 || dtype == PGV_BF16, "pgv_llm_create: dtype must be PGV_F16 or PGV_BF16");
    PGV_CHECK(cfg->heads * kHD == cfg->hidden, "pgv_llm_create: head_dim must be 128 (hidden %d, heads %d)", cfg->hidden, cfg->heads);
    PGV_CHECK(cfg->hidden % 256 == 0, "pgv_llm_create: hidden must be a multiple of 256");
    PGV_CHECK(cfg->inter % 64 == 0, "pgv_llm_create: intermediate size must be a multiple of 64");
    PGV_CHECK(cfg->vocab > 0 && cfg->layers >= 0, "pgv_llm_create: bad vocab/layers");
    pgv_llm* m = new pgv_llm();
    m->ctx = ctx; m->cfg = *cfg; m->dtype = dtype;
    m->vocab_cap = (cfg->vocab + 64 + 15) / 16 * 16;   // lm_head is fragment-blocked: rows padded to 16 (zero rows)
    const size_t H = cfg->hidden, V = m->vocab_cap, L = cfg->layers;
    const LlmLayout& lo = m->lo = llm_layout({cfg->hidden, cfg->inter, m->vocab_cap, cfg->layers});
    hipError_t e = hipMalloc((void**)&m->blob, lo.total16);
    if (e != hipSuccess) { delete m; pgv_set_error("pgv_llm_create: hipMalloc(%zu MiB): %s", lo.total16 >> 20, hipGetErrorString(e)); return PGV_ENOMEM; }
    m->blob_bytes = lo.total16;
    (void)hipMemset(m->blob + lo.mat[0].w16, 0, V * H * 2);     // padded lm_head rows must be finite
    char* b = m->blob;
    m->embed = b + lo.embed; m->norm_g = (float*)(b + lo.norm_g); m->rope = (float*)(b + lo.rope);
    for (size_t i = 0; i < L; ++i) m->layers.push_back({(float*)(b + lo.in_g[i]), (float*)(b + lo.post_g[i])});
    for (const LlmMatSlot& x : lo.mat) m->mats.push_back({x.N, x.K, x.N, b + x.w16});
    m->mats[0].N = cfg->vocab;
    // RoPE table exactly as LlamaRotaryEmbedding (HF:llama/modeling_llama.py:96-126): fp32 inv_freq, fp32 angle, fp32 cos/sin
    std::vector<float> tab((size_t)kMaxPos * 64 * 2);
    for (int j = 0; j < 64; ++j) {
        const float inv = 1.0f / powf(cfg->rope_theta, (float)(2 * j) / (float)kHD);
        for (int p = 0; p < kMaxPos; ++p) {
            const float ang = (float)p * inv;
            tab[((size_t)p * 64 + j) * 2] = cosf(ang);
            tab[((size_t)p * 64 + j) * 2 + 1] = sinf(ang);
        }
    }
    e = hipMemcpy(m->rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(m->blob); delete m; pgv_set_error("pgv_llm_create: rope upload: %s", hipGetErrorString(e)); return PGV_EHIP; }
    m->expected = 3 + 9 * (int)L;
    *out = m;
    return PGV_OK;
}

extern "C" void pgv_llm_destroy(pgv_llm* llm) {
    if (!llm) return;
    if (llm->blob) (void)hipFree(llm->blob);
    if (llm->blob8) (void)hipFree(llm->blob8);
    if (llm->blob12) (void)hipFree(llm->blob12);
    delete llm;
}

extern "C" int pgv_llm_missing(const pgv_llm* llm) { return llm ? llm->expected - (int)llm->loaded.size() : -1; }

// ---------------------------------------------------------------------------------------------
// 12-bit decode copies (bf16 models, w12.h): what the decode GEMVs stream at batches of up to 16 sequences
// ---------------------------------------------------------------------------------------------
// (Re)build the 12-bit copy of matrix `only` of m->mats (the first time: of every matrix, once the model is complete; negative later: nothing).  A matrix
// with more than kW12MaxExc exceptions in a row block keeps its 16-bit stream.  Synchronous (model setup / weight loads, never inside a capture).
static int w12_sync(pgv_llm* m, int only, hipStream_t s) {
    if (m->dtype != PGV_BF16 || m->fp8 || pgv_llm_missing(m) != 0) return PGV_OK;
    if (m->blob12 && only < 0) return PGV_OK;
    if (!m->blob12) {
        only = -1;
        hipError_t e = hipMalloc((void**)&m->blob12, m->lo.total12);
        if (e != hipSuccess) { pgv_set_error("12-bit weight copies: hipMalloc(%zu MiB): %s", m->lo.total12 >> 20, hipGetErrorString(e)); return PGV_ENOMEM; }
    }
    std::vector<size_t> coff;     // first row block of every matrix in the exception counts
    size_t nrb = 0;
    for (const LlmMat& x : m->mats) { coff.push_back(nrb); nrb += x.cap / 16; }
    int* d_counts = nullptr;
    PGV_HIP(hipMalloc((void**)&d_counts, nrb * sizeof(int)));
    int rc = PGV_OK;
    for (size_t i = 0; i < m->mats.size(); ++i) {
        const LlmMat& x = m->mats[i];
        if ((only < 0 || (int)i == only) && rc == PGV_OK) rc = pgv_launch_encode_w12(x.w16, m->blob12 + m->lo.mat[i].w12, d_counts + coff[i], x.cap, x.K, s);
    }
    std::vector<int> counts(nrb, 0);
    hipError_t e = rc == PGV_OK ? hipMemcpyAsync(counts.data(), d_counts, nrb * sizeof(int), hipMemcpyDeviceToHost, s) : hipSuccess;
    if (e == hipSuccess && rc == PGV_OK) e = hipStreamSynchronize(s);
    (void)hipFree(d_counts);
    PGV_TRY(rc);
    if (e != hipSuccess) { pgv_set_error("12-bit weight copies: %s", hipGetErrorString(e)); return PGV_EHIP; }
    for (size_t i = 0; i < m->mats.size(); ++i) {
        LlmMat& x = m->mats[i];
        if (only >= 0 && (int)i != only) continue;
        int worst = 0;
        for (long long r = 0; r < x.cap / 16; ++r) worst = counts[coff[i] + r] > worst ? counts[coff[i] + r] : worst;
        x.z = {worst <= kW12MaxExc ? m->blob12 + m->lo.mat[i].w12 : nullptr, x.cap};
    }
    m->generation += 1;           // captured decode graphs stream the previous copies
    return PGV_OK;
}

static void w12_drop(pgv_llm* m) {
    if (m->blob12) (void)hipFree(m->blob12);
    m->blob12 = nullptr;
    for (LlmMat& x : m->mats) x.z = W12Ref{};
}

// the copy a decode GEMV streams for a matrix (null: its 16-bit / fp8 matrix)
static const W12Ref* z12(const pgv_llm* m, const W12Ref& r) { return (m->use12 && r.buf) ? &r : nullptr; }

extern "C" int pgv_llm_set_weight_stream(pgv_llm* m, int use12) {
    PGV_CHECK(m != nullptr && (use12 == 0 || use12 == 1), "pgv_llm_set_weight_stream: bad arguments");
    if (m->use12 != (use12 == 1)) { m->use12 = use12 == 1; m->generation += 1; }
    return PGV_OK;
}

extern "C" int64_t pgv_llm_weight_stream_bytes(const pgv_llm* m, int batch) {
    if (!m || batch < 1) return -1;
    double b = 0;
    GemvChoice c; c.ct = gemv_col_tiles(batch);       // (the 8-phase form at one column tile is fp8-only, choose_gemv: the format does not depend on it)
    for (const LlmMat& x : m->mats) {
        const long long N = (x.N + 15) / 16 * 16, K = x.K;        // the GEMVs stream whole 16-row blocks (only the lm_head's N is no multiple of 16)
        const int wf = gemv_weight_format(m->fp8, z12(m, x.z) != nullptr, c);
        if (wf == WF_FP8) b += (double)N * K + 4.0 * N;                                 // e4m3 + per-row fp32 scales
        else if (wf == WF_12) b += (double)pgv_w12_total_bytes(N, K);
        else b += 2.0 * N * K;
    }
    return (int64_t)b;
}
extern "C" int pgv_llm_vocab(const pgv_llm* llm) { return llm ? llm->cfg.vocab : -1; }

extern "C" int pgv_llm_resize_vocab(pgv_llm* m, int new_vocab, void* stream) {
    PGV_CHECK(m != nullptr, "pgv_llm_resize_vocab: null model");
    PGV_CHECK(new_vocab >= 1 && new_vocab <= m->vocab_cap, "pgv_llm_resize_vocab: %d outside [1,%d] (64 spare rows are allocated at creation)", new_vocab, m->vocab_cap);
    if (new_vocab == m->cfg.vocab) return PGV_OK;
    if (m->fp8) { pgv_set_error("pgv_llm_resize_vocab: the weights are already quantised to fp8; resize before pgv_llm_quantize_fp8"); return PGV_ESTATE; }
    const size_t H = m->cfg.hidden;
    if (new_vocab > m->cfg.vocab) {
        const size_t off = (size_t)m->cfg.vocab * H * 2, bytes = (size_t)(new_vocab - m->cfg.vocab) * H * 2;
        PGV_HIP(hipMemsetAsync((char*)m->embed + off, 0, bytes, (hipStream_t)stream));
        // lm_head is fragment-blocked (rows interleaved inside 1 KiB blocks): zero the new rows in place (a shrink followed by a
        // grow must not resurrect old rows)
        PGV_TRY(pgv_zero_rows_blocked(m->mats[0].w16, m->cfg.vocab, new_vocab - m->cfg.vocab, (long long)H, (hipStream_t)stream));
    }
    m->cfg.vocab = new_vocab; m->mats[0].N = new_vocab;
    PGV_TRY(w12_sync(m, 0, (hipStream_t)stream));
    m->generation += 1;           // captured decode graphs have the old vocabulary baked into lm_head / the token pick
    return PGV_OK;
}

extern "C" int pgv_llm_load_rows(pgv_llm* m, const char* name, const void* data, int src_dtype, int on_device, int row0, int nrows, int64_t numel, void* stream) {
    PGV_CHECK(m && name && data, "pgv_llm_load_rows: null argument");
    PGV_CHECK(row0 >= 0 && nrows >= 1 && row0 + nrows <= m->cfg.vocab, "pgv_llm_load_rows: rows [%d,%d) outside the vocabulary (%d)", row0, row0 + nrows, m->cfg.vocab);
    PGV_CHECK(numel == (int64_t)nrows * m->cfg.hidden, "pgv_llm_load_rows: size mismatch for '%s': %lld elements given for %d rows of %d", name, (long long)numel,
              nrows, m->cfg.hidden);
    if (m->fp8) { pgv_set_error("pgv_llm_load_rows: the weights are quantised to fp8 (the fp8 copies would go stale); load into a fresh model"); return PGV_ESTATE; }
    PackDst d;
    d.dst_dtype = m->dtype; d.rows = nrows; d.cols = m->cfg.hidden; d.dst_stride = d.cols; d.row_off = row0;
    if (!strcmp(name, "model.embed_tokens.weight")) d.ptr = m->embed;
    else if (!strcmp(name, "lm_head.weight")) { d.ptr = m->mats[0].w16; d.blocked = true; }
    else { pgv_set_error("pgv_llm_load_rows: '%s' is not a vocabulary matrix", name); return PGV_ENAME; }
    PGV_TRY(pgv_pack_tensor(d, data, src_dtype, on_device, (hipStream_t)stream));
    m->loaded.insert(name);
    return w12_sync(m, d.blocked ? 0 : -1, (hipStream_t)stream);
}

extern "C" int pgv_llm_load_tensor(pgv_llm* m, const char* name_in, const void* data, int src_dtype, int on_device, int64_t numel, void* stream) {
    PGV_CHECK(m && name_in && data, "pgv_llm_load_tensor: null argument");
    if (m->fp8) { pgv_set_error("pgv_llm_load_tensor: the weights are quantised to fp8 (the fp8 copies would go stale); load into a fresh model"); return PGV_ESTATE; }
    const long long H = m->cfg.hidden, I = m->cfg.inter, V = m->cfg.vocab;
    PackDst d;
    int idx = -1;            // the matrix of m->mats the tensor lands in (none: embed and the norm vectors)
    auto vec = [&](float* ptr, long long n) { d.ptr = ptr; d.rows = 1; d.cols = n; };
    auto mat = [&](void* ptr, long long r, long long c, long long roff) { d.ptr = ptr; d.dst_dtype = m->dtype; d.rows = r; d.cols = c; d.row_off = roff; };
    const LlmLayerKey k = llm_parse_layer_key(name_in, m->cfg.layers);
    if (!strcmp(name_in, "model.embed_tokens.weight")) mat(m->embed, V, H, 0);
    else if (!strcmp(name_in, "lm_head.weight")) { idx = 0; mat(m->mats[0].w16, V, H, 0); }
    else if (!strcmp(name_in, "model.norm.weight")) vec(m->norm_g, H);
    else if (k.status == LLM_KEY_BAD_INDEX) { pgv_set_error("pgv_llm_load_tensor: bad layer index in '%s'", name_in); return PGV_ENAME; }
    else if (k.status == LLM_KEY_MATRIX) {
        idx = llm_mat_index(k.layer, k.mat->kind);
        mat(m->mats[idx].w16, llm_dim(k.mat->rows, H, I), m->mats[idx].K, llm_dim(k.mat->row_off, H, I));
        d.row_blk = k.mat->row_blk; d.blk_stride = k.mat->blk_stride;
    } else if (!strcmp(k.rest, "input_layernorm.weight")) vec(m->layers[k.layer].in_g, H);
    else if (!strcmp(k.rest, "post_attention_layernorm.weight")) vec(m->layers[k.layer].post_g, H);
    else if (!strcmp(k.rest, "self_attn.rotary_emb.inv_freq")) return PGV_OK;
    else { pgv_set_error("pgv_llm_load_tensor: unexpected key '%s'", name_in); return PGV_ENAME; }
    d.blocked = idx >= 0;
    d.dst_stride = d.cols;
    PGV_CHECK(numel == d.rows * d.cols, "pgv_llm_load_tensor: size mismatch for '%s': %lld elements given, the model expects %lld x %lld", name_in,
              (long long)numel, d.rows, d.cols);
    PGV_TRY(pgv_pack_tensor(d, data, src_dtype, on_device, (hipStream_t)stream));
    m->loaded.insert(name_in);
    return w12_sync(m, idx, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// fp8 weight path (BASELINE config 5): quantise every decoder matrix + lm_head once, after loading
// ---------------------------------------------------------------------------------------------
extern "C" int pgv_llm_quantize_fp8(pgv_ctx* ctx, pgv_llm* m, void* stream) {
    PGV_CHECK(ctx && m, "pgv_llm_quantize_fp8: null argument");
    if (pgv_llm_missing(m) != 0) { pgv_set_error("pgv_llm_quantize_fp8: %d weight tensors not loaded", pgv_llm_missing(m)); return PGV_ESTATE; }
    if (m->fp8) return PGV_OK;
    PGV_CHECK(m->cfg.hidden % 64 == 0 && m->cfg.inter % 64 == 0, "pgv_llm_quantize_fp8: hidden and intermediate sizes must be multiples of 64");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMalloc((void**)&m->blob8, m->lo.total8);
    if (e != hipSuccess) { pgv_set_error("pgv_llm_quantize_fp8: hipMalloc(%zu MiB): %s", m->lo.total8 >> 20, hipGetErrorString(e)); return PGV_ENOMEM; }
    for (size_t i = 0; i < m->mats.size(); ++i) {
        LlmMat& x = m->mats[i];
        x.w8 = m->blob8 + m->lo.mat[i].w8; x.scale = (float*)(m->blob8 + m->lo.mat[i].scale);
        PGV_TRY(pgv_launch_quantize_fp8(m->dtype, x.w16, x.w8, x.scale, x.cap, x.K, s));
    }
    PGV_HIP(hipStreamSynchronize(s));
    w12_drop(m);                  // decode streams the fp8 copies
    m->fp8 = true;
    m->generation += 1;           // decode graphs captured before now stream the 16-bit matrices
    return PGV_OK;
}

extern "C" int pgv_llm_is_fp8(const pgv_llm* m) { return (m && m->fp8) ? 1 : 0; }

// Read one decoder matrix back as row-major fp32 [rows, cols] under its HF key (after quantisation: the dequantised values the
// whole path computes with) -- what a parity test or a checkpoint writer needs.
extern "C" int pgv_llm_get_weight(pgv_ctx* ctx, pgv_llm* m, const char* name_in, float* d_out, void* stream) {
    PGV_CHECK(ctx && m && name_in && d_out, "pgv_llm_get_weight: null argument");
    const long long H = m->cfg.hidden, I = m->cfg.inter;
    hipStream_t s = (hipStream_t)stream;
    const LlmMat& head = m->mats[0];        // its live rows of the allocated ones
    if (!strcmp(name_in, "lm_head.weight")) return pgv_launch_unpack_blocked(m->dtype, head.w16, d_out, head.cap, head.K, 0, 0, 0, head.N, s);
    const LlmLayerKey k = llm_parse_layer_key(name_in, m->cfg.layers);
    if (k.status == LLM_KEY_BAD_INDEX) { pgv_set_error("pgv_llm_get_weight: bad layer index in '%s'", name_in); return PGV_ENAME; }
    if (k.status != LLM_KEY_MATRIX) { pgv_set_error("pgv_llm_get_weight: unsupported key '%s'", name_in); return PGV_ENAME; }
    const LlmMat& x = layer_mat(m, k.layer, k.mat->kind);
    return pgv_launch_unpack_blocked(m->dtype, x.w16, d_out, x.N, x.K, k.mat->row_blk, k.mat->blk_stride, llm_dim(k.mat->row_off, H, I),
                                     llm_dim(k.mat->rows, H, I), s);
}

// ---------------------------------------------------------------------------------------------
// KV cache
// ---------------------------------------------------------------------------------------------
// The ONE list of what a decode step keeps per row (DecodeScratch), laid out for `rows` rows with the caller's `take`: the cache's own buffers
// (rows = its batch) and the row scratch of pgv_kv_set_lookup come from here.  CT = the column tiles the decode GEMVs run with at that width (1 / 2 /
// 4): every tile's slice of the side arrays is written, also the empty ones.
struct ScratchLayout { size_t resid, xn, qkv, ao, act, logits, ssq, av, ai, dpart, dtick, k8, xn_bytes, ssq_bytes, dtick_bytes; };
template <class Take>
static ScratchLayout scratch_layout(const pgv_llm* llm, size_t rows, Take&& take) {
    const size_t H = llm->cfg.hidden, I = llm->cfg.inter, V = llm->vocab_cap, heads = llm->cfg.heads, CT = gemv_col_tiles((int)rows);
    ScratchLayout o{};
    o.xn_bytes = CT * 16 * H * 2; o.ssq_bytes = CT * H * 4; o.dtick_bytes = rows * heads * 4;
    o.resid = take(rows * H * 4);
    o.xn = take(o.xn_bytes);            // row-major [rows][H] up to 8 rows, fragment-blocked [H / 32][CT][4][16][8] beyond (gv_xblk_offset)
    o.qkv = take(rows * 3 * H * 2); o.ao = take(rows * H * 2); o.act = take(rows * I * 2); o.logits = take(rows * V * 4);
    o.ssq = take(o.ssq_bytes); o.av = take(CT * V * 4); o.ai = take(CT * V * 4);
    o.dpart = take(rows * heads * (size_t)kDattnSplitMax * kDattnPart * 4); o.dtick = take(o.dtick_bytes);
    o.k8 = take(gemv_k8_part_bytes((int)(H / 16), (int)CT));
    return o;
}
static DecodeScratch scratch_bind(char* b, const ScratchLayout& o, const pgv_llm* llm) {
    DecodeScratch sc;
    sc.resid = (float*)(b + o.resid); sc.xn = b + o.xn; sc.qkv = b + o.qkv; sc.ao = b + o.ao; sc.act = b + o.act; sc.logits = (float*)(b + o.logits);
    sc.ssq = (float*)(b + o.ssq); sc.amax_val = (float*)(b + o.av); sc.amax_idx = (int*)(b + o.ai); sc.ssq_ts = llm->cfg.hidden; sc.amax_ts = llm->vocab_cap;
    sc.dattn_part = (float*)(b + o.dpart); sc.dattn_ticket = (unsigned*)(b + o.dtick); sc.k8_part = b + o.k8;
    return sc;
}
// tickets armed at 0; the xn columns / ssq partials of absent rows are read (never stored): finite
static hipError_t scratch_clear(const DecodeScratch& sc, const ScratchLayout& o) {
    hipError_t e = hipMemset(sc.dattn_ticket, 0, o.dtick_bytes);
    if (e == hipSuccess) e = hipMemset(sc.ssq, 0, o.ssq_bytes);
    if (e == hipSuccess) e = hipMemset(sc.xn, 0, o.xn_bytes);
    return e;
}

extern "C" int pgv_kv_create(pgv_ctx* ctx, pgv_llm* llm, int batch, int max_seq, pgv_kv** out) {
    PGV_CHECK(ctx && llm && out, "pgv_kv_create: null argument");
    PGV_CHECK(batch >= 1 && batch <= kMaxBatch, "pgv_kv_create: batch %d outside [1,%d] (the decode GEMVs tile up to 4 x 16 sequences)", batch, kMaxBatch);
    PGV_CHECK(max_seq >= 1 && max_seq <= kMaxPos, "pgv_kv_create: max_seq %d outside [1,%d]", max_seq, kMaxPos);
    pgv_kv* kv = new pgv_kv();
    kv->llm = llm; kv->B = batch; kv->max_seq = max_seq;
    const size_t V = llm->vocab_cap, L = llm->cfg.layers, B = batch;
    const size_t per = pgv_align(B * llm->cfg.heads * (size_t)max_seq * kHD * 2);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += pgv_align(bytes); return o; };
    const size_t o_cache = take(per * 2 * L);
    const ScratchLayout so = scratch_layout(llm, B, take);
    const size_t o_ints = take((4 * B + B * (size_t)max_seq) * 4), o_u = take(B * (size_t)max_seq * 4);
    kv->seen_words = (int)(V / 32);                          // vocab_cap is a multiple of 16: round up
    if ((size_t)kv->seen_words * 32 < V) kv->seen_words += 1;
    const size_t o_seen = take(B * (size_t)kv->seen_words * 4);
    const size_t n_lp = 4 * B + 2 * B * (size_t)max_seq, o_lp = take(n_lp * 4);
    if (kv->blob.alloc("pgv_kv_create", off, 20) != PGV_OK) { delete kv; return PGV_ENOMEM; }
    char* b = kv->blob.p;
    for (size_t i = 0; i < L; ++i) { kv->Kc.push_back(b + o_cache + per * 2 * i); kv->Vc.push_back(b + o_cache + per * (2 * i + 1)); }
    kv->plane_bytes = per;
    kv->sc = scratch_bind(b, so, llm);
    int* ints = (int*)(b + o_ints);
    kv->d_pos = ints; kv->d_cur = ints + B; kv->d_step = ints + 2 * B; kv->d_done = ints + 3 * B; kv->d_hist = ints + 4 * B;
    kv->d_u = (float*)(b + o_u);
    kv->d_seen = (unsigned*)(b + o_seen);
    kv->lp.stat = (float*)(b + o_lp); kv->lp.last = kv->lp.stat + 2 * B; kv->lp.hist = kv->lp.last + 2 * B;
    hipError_t e = hipMemset(ints, 0, (4 * B + B * (size_t)max_seq) * 4);
    if (e == hipSuccess) e = hipMemset(kv->d_seen, 0, B * (size_t)kv->seen_words * 4);
    if (e == hipSuccess) e = hipMemset(kv->lp.stat, 0, n_lp * 4);
    if (e == hipSuccess) e = scratch_clear(kv->sc, so);
    if (e != hipSuccess) { delete kv; pgv_set_error("pgv_kv_create: memset: %s", hipGetErrorString(e)); return PGV_EHIP; }
    kv->h_len.assign(batch, 0);
    *out = kv;
    return PGV_OK;
}

extern "C" void pgv_kv_destroy(pgv_kv* kv) {
    if (!kv) return;
    for (auto g : kv->gexec) if (g) (void)hipGraphExecDestroy(g);
    delete kv;                          // every device block is freed by its owner (DevBlock)
}

extern "C" int pgv_kv_set_warpers(pgv_kv* kv, float top_p, float repetition_penalty) {
    PGV_CHECK(kv != nullptr, "pgv_kv_set_warpers: null cache");
    PGV_TRY(pgv_check_warpers("pgv_kv_set_warpers", top_p, repetition_penalty));
    kv->warpers.top_p = top_p; kv->warpers.penalty = repetition_penalty;
    return PGV_OK;
}

// The id record of a cache -- each slot's ids at their cache positions [B][max_seq] and its prompt length [B] -- with the ban lists and the banned
// logits copy behind it: one allocation by the first configuration that needs the record (pgv_kv_set_bans, pgv_kv_set_lookup)
constexpr size_t kBanListWords = PGV_BAN_MAX_IDS + PGV_BAN_MAX_WORDS + 1;
static int kv_ids_alloc(pgv_kv* kv, const char* who) {
    if (kv->ids.blob.p) return PGV_OK;
    const size_t B = kv->B;
    const size_t b_ids = pgv_align(B * kv->max_seq * 4), b_plen = pgv_align(B * 4), b_lists = pgv_align(kBanListWords * 4),
                 b_logits = pgv_align(B * (size_t)kv->llm->vocab_cap * 4);
    PGV_TRY(kv->ids.blob.alloc(who, b_ids + b_plen + b_lists + b_logits));
    char* b = kv->ids.blob.p;
    kv->ids.ids = (int*)b; kv->ids.plen = (int*)(b + b_ids); kv->ban.lists = (int*)(b + b_ids + b_plen); kv->ids.logits = (float*)(b + b_ids + b_plen + b_lists);
    PGV_HIP(hipMemset(b, 0, b_ids + b_plen + b_lists));
    return PGV_OK;
}

// HF's four filter warpers behind top-p (pgv.h): stored next to top_p and the penalty, read by every later sampled pick (kv_sampled)
extern "C" int pgv_kv_set_filters(pgv_kv* kv, const pgv_filter_config* cfg) {
    PGV_CHECK(kv != nullptr, "pgv_kv_set_filters: null cache");
    const pgv_filter_config off{0.f, 1.f, 0.f, 0.f};
    const pgv_filter_config& c = cfg ? *cfg : off;
    PGV_TRY(pgv_check_filters("pgv_kv_set_filters", c.min_p, c.typical_p, c.epsilon_cutoff, c.eta_cutoff));
    kv->warpers.min_p = c.min_p; kv->warpers.typical_p = c.typical_p; kv->warpers.epsilon = c.epsilon_cutoff; kv->warpers.eta = c.eta_cutoff;
    return PGV_OK;
}

// The upload protocol of a device-resident configuration.  The one the device copy already holds (a caller that sets and clears it around every
// run): nothing to upload, the graphs stay valid.  Anything else waits for the picks that may still read the copy before (sync; false: the caller
// has waited), uploads, and moves the counter in the graphs' key.
template <class Upload>
static int config_upload(DevConfig& c, std::vector<int>& words, int eos, bool same_shape, bool sync, Upload&& upload) {
    if (c.gen > 0 && same_shape && eos == c.eos && words == c.host) return PGV_OK;
    if (sync) PGV_HIP(hipDeviceSynchronize());
    PGV_TRY(upload());
    c.host.swap(words); c.eos = eos; c.gen += 1;
    return PGV_OK;
}

// HF's -inf processors (pgv.h): the lists are a DevConfig of the cache.
extern "C" int pgv_kv_set_bans(pgv_kv* kv, const pgv_ban_config* cfg) {
    PGV_CHECK(kv != nullptr, "pgv_kv_set_bans: null cache");
    if (!cfg) { kv->ban.on = false; return PGV_OK; }
    std::vector<int> blob;
    BanPacked at;
    PGV_TRY(pgv_ban_pack("pgv_kv_set_bans", cfg, kv->llm->cfg.vocab, blob, at));
    PGV_CHECK(cfg->eos_id < kv->llm->cfg.vocab, "pgv_kv_set_bans: eos_id %d outside the vocabulary (%d)", cfg->eos_id, kv->llm->cfg.vocab);
    if (pgv_ban_neutral(cfg, cfg->eos_id)) { kv->ban.on = false; return PGV_OK; }
    const size_t n_lists = kBanListWords;
    PGV_TRY(kv_ids_alloc(kv, "pgv_kv_set_bans"));
    PGV_CHECK(blob.size() <= n_lists, "pgv_kv_set_bans: %zu list words exceed the %zu reserved", blob.size(), n_lists);
    const BanLists& o = kv->ban.cfg;
    const BanLists& n = at.cfg;
    const bool same = n.ngram == o.ngram && n.n_sup == o.n_sup && n.n_beg == o.n_beg && n.n_words == o.n_words && n.min_length == o.min_length && n.min_new == o.min_new;
    PGV_TRY(config_upload(kv->ban, blob, cfg->eos_id, same, true, [&]() -> int {
        PGV_HIP(hipMemcpy(kv->ban.lists, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
        kv->ban.cfg = ban_lists(at, kv->ban.lists); return PGV_OK;
    }));
    kv->ban.on = true;
    return PGV_OK;
}

// `n` entries of slot `slot` of a per-slot record [B][max_seq] and the slot's word of `one` [B], device to device
static int record_peek(pgv_kv* kv, const char* who, const char* what, const char* by, const int* rec, const int* one, int slot, int n, int32_t* d_out, int32_t* d_one, void* stream) {
    PGV_CHECK(kv != nullptr, "%s: null cache", who);
    if (!rec) { pgv_set_error("%s: this cache has no %s record (%s allocates it)", who, what, by); return PGV_ESTATE; }
    PGV_CHECK(slot >= 0 && slot < kv->B, "%s: slot %d outside the %d of the cache", who, slot, kv->B);
    PGV_CHECK(n >= 0 && n <= kv->max_seq, "%s: %d entries outside the cache's %d", who, n, kv->max_seq);
    if (d_out && n > 0) PGV_HIP(hipMemcpyAsync(d_out, rec + (size_t)slot * kv->max_seq, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d_one) PGV_HIP(hipMemcpyAsync(d_one, one + slot, 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PGV_OK;
}
extern "C" int pgv_kv_ids_peek(pgv_kv* kv, int slot, int n, int32_t* d_out, int32_t* d_prompt_len, void* stream) {
    return record_peek(kv, "pgv_kv_ids_peek", "id", "pgv_kv_set_bans", kv ? kv->ids.ids : nullptr, kv ? kv->ids.plen : nullptr, slot, n, d_out, d_prompt_len, stream);
}

// Constrained decoding (pgv.h): the automaton is a DevConfig of the cache, as the ban lists are.  The roots are per-slot state (pgv_kv_fork and the
// refills move them), so they are written by every call that switches the feature on.
extern "C" int pgv_kv_set_allowed(pgv_kv* kv, const pgv_allow_config* cfg) {
    PGV_CHECK(kv != nullptr, "pgv_kv_set_allowed: null cache");
    if (!cfg) { kv->allow.on = false; return PGV_OK; }
    PGV_TRY(pgv_allow_check("pgv_kv_set_allowed", cfg, kv->llm->cfg.vocab, kv->B));
    PGV_TRY(kv_allows(kv, KV_SET_ALLOWED, "pgv_kv_set_allowed"));
    PGV_TRY(kv_ids_alloc(kv, "pgv_kv_set_allowed"));          // the prompt lengths and the pick's copy of the logits
    const size_t B = kv->B;
    KvAllow& al = kv->allow;
    if (!al.blob.p) {
        const size_t b_state = pgv_align(B * kv->max_seq * 4), b_root = pgv_align(B * 4);
        PGV_TRY(al.blob.alloc("pgv_kv_set_allowed", b_state + b_root));
        al.state = (int*)al.blob.p; al.root = (int*)(al.blob.p + b_state);
        PGV_HIP(hipMemset(al.blob.p, 0xff, b_state));         // DEAD until a step stores a state
    }
    std::vector<int> blob;
    pgv_allow_pack(cfg, blob);
    PGV_HIP(hipDeviceSynchronize());              // a pick not yet done may still read the automaton and the roots of the configuration before
    PGV_TRY(config_upload(al, blob, cfg->eos_id, cfg->n_states == al.au.n_states && cfg->n_edges == al.au.n_edges, false, [&]() -> int {
        if (blob.size() > al.cap) {
            al.dev.drop();
            al.cap = 0; al.host.clear();          // (the counter moves behind this: graphs that baked the old address in never match again)
            if (al.dev.alloc("pgv_kv_set_allowed", blob.size() * 4) != PGV_OK) { al.on = false; return PGV_ENOMEM; }
            al.cap = blob.size();
        }
        PGV_HIP(hipMemcpy(al.dev.p, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
        al.au = allow_auto((const int*)al.dev.p, cfg->n_states, cfg->n_edges); return PGV_OK;
    }));
    std::vector<int> roots(B, 0);
    for (size_t b = 0; cfg->h_roots && b < B; ++b) roots[b] = cfg->h_roots[b];
    PGV_HIP(hipMemcpy(al.root, roots.data(), B * 4, hipMemcpyHostToDevice));
    al.on = true;
    return PGV_OK;
}
extern "C" int pgv_kv_allow_peek(pgv_kv* kv, int slot, int n, int32_t* d_out, int32_t* d_root, void* stream) {
    return record_peek(kv, "pgv_kv_allow_peek", "state", "pgv_kv_set_allowed", kv ? kv->allow.state : nullptr, kv ? kv->allow.root : nullptr, slot, n, d_out, d_root, stream);
}

// a sampled pick on this cache: the caller's temperature and top_k, the cache's warpers
static PickParams kv_sampled(const pgv_kv* kv, float temperature, int top_k) {
    PickParams p = kv->warpers;         // top_p, penalty and the filter tail (pgv_kv_set_filters)
    p.temperature = temperature; p.top_k = top_k; p.greedy = false;
    return p;
}

extern "C" int pgv_kv_set_logprobs(pgv_kv* kv, int on) {
    PGV_CHECK(kv != nullptr, "pgv_kv_set_logprobs: null cache");
    if (on) PGV_TRY(kv_allows(kv, KV_SET_LOGPROBS, "pgv_kv_set_logprobs"));
    if (kv->lp.on != (on != 0)) { kv->lp.on = on != 0; kv->lp.steps = -1; }
    return PGV_OK;
}

// Classifier-free guidance (pgv.h).  Nothing is copied: the next covered pick reads the two values, and the decode graphs' key carries them.
extern "C" int pgv_kv_set_guidance(pgv_kv* kv, float scale, int pairs) {
    PGV_CHECK(kv != nullptr, "pgv_kv_set_guidance: null cache");
    PGV_CHECK(scale == scale && scale - scale == 0.f, "pgv_kv_set_guidance: scale %g is not finite", (double)scale);
    PGV_CHECK(pairs >= 0 && 2 * (long long)pairs <= kv->B, "pgv_kv_set_guidance: %d pairs need %lld slots, outside the cache's %d", pairs, 2 * (long long)pairs, kv->B);
    if (pairs == 0 || scale == 1.f) { kv->guide.pairs = 0; kv->guide.scale = 1.f; return PGV_OK; }
    PGV_TRY(kv_allows(kv, KV_SET_GUIDANCE, "pgv_kv_set_guidance"));
    if (!kv->guide.logits.p) PGV_TRY(kv->guide.logits.alloc("pgv_kv_set_guidance", (size_t)(kv->B / 2) * kv->llm->vocab_cap * 4));
    kv->guide.pairs = pairs; kv->guide.scale = scale;
    return PGV_OK;
}
extern "C" int pgv_kv_guidance(const pgv_kv* kv) { return kv ? kv->guide.pairs : -1; }
// a covered call under guidance needs the live group to be exactly the pairs; a call that guidance does not cover is refused outright (kv_features.h)
static int guidance_width(const pgv_kv* kv, const char* who) {
    if (kv->guide.pairs > 0 && kv->active != 2 * kv->guide.pairs) {
        pgv_set_error("%s: guidance is on for %d pairs, the live group has %d sequences (need %d)", who, kv->guide.pairs, kv->active, 2 * kv->guide.pairs);
        return PGV_ESTATE;
    }
    return PGV_OK;
}

extern "C" int pgv_kv_logprobs_last(pgv_kv* kv, float* d_model, float* d_pick, void* stream) {
    PGV_CHECK(kv != nullptr, "pgv_kv_logprobs_last: null cache");
    if (!kv->lp.on || kv->active < 1) { pgv_set_error("pgv_kv_logprobs_last: %s", kv->lp.on ? "no prefilled sequences in this cache" : "pgv_kv_set_logprobs is off"); return PGV_ESTATE; }
    if (d_model) PGV_HIP(hipMemcpyAsync(d_model, kv->lp.last, (size_t)kv->active * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d_pick) PGV_HIP(hipMemcpyAsync(d_pick, kv->lp.last + kv->B, (size_t)kv->active * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PGV_OK;
}

extern "C" int pgv_kv_logprobs_steps(pgv_kv* kv, int n, float* d_model, float* d_pick, void* stream) {
    PGV_CHECK(kv != nullptr, "pgv_kv_logprobs_steps: null cache");
    if (!kv->lp.on || kv->lp.steps < 0) { pgv_set_error("pgv_kv_logprobs_steps: pgv_kv_set_logprobs was off during the last pgv_llm_decode_greedy / _sample call"); return PGV_ESTATE; }
    PGV_CHECK(n >= 1 && n <= kv->lp.steps, "pgv_kv_logprobs_steps: %d steps asked for, the last call ran %d", n, kv->lp.steps);
    const size_t row = (size_t)kv->max_seq * 4;
    if (d_model) PGV_HIP(hipMemcpy2DAsync(d_model, (size_t)n * 4, kv->lp.hist, row, (size_t)n * 4, kv->active, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d_pick)
        PGV_HIP(hipMemcpy2DAsync(d_pick, (size_t)n * 4, kv->lp.hist + (size_t)kv->B * kv->max_seq, row, (size_t)n * 4, kv->active, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PGV_OK;
}

extern "C" int pgv_kv_len(const pgv_kv* kv, int b) { return (kv && b >= 0 && b < kv->B) ? kv->h_len[b] : -1; }

// ---------------------------------------------------------------------------------------------
// shared tail: final norm + lm_head + argmax on kv->sc.resid [B,H]
// ---------------------------------------------------------------------------------------------
// kv->sc.xn holds round16(resid * norm_g) and kv->sc.ssq the `nparts` sum-of-squares partials of resid (folded final RMSNorm): lm_head scales its
// fp32 accumulators by rstd.
// PGV_LLM_NORM_FOLD=0: decode with a standalone RMSNorm launch in front of every consumer GEMV (HF's order of operations: normalise, round
// to 16 bits, multiply) instead of the folded form -- a bisect switch for real-checkpoint regressions, not a fallback: both paths
// are tested against the same goldens (tests/test_gpu_llm.py::test_unfolded_decoder_path_matches_goldens).
static bool norm_fold_enabled() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("PGV_LLM_NORM_FOLD"); v = (e && e[0] == '0') ? 0 : 1; }
    return v == 1;
}

// One decode GEMV over a matrix, streaming the copy decode reads: the fp8 codes once quantised (weight-only form: 16-bit x, e4m3 codes
// widened in registers; gemv.hip), else the 12-bit copy where there is one, else the 16-bit matrix.  x is [B][K].
static int gemv_mat(pgv_ctx* ctx, const pgv_llm* m, int mode, const LlmMat& w, const void* x, void* out, int ldo, int B, hipStream_t s, const GemvNorm* nm) {
    return pgv_launch_gemv(ctx, m->dtype, mode, m->fp8 ? w.w8 : w.w16, x, (int)w.K, out, ldo, (int)w.N, (int)w.K, B, s, m->fp8 ? w.scale : nullptr, nm, z12(m, w.z));
}

// lm_head GEMV on sc.xn (B rows) -> sc.logits and, for a greedy pick, the per-workgroup argmax candidates
static int lm_head_rows(pgv_ctx* ctx, pgv_llm* m, const DecodeScratch& sc, int B, bool greedy, hipStream_t s, int nparts) {
    const int H = m->cfg.hidden, V = m->cfg.vocab;
    GemvNorm nm; nm.ssq_in = nparts > 0 ? sc.ssq : nullptr; nm.nparts_in = nparts; nm.hidden = H; nm.eps = m->cfg.eps;     // nparts 0: sc.xn is already normalised
    nm.ssq_ts = sc.ssq_ts; nm.amax_ts = sc.amax_ts;
    nm.x_blocked = nparts > 0;                       // the folded path hands sc.xn over blocked at batches beyond 16 (pgv_gemv_xblk_tiles)
    if (greedy) { nm.amax_val = sc.amax_val; nm.amax_idx = sc.amax_idx; }
    return gemv_mat(ctx, m, GV_F32, m->mats[0], sc.xn, sc.logits, V, B, s, &nm);
}
static int lm_head(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int B, bool greedy, hipStream_t s, int nparts) { return lm_head_rows(ctx, m, kv->sc, B, greedy, s, nparts); }

// Every pick on rows [0, B) of kv->sc.logits.  `sampled` null: the arg-max of the candidates lm_head left; else the sampled pick with those parameters
// and the uniforms u [B], or u [steps][B] indexed by the device-side step counter (u_by_step).  `st`: the cache's own state (kv_state) or a refill's
// scratch.  Row b reads the seen-set of slot slot_map[b] (null: b) and, with pgv_kv_set_logprobs on, records its log-probabilities there.
static PickState kv_state(pgv_kv* kv, int eos, int advance) { return {kv->d_cur, kv->d_pos, kv->d_step, kv->d_hist, kv->max_seq, kv->d_done, eos, advance}; }
// With pgv_kv_set_bans on, a sampled pick (the greedy ones take that route then, kv_greedy_sampled) reads a copy of the logits with HF's -inf
// processors applied, made by logit_ban_kernel behind the row statistics: kv->sc.logits itself stays raw for the statistics, a re-pick, a fork and the
// d_logits outputs.  Row b's sequence is the record of its slot at length ban_lens[b] (null: the cache's positions) -- plus, for the pick of a decode
// step (AM_INC_POS), the token that step consumed, which the kernel appends to the record.
// With pgv_kv_set_allowed on, logit_allow_kernel makes that copy -- the row with -inf outside what the slot's automaton state allows, the state
// advanced by the token the step consumed -- and logit_ban_kernel, where bans are on too, runs in place behind it: the union of the two -inf sets.
// With only bans on, the ban kernel's launch is the one it has always been.
static bool kv_greedy_sampled(const pgv_kv* kv) { return kv->warpers.penalty != 1.f || kv->ban.on || kv->guide.pairs > 0 || kv->allow.on; }
static int kv_pick(pgv_kv* kv, int B, const PickParams* sampled, const float* u, bool u_by_step, const PickState& st, const int* slot_map, hipStream_t s,
                   const int* ban_lens = nullptr) {
    const int V = kv->llm->cfg.vocab;
    PickLp lp;
    if (kv->lp.on) {
        lp.stat = kv->lp.stat; lp.last_model = kv->lp.last; lp.last_pick = kv->lp.last + kv->B; lp.slot = slot_map;
        if (st.advance & AM_RECORD) { lp.hist_model = kv->lp.hist; lp.hist_pick = kv->lp.hist + (size_t)kv->B * kv->max_seq; lp.hist_stride = kv->max_seq; }
        PGV_TRY(pgv_launch_row_lse(kv->sc.logits, V, V, B, kv->lp.stat, s));
    }
    if (!sampled) return pgv_launch_argmax_parts(kv->sc.amax_val, kv->sc.amax_idx, (V + 15) / 16, kv->sc.amax_ts, V, B, st, s, kv->sc.logits, &lp);
    const float* logits = kv->sc.logits;
    // Guidance: the B = 2P rows of the group become P guided rows -- scale * (log_softmax(row p) - log_softmax(row P + p)) + log_softmax(row P + p) --
    // in a buffer of their own (kv->sc.logits stays raw); bans, penalty and pick run over those P rows with the conditional slots' records and
    // seen-sets, the uniforms keep the group's width as their stride, and the follow kernel hands the outcome to the twins.
    const int P = (kv->guide.pairs > 0 && !slot_map) ? kv->guide.pairs : 0, rows = P > 0 ? P : B;
    if (P > 0) {
        PGV_CHECK(B == 2 * P && st.next == kv->d_cur, "kv_pick: a guided pick runs on the cache's own state at width 2 x pairs");
        PGV_TRY(pgv_launch_guidance_mix(kv->sc.logits, kv->sc.logits + (size_t)P * V, V, V, P, kv->guide.scale, (float*)kv->guide.logits.p, V, s));
        logits = (const float*)kv->guide.logits.p;
    }
    if (kv->allow.on) {
        AllowArgs a;
        a.src = logits; a.dst = kv->ids.logits; a.V = V;
        a.au = kv->allow.au; a.state = kv->allow.state; a.state_stride = kv->max_seq; a.root = kv->allow.root;
        a.slot_map = slot_map; a.lens = ban_lens ? ban_lens : kv->d_pos; a.prompt_lens = kv->ids.plen;
        a.cur = kv->d_cur; a.inc = (st.advance & AM_INC_POS) ? 1 : 0;
        a.done = (st.advance & AM_RECORD) ? st.done : nullptr;       // as for the bans below
        a.eos = kv->allow.eos;
        PGV_TRY(pgv_launch_logit_allow(a, rows, s));
        logits = kv->ids.logits; lp.banned = 1;
    }
    if (kv->ban.on) {
        BanArgs a;
        a.src = logits; a.dst = kv->ids.logits; a.V = V;
        a.ids = kv->ids.ids; a.ids_stride = kv->max_seq; a.slot_map = slot_map; a.lens = ban_lens ? ban_lens : kv->d_pos; a.prompt_lens = kv->ids.plen;
        a.rec = kv->ids.ids; a.cur = kv->d_cur; a.inc = (st.advance & AM_INC_POS) ? 1 : 0;
        a.done = (st.advance & AM_RECORD) ? st.done : nullptr;       // a pick that does not record must not look at a flag an earlier run left set
        a.eos = kv->ban.eos; a.cfg = kv->ban.cfg;
        PGV_TRY(pgv_launch_logit_ban(a, rows, s));
        logits = kv->ids.logits; lp.banned = 1;
    }
    SampleWarp w;
    w.seen_bits = kv->d_seen; w.seen_words = kv->seen_words; w.seen_slot = slot_map;
    PGV_TRY(pgv_launch_sample(logits, V, rows, *sampled, u, B, u_by_step, st, s, &w, &lp));
    return P > 0 ? pgv_launch_guidance_follow(P, st, s) : PGV_OK;
}

// The pick of a beam step on the logits of rows [0, P * K): row statistics, the beam pick (token -> d_cur, parent -> the gather map, both into the
// history; `advance`: d_pos += 1), then the in-group gather of the cache rows generated since the fork.  K == 1 has nothing to gather.
static KvGatherArgs kv_gather_args(pgv_kv* kv, int K, int groups, const int* map, const int* row0, int* cur) {
    const pgv_llm* m = kv->llm;
    const int heads = m->cfg.heads, L = m->cfg.layers;
    KvGatherArgs g{};
    g.cache = L > 0 ? (char*)kv->Kc[0] : kv->blob.p;
    g.head_stride = (size_t)kv->max_seq * kHD * 2; g.slot_stride = g.head_stride * heads; g.plane_stride = kv->plane_bytes;
    g.heads = heads; g.nrun = 2 * L * heads; g.K = K; g.groups = groups; g.max_seq = kv->max_seq;
    g.map = map; g.row0 = row0; g.len = kv->d_pos; g.cur = cur;
    return g;
}
static int beam_pick_and_gather(pgv_ctx* ctx, pgv_kv* kv, bool advance, hipStream_t s) {
    const int V = kv->llm->cfg.vocab, K = kv->beam.K, P = kv->beam.P;
    pgv_prof_begin(ctx, 6, s);
    PGV_TRY(pgv_launch_row_lse(kv->sc.logits, V, V, P * K, kv->lp.stat, s));
    BeamPickArgs a{};
    a.logits = kv->sc.logits; a.ld = V; a.V = V; a.K = K; a.stat = kv->lp.stat;
    a.state = kv->beam.state; a.state_stride = PGV_BEAM_STATE_WORDS(K);
    a.t_dev = kv->beam.t; a.prm_dev = kv->beam.prm; a.denom = kv->beam.denom;
    a.cur = kv->d_cur; a.map = kv->beam.map; a.pos = kv->d_pos; a.advance = advance ? 1 : 0;
    a.hist_tok = kv->beam.hist; a.hist_par = kv->beam.hist + (size_t)kv->max_seq * kv->B; a.hist_stride = kv->B; a.hist_steps = kv->max_seq;
    PGV_TRY(pgv_launch_beam_pick(a, P, s));
    pgv_prof_end(ctx, 6, s, 0.0, 0.0);
    if (K > 1 && advance) {
        pgv_prof_begin(ctx, 5, s);
        PGV_TRY(pgv_launch_kv_gather(kv_gather_args(kv, K, P, kv->beam.map, kv->beam.row0, nullptr), s));
        pgv_prof_end(ctx, 5, s, 0.0, 0.0);
    }
    return PGV_OK;
}

static int lm_head_and_pick(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int B, int eos, int flags, hipStream_t s, int nparts) {
    if (flags & AM_BEAM) {
        PGV_TRY(lm_head(ctx, m, kv, B, false, s, nparts));
        return beam_pick_and_gather(ctx, kv, true, s);
    }
    const bool sampled = flags & AM_SAMPLE;
    PGV_TRY(lm_head(ctx, m, kv, B, !sampled, s, nparts));
    pgv_prof_begin(ctx, 6, s);
    PGV_TRY(kv_pick(kv, B, sampled ? &kv->run : nullptr, kv->d_u, true, kv_state(kv, eos, flags & (AM_INC_POS | AM_RECORD)), nullptr, s));
    pgv_prof_end(ctx, 6, s, 0.0, 0.0);
    return PGV_OK;
}

// ---------------------------------------------------------------------------------------------
// prefill
// ---------------------------------------------------------------------------------------------
// `append`: the rows continue the sequences already in the cache (row p of sequence b sits at position h_len[b] + p and attends to the cached
// prefix as well): VideoChatGPTLlamaForCausalLM.forward with past_key_values and input_ids.shape[1] > 1 (video_chatgpt/model/video_chatgpt.py:193-251;
// the splice still runs when the new ids carry a placeholder run, :103).  Same kernels, same per-row arithmetic: an appended row is bitwise the
// row of one full prefill over prefix + new tokens.
// `h_slots` (pgv_llm_prefill_slots): sequence b of the call is a NEW prompt for cache slot h_slots[b] of the live group; the other slots keep their
// cache rows, lengths, current tokens and flags.  The new rows run through the same kernels (the slot only redirects the cache rows they write and
// read), the pick (`pick`, d_u: as kv_pick takes them; pick->greedy: zeroed uniforms) lands in rows [0, B) of the scratch and is scattered to the slots.
// `h_counts` (pgv_llm_prefill_slots_n): sequence b of the call is answered h_counts[b] times and h_slots lists one slot per SAMPLE, those of sequence 0
// first.  The trunk runs over the sequences' rows once and writes the first slot of every run; kv_fork_list copies those cache rows to the run's other
// slots; the tail (last-row gather, final norm, lm_head, pick, scatter) and seen_mark run per sample, sample j on the last row / the ids of its
// sequence -- bit for bit what PREFILL_SLOTS leaves for the sequences repeated.
// `score` (pgv_llm_score): a plain prefill with a scoring tail.  The rows with a target go, PGV_SCORE_CHUNK_ROWS at a time, through the final norm
// and the lm_head GEMM of the d_all_logits branch into a workspace buffer (so their logits are bit for bit that branch's: the GEMM has one tile
// shape and no split-K, a row does not depend on M), and logprob_rows (score.hip) reduces every row to (log-probability, logsumexp, argmax).
// The row maps every stage reads (which row is which token or video row, of which sequence, at which position, in which slot) are one int block:
// prefill_plan.h owns its layout and the loops that fill and check it; the host staging copy and the device copy are read through the same accessor.
struct ScoreReq { const int32_t* h_targets; float* d_logprob; float* d_lse; int32_t* d_argmax; };
enum PrefillMode { PREFILL_PLAIN, PREFILL_APPEND, PREFILL_SLOTS, PREFILL_SCORE };
// One prefill call as its entry point states it; what a mode does not use stays null.
struct PrefillReq {
    const char* who = nullptr; PrefillMode mode = PREFILL_PLAIN;
    const int32_t *h_ids = nullptr, *h_seq_lens = nullptr; int B = 0;                                  // the token rows
    const void* d_video = nullptr; int Vt = 0; const int32_t* h_vid_pos = nullptr;                     // the optional video
    float* d_logits = nullptr; int32_t* d_next = nullptr; float* d_all_logits = nullptr; int ld_all = 0;
    const int32_t* h_slots = nullptr; const PickParams* pick = nullptr; const float* d_u = nullptr;    // PREFILL_SLOTS
    const int32_t* h_counts = nullptr;                                                                 // PREFILL_SLOTS, pgv_llm_prefill_slots_n only
    ScoreReq score{};                                                                                  // PREFILL_SCORE
};
// What the stages hand on: the plan, the two views of its block (kv->h_meta, the device copy) and the workspace buffers.
struct PrefillWork {
    PrefillPlan plan;
    PrefillMaps<const int> h, d;
    const int *d_offs, *d_slots;         // d.offs / d.slots for the calls whose kernels read them (append / slots), else null
    float* resid; char *xn, *qkv, *ao, *act;
    int T; const int *t_last, *t_lens, *t_slots, *ht_lens;      // the tail's rows: one per sample (the plan's samp_* maps), without counts one per sequence (last / lens / d_slots)
    int* d_pick;                         // the refilled samples' first tokens, before they go to their slots
    int schunk; float* sres; char* sxn; float* slog;     // scoring tail: gathered residual rows, their normalised 16-bit form and the fp32 logits of one chunk
};
// prefill_plan_build with its refusal forwarded as this library reports errors
static int plan_build(const PrefillRows& rows, std::vector<int>& meta, PrefillPlan& plan) {
    char err[512];
    if (prefill_plan_build(rows, meta, plan, err, sizeof(err)) != PLAN_OK) { pgv_set_error("%s", err); return PGV_EINVAL; }
    return PGV_OK;
}
static int vocab16(const pgv_llm* m) { return (m->cfg.vocab + 15) & ~15; }      // the lm_head rows a GEMM computes: whole 16-row fragments

// One prefill GEMM over a matrix's 16-bit blocked copy, the twin of gemv_mat: C [rows][ldc] = epi(A [rows][K] * W[0, N)^T)
static int gemm_mat(pgv_ctx* ctx, const pgv_llm* m, const LlmMat& w, int N, const void* A, void* C, int ldc, int rows, int epi, hipStream_t s) {
    GemmArgs g{};
    g.A = A; g.lda = (int)w.K; g.W = w.w16; g.ldw = (int)w.K; g.bias = nullptr; g.C = C; g.ldc = ldc; g.M = rows; g.N = N; g.K = (int)w.K; g.epi = epi; g.w_blocked = true;
    return pgv_launch_gemm(ctx, m->dtype, g, s);
}
// Final RMSNorm of `rows` residual rows into the 16-bit buffer x16, then lm_head to fp32 logits [rows][ld >= vocab16]: one tile shape, no
// split-K, so a row's logits do not depend on which rows go with it
static int head_logits(pgv_ctx* ctx, const pgv_llm* m, const float* resid, void* x16, int rows, float* logits, int ld, hipStream_t s) {
    PGV_TRY(pgv_launch_rmsnorm(m->dtype, resid, m->norm_g, m->cfg.eps, x16, rows, m->cfg.hidden, s));
    return gemm_mat(ctx, m, m->mats[0], vocab16(m), x16, logits, ld, rows, PGV_EPI_F32, s);
}

static int prefill_check(const pgv_ctx* ctx, const pgv_llm* m, const pgv_kv* kv, const PrefillReq& q) {
    const char* who = q.who;
    PGV_CHECK(ctx && m && kv && q.h_ids && q.h_seq_lens, "%s: null argument", who);
    PGV_CHECK(kv->llm == m, "%s: kv cache belongs to another model", who);
    PGV_CHECK(q.B >= 1 && q.B <= kv->B, "%s: batch %d outside [1,%d]", who, q.B, kv->B);
    if (pgv_llm_missing(m) != 0) { pgv_set_error("%s: %d weight tensors not loaded", who, pgv_llm_missing(m)); return PGV_ESTATE; }
    if (q.mode == PREFILL_APPEND && kv->active != q.B) { pgv_set_error("pgv_llm_prefill_append: %d sequences for a cache that holds %d prefilled ones", q.B, kv->active); return PGV_ESTATE; }
    if (q.mode == PREFILL_SLOTS) {
        if (kv->active < 1) { pgv_set_error("%s: no live group in this cache (run pgv_llm_prefill first)", who); return PGV_ESTATE; }
        PGV_CHECK(q.B <= kv->active, "%s: %d sequences for a group of %d", who, q.B, kv->active);
        PGV_CHECK(!q.pick || q.pick->temperature > 0.f, "%s: temperature must be positive (got %g)", who, (double)q.pick->temperature);
        PGV_CHECK(q.d_all_logits == nullptr, "%s: no all-position logits", who);
    }
    if (q.mode == PREFILL_SCORE) PGV_CHECK(vocab16(m) <= m->vocab_cap, "%s: vocabulary %d beyond the %d allocated lm_head rows", who, m->cfg.vocab, m->vocab_cap);
    return PGV_OK;
}

// Builds the plan into kv->h_meta (it outlives the async copy), reserves the workspace and uploads the block; resets what a new prompt resets.
static int prefill_plan_upload(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const PrefillReq& q, PrefillWork& w, hipStream_t s) {
    const bool append = q.mode == PREFILL_APPEND, slots = q.mode == PREFILL_SLOTS;
    const int B = q.B, H = m->cfg.hidden, I = m->cfg.inter, vocab = m->cfg.vocab;
    const char* who = q.who;
    PrefillRows rows;
    rows.who = who; rows.ids = q.h_ids; rows.seq_lens = q.h_seq_lens; rows.B = B;
    rows.start = append ? kv->h_len.data() : nullptr;
    rows.slots = q.h_slots; rows.active = kv->active; rows.counts = q.h_counts;
    rows.vid_pos = q.d_video ? q.h_vid_pos : nullptr; rows.Vt = q.Vt;
    rows.targets = q.score.h_targets;
    rows.vocab = vocab; rows.max_seq = kv->max_seq; rows.hidden = H;
    PGV_TRY(plan_build(rows, kv->h_meta, w.plan));
    const std::vector<int>& meta = kv->h_meta;
    const int M = w.plan.M, nscore = w.plan.nscore, T = w.T = q.h_counts ? w.plan.S : B;
    // arrival tickets of the context-split decode attention: a launch re-arms its own, but an ABORTED decode launch (device fault, process kill
    // between launches) would leave one non-zero for the next user of this cache -- every prefill starts from zeros
    PGV_HIP(hipMemsetAsync(kv->sc.dattn_ticket, 0, (size_t)kv->B * m->cfg.heads * sizeof(unsigned), s));

    const size_t b_meta = pgv_align(meta.size() * 4), b_resid = pgv_align((size_t)M * H * 4), b_xn = pgv_align((size_t)M * H * 2),
                 b_qkv = pgv_align((size_t)M * 3 * H * 2), b_ao = pgv_align((size_t)M * H * 2), b_act = pgv_align((size_t)M * I * 2);
    const size_t b_pick = slots ? pgv_align((size_t)T * 4) : 0;
    const int schunk = w.schunk = nscore < PGV_SCORE_CHUNK_ROWS ? nscore : PGV_SCORE_CHUNK_ROWS;
    const size_t b_sres = pgv_align((size_t)schunk * H * 4), b_sxn = pgv_align((size_t)schunk * H * 2), b_slog = pgv_align((size_t)schunk * vocab16(m) * 4);
    PGV_TRY(pgv_ws_reserve(ctx, b_meta + b_resid + b_xn + b_qkv + b_ao + b_act + b_pick + b_sres + b_sxn + b_slog, s));
    int* d_meta = (int*)pgv_ws_alloc(ctx, b_meta);
    w.resid = (float*)pgv_ws_alloc(ctx, b_resid);
    w.xn = (char*)pgv_ws_alloc(ctx, b_xn);
    w.qkv = (char*)pgv_ws_alloc(ctx, b_qkv);
    w.ao = (char*)pgv_ws_alloc(ctx, b_ao);
    w.act = (char*)pgv_ws_alloc(ctx, b_act);
    w.d_pick = slots ? (int*)pgv_ws_alloc(ctx, b_pick) : nullptr;
    w.sres = schunk ? (float*)pgv_ws_alloc(ctx, b_sres) : nullptr;
    w.sxn = schunk ? (char*)pgv_ws_alloc(ctx, b_sxn) : nullptr;
    w.slog = schunk ? (float*)pgv_ws_alloc(ctx, b_slog) : nullptr;
    PGV_CHECK(d_meta && w.resid && w.xn && w.qkv && w.ao && w.act && (!slots || w.d_pick) && (!schunk || (w.sres && w.sxn && w.slog)), "%s: workspace exhausted", who);
    PGV_HIP(hipMemcpyAsync(d_meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, s));
    w.h = w.plan.lo.maps(meta.data());
    w.d = w.plan.lo.maps((const int*)d_meta);
    w.d_offs = append ? w.d.offs : nullptr;
    w.d_slots = slots ? w.d.slots : nullptr;
    if (q.h_counts) { w.t_last = w.d.samp_last; w.t_lens = w.d.samp_lens; w.t_slots = w.d.samp_slots; w.ht_lens = w.h.samp_lens; }
    else { w.t_last = w.d.last; w.t_lens = w.d.lens; w.t_slots = w.d_slots; w.ht_lens = w.h.lens; }
    // HF's repetition penalty sees the prompt ids as given, placeholder ids included: a new prompt starts its slot's set, an appended turn adds to it
    // (and every sample of a prompt starts from the prompt's ids alone: the pick adds its own token to the set of its own slot)
    PGV_TRY(pgv_launch_seen_mark(w.d.raw_ids, w.d.cu, w.t_slots, T, vocab, kv->d_seen, kv->seen_words, append ? 0 : 1, s, q.h_counts ? w.d.samp_seq : nullptr));
    // the ordered twin of the seen-set (pgv_kv_set_bans): each slot's ids at their cache positions and its prompt length, same indirection
    if (kv->ban.on || kv->lookup.D > 0 || kv->allow.on) PGV_TRY(pgv_launch_ids_write(w.d.raw_ids, w.d.cu, w.d.offs, w.t_slots, q.h_counts ? w.d.samp_seq : nullptr, T, kv->ids.ids, kv->max_seq, kv->ids.plen, s));
    // pgv_kv_set_allowed: a refilled slot starts at root 0 (one automaton for every task of a refill run); its state rows need no action, the
    // first pick reads the root and every later step stores the entry the next one reads
    if (kv->allow.on && slots) PGV_TRY(pgv_launch_allow_root_zero(w.t_slots, T, kv->allow.root, s));
    if (!slots) {       // a refill sets the state of its own slots only, after the pick (pgv_launch_slot_scatter)
        PGV_HIP(hipMemcpyAsync(kv->d_pos, w.d.lens, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
        PGV_HIP(hipMemsetAsync(kv->d_step, 0, (size_t)2 * kv->B * 4, s));      // step + done
    }
    return PGV_OK;
}

// Embedding + video splice, then every decoder layer over the M rows: w.resid holds the final residual stream.
static int prefill_trunk(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const PrefillReq& q, const PrefillWork& w, hipStream_t s) {
    const int M = w.plan.M, H = m->cfg.hidden, I = m->cfg.inter, heads = m->cfg.heads;
    PGV_TRY(pgv_launch_embed_splice(m->dtype, w.d.row_src, m->embed, q.d_video, w.resid, M, H, s));
    for (int li = 0; li < m->cfg.layers; ++li) {
        const LlmLayer& l = m->layers[li];
        const LlmMat &wqkv = layer_mat(m, li, MAT_QKV), &wo = layer_mat(m, li, MAT_O), &wgu = layer_mat(m, li, MAT_GU), &wdown = layer_mat(m, li, MAT_DOWN);
        PGV_TRY(pgv_launch_rmsnorm(m->dtype, w.resid, l.in_g, m->cfg.eps, w.xn, M, H, s));
        PGV_TRY(gemm_mat(ctx, m, wqkv, (int)wqkv.N, w.xn, w.qkv, 3 * H, M, PGV_EPI_NONE, s));
        PGV_TRY(pgv_launch_rope_kv_write(m->dtype, w.qkv, w.d.row_b, w.d.row_pos, m->rope, kv->Kc[li], kv->Vc[li], M, H, heads, kv->max_seq, s));
        PGV_TRY(pgv_launch_prefill_attn(ctx, m->dtype, w.qkv, w.ao, kv->Kc[li], kv->Vc[li], w.d.cu, w.d_offs, q.B, w.plan.max_len, H, heads, kv->max_seq,
                                        w.plan.attn_flops, s, w.d_slots));
        PGV_TRY(gemm_mat(ctx, m, wo, (int)wo.N, w.ao, w.resid, H, M, PGV_EPI_RESID, s));
        PGV_TRY(pgv_launch_rmsnorm(m->dtype, w.resid, l.post_g, m->cfg.eps, w.xn, M, H, s));
        PGV_TRY(gemm_mat(ctx, m, wgu, (int)wgu.N, w.xn, w.act, I, M, PGV_EPI_SWIGLU, s));
        PGV_TRY(gemm_mat(ctx, m, wdown, (int)wdown.N, w.act, w.resid, H, M, PGV_EPI_RESID, s));
    }
    return PGV_OK;
}

// pgv_llm_prefill_slots_n: the cache rows [0, len) the trunk wrote into the first slot of every run go to the run's other slots, one launch per
// sequence that has more than one sample.  The destinations are the entries behind the run's first in the device copy of the sample slot map.
static int prefill_fork_runs(pgv_llm* m, pgv_kv* kv, const PrefillReq& q, const PrefillWork& w, hipStream_t s) {
    const int heads = m->cfg.heads, L = m->cfg.layers;
    if (L < 1) return PGV_OK;
    KvForkArgs a{};
    a.cache = (char*)kv->Kc[0];
    a.head_stride = (size_t)kv->max_seq * kHD * 2; a.slot_stride = a.head_stride * heads; a.plane_stride = kv->plane_bytes;
    a.heads = heads; a.nrun = 2 * L * heads;
    for (int b = 0, j = 0; b < q.B; j += q.h_counts[b], ++b) {
        if (q.h_counts[b] < 2) continue;
        a.src = w.h.slots[b]; a.dst = w.d.samp_slots + j + 1; a.nd = q.h_counts[b] - 1; a.run_pieces = (unsigned)w.h.lens[b] * (kHD * 2 / 16);
        PGV_TRY(pgv_launch_kv_fork_list(a, s));
    }
    return PGV_OK;
}

// The reference's forward output: final norm + lm_head over ALL positions (video_chatgpt.py:225-226) -- on request only
static int prefill_all_logits(pgv_ctx* ctx, pgv_llm* m, const PrefillReq& q, const PrefillWork& w, hipStream_t s) {
    const int n16 = vocab16(m);
    PGV_CHECK(q.ld_all >= n16 && q.ld_all % 4 == 0 && n16 <= m->vocab_cap, "%s: ld_all %d must be a multiple of 4 and at least %d", q.who, q.ld_all, n16);
    return head_logits(ctx, m, w.resid, w.xn, w.plan.M, q.d_all_logits, q.ld_all, s);
}

// What the reference's loss reads (video_chatgpt.py:228-239), for the rows that have a target only; unscored rows: 0 / 0 / -1
static int prefill_score(pgv_ctx* ctx, pgv_llm* m, const ScoreReq& sc, const PrefillWork& w, hipStream_t s) {
    const int M = w.plan.M, nscore = w.plan.nscore, n16 = vocab16(m);
    if (sc.d_logprob) PGV_HIP(hipMemsetAsync(sc.d_logprob, 0, (size_t)M * 4, s));
    if (sc.d_lse) PGV_HIP(hipMemsetAsync(sc.d_lse, 0, (size_t)M * 4, s));
    if (sc.d_argmax) PGV_HIP(hipMemsetAsync(sc.d_argmax, 0xff, (size_t)M * 4, s));
    for (int c0 = 0; c0 < nscore; c0 += w.schunk) {
        const int n = nscore - c0 < w.schunk ? nscore - c0 : w.schunk;
        PGV_TRY(pgv_launch_gather_rows(w.resid, w.d.srows + c0, w.sres, n, m->cfg.hidden, s));
        PGV_TRY(head_logits(ctx, m, w.sres, w.sxn, n, w.slog, n16, s));
        PGV_TRY(pgv_launch_logprob_rows(ctx, w.slog, n16, m->cfg.vocab, n, w.d.stgts + c0, w.d.srows + c0, sc.d_logprob, sc.d_lse, sc.d_argmax, s));
    }
    return PGV_OK;
}

// lm_head only on the last position of every sequence (the reference computes all S positions, video_chatgpt.py:226), the pick, the outputs and
// the host-side lengths.  (A refill runs this tail in rows [0, B) of the decode scratch: every decode step rebuilds resid / xn / ssq / logits /
// amax_* from d_cur.)
static int prefill_last_rows(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const PrefillReq& q, const PrefillWork& w, hipStream_t s) {
    const bool slots = q.mode == PREFILL_SLOTS;
    const int B = w.T, H = m->cfg.hidden;          // rows of the tail: the samples
    PGV_TRY(pgv_launch_gather_rows(w.resid, w.t_last, kv->sc.resid, B, H, s));
    const int nparts = norm_fold_enabled() ? 1 : 0;
    if (nparts) PGV_TRY(pgv_launch_final_prep(m->dtype, kv->sc.resid, m->norm_g, kv->sc.xn, kv->sc.ssq, B, H, s, true));
    else PGV_TRY(pgv_launch_rmsnorm(m->dtype, kv->sc.resid, m->norm_g, m->cfg.eps, kv->sc.xn, B, H, s));
    if (!slots) {
        PGV_TRY(lm_head_and_pick(ctx, m, kv, B, -1, 0, s, nparts));
    } else {
        PGV_TRY(lm_head(ctx, m, kv, B, true, s, nparts));           // the greedy candidates too: the same launch as a plain prefill, same logits
        pgv_prof_begin(ctx, 6, s);
        const float* d_u = q.d_u;
        if (q.pick && q.pick->greedy) { d_u = kv->d_u; PGV_TRY(pgv_zero_uniforms(kv->d_u, B, s)); }
        PGV_TRY(kv_pick(kv, B, q.pick, d_u, false, PickState{w.d_pick}, w.t_slots, s, w.t_lens));      // in scratch rows [0, B): what it records lands at the slots
        PGV_TRY(pgv_launch_slot_scatter(w.t_slots, w.d_pick, w.t_lens, B, kv->d_cur, kv->d_pos, kv->d_step, kv->d_done, s));
        pgv_prof_end(ctx, 6, s, 0.0, 0.0);
    }
    if (q.d_logits) PGV_HIP(hipMemcpyAsync(q.d_logits, kv->sc.logits, (size_t)B * m->cfg.vocab * 4, hipMemcpyDeviceToDevice, s));
    if (q.d_next) PGV_HIP(hipMemcpyAsync(q.d_next, slots ? w.d_pick : kv->d_cur, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (slots) {
        for (int b = 0; b < B; ++b) kv->h_len[q.h_slots[b]] = w.ht_lens[b];
    } else {
        for (int b = 0; b < kv->B; ++b) kv->h_len[b] = b < B ? w.h.lens[b] : 0;
        kv->active = B;
    }
    return PGV_OK;
}

static int prefill_impl(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const PrefillReq& q, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    PrefillWork w;
    PGV_TRY(prefill_check(ctx, m, kv, q));
    beam_drop(kv);
    kv->lookup.valid = false;
    PGV_TRY(prefill_plan_upload(ctx, m, kv, q, w, s));
    PGV_TRY(prefill_trunk(ctx, m, kv, q, w, s));
    if (q.h_counts) PGV_TRY(prefill_fork_runs(m, kv, q, w, s));
    if (q.d_all_logits) PGV_TRY(prefill_all_logits(ctx, m, q, w, s));
    if (q.mode == PREFILL_SCORE) PGV_TRY(prefill_score(ctx, m, q.score, w, s));
    PGV_TRY(prefill_last_rows(ctx, m, kv, q, w, s));
    kv->lookup.valid = kv->lookup.D > 0 && q.mode == PREFILL_PLAIN;
    PGV_HIP(hipGetLastError());
    PGV_TRY(pgv_ws_release(ctx, s));
    return PGV_OK;
}

extern "C" int pgv_llm_prefill(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* h_ids, const int32_t* h_seq_lens, int B, const void* d_video,
                               int Vt, const int32_t* h_vid_pos, float* d_logits, int32_t* d_next, float* d_all_logits, int ld_all, void* stream) {
    PrefillReq q;
    q.who = "pgv_llm_prefill"; q.mode = PREFILL_PLAIN;
    q.h_ids = h_ids; q.h_seq_lens = h_seq_lens; q.B = B;
    q.d_video = d_video; q.Vt = Vt; q.h_vid_pos = h_vid_pos;
    q.d_logits = d_logits; q.d_next = d_next; q.d_all_logits = d_all_logits; q.ld_all = ld_all;
    return prefill_impl(ctx, m, kv, q, stream);
}

extern "C" int pgv_llm_prefill_append(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* h_ids, const int32_t* h_seq_lens, int B, const void* d_video,
                                      int Vt, const int32_t* h_vid_pos, float* d_logits, int32_t* d_next, float* d_all_logits, int ld_all, void* stream) {
    PrefillReq q;
    q.who = "pgv_llm_prefill_append"; q.mode = PREFILL_APPEND;
    q.h_ids = h_ids; q.h_seq_lens = h_seq_lens; q.B = B;
    q.d_video = d_video; q.Vt = Vt; q.h_vid_pos = h_vid_pos;
    q.d_logits = d_logits; q.d_next = d_next; q.d_all_logits = d_all_logits; q.ld_all = ld_all;
    return prefill_impl(ctx, m, kv, q, stream);
}

extern "C" int pgv_llm_prefill_slots(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* h_slots, int n, const int32_t* h_ids, const int32_t* h_seq_lens,
                                     const void* d_video, int Vt, const int32_t* h_vid_pos, float temperature, int top_k, const float* d_u, float* d_logits,
                                     int32_t* d_next, void* stream) {
    PGV_CHECK(h_slots, "pgv_llm_prefill_slots: null slot list");
    PGV_TRY(kv_allows(kv, KV_PREFILL_SLOTS, "pgv_llm_prefill_slots"));
    // uniforms: sampled; none: greedy, from the lm_head candidates unless a penalty or a ban applies (prefill_check refuses a null cache)
    const PickParams p = !kv ? PickParams{} : d_u ? kv_sampled(kv, temperature, top_k) : pick_greedy(kv->warpers.penalty);
    PrefillReq q;
    q.who = "pgv_llm_prefill_slots"; q.mode = PREFILL_SLOTS;
    q.h_ids = h_ids; q.h_seq_lens = h_seq_lens; q.B = n;
    q.d_video = d_video; q.Vt = Vt; q.h_vid_pos = h_vid_pos;
    q.d_logits = d_logits; q.d_next = d_next;
    q.h_slots = h_slots; q.pick = !d_u && !(kv && kv_greedy_sampled(kv)) ? nullptr : &p; q.d_u = d_u;
    return prefill_impl(ctx, m, kv, q, stream);
}

extern "C" int pgv_llm_prefill_slots_n(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* h_slots, const int32_t* h_counts, int n, const int32_t* h_ids,
                                       const int32_t* h_seq_lens, const void* d_video, int Vt, const int32_t* h_vid_pos, float temperature, int top_k,
                                       const float* d_u, float* d_logits, int32_t* d_next, void* stream) {
    PGV_CHECK(h_slots && h_counts, "pgv_llm_prefill_slots_n: null slot or count list");
    PGV_TRY(kv_allows(kv, KV_PREFILL_SLOTS, "pgv_llm_prefill_slots_n"));
    const PickParams p = !kv ? PickParams{} : d_u ? kv_sampled(kv, temperature, top_k) : pick_greedy(kv->warpers.penalty);       // as pgv_llm_prefill_slots
    PrefillReq q;
    q.who = "pgv_llm_prefill_slots_n"; q.mode = PREFILL_SLOTS;
    q.h_ids = h_ids; q.h_seq_lens = h_seq_lens; q.B = n;
    q.d_video = d_video; q.Vt = Vt; q.h_vid_pos = h_vid_pos;
    q.d_logits = d_logits; q.d_next = d_next;
    q.h_slots = h_slots; q.h_counts = h_counts; q.pick = !d_u && !(kv && kv_greedy_sampled(kv)) ? nullptr : &p; q.d_u = d_u;
    return prefill_impl(ctx, m, kv, q, stream);
}

extern "C" int pgv_llm_score(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* h_ids, const int32_t* h_seq_lens, int B, const void* d_video, int Vt,
                             const int32_t* h_vid_pos, const int32_t* h_targets, float* d_logprob, float* d_lse, int32_t* d_argmax, void* stream) {
    PGV_CHECK(h_targets, "pgv_llm_score: null target list");
    PrefillReq q;
    q.who = "pgv_llm_score"; q.mode = PREFILL_SCORE;
    q.h_ids = h_ids; q.h_seq_lens = h_seq_lens; q.B = B;
    q.d_video = d_video; q.Vt = Vt; q.h_vid_pos = h_vid_pos;
    q.score = ScoreReq{h_targets, d_logprob, d_lse, d_argmax};
    return prefill_impl(ctx, m, kv, q, stream);
}

// Drop the tail of sequence b: the next pgv_llm_prefill_append / decode call continues at position `len` (the entries beyond it are simply
// overwritten).  What a chat turn needs when the new prompt shares only a prefix with the cached conversation (surplus decode steps past a stop
// string, a re-tokenised answer).
extern "C" int pgv_kv_truncate(pgv_kv* kv, int b, int len, void* stream) {
    PGV_CHECK(kv != nullptr, "pgv_kv_truncate: null cache");
    PGV_CHECK(b >= 0 && b < kv->active, "pgv_kv_truncate: sequence %d outside the %d prefilled ones", b, kv->active);
    PGV_CHECK(len >= 1 && len <= kv->h_len[b], "pgv_kv_truncate: length %d outside [1,%d]", len, kv->h_len[b]);
    kv->h_len[b] = len;
    beam_drop(kv);
    PGV_HIP(hipMemcpyAsync(kv->d_pos + b, &kv->h_len[b], 4, hipMemcpyHostToDevice, (hipStream_t)stream));
    PGV_HIP(hipStreamSynchronize((hipStream_t)stream));          // the source is host bookkeeping that the next call may change
    return PGV_OK;
}

// Fork the live group: sequence p becomes h_counts[p] consecutive slots (new slot i = old slot src(i), src = [0]*c0 + [1]*c1 + ...).
// What defines a slot, and is therefore copied: its cache rows [0, len), its length, and the state a decode step does not rebuild from the
// current token and position -- position, current token, done flag, seen-set bitmap, logits row (the first token of a fresh prefill is drawn
// from it) and the two lp_last values.  Residual, norms, candidates and qkv are rebuilt by every step; the token / log-probability histories
// restart with every stepping call.
// IN PLACE, one launch per source on the stream, sources in DESCENDING order.  The destinations of source p are slots [base_p, base_p + c_p)
// with base_p = c_0 + ... + c_(p-1) >= p (every count is >= 1).  When source p runs, every source q > p has run already and is never read
// again; every source q < p is still unread and every destination of p is >= base_p >= p > q: no slot is overwritten before it has been
// read.  Inside a launch the source slot itself is skipped as a destination, so no launch reads what it writes.  The result is as if every
// read preceded every write.  (counts [2,2,2]: slot 1 is source 1 and second destination of source 0 -- source 2 -> slots 4, 5; then source
// 1 -> slots 2, 3; only then source 0 -> slot 1.)
// The feature records of slot src, rows [0, len), go to slots [d0, d0 + nd) (src itself skipped).  Id rows are copied iff bans are on; automaton
// state rows and the root iff the automaton is on; the prompt length iff either is on (once: with the id rows if there are any, else with the root).
static int slot_records_copy(pgv_kv* kv, int src, int d0, int nd, int len, hipStream_t s) {
    const bool ids = kv->ban.on, states = kv->allow.on;
    auto rows = [&](int* rec, int dst) { return hipMemcpyAsync(rec + (size_t)dst * kv->max_seq, rec + (size_t)src * kv->max_seq, (size_t)len * 4, hipMemcpyDeviceToDevice, s); };
    auto word = [&](int* rec, int dst) { return hipMemcpyAsync(rec + dst, rec + src, 4, hipMemcpyDeviceToDevice, s); };
    for (int dst = d0; ids && dst < d0 + nd; ++dst)
        if (dst != src) { PGV_HIP(rows(kv->ids.ids, dst)); PGV_HIP(word(kv->ids.plen, dst)); }
    for (int dst = d0; states && dst < d0 + nd; ++dst) {
        if (dst != src) { PGV_HIP(rows(kv->allow.state, dst)); PGV_HIP(word(kv->allow.root, dst)); }
        if (dst != src && !ids) PGV_HIP(word(kv->ids.plen, dst));
    }
    return PGV_OK;
}

extern "C" int pgv_kv_fork(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* h_counts, int P, void* stream) {
    PGV_CHECK(ctx && m && kv && h_counts, "pgv_kv_fork: null argument");
    PGV_CHECK(kv->llm == m, "pgv_kv_fork: kv cache belongs to another model");
    PGV_TRY(kv_allows(kv, KV_FORK, "pgv_kv_fork"));
    if (kv->active < 1) { pgv_set_error("pgv_kv_fork: no live group in this cache (run pgv_llm_prefill first)"); return PGV_ESTATE; }
    PGV_CHECK(P == kv->active, "pgv_kv_fork: %d counts for a live group of %d sequences", P, kv->active);
    long long W = 0;
    for (int p = 0; p < P; ++p) {
        PGV_CHECK(h_counts[p] >= 1, "pgv_kv_fork: count %d of sequence %d is below 1", h_counts[p], p);
        W += h_counts[p];
    }
    PGV_CHECK(W <= kv->B, "pgv_kv_fork: new width %lld exceeds the %d sequences the cache was created with", W, kv->B);
    if (W == P) return PGV_OK;            // every count is 1: the group is its own fork
    beam_drop(kv);
    kv->lookup.valid = false;
    hipStream_t s = (hipStream_t)stream;
    const int heads = m->cfg.heads, L = m->cfg.layers;
    KvForkArgs a;
    a.cache = L > 0 ? (char*)kv->Kc[0] : kv->blob.p;
    a.head_stride = (size_t)kv->max_seq * kHD * 2; a.slot_stride = a.head_stride * heads; a.plane_stride = kv->plane_bytes;
    a.heads = heads; a.nrun = 2 * L * heads;
    a.pos = kv->d_pos; a.cur = kv->d_cur; a.done = kv->d_done; a.lp_last = kv->lp.last; a.lp_stride = kv->B;
    a.seen = kv->d_seen; a.seen_words = kv->seen_words; a.logits = kv->sc.logits; a.vocab = m->cfg.vocab;
    PGV_HIP(hipMemsetAsync(kv->d_step, 0, (size_t)kv->B * 4, s));
    std::vector<int> len((size_t)W);
    int base = (int)W;
    for (int p = P - 1; p >= 0; --p) {
        const int c = h_counts[p];
        base -= c;
        for (int i = 0; i < c; ++i) len[(size_t)base + i] = kv->h_len[p];
        if (c == 1 && base == p) continue;                 // the slot stays where it is
        a.src = p; a.d0 = base; a.nd = c; a.run_pieces = (unsigned)kv->h_len[p] * (kHD * 2 / 16);
        PGV_TRY(pgv_launch_kv_fork(a, s));
        PGV_TRY(slot_records_copy(kv, p, base, c, kv->h_len[p], s));       // in the same order as the cache rows
    }
    for (int i = 0; i < (int)W; ++i) kv->h_len[i] = len[i];
    kv->active = (int)W;
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

extern "C" int pgv_kv_peek(pgv_kv* kv, int layer, int which, int slot, int row0, int nrows, void* d_out, void* stream) {
    PGV_CHECK(kv && d_out, "pgv_kv_peek: null argument");
    PGV_CHECK(layer >= 0 && layer < (int)kv->Kc.size(), "pgv_kv_peek: layer %d outside [0,%d)", layer, (int)kv->Kc.size());
    PGV_CHECK(which == 0 || which == 1, "pgv_kv_peek: which = %d is neither 0 (K) nor 1 (V)", which);
    PGV_CHECK(slot >= 0 && slot < kv->B, "pgv_kv_peek: slot %d outside the %d of the cache", slot, kv->B);
    PGV_CHECK(row0 >= 0 && nrows >= 1 && row0 <= kv->max_seq - nrows, "pgv_kv_peek: rows [%d,%d + %d) outside the cache's %d", row0, row0, nrows, kv->max_seq);
    const int heads = kv->llm->cfg.heads;
    const size_t row = (size_t)kHD * 2, head = (size_t)kv->max_seq * row;
    const char* src = (const char*)(which ? kv->Vc[layer] : kv->Kc[layer]) + ((size_t)slot * heads) * head + (size_t)row0 * row;
    PGV_HIP(hipMemcpy2DAsync(d_out, (size_t)nrows * row, src, head, (size_t)nrows * row, heads, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PGV_OK;
}

// ---------------------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------------------
// One token step up to the input of lm_head, over `rows` rows of the scratch `sc` fed the tokens tok [rows]: the cache's B slots on its own scratch
// (row_slot null: row b is slot b at d_pos[b], the launches and arguments of every release so far), or mapped rows on the row scratch (row r is
// slot row_slot[r] at d_pos[slot] + row_j[r]; a negative slot: no row).  The GEMVs only see another batch, so every row's arithmetic is the one of
// a plain step at its position (choose_gemv picks the shape by batch; the results are batch-invariant).  *nparts: what lm_head takes.
struct RowMap { const int *d_slot = nullptr, *d_j = nullptr, *h_slot = nullptr, *h_j = nullptr; };     // device maps for the kernels; host copies for the byte count of the profile
static double step_kv_bytes(const pgv_kv* kv, int rows, const RowMap& rm, int H) {
    if (rm.d_slot && !rm.h_slot) return 0.0;       // a lookup step: its rows are drawn on the device
    double bytes = 0;
    for (int r = 0; r < rows; ++r) {
        const int b = rm.h_slot ? rm.h_slot[r] : r;
        if (b >= 0) bytes += 2.0 * 2.0 * (double)(kv->h_len[b] + (rm.h_j ? rm.h_j[r] : 0) + 1) * H;
    }
    return bytes;
}
static int step_attn(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const DecodeScratch& sc, int li, int rows, const RowMap& rm, double kv_bytes, hipStream_t s) {
    const int H = m->cfg.hidden, heads = m->cfg.heads;
    if (!rm.d_slot)
        return pgv_launch_decode_attn(ctx, m->dtype, sc.qkv, kv->d_pos, m->rope, kv->Kc[li], kv->Vc[li], sc.ao, rows, H, heads, kv->max_seq, kv_bytes, s, sc.dattn_part, sc.dattn_ticket, 0);
    return pgv_launch_decode_attn_rows(ctx, m->dtype, sc.qkv, kv->d_pos, rm.d_slot, rm.d_j, m->rope, kv->Kc[li], kv->Vc[li], sc.ao, rows, H, heads, kv->max_seq, kv_bytes, s,
                                       sc.dattn_part, sc.dattn_ticket, 0);
}
static int decode_trunk_unfolded(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const DecodeScratch& sc, const int* tok, int rows, const RowMap& rm, hipStream_t s, int* nparts_out) {
    const int H = m->cfg.hidden, I = m->cfg.inter, B = rows, L = m->cfg.layers;
    pgv_prof_begin(ctx, 6, s);
    PGV_TRY(pgv_launch_embed_tok_norm(m->dtype, tok, m->embed, sc.resid, L > 0 ? m->layers[0].in_g : m->norm_g, sc.xn, sc.ssq, B, H, s, false));   // resid is what matters here
    pgv_prof_end(ctx, 6, s, 0.0, 0.0);
    const double kv_bytes = step_kv_bytes(kv, rows, rm, H);
    for (int li = 0; li < L; ++li) {
        const LlmLayer& l = m->layers[li];
        PGV_TRY(pgv_launch_rmsnorm(m->dtype, sc.resid, l.in_g, m->cfg.eps, sc.xn, B, H, s));
        PGV_TRY(gemv_mat(ctx, m, GV_STORE16, layer_mat(m, li, MAT_QKV), sc.xn, sc.qkv, 3 * H, B, s, nullptr));
        PGV_TRY(step_attn(ctx, m, kv, sc, li, rows, rm, kv_bytes, s));
        PGV_TRY(gemv_mat(ctx, m, GV_RESID, layer_mat(m, li, MAT_O), sc.ao, sc.resid, H, B, s, nullptr));
        PGV_TRY(pgv_launch_rmsnorm(m->dtype, sc.resid, l.post_g, m->cfg.eps, sc.xn, B, H, s));
        PGV_TRY(gemv_mat(ctx, m, GV_SWIGLU, layer_mat(m, li, MAT_GU), sc.xn, sc.act, I, B, s, nullptr));
        PGV_TRY(gemv_mat(ctx, m, GV_RESID, layer_mat(m, li, MAT_DOWN), sc.act, sc.resid, H, B, s, nullptr));
    }
    PGV_TRY(pgv_launch_rmsnorm(m->dtype, sc.resid, m->norm_g, m->cfg.eps, sc.xn, B, H, s));
    *nparts_out = 0;
    return PGV_OK;
}

static int decode_trunk(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const DecodeScratch& sc, const int* tok, int rows, const RowMap& rm, hipStream_t s, int* nparts_out) {
    if (!norm_fold_enabled()) return decode_trunk_unfolded(ctx, m, kv, sc, tok, rows, rm, s, nparts_out);
    const int H = m->cfg.hidden, I = m->cfg.inter, B = rows, L = m->cfg.layers;
    const int nparts = H / 16;                     // one sum-of-squares partial per 16-row workgroup of a residual producer
    // RMSNorm has no launch of its own in decode (GemvArgs, gemv.hip): the kernel that completes the residual also writes
    // xg = round16(resid * gamma_next) and sum-of-squares partials; the consumer GEMV scales its accumulators by rstd.
    pgv_prof_begin(ctx, 6, s);
    PGV_TRY(pgv_launch_embed_tok_norm(m->dtype, tok, m->embed, sc.resid, L > 0 ? m->layers[0].in_g : m->norm_g, sc.xn, sc.ssq, B, H, s, true));
    pgv_prof_end(ctx, 6, s, 0.0, 0.0);
    const double kv_bytes = step_kv_bytes(kv, rows, rm, H);
    int parts_in = 1;                              // the embedding kernel leaves one partial per sequence
    for (int li = 0; li < L; ++li) {
        const LlmLayer& l = m->layers[li];
        GemvNorm cons; cons.ssq_in = sc.ssq; cons.nparts_in = parts_in; cons.hidden = H; cons.eps = m->cfg.eps; cons.ssq_ts = sc.ssq_ts; cons.x_blocked = true;
        PGV_TRY(gemv_mat(ctx, m, GV_STORE16, layer_mat(m, li, MAT_QKV), sc.xn, sc.qkv, 3 * H, B, s, &cons));
        PGV_TRY(step_attn(ctx, m, kv, sc, li, rows, rm, kv_bytes, s));
        GemvNorm prod; prod.gamma = l.post_g; prod.xg = sc.xn; prod.ssq_out = sc.ssq; prod.ssq_ts = sc.ssq_ts; prod.k8_part = sc.k8_part; prod.x_blocked = true;
        PGV_TRY(gemv_mat(ctx, m, GV_RESIDNORM, layer_mat(m, li, MAT_O), sc.ao, sc.resid, H, B, s, &prod));
        cons.nparts_in = nparts;
        PGV_TRY(gemv_mat(ctx, m, GV_SWIGLU, layer_mat(m, li, MAT_GU), sc.xn, sc.act, I, B, s, &cons));
        prod.gamma = li + 1 < L ? m->layers[li + 1].in_g : m->norm_g;
        PGV_TRY(gemv_mat(ctx, m, GV_RESIDNORM, layer_mat(m, li, MAT_DOWN), sc.act, sc.resid, H, B, s, &prod));
        parts_in = nparts;
    }
    *nparts_out = parts_in;
    return PGV_OK;
}

// a plain token step: the trunk over the live slots on the cache's own scratch, then lm_head and the pick
static int decode_enqueue(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int eos, int flags, hipStream_t s) {
    int nparts = 0;
    PGV_TRY(decode_trunk(ctx, m, kv, kv->sc, kv->d_cur, kv->active, RowMap{}, s, &nparts));
    return lm_head_and_pick(ctx, m, kv, kv->active, eos, flags, s, nparts);
}

static bool graphs_enabled() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("PGV_NO_GRAPH"); v = (e && e[0] == '1') ? 0 : 1; }
    return v == 1;
}

// Decode steps: eager the first time (loads code objects), then replayed from captured hipGraphs -- one graph holding kGraphSteps
// consecutive token steps (positions, current tokens and step counters live in device memory and are advanced by the pick kernel, so
// a graph is valid for any starting position) and one holding a single step for the remainder.  Per-family event timers need eager
// launches, so profiling disables the graphs.
constexpr int kGraphSteps = 8;

static int lookup_enqueue(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int eos, int flags, hipStream_t s);      // below: one prompt-lookup step
// one step of the kind on the stream: a plain token step, or a lookup step (pgv_llm_decode_lookup, with AM_SAMPLE pgv_llm_decode_lookup_sample)
static int step_enqueue(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, StepKind kind, int eos, int flags, hipStream_t s) {
    return kind == STEP_PLAIN ? decode_enqueue(ctx, m, kv, eos, flags, s) : lookup_enqueue(ctx, m, kv, eos, flags, s);
}
// captured lookup steps bake in the cache's D and n, which join the key
static int decode_graph(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, StepKind kind, int eos, int flags, int which, int steps, hipStream_t s) {
    const DecodeGraphKey key = decode_graph_key(kv_features(kv), kv->active, eos, flags, m->generation, kv->run, kind != STEP_PLAIN);
    if (!(kv->gkey == key)) {
        for (auto& g : kv->gexec) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
        kv->gkey = key;
    }
    if (!kv->gexec[which]) {
        // capture on a library-owned stream (the caller's may be the legacy default stream, which cannot be
        // captured); capture executes nothing, the instantiated graph is then launched on the caller's stream
        hipGraph_t graph = nullptr;
        if (!ctx->cap_stream) PGV_HIP(hipStreamCreateWithFlags(&ctx->cap_stream, hipStreamNonBlocking));
        PGV_HIP(hipStreamBeginCapture(ctx->cap_stream, hipStreamCaptureModeRelaxed));
        int rc = PGV_OK;
        for (int i = 0; i < steps && rc == PGV_OK; ++i) rc = step_enqueue(ctx, m, kv, kind, eos, flags, ctx->cap_stream);
        hipError_t e = hipStreamEndCapture(ctx->cap_stream, &graph);
        if (rc != PGV_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) { pgv_set_error("decode graph capture failed: %s", hipGetErrorString(e)); return PGV_EHIP; }
        e = hipGraphInstantiate(&kv->gexec[which], graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { kv->gexec[which] = nullptr; pgv_set_error("decode graph instantiate failed: %s", hipGetErrorString(e)); return PGV_EHIP; }
    }
    PGV_HIP(hipGraphLaunch(kv->gexec[which], s));
    return PGV_OK;
}

// n steps of one kind: eager while the kind has not run eagerly on this cache, under profiling or with PGV_NO_GRAPH=1; else the kGraphSteps-step
// graph while that many remain; else the one-step graph.  Only plain steps advance the host's lengths (a lookup step's live on the device).
static int run_steps(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, StepKind kind, int eos, int flags, int n, hipStream_t s) {
    while (n > 0) {
        int k = 1;
        if (ctx->prof || !graphs_enabled() || !kv->warmed[kind]) {
            kv->warmed[kind] = true;
            PGV_TRY(step_enqueue(ctx, m, kv, kind, eos, flags, s));
        } else if (n >= kGraphSteps) {
            k = kGraphSteps;
            PGV_TRY(decode_graph(ctx, m, kv, kind, eos, flags, 1, kGraphSteps, s));
        } else {
            PGV_TRY(decode_graph(ctx, m, kv, kind, eos, flags, 0, 1, s));
        }
        for (int b = 0; kind == STEP_PLAIN && b < kv->active; ++b) kv->h_len[b] += k;
        n -= k;
    }
    return PGV_OK;
}
static int decode_steps(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int eos, int flags, int n, hipStream_t s) {
    kv->lookup.valid = false;               // a plain step appends nothing to the id record
    return run_steps(ctx, m, kv, STEP_PLAIN, eos, flags, n, s);
}

static int check_decode(pgv_llm* m, pgv_kv* kv, int steps, const char* who) {
    PGV_CHECK(m && kv && kv->llm == m, "%s: bad model / cache", who);
    if (kv->active < 1) { pgv_set_error("%s: no prefilled sequences in this cache", who); return PGV_ESTATE; }
    for (int b = 0; b < kv->active; ++b)
        PGV_CHECK(kv->h_len[b] + steps <= kv->max_seq, "%s: sequence %d would grow to %d tokens (cache holds %d)", who, b, kv->h_len[b] + steps, kv->max_seq);
    return PGV_OK;
}

extern "C" int pgv_llm_decode(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* d_last, float* d_logits, int32_t* d_next, void* stream) {
    PGV_CHECK(ctx && d_last, "pgv_llm_decode: null argument");
    PGV_TRY(check_decode(m, kv, 1, "pgv_llm_decode"));
    hipStream_t s = (hipStream_t)stream;
    const int B = kv->active;
    beam_drop(kv);
    if (d_last != kv->d_cur) PGV_HIP(hipMemcpyAsync(kv->d_cur, d_last, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    PGV_TRY(decode_steps(ctx, m, kv, -1, AM_INC_POS, 1, s));
    if (d_logits) PGV_HIP(hipMemcpyAsync(d_logits, kv->sc.logits, (size_t)B * m->cfg.vocab * 4, hipMemcpyDeviceToDevice, s));
    if (d_next) PGV_HIP(hipMemcpyAsync(d_next, kv->d_cur, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

// n recorded steps from d_first, picking with *run (null: the arg-max of the lm_head candidates); a run's uniforms are in kv->d_u already
static int decode_run(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* d_first, int n, int eos_id, const PickParams* run, int32_t* d_tokens, hipStream_t s) {
    const int B = kv->active;
    beam_drop(kv);
    if (d_first != kv->d_cur) PGV_HIP(hipMemcpyAsync(kv->d_cur, d_first, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    PGV_HIP(hipMemsetAsync(kv->d_step, 0, (size_t)kv->B * 4, s));
    if (run) kv->run = *run;
    PGV_TRY(decode_steps(ctx, m, kv, eos_id, AM_INC_POS | AM_RECORD | (run ? AM_SAMPLE : 0), n, s));
    kv->lp.steps = kv->lp.on ? n : -1;
    PGV_HIP(hipMemcpy2DAsync(d_tokens, (size_t)n * 4, kv->d_hist, (size_t)kv->max_seq * 4, (size_t)n * 4, B, hipMemcpyDeviceToDevice, s));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

extern "C" int pgv_llm_decode_greedy(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* d_first, int n, int eos_id, int32_t* d_tokens, void* stream) {
    PGV_CHECK(ctx && d_first && d_tokens, "pgv_llm_decode_greedy: null argument");
    PGV_CHECK(n >= 1, "pgv_llm_decode_greedy: n must be positive");
    PGV_TRY(check_decode(m, kv, n, "pgv_llm_decode_greedy"));
    PGV_TRY(guidance_width(kv, "pgv_llm_decode_greedy"));
    if (!kv_greedy_sampled(kv)) return decode_run(ctx, m, kv, d_first, n, eos_id, nullptr, d_tokens, (hipStream_t)stream);
    const PickParams p = pick_greedy(kv->warpers.penalty);
    PGV_TRY(pgv_zero_uniforms(kv->d_u, (size_t)n * kv->active, (hipStream_t)stream));
    return decode_run(ctx, m, kv, d_first, n, eos_id, &p, d_tokens, (hipStream_t)stream);
}

// one pick on the logits the last prefill / decode call left: the cache's state takes the token, nothing advances
static int pick_last(pgv_kv* kv, const PickParams& p, const float* d_u, int32_t* d_next, hipStream_t s) {
    beam_drop(kv);
    PGV_TRY(kv_pick(kv, kv->active, &p, d_u, false, kv_state(kv, -1, 0), nullptr, s));
    if (d_next) PGV_HIP(hipMemcpyAsync(d_next, kv->d_cur, (size_t)kv->active * 4, hipMemcpyDeviceToDevice, s));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

extern "C" int pgv_llm_sample(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, float temperature, int top_k, const float* d_u, int32_t* d_next, void* stream) {
    PGV_CHECK(ctx && d_u, "pgv_llm_sample: null argument");
    PGV_TRY(check_decode(m, kv, 0, "pgv_llm_sample"));
    PGV_TRY(guidance_width(kv, "pgv_llm_sample"));
    return pick_last(kv, kv_sampled(kv, temperature, top_k), d_u, d_next, (hipStream_t)stream);
}

extern "C" int pgv_llm_pick_greedy(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int32_t* d_next, void* stream) {
    PGV_CHECK(ctx != nullptr, "pgv_llm_pick_greedy: null argument");
    PGV_TRY(check_decode(m, kv, 0, "pgv_llm_pick_greedy"));
    PGV_TRY(guidance_width(kv, "pgv_llm_pick_greedy"));
    PGV_TRY(pgv_zero_uniforms(kv->d_u, kv->active, (hipStream_t)stream));
    return pick_last(kv, pick_greedy(kv->warpers.penalty), kv->d_u, d_next, (hipStream_t)stream);      // as pgv_llm_decode_greedy steps under a penalty
}

extern "C" int pgv_llm_decode_sample(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* d_first, int n, int eos_id, float temperature, int top_k,
                                     const float* d_u, int32_t* d_tokens, void* stream) {
    PGV_CHECK(ctx && d_first && d_tokens && d_u, "pgv_llm_decode_sample: null argument");
    PGV_CHECK(n >= 1, "pgv_llm_decode_sample: n must be positive");
    PGV_CHECK(temperature > 0.f, "pgv_llm_decode_sample: temperature must be positive (got %g)", (double)temperature);
    PGV_TRY(check_decode(m, kv, n, "pgv_llm_decode_sample"));
    PGV_TRY(guidance_width(kv, "pgv_llm_decode_sample"));
    PGV_HIP(hipMemcpyAsync(kv->d_u, d_u, (size_t)n * kv->active * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));     // n <= max_seq (check_decode)
    const PickParams p = kv_sampled(kv, temperature, top_k);
    return decode_run(ctx, m, kv, d_first, n, eos_id, &p, d_tokens, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// beam search (pgv.h; kernels: beam.hip)
// ---------------------------------------------------------------------------------------------
static int upload_ints(pgv_ctx* ctx, const std::vector<int>& h, int** d, hipStream_t s);      // below: host values through the workspace arena
static int beam_check_config(const char* who, const pgv_beam_config* c, int V) {
    PGV_CHECK(c != nullptr, "%s: null configuration", who);
    PGV_CHECK(c->beams >= 1 && c->beams <= 8, "%s: beams %d outside [1,8]", who, c->beams);
    PGV_CHECK(c->max_new_tokens >= 1, "%s: max_new_tokens %d is below 1", who, c->max_new_tokens);
    PGV_CHECK(c->early_stopping >= 0 && c->early_stopping <= 2, "%s: early_stopping %d is not 0 (False), 1 (True) or 2 (\"never\")", who, c->early_stopping);
    PGV_CHECK(isfinite(c->length_penalty), "%s: length_penalty is not finite", who);
    PGV_CHECK(c->eos_id < V, "%s: eos_id %d outside the vocabulary (%d)", who, c->eos_id, V);
    PGV_CHECK(V >= 2 * c->beams, "%s: a vocabulary of %d has no %d candidates", who, V, 2 * c->beams);
    return PGV_OK;
}
// HF divides by (length ** length_penalty), a Python float, rounded to fp32 by the division
static float beam_denom(int len, float length_penalty) { return (float)pow((double)len, (double)length_penalty); }

extern "C" int pgv_kv_gather(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int K, const int32_t* h_src, const int32_t* h_row0, void* stream) {
    PGV_CHECK(ctx && m && kv && h_src && h_row0, "pgv_kv_gather: null argument");
    PGV_CHECK(kv->llm == m, "pgv_kv_gather: kv cache belongs to another model");
    if (kv->active < 1) { pgv_set_error("pgv_kv_gather: no live group in this cache (run pgv_llm_prefill first)"); return PGV_ESTATE; }
    const int W = kv->active;
    PGV_CHECK(K >= 1 && K <= 8, "pgv_kv_gather: group width %d outside [1,8]", K);
    PGV_CHECK(W % K == 0, "pgv_kv_gather: the live group of %d sequences is no multiple of the group width %d", W, K);
    const int P = W / K;
    std::vector<int> up((size_t)W + P);
    for (int i = 0; i < W; ++i) {
        PGV_CHECK(h_src[i] >= 0 && h_src[i] < K, "pgv_kv_gather: source %d of slot %d outside [0,%d)", h_src[i], i, K);
        PGV_CHECK(kv->h_len[i] == kv->h_len[i / K * K], "pgv_kv_gather: slots %d and %d of one group hold %d and %d tokens", i / K * K, i, kv->h_len[i / K * K], kv->h_len[i]);
        up[i] = h_src[i];
    }
    for (int p = 0; p < P; ++p) {
        PGV_CHECK(h_row0[p] >= 1 && h_row0[p] <= kv->h_len[p * K], "pgv_kv_gather: row0 %d of group %d outside [1,%d]", h_row0[p], p, kv->h_len[p * K]);
        up[(size_t)W + p] = h_row0[p];
    }
    beam_drop(kv);
    hipStream_t s = (hipStream_t)stream;
    int* d_up = nullptr;
    PGV_TRY(upload_ints(ctx, up, &d_up, s));
    PGV_TRY(pgv_launch_kv_gather(kv_gather_args(kv, K, P, d_up, d_up + W, kv->d_cur), s));
    PGV_HIP(hipGetLastError());
    PGV_TRY(pgv_ws_release(ctx, s));
    return PGV_OK;
}

extern "C" int pgv_beam_begin(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const pgv_beam_config* cfg, void* stream) {
    PGV_CHECK(ctx && m && kv, "pgv_beam_begin: null argument");
    PGV_CHECK(kv->llm == m, "pgv_beam_begin: kv cache belongs to another model");
    PGV_TRY(beam_check_config("pgv_beam_begin", cfg, m->cfg.vocab));
    PGV_TRY(kv_allows(kv, KV_BEAM_BEGIN, "pgv_beam_begin"));
    if (kv->active < 1) { pgv_set_error("pgv_beam_begin: no live group in this cache (run pgv_llm_prefill first)"); return PGV_ESTATE; }
    PGV_TRY(kv_allows(kv, KV_BEAM_BEGIN, "pgv_beam_begin", 1));
    const int P = kv->active, K = cfg->beams, N = cfg->max_new_tokens, B = kv->B;
    PGV_CHECK((long long)P * K <= B, "pgv_beam_begin: %d prompts x %d beams exceed the %d sequences the cache was created with", P, K, B);
    PGV_CHECK(N <= kv->max_seq, "pgv_beam_begin: max_new_tokens %d exceeds the cache's %d positions", N, kv->max_seq);
    for (int p = 0; p < P; ++p)
        PGV_CHECK(kv->h_len[p] + N - 1 <= kv->max_seq, "pgv_beam_begin: sequence %d would grow to %d tokens (cache holds %d)", p, kv->h_len[p] + N - 1, kv->max_seq);
    hipStream_t s = (hipStream_t)stream;
    const size_t SW = PGV_BEAM_STATE_WORDS(8);
    if (!kv->beam.blob.p) {
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off += pgv_align(bytes); return o; };
        const size_t o_state = take((size_t)B * SW * 4), o_map = take((size_t)B * 4), o_row0 = take((size_t)B * 4), o_t = take((size_t)B * 4), o_prm = take(sizeof(BeamParams)),
                     o_den = take((size_t)kv->max_seq * 4), o_hist = take((size_t)2 * kv->max_seq * B * 4);
        PGV_TRY(kv->beam.blob.alloc("pgv_beam_begin", off));
        char* b = kv->beam.blob.p;
        kv->beam.state = (unsigned*)(b + o_state); kv->beam.map = (int*)(b + o_map); kv->beam.row0 = (int*)(b + o_row0); kv->beam.t = (int*)(b + o_t);
        kv->beam.prm = (BeamParams*)(b + o_prm); kv->beam.denom = (float*)(b + o_den); kv->beam.hist = (int*)(b + o_hist);
    }
    // host staging: state words of the P prompts | row0 [P] | parameters | denom [N]
    const int S = PGV_BEAM_STATE_WORDS(K);
    std::vector<unsigned>& st = kv->beam.stage;
    st.assign((size_t)P * S + P + 4 + N, 0u);
    auto fbits = [](float f) { unsigned u; memcpy(&u, &f, 4); return u; };
    for (int p = 0; p < P; ++p) {
        unsigned* w = st.data() + (size_t)p * S;
        for (int i = 0; i < K; ++i) { w[i] = fbits(i == 0 ? 0.f : -1.0e9f); w[K + i] = fbits(-1.0e9f); }
        w[6 * K] = 1u; w[6 * K + 1] = 1u;
        st[(size_t)P * S + p] = (unsigned)kv->h_len[p];
    }
    unsigned* hp = st.data() + (size_t)P * S + P;
    hp[0] = (unsigned)N; hp[1] = (unsigned)cfg->eos_id; hp[2] = (unsigned)cfg->early_stopping; hp[3] = fbits(cfg->length_penalty);
    for (int i = 0; i < N; ++i) hp[4 + i] = fbits(beam_denom(i + 1, cfg->length_penalty));
    if (K > 1) {
        std::vector<int32_t> counts((size_t)P, K);
        PGV_TRY(pgv_kv_fork(ctx, m, kv, counts.data(), P, stream));
    }
    PGV_HIP(hipMemcpyAsync(kv->beam.state, st.data(), (size_t)P * S * 4, hipMemcpyHostToDevice, s));
    PGV_HIP(hipMemcpyAsync(kv->beam.row0, st.data() + (size_t)P * S, (size_t)P * 4, hipMemcpyHostToDevice, s));
    PGV_HIP(hipMemcpyAsync(kv->beam.prm, hp, sizeof(BeamParams), hipMemcpyHostToDevice, s));
    PGV_HIP(hipMemcpyAsync(kv->beam.denom, hp + 4, (size_t)N * 4, hipMemcpyHostToDevice, s));
    PGV_HIP(hipMemsetAsync(kv->beam.t, 0, (size_t)B * 4, s));
    kv->beam.K = K; kv->beam.P = P; kv->beam.N = N; kv->beam.steps = 0;
    // the first pick, on the logits of the prefill (pgv_kv_fork copied the row of every prompt to its K slots); nothing to gather yet
    int rc = beam_pick_and_gather(ctx, kv, false, s);
    if (rc == PGV_OK) { hipError_t e = hipGetLastError(); if (e != hipSuccess) { pgv_set_error("pgv_beam_begin: %s", hipGetErrorString(e)); rc = PGV_EHIP; } }
    if (rc != PGV_OK) { beam_drop(kv); return rc; }
    kv->beam.steps = 1;
    return PGV_OK;
}

static int beam_live(const pgv_kv* kv, const char* who) {
    PGV_CHECK(kv != nullptr, "%s: null cache", who);
    if (kv->beam.K < 1 || kv->active != kv->beam.P * kv->beam.K) { pgv_set_error("%s: no beam run on this cache (pgv_beam_begin starts one; any other call that moves its slots ends it)", who); return PGV_ESTATE; }
    return PGV_OK;
}

extern "C" int pgv_llm_decode_beam(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int n, void* stream) {
    PGV_CHECK(ctx != nullptr, "pgv_llm_decode_beam: null argument");
    PGV_CHECK(n >= 1, "pgv_llm_decode_beam: n must be positive");
    PGV_TRY(check_decode(m, kv, n, "pgv_llm_decode_beam"));
    PGV_TRY(beam_live(kv, "pgv_llm_decode_beam"));
    PGV_CHECK(kv->beam.steps + n <= kv->beam.N, "pgv_llm_decode_beam: %d picks done + %d steps exceed max_new_tokens %d", kv->beam.steps, n, kv->beam.N);
    PGV_TRY(decode_steps(ctx, m, kv, -1, AM_INC_POS | AM_BEAM, n, (hipStream_t)stream));
    kv->beam.steps += n;
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

extern "C" int pgv_beam_open(pgv_kv* kv, int32_t* h_open, void* stream) {
    PGV_TRY(beam_live(kv, "pgv_beam_open"));
    PGV_CHECK(h_open != nullptr, "pgv_beam_open: null argument");
    const int K = kv->beam.K, S = PGV_BEAM_STATE_WORDS(K);
    PGV_HIP(hipMemcpy2DAsync(h_open, 4, kv->beam.state + 6 * K + 1, (size_t)S * 4, 4, kv->beam.P, hipMemcpyDeviceToHost, (hipStream_t)stream));
    PGV_HIP(hipStreamSynchronize((hipStream_t)stream));
    return PGV_OK;
}

extern "C" int pgv_beam_result(pgv_kv* kv, int p, int rank, int32_t* h_tokens, int cap, int32_t* n_out, float* score_out, int32_t* finished_out, void* stream) {
    PGV_TRY(beam_live(kv, "pgv_beam_result"));
    const int K = kv->beam.K, S = PGV_BEAM_STATE_WORDS(K);
    PGV_CHECK(p >= 0 && p < kv->beam.P && rank >= 0 && rank < K, "pgv_beam_result: prompt %d / rank %d outside the run's %d prompts x %d beams", p, rank, kv->beam.P, K);
    hipStream_t s = (hipStream_t)stream;
    std::vector<unsigned> st((size_t)S);
    PGV_HIP(hipMemcpyAsync(st.data(), kv->beam.state + (size_t)p * S, (size_t)S * 4, hipMemcpyDeviceToHost, s));
    PGV_HIP(hipStreamSynchronize(s));
    float score; memcpy(&score, &st[K + rank], 4);
    const int n = (int)st[2 * K + rank], flag = (int)st[5 * K + rank];
    int par = (int)st[3 * K + rank];
    PGV_CHECK(n >= 0 && n <= kv->beam.steps, "pgv_beam_result: the state holds a hypothesis of %d tokens after %d picks", n, kv->beam.steps);
    if (n_out) *n_out = n;
    if (score_out) *score_out = score;
    if (finished_out) *finished_out = flag;
    if (!h_tokens || n == 0) return PGV_OK;
    PGV_CHECK(cap >= n, "pgv_beam_result: room for %d tokens, the hypothesis has %d", cap, n);
    h_tokens[n - 1] = (int32_t)st[4 * K + rank];
    if (n == 1) return PGV_OK;
    // the tokens before the last: back through the parents of picks n - 2 .. 0 (the group's K columns of the history)
    std::vector<int> hist((size_t)2 * (n - 1) * K);
    const size_t pitch = (size_t)kv->B * 4;
    PGV_HIP(hipMemcpy2DAsync(hist.data(), (size_t)K * 4, kv->beam.hist + p * K, pitch, (size_t)K * 4, n - 1, hipMemcpyDeviceToHost, s));
    PGV_HIP(hipMemcpy2DAsync(hist.data() + (size_t)(n - 1) * K, (size_t)K * 4, kv->beam.hist + (size_t)kv->max_seq * kv->B + p * K, pitch, (size_t)K * 4, n - 1, hipMemcpyDeviceToHost, s));
    PGV_HIP(hipStreamSynchronize(s));
    for (int u = n - 2; u >= 0; --u) {
        PGV_CHECK(par >= 0 && par < K, "pgv_beam_result: parent %d outside the group at pick %d", par, u + 1);
        h_tokens[u] = hist[(size_t)u * K + par];
        par = hist[(size_t)(n - 1 + u) * K + par];
    }
    return PGV_OK;
}

extern "C" int pgv_beam_pick_logits(pgv_ctx* ctx, const float* d_logits, int V, int P, const pgv_beam_config* cfg, int t, uint32_t* d_state, int32_t* d_tokens,
                                    int32_t* d_parents, void* stream) {
    PGV_CHECK(ctx && d_logits && d_state && d_tokens && d_parents, "pgv_beam_pick_logits: null argument");
    PGV_CHECK(V >= 1, "pgv_beam_pick_logits: vocabulary %d is below 1", V);
    PGV_TRY(beam_check_config("pgv_beam_pick_logits", cfg, V));
    const int K = cfg->beams;
    PGV_CHECK(P >= 1 && P * K <= kMaxBatch, "pgv_beam_pick_logits: %d prompts x %d beams outside [1,%d] rows", P, K, kMaxBatch);
    PGV_CHECK(t >= 0 && t < cfg->max_new_tokens, "pgv_beam_pick_logits: step %d outside [0,%d)", t, cfg->max_new_tokens);
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = pgv_align((size_t)P * K * 2 * 4);
    PGV_TRY(pgv_ws_reserve(ctx, bytes, s));
    float* stat = (float*)pgv_ws_alloc(ctx, bytes);
    PGV_CHECK(stat != nullptr, "pgv_beam_pick_logits: workspace exhausted");
    PGV_TRY(pgv_launch_row_lse(d_logits, V, V, P * K, stat, s));
    BeamPickArgs a{};
    a.logits = d_logits; a.ld = V; a.V = V; a.K = K; a.stat = stat;
    a.state = d_state; a.state_stride = PGV_BEAM_STATE_WORDS(K);
    a.t_val = t; a.prm_val = BeamParams{cfg->max_new_tokens, cfg->eos_id, cfg->early_stopping, cfg->length_penalty};
    a.den_t = beam_denom(t + 1, cfg->length_penalty); a.den_n = beam_denom(cfg->max_new_tokens, cfg->length_penalty);
    a.cur = d_tokens; a.map = d_parents;
    PGV_TRY(pgv_launch_beam_pick(a, P, s));
    PGV_HIP(hipGetLastError());
    PGV_TRY(pgv_ws_release(ctx, s));
    return PGV_OK;
}

// ---------------------------------------------------------------------------------------------
// row-wise steps (pgv.h: pgv_kv_set_lookup, pgv_llm_decode_rows)
// ---------------------------------------------------------------------------------------------
extern "C" int pgv_kv_set_lookup(pgv_kv* kv, int D, int n) {
    PGV_CHECK(kv != nullptr, "pgv_kv_set_lookup: null cache");
    PGV_CHECK(D >= 0 && D <= 15, "pgv_kv_set_lookup: %d draft rows per slot outside [0,15]", D);
    if (D == 0) { kv->lookup.D = 0; kv->lookup.valid = false; return PGV_OK; }
    PGV_TRY(kv_allows(kv, KV_SET_LOOKUP, "pgv_kv_set_lookup"));
    PGV_CHECK(n >= 1 && n <= 4, "pgv_kv_set_lookup: ngram size %d outside [1,4]", n);
    PGV_TRY(kv_ids_alloc(kv, "pgv_kv_set_lookup"));
    if (!kv->lookup.blob.p) {
        // sized once for the most rows any setting can ask of this cache: the per-row decode buffers for R rows, then the lookup ints
        const size_t B = kv->B, R = kMaxBatch < kv->B * 16 ? kMaxBatch : kv->B * 16;
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off += pgv_align(bytes); return o; };
        const ScratchLayout so = scratch_layout(kv->llm, R, take);
        const size_t o_ints = take((5 * R + 3 * B + 1 + B * (size_t)kv->max_seq) * 4);
        PGV_TRY(kv->lookup.blob.alloc("pgv_kv_set_lookup", off, 20));
        char* b = kv->lookup.blob.p;
        const hipError_t e = hipMemset(b, 0, off);       // beyond scratch_clear: rows no step has written yet are read by the GEMVs of a step with absent rows
        if (e != hipSuccess) { kv->lookup.blob.drop(); pgv_set_error("pgv_kv_set_lookup: memset: %s", hipGetErrorString(e)); return PGV_EHIP; }
        kv->lookup.sc = scratch_bind(b, so, kv->llm);
        int* ints = (int*)(b + o_ints);
        kv->lookup.slot = ints; kv->lookup.j = ints + R; kv->lookup.tok = ints + 2 * R; kv->lookup.t = ints + 3 * R;
        kv->lookup.u = (float*)(ints + 4 * R);
        kv->lookup.ndraft = ints + 5 * R; kv->lookup.budget = kv->lookup.ndraft + B; kv->lookup.ubase = kv->lookup.budget + B; kv->lookup.k = kv->lookup.ubase + B; kv->lookup.counts = kv->lookup.k + 1;
        kv->lookup.rows = (int)R;
    }
    kv->lookup.D = D; kv->lookup.n = n;
    return PGV_OK;
}

extern "C" int pgv_kv_lookup(const pgv_kv* kv) { return kv ? kv->lookup.D : -1; }

// One prompt-lookup step over the live slots: draft -> row-wise trunk -> lm_head -> row-wise pick -> accept.  The pick is the arg-max of the lm_head
// candidates, or with AM_SAMPLE the sampled pick with kv->run over the full logits of every row, fed the uniform the draft kernel gathered for the
// row (pgv.h: u[u_base + step + j][b]).  Either pick writes the row's token and nothing else: the accept kernel keeps the slots' state.
static int lookup_enqueue(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, int eos, int flags, hipStream_t s) {
    const int B = kv->active, R = B * (1 + kv->lookup.D), V = m->cfg.vocab;
    const bool sampled = flags & AM_SAMPLE;
    LookupArgs a;
    a.D = kv->lookup.D; a.n = kv->lookup.n; a.eos = eos; a.max_seq = kv->max_seq;
    a.pos = kv->d_pos; a.cur = kv->d_cur; a.step = kv->d_step; a.done = kv->d_done; a.hist = kv->d_hist; a.hist_stride = kv->max_seq;
    a.rec = kv->ids.ids; a.budget = kv->lookup.budget;
    a.tok = kv->lookup.tok; a.row_slot = kv->lookup.slot; a.row_j = kv->lookup.j; a.n_draft = kv->lookup.ndraft; a.t = kv->lookup.t;
    a.counts = kv->lookup.counts; a.counts_stride = kv->B; a.k = kv->lookup.k;
    if (sampled) {
        a.u = kv->d_u; a.u_stride = B; a.u_base = kv->lookup.ubase; a.u_row = kv->lookup.u;
        // a plain sampled step marks the token it returns in the slot's seen-set in the instantiations that carry the set (pgv_launch_sample)
        if (kv->run.filtered() || kv->run.top_p < 1.f) { a.seen = kv->d_seen; a.seen_words = kv->seen_words; a.vocab = V; }
    }
    pgv_prof_begin(ctx, 6, s);
    PGV_TRY(pgv_launch_lookup_draft(a, B, s));
    pgv_prof_end(ctx, 6, s, 0.0, 0.0);
    RowMap rm; rm.d_slot = kv->lookup.slot; rm.d_j = kv->lookup.j;
    int nparts = 0;
    PGV_TRY(decode_trunk(ctx, m, kv, kv->lookup.sc, kv->lookup.tok, R, rm, s, &nparts));
    PGV_TRY(lm_head_rows(ctx, m, kv->lookup.sc, R, !sampled, s, nparts));
    pgv_prof_begin(ctx, 6, s);
    if (sampled) PGV_TRY(pgv_launch_sample(kv->lookup.sc.logits, V, R, kv->run, kv->lookup.u, R, false, PickState{kv->lookup.t}, s));
    else PGV_TRY(pgv_launch_argmax_parts(kv->lookup.sc.amax_val, kv->lookup.sc.amax_idx, (V + 15) / 16, kv->lookup.sc.amax_ts, V, R, PickState{kv->lookup.t}, s));
    PGV_TRY(pgv_launch_lookup_accept(a, B, s));
    pgv_prof_end(ctx, 6, s, 0.0, 0.0);
    return PGV_OK;
}

// what both lookup entries refuse, before any device work
static int check_lookup_run(pgv_llm* m, pgv_kv* kv, int steps, int eos_id, const int32_t* h_budget, const char* who, const char* verifies) {
    PGV_TRY(check_decode(m, kv, 0, who));
    PGV_TRY(kv_allows(kv, KV_LOOKUP_RUN, who));
    const int B = kv->active, D = kv->lookup.D, W = 1 + D;
    if (D < 1) { pgv_set_error("%s: lookup is off on this cache (pgv_kv_set_lookup)", who); return PGV_ESTATE; }
    if (!kv->lookup.valid) { pgv_set_error("%s: the cache's id record does not cover its sequences: set pgv_kv_set_lookup before pgv_llm_prefill and step with pgv_llm_decode_lookup only", who); return PGV_ESTATE; }
    PGV_TRY(kv_allows(kv, KV_LOOKUP_RUN, who, 1, verifies));
    PGV_CHECK(B * W <= kv->lookup.rows && B * W <= kMaxBatch, "%s: %d sequences x %d rows exceed the %d rows of a step", who, B, W, kv->lookup.rows < kMaxBatch ? kv->lookup.rows : kMaxBatch);
    PGV_CHECK(steps >= 1 && steps <= kv->max_seq, "%s: %d steps outside [1,%d]", who, steps, kv->max_seq);
    PGV_CHECK(eos_id < m->cfg.vocab, "%s: eos_id %d outside the vocabulary (%d)", who, eos_id, m->cfg.vocab);
    for (int b = 0; b < B; ++b)
        PGV_CHECK(h_budget[b] >= 0 && kv->h_len[b] + h_budget[b] <= kv->max_seq, "%s: sequence %d would grow to %d tokens (cache holds %d)", who, b,
                  kv->h_len[b] + h_budget[b], kv->max_seq);
    return PGV_OK;
}

// `steps` lookup steps behind the checks.  run null: the greedy form; else the sampled one, picking with *run from the uniforms d_u [u_rows][B]
// (copied into the cache's) at the rows h_u_base counts from.
static int lookup_run(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* d_first, int steps, int eos_id, const int32_t* h_budget, const int32_t* h_u_base,
                      const PickParams* run, const float* d_u, int u_rows, int32_t* d_tokens, int32_t* d_counts, hipStream_t s) {
    const int B = kv->active, W = 1 + kv->lookup.D;
    const int flags = AM_INC_POS | AM_RECORD | (run ? AM_SAMPLE : 0);
    PGV_HIP(hipStreamSynchronize(s));             // an earlier call's copy of the staging may still be pending
    kv->lookup.stage.assign(h_budget, h_budget + B);
    if (run) kv->lookup.stage.insert(kv->lookup.stage.end(), h_u_base, h_u_base + B);
    PGV_HIP(hipMemcpyAsync(kv->lookup.budget, kv->lookup.stage.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    if (run) {
        PGV_HIP(hipMemcpyAsync(kv->lookup.ubase, kv->lookup.stage.data() + B, (size_t)B * 4, hipMemcpyHostToDevice, s));
        PGV_HIP(hipMemcpyAsync(kv->d_u, d_u, (size_t)u_rows * B * 4, hipMemcpyDeviceToDevice, s));      // u_rows <= max_seq (checked by the entry)
        kv->run = *run;
    }
    if (d_first && d_first != kv->d_cur) PGV_HIP(hipMemcpyAsync(kv->d_cur, d_first, (size_t)B * 4, hipMemcpyDeviceToDevice, s));      // null: the cache's current tokens
    PGV_HIP(hipMemsetAsync(kv->d_step, 0, (size_t)kv->B * 4, s));
    PGV_HIP(hipMemsetAsync(kv->lookup.k, 0, 4, s));
    PGV_HIP(hipMemsetAsync(kv->lookup.sc.dattn_ticket, 0, (size_t)B * W * m->cfg.heads * sizeof(unsigned), s));
    PGV_TRY(run_steps(ctx, m, kv, run ? STEP_LOOKUP_SAMPLED : STEP_LOOKUP, eos_id, flags, steps, s));
    kv->lp.steps = -1;
    const int cap = steps * W < kv->max_seq ? steps * W : kv->max_seq;
    PGV_HIP(hipMemcpy2DAsync(d_tokens, (size_t)steps * W * 4, kv->d_hist, (size_t)kv->max_seq * 4, (size_t)cap * 4, B, hipMemcpyDeviceToDevice, s));
    PGV_HIP(hipMemcpy2DAsync(d_counts, (size_t)B * 4, kv->lookup.counts, (size_t)kv->B * 4, (size_t)B * 4, steps, hipMemcpyDeviceToDevice, s));
    // the lengths now live on the device only: one blocking copy makes h_len true again (the caller reads the tokens at this point anyway)
    PGV_HIP(hipMemcpyAsync(kv->h_len.data(), kv->d_pos, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    PGV_HIP(hipStreamSynchronize(s));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

extern "C" int pgv_llm_decode_lookup(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* d_first, int steps, int eos_id, const int32_t* h_budget,
                                     int32_t* d_tokens, int32_t* d_counts, void* stream) {
    PGV_CHECK(ctx && h_budget && d_tokens && d_counts, "pgv_llm_decode_lookup: null argument");
    PGV_TRY(check_lookup_run(m, kv, steps, eos_id, h_budget, "pgv_llm_decode_lookup", "the plain arg-max"));
    return lookup_run(ctx, m, kv, d_first, steps, eos_id, h_budget, nullptr, nullptr, nullptr, 0, d_tokens, d_counts, (hipStream_t)stream);
}

extern "C" int pgv_llm_decode_lookup_sample(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* d_first, int steps, int eos_id, const int32_t* h_budget,
                                            const int32_t* h_u_base, float temperature, int top_k, const float* d_u, int u_rows, int32_t* d_tokens,
                                            int32_t* d_counts, void* stream) {
    const char* who = "pgv_llm_decode_lookup_sample";
    PGV_CHECK(ctx && h_budget && h_u_base && d_u && d_tokens && d_counts, "%s: null argument", who);
    PGV_CHECK(temperature > 0.f, "%s: temperature must be positive (got %g)", who, (double)temperature);
    PGV_TRY(check_lookup_run(m, kv, steps, eos_id, h_budget, who, "the plain pick without them"));
    PGV_CHECK(u_rows >= 1 && u_rows <= kv->max_seq, "%s: %d rows of uniforms outside [1,%d]", who, u_rows, kv->max_seq);
    for (int b = 0; b < kv->active; ++b)
        PGV_CHECK(h_u_base[b] >= 0 && (long long)h_u_base[b] + h_budget[b] <= u_rows, "%s: sequence %d would read uniform rows [%d,%lld) of %d", who, b, h_u_base[b],
                  (long long)h_u_base[b] + h_budget[b], u_rows);
    const PickParams p = kv_sampled(kv, temperature, top_k);
    return lookup_run(ctx, m, kv, d_first, steps, eos_id, h_budget, h_u_base, &p, d_u, u_rows, d_tokens, d_counts, (hipStream_t)stream);
}

extern "C" int pgv_llm_decode_rows(pgv_ctx* ctx, pgv_llm* m, pgv_kv* kv, const int32_t* h_slots, const int32_t* d_tokens, int R, float* d_logits, void* stream) {
    PGV_CHECK(ctx && h_slots && d_tokens && d_logits, "pgv_llm_decode_rows: null argument");
    PGV_TRY(check_decode(m, kv, 0, "pgv_llm_decode_rows"));
    if (kv->lookup.D < 1) { pgv_set_error("pgv_llm_decode_rows: this cache has no row scratch (pgv_kv_set_lookup allocates it)"); return PGV_ESTATE; }
    PGV_CHECK(R >= 1 && R <= kv->lookup.rows, "pgv_llm_decode_rows: %d rows outside [1,%d]", R, kv->lookup.rows);
    // rows are listed per slot in order: row j of a slot's run sits at position h_len + j
    std::vector<int>& map = kv->lookup.stage;
    std::vector<int> count((size_t)kv->active, 0);
    map.assign((size_t)2 * R, 0);
    for (int r = 0; r < R; ++r) {
        const int b = h_slots[r];
        PGV_CHECK(b >= 0 && b < kv->active, "pgv_llm_decode_rows: slot %d of row %d outside the %d prefilled sequences", b, r, kv->active);
        PGV_CHECK(count[b] == 0 || h_slots[r - 1] == b, "pgv_llm_decode_rows: the rows of slot %d are not consecutive (row %d)", b, r);
        PGV_CHECK(count[b] <= kv->lookup.D, "pgv_llm_decode_rows: more than the %d rows per slot pgv_kv_set_lookup set (slot %d)", 1 + kv->lookup.D, b);
        PGV_CHECK(kv->h_len[b] + count[b] < kv->max_seq, "pgv_llm_decode_rows: sequence %d would grow to %d tokens (cache holds %d)", b, kv->h_len[b] + count[b] + 1, kv->max_seq);
        map[r] = b; map[(size_t)R + r] = count[b]++;
    }
    hipStream_t s = (hipStream_t)stream;
    PGV_HIP(hipStreamSynchronize(s));             // an earlier call's copy of the staging may still be pending
    PGV_HIP(hipMemcpyAsync(kv->lookup.slot, map.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    PGV_HIP(hipMemcpyAsync(kv->lookup.j, map.data() + R, (size_t)R * 4, hipMemcpyHostToDevice, s));
    PGV_HIP(hipMemsetAsync(kv->lookup.sc.dattn_ticket, 0, (size_t)R * m->cfg.heads * sizeof(unsigned), s));      // as every prefill does for the cache's own
    RowMap rm; rm.d_slot = kv->lookup.slot; rm.d_j = kv->lookup.j; rm.h_slot = map.data(); rm.h_j = map.data() + R;
    int nparts = 0;
    PGV_TRY(decode_trunk(ctx, m, kv, kv->lookup.sc, d_tokens, R, rm, s, &nparts));
    PGV_TRY(lm_head_rows(ctx, m, kv->lookup.sc, R, false, s, nparts));
    PGV_HIP(hipMemcpyAsync(d_logits, kv->lookup.sc.logits, (size_t)R * m->cfg.vocab * 4, hipMemcpyDeviceToDevice, s));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

// ---------------------------------------------------------------------------------------------
// attention building blocks (pgv.h): the launchers of prefill_impl / decode_enqueue* on caller buffers, for unit parity tests
// ---------------------------------------------------------------------------------------------
// Host values reach the device through the workspace arena; the stream is synchronised once after the upload so the host staging need not
// outlive the call.  Every position is checked here, on the host: the kernels index the cache and the RoPE table with them unchecked.
static int upload_ints(pgv_ctx* ctx, const std::vector<int>& h, int** d, hipStream_t s) {
    const size_t bytes = pgv_align(h.size() * 4);
    PGV_TRY(pgv_ws_reserve(ctx, bytes, s));
    *d = (int*)pgv_ws_alloc(ctx, bytes);
    PGV_CHECK(*d != nullptr, "attention building block: workspace exhausted");
    PGV_HIP(hipMemcpyAsync(*d, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
    PGV_HIP(hipStreamSynchronize(s));
    return PGV_OK;
}

extern "C" int pgv_decode_attention(pgv_ctx* ctx, pgv_llm* m, const void* d_qkv, const int32_t* h_pos, void* d_Kc, void* d_Vc, void* d_out, int B,
                                    int max_seq, int split, float* d_part, uint32_t* d_ticket, void* stream) {
    PGV_CHECK(ctx && m && d_qkv && h_pos && d_Kc && d_Vc && d_out && d_part && d_ticket, "pgv_decode_attention: null argument");
    PGV_CHECK(B >= 1 && B <= kMaxBatch, "pgv_decode_attention: batch %d outside [1,%d]", B, kMaxBatch);
    PGV_CHECK(max_seq >= 1 && max_seq <= kMaxPos, "pgv_decode_attention: max_seq %d outside [1,%d]", max_seq, kMaxPos);
    PGV_CHECK(split == 0 || split == 1 || split == 2 || split == 4 || split == 8, "pgv_decode_attention: split %d is not 0, 1, 2, 4 or 8", split);
    std::vector<int> pos(h_pos, h_pos + B);
    double bytes = 0;
    for (int b = 0; b < B; ++b) {
        PGV_CHECK(pos[b] >= 0 && pos[b] < max_seq, "pgv_decode_attention: position %d of sequence %d outside [0,%d)", pos[b], b, max_seq);
        bytes += 2.0 * 2.0 * (pos[b] + 1.0) * m->cfg.hidden;
    }
    hipStream_t s = (hipStream_t)stream;
    int* d_pos = nullptr;
    PGV_TRY(upload_ints(ctx, pos, &d_pos, s));
    PGV_TRY(pgv_launch_decode_attn(ctx, m->dtype, d_qkv, d_pos, m->rope, d_Kc, d_Vc, d_out, B, m->cfg.hidden, m->cfg.heads, max_seq, bytes, s, d_part,
                                   d_ticket, split));
    PGV_HIP(hipGetLastError());
    PGV_TRY(pgv_ws_release(ctx, s));
    return PGV_OK;
}

extern "C" int pgv_decode_attention_rows(pgv_ctx* ctx, pgv_llm* m, const void* d_qkv, const int32_t* h_pos, int S, const int32_t* h_row_slot,
                                         const int32_t* h_row_j, void* d_Kc, void* d_Vc, void* d_out, int R, int max_seq, int split, float* d_part,
                                         uint32_t* d_ticket, void* stream) {
    PGV_CHECK(ctx && m && d_qkv && h_pos && h_row_slot && h_row_j && d_Kc && d_Vc && d_out && d_part && d_ticket, "pgv_decode_attention_rows: null argument");
    PGV_CHECK(S >= 1 && S <= kMaxBatch && R >= 1 && R <= kMaxBatch, "pgv_decode_attention_rows: %d slots / %d rows outside [1,%d]", S, R, kMaxBatch);
    PGV_CHECK(max_seq >= 1 && max_seq <= kMaxPos, "pgv_decode_attention_rows: max_seq %d outside [1,%d]", max_seq, kMaxPos);
    PGV_CHECK(split == 0 || split == 1 || split == 2 || split == 4 || split == 8, "pgv_decode_attention_rows: split %d is not 0, 1, 2, 4 or 8", split);
    std::vector<int> up((size_t)S + 2 * R);       // positions | row slots | row offsets
    std::set<std::pair<int, int>> seen;
    double bytes = 0;
    for (int b = 0; b < S; ++b) {
        PGV_CHECK(h_pos[b] >= 0 && h_pos[b] < max_seq, "pgv_decode_attention_rows: position %d of slot %d outside [0,%d)", h_pos[b], b, max_seq);
        up[b] = h_pos[b];
    }
    for (int r = 0; r < R; ++r) {
        const int b = h_row_slot[r], j = h_row_j[r];
        PGV_CHECK(b >= -1 && b < S, "pgv_decode_attention_rows: slot %d of row %d outside [-1,%d)", b, r, S);
        up[(size_t)S + r] = b; up[(size_t)S + R + r] = j;
        if (b < 0) continue;
        PGV_CHECK(j >= 0 && h_pos[b] + j < max_seq, "pgv_decode_attention_rows: row %d sits at position %d + %d, outside [0,%d)", r, h_pos[b], j, max_seq);
        PGV_CHECK(seen.insert({b, j}).second, "pgv_decode_attention_rows: two rows write cache row %d + %d of slot %d", h_pos[b], j, b);
        bytes += 2.0 * 2.0 * (h_pos[b] + j + 1.0) * m->cfg.hidden;
    }
    hipStream_t s = (hipStream_t)stream;
    int* d_up = nullptr;
    PGV_TRY(upload_ints(ctx, up, &d_up, s));
    PGV_TRY(pgv_launch_decode_attn_rows(ctx, m->dtype, d_qkv, d_up, d_up + S, d_up + S + R, m->rope, d_Kc, d_Vc, d_out, R, m->cfg.hidden, m->cfg.heads, max_seq, bytes,
                                        s, d_part, d_ticket, split));
    PGV_HIP(hipGetLastError());
    PGV_TRY(pgv_ws_release(ctx, s));
    return PGV_OK;
}

extern "C" int pgv_prefill_attention(pgv_ctx* ctx, pgv_llm* m, void* d_qkv, const int32_t* h_seq_lens, const int32_t* h_koff, void* d_Kc, void* d_Vc,
                                     void* d_out, int B, int max_seq, void* stream) {
    PGV_CHECK(ctx && m && d_qkv && h_seq_lens && d_Kc && d_Vc && d_out, "pgv_prefill_attention: null argument");
    PGV_CHECK(B >= 1 && B <= kMaxBatch, "pgv_prefill_attention: batch %d outside [1,%d]", B, kMaxBatch);
    PGV_CHECK(max_seq >= 1 && max_seq <= kMaxPos, "pgv_prefill_attention: max_seq %d outside [1,%d]", max_seq, kMaxPos);
    const int H = m->cfg.hidden, heads = m->cfg.heads;
    // the row maps of a prefill without ids, video or targets (prefill_plan.h)
    PrefillRows rows;
    rows.who = "pgv_prefill_attention"; rows.seq_lens = h_seq_lens; rows.B = B; rows.start = h_koff; rows.max_seq = max_seq; rows.hidden = H;
    std::vector<int> meta;
    PrefillPlan plan;
    PGV_TRY(plan_build(rows, meta, plan));
    hipStream_t s = (hipStream_t)stream;
    int* d_meta = nullptr;
    PGV_TRY(upload_ints(ctx, meta, &d_meta, s));
    const PrefillMaps<const int> d = plan.lo.maps((const int*)d_meta);
    PGV_TRY(pgv_launch_rope_kv_write(m->dtype, d_qkv, d.row_b, d.row_pos, m->rope, d_Kc, d_Vc, plan.M, H, heads, max_seq, s));
    PGV_TRY(pgv_launch_prefill_attn(ctx, m->dtype, d_qkv, d_out, d_Kc, d_Vc, d.cu, h_koff ? d.offs : nullptr, B, plan.max_len, H, heads, max_seq, plan.attn_flops, s));
    PGV_HIP(hipGetLastError());
    PGV_TRY(pgv_ws_release(ctx, s));
    return PGV_OK;
}

// ---------------------------------------------------------------------------------------------
// mm_projector
// ---------------------------------------------------------------------------------------------
extern "C" int pgv_projector(pgv_ctx* ctx, int dtype, int depth, const void* const* d_weights, const float* const* d_biases, int mm_hidden,
                             int hidden, const void* d_x, int rows, void* d_y, void* stream) {
    PGV_CHECK(ctx && d_weights && d_biases && d_x && d_y, "pgv_projector: null argument");
    PGV_CHECK(depth >= 1 && depth <= 8, "pgv_projector: depth %d unsupported (identity has nothing to run)", depth);
    PGV_CHECK(rows > 0, "pgv_projector: rows must be positive");
    hipStream_t s = (hipStream_t)stream;
    void* tmp[2] = {nullptr, nullptr};
    if (depth > 1) {
        PGV_TRY(pgv_ws_reserve(ctx, 2 * pgv_align((size_t)rows * hidden * 2), s));
        tmp[0] = pgv_ws_alloc(ctx, (size_t)rows * hidden * 2);
        tmp[1] = pgv_ws_alloc(ctx, (size_t)rows * hidden * 2);
    }
    const void* in = d_x;
    int K = mm_hidden;
    for (int i = 0; i < depth; ++i) {
        const bool last = (i == depth - 1);
        GemmArgs g{};
        g.A = in; g.lda = K; g.W = d_weights[i]; g.ldw = K; g.bias = d_biases[i];
        g.C = last ? d_y : tmp[i & 1]; g.ldc = hidden; g.M = rows; g.N = hidden; g.K = K;
        g.epi = last ? PGV_EPI_BIAS : PGV_EPI_BIAS_GELU;     // GELU sits between Linear i and Linear i+1 (builder.py:42-45)
        PGV_TRY(pgv_launch_gemm(ctx, dtype, g, s));
        in = g.C; K = hidden;
    }
    if (depth > 1) PGV_TRY(pgv_ws_release(ctx, s));
    return PGV_OK;
}
