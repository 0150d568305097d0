// Logit bans on the device: HF's processors that set scores to -inf (generation/logits_process.py: NoRepeatNGramLogitsProcessor,
// NoBadWordsLogitsProcessor = SequenceBiasLogitsProcessor with bias -inf, MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
// SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor), as one kernel between the lm_head and the pick, and the per-slot record of
// `input_ids` it reads.  The rules are stated in include/pgv.h (pgv_kv_set_bans) and, in Python, in video_llava_amd/logit_bans.py (banned_ids): the
// kernel is tested against the latter, the latter against HF.
#include "llm_internal.h"

namespace {

constexpr int kBanMaxVocab = 65536;      // the ban set of a row is a bitmap in LDS (8 KB), as the seen-set of sample_kernel

// ---------------------------------------------------------------------------------------------
// One workgroup per logits row.  Phase 1: every rule marks the ids it bans in an LDS bitmap (integer LDS atomics: order-free) -- threads stride over
// the L - n + 1 n-gram windows, one thread per bad word, one per listed id.  Phase 2: the row is written through the bitmap, every entry by exactly
// one thread with a plain store: dst = src with -inf at the marked ids (src == dst: only the marked entries are stored).  Entries outside the set keep
// their bits, NaN and -inf included.
// The sequence is read through `id(i)`: with `inc` the token this step consumed belongs at position lens[b] and is taken from cur[b] directly (thread
// 0 also stores it to the record for the steps to come), so no thread depends on that store.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void logit_ban_kernel(BanArgs p) {
    __shared__ unsigned bits[kBanMaxVocab / 32];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int V = p.V, words = (V + 31) >> 5;
    const int slot = p.slot_map ? p.slot_map[b] : b;
    const int* row = p.ids + (size_t)slot * p.ids_stride;
    const int at = p.lens[b];                       // with inc: where the consumed token goes
    const int cur = p.inc ? p.cur[b] : 0;
    int L = at;
    if (p.inc) {
        if (tid == 0 && at >= 0 && at < p.ids_stride) p.rec[(size_t)slot * p.ids_stride + at] = cur;
        L = at + 1;
    }
    if (L > p.ids_stride) L = p.ids_stride;        // never read past the record (the host checks keep a live sequence inside it)
    if (L < 0) L = 0;
    const bool live = !(p.done && p.done[b]);
    for (int i = tid; i < words; i += 1024) bits[i] = 0u;
    __syncthreads();
    if (live) {
        auto id = [&](int i) -> int { return (p.inc && i == at) ? cur : row[i]; };
        auto ban = [&](int t) { if (t >= 0 && t < V) atomicOr(&bits[t >> 5], 1u << (t & 31)); };
        const BanLists& c = p.cfg;
        // no-repeat n-gram: every window [j, j + n) whose first n - 1 ids equal the last n - 1 of the sequence bans its last id
        const int n = c.ngram;
        if (n > 0 && L >= n) {
            const int s0 = L - n + 1;
            for (int j = tid; j <= L - n; j += 1024) {
                bool eq = true;
                for (int k = 0; k < n - 1 && eq; ++k) eq = id(j + k) == id(s0 + k);
                if (eq) ban(id(j + n - 1));
            }
        }
        // bad words: one id -- always; m ids -- the last one when the sequence ends in the first m - 1
        for (int w = tid; w < c.n_words; w += 1024) {
            const int o = c.word_off[w], m = c.word_off[w + 1] - o;
            if (m == 1) ban(c.word_ids[o]);
            else if (m > 1 && m <= L) {
                bool eq = true;
                for (int k = 0; k < m - 1 && eq; ++k) eq = id(L - m + 1 + k) == c.word_ids[o + k];
                if (eq) ban(c.word_ids[o + m - 1]);
            }
        }
        const int plen = p.prompt_lens ? p.prompt_lens[slot] : 0;
        for (int i = tid; i < c.n_sup; i += 1024) ban(c.sup[i]);
        if (L == plen)
            for (int i = tid; i < c.n_beg; i += 1024) ban(c.beg[i]);
        if (tid == 0 && p.eos >= 0 && (L < c.min_length || L - plen < c.min_new)) ban(p.eos);
    }
    __syncthreads();
    const float* src = p.src + (size_t)b * V;
    float* dst = p.dst + (size_t)b * V;
    if (src != dst) {
        for (int i = tid; i < V; i += 1024) dst[i] = ((bits[i >> 5] >> (i & 31)) & 1u) ? -INFINITY : src[i];
    } else {
        for (int wd = tid; wd < words; wd += 1024) {
            unsigned m = bits[wd];
            while (m) {
                const int k = __ffs((int)m) - 1;
                m &= m - 1u;
                dst[wd * 32 + k] = -INFINITY;        // k < 32 and the bit was set by ban(): wd * 32 + k < V
            }
        }
    }
}

__global__ __launch_bounds__(256) void ids_write_kernel(const int* __restrict__ ids, const int* __restrict__ cu, const int* __restrict__ offs,
                                                        const int* __restrict__ slots, const int* __restrict__ seq, int* __restrict__ rec, int stride,
                                                        int* __restrict__ prompt_lens) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const int slot = slots ? slots[t] : t, q = seq ? seq[t] : t;
    const int off = offs ? offs[q] : 0, r0 = cu[q], n = cu[q + 1] - r0;
    int* row = rec + (size_t)slot * stride;
    for (int r = tid; r < n; r += 256)
        if (off + r < stride) row[off + r] = ids[r0 + r];
    if (tid == 0) prompt_lens[slot] = off + n;
}

}  // namespace

int pgv_launch_logit_ban(const BanArgs& a, int B, hipStream_t s) {
    PGV_CHECK(a.V >= 1 && a.V <= kBanMaxVocab, "logit_ban: vocabulary %d outside [1, %d]", a.V, kBanMaxVocab);
    PGV_CHECK(a.src && a.dst && a.ids && a.lens && B >= 1 && a.ids_stride >= 0, "logit_ban: bad arguments");
    PGV_CHECK(!a.inc || (a.rec && a.cur), "logit_ban: a stepping pick needs the record and the current tokens");
    hipLaunchKernelGGL(logit_ban_kernel, dim3(B), dim3(1024), 0, s, a);
    return PGV_OK;
}

int pgv_launch_ids_write(const int* ids, const int* cu, const int* offs, const int* slots, const int* seq, int T, int* rec, int stride, int* prompt_lens,
                         hipStream_t s) {
    hipLaunchKernelGGL(ids_write_kernel, dim3(T), dim3(256), 0, s, ids, cu, offs, slots, seq, rec, stride, prompt_lens);
    return PGV_OK;
}

bool pgv_ban_neutral(const pgv_ban_config* c, int eos) {
    if (!c) return true;
    const bool lengths = eos >= 0 && (c->min_length > 0 || c->min_new_tokens > 0);
    return c->no_repeat_ngram == 0 && c->n_bad_words == 0 && c->n_suppress == 0 && c->n_begin_suppress == 0 && !lengths;
}

int pgv_ban_pack(const char* who, const pgv_ban_config* c, int V, std::vector<int>& blob, BanPacked& at) {
    PGV_CHECK(c != nullptr, "%s: null configuration", who);
    // HF's wording where HF has one (NoRepeatNGramLogitsProcessor; 0 = off is the caller's `no processor`)
    PGV_CHECK(c->no_repeat_ngram >= 0, "%s: `ngram_size` has to be a strictly positive integer, but is %d", who, c->no_repeat_ngram);
    PGV_CHECK(c->min_length >= 0, "%s: `min_length` has to be a non-negative integer, but is %d", who, c->min_length);
    PGV_CHECK(c->min_new_tokens >= 0, "%s: `min_new_tokens` has to be a non-negative integer, but is %d", who, c->min_new_tokens);
    PGV_CHECK(c->n_bad_words >= 0 && c->n_bad_words <= PGV_BAN_MAX_WORDS, "%s: %d bad words, the limit is %d", who, c->n_bad_words, PGV_BAN_MAX_WORDS);
    PGV_CHECK(c->n_suppress >= 0 && c->n_begin_suppress >= 0, "%s: negative list length (%d, %d)", who, c->n_suppress, c->n_begin_suppress);
    PGV_CHECK(c->n_bad_words == 0 || (c->h_bad_words && c->h_bad_word_lens), "%s: %d bad words without their ids", who, c->n_bad_words);
    PGV_CHECK((c->n_suppress == 0 || c->h_suppress) && (c->n_begin_suppress == 0 || c->h_begin_suppress), "%s: a listed id count without its list", who);
    long long total = (long long)c->n_suppress + c->n_begin_suppress;
    for (int w = 0; w < c->n_bad_words; ++w) {
        const int m = c->h_bad_word_lens[w];
        PGV_CHECK(m >= 1 && m <= PGV_BAN_MAX_WORD_LEN, "%s: bad word %d has %d ids, outside [1, %d]", who, w, m, PGV_BAN_MAX_WORD_LEN);
        total += m;
    }
    PGV_CHECK(total <= PGV_BAN_MAX_IDS, "%s: %lld listed ids in total, the limit is %d", who, total, PGV_BAN_MAX_IDS);
    at = BanPacked{};
    at.cfg.ngram = c->no_repeat_ngram; at.cfg.n_sup = c->n_suppress; at.cfg.n_beg = c->n_begin_suppress; at.cfg.n_words = c->n_bad_words;
    at.cfg.min_length = c->min_length; at.cfg.min_new = c->min_new_tokens;
    blob.clear();
    auto put = [&](const int32_t* ids, int n, const char* what) -> int {
        for (int i = 0; i < n; ++i) {
            // SequenceBiasLogitsProcessor._prepare_bias_variables refuses ids >= the vocabulary; a negative id is refused by every constructor
            PGV_CHECK(ids[i] >= 0 && ids[i] < V, "%s: %s id %d outside the vocabulary [0, %d)", who, what, ids[i], V);
            blob.push_back(ids[i]);
        }
        return PGV_OK;
    };
    at.sup = blob.size();
    PGV_TRY(put(c->h_suppress, c->n_suppress, "suppressed"));
    at.beg = blob.size();
    PGV_TRY(put(c->h_begin_suppress, c->n_begin_suppress, "begin-suppressed"));
    at.word_off = blob.size();
    int o = 0;
    for (int w = 0; w < c->n_bad_words; ++w) { blob.push_back(o); o += c->h_bad_word_lens[w]; }
    blob.push_back(o);
    at.word_ids = blob.size();
    PGV_TRY(put(c->h_bad_words, o, "bad-word"));
    return PGV_OK;
}

extern "C" int pgv_ban_logits(pgv_ctx* ctx, float* d_logits, int V, int B, const int32_t* d_ids, int ids_stride, const int32_t* d_lens,
                              const int32_t* d_prompt_lens, int eos_id, const pgv_ban_config* cfg, void* stream) {
    PGV_CHECK(ctx && d_logits && d_ids && d_lens && d_prompt_lens && B >= 1 && ids_stride >= 0, "pgv_ban_logits: bad arguments");
    std::vector<int> blob;
    BanPacked at;
    PGV_TRY(pgv_ban_pack("pgv_ban_logits", cfg, V, blob, at));
    if (pgv_ban_neutral(cfg, eos_id)) return PGV_OK;          // nothing asked: nothing launched, the buffer untouched
    hipStream_t s = (hipStream_t)stream;
    PGV_TRY(pgv_ws_reserve(ctx, pgv_align(blob.size() * 4), s));
    int* d_blob = (int*)pgv_ws_alloc(ctx, blob.size() * 4);
    PGV_CHECK(d_blob != nullptr, "pgv_ban_logits: workspace exhausted");
    PGV_HIP(hipMemcpyAsync(d_blob, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, s));
    BanArgs a;
    a.src = d_logits; a.dst = d_logits; a.V = V;
    a.ids = d_ids; a.ids_stride = ids_stride; a.lens = d_lens; a.prompt_lens = d_prompt_lens;
    a.eos = eos_id; a.cfg = ban_lists(at, d_blob);
    PGV_TRY(pgv_launch_logit_ban(a, B, s));
    PGV_HIP(hipGetLastError());
    PGV_TRY(pgv_ws_release(ctx, s));
    PGV_HIP(hipStreamSynchronize(s));                          // `blob` is host staging of this call
    return PGV_OK;
}
