// The row maps of a prefill: the layout of the one int block the host builds and the device reads, and the loops that fill and check it.
// Host-only, plain C++ without HIP headers: llm.hip includes it, and tests/test_host_cpu.py compiles it on its own.
#pragma once
#include <stdio.h>

#include <vector>

// The sections of the block, over any base pointer (T = int: the host staging vector; const int: the device copy).
//   row_src [M]   token id of row r, or -(video row + 1) for a spliced row (embed_splice)
//   row_b   [M]   cache slot the row writes and reads;  row_pos [M]  its RoPE / cache position
//   cu    [B + 1] first row of every sequence, then M;  last [B]  its last row
//   lens    [B]   positions of the sequence after this call;  offs [B]  positions before it (the cached prefix);  slots [B]  its cache slot
//   raw_ids [M]   the ids as given, placeholder ids included (seen_mark)
//   srows [nscore] the rows that have a target;  stgts [nscore]  their targets (pgv_llm_score)
//   samp_seq [S]  the sequence sample j is an answer to;  samp_last [S]  that sequence's last row;  samp_lens [S]  its positions;  samp_slots [S]  the
//                 cache slot of sample j (pgv_llm_prefill_slots_n: S = sum of the counts; no counts: S = 0, one sample per sequence, read last / lens / slots)
template <class T> struct PrefillMaps { T *row_src, *row_b, *row_pos, *cu, *last, *lens, *offs, *slots, *raw_ids, *srows, *stgts, *samp_seq, *samp_last, *samp_lens, *samp_slots; };

struct PrefillLayout {
    size_t row_src, row_b, row_pos, cu, last, lens, offs, slots, raw_ids, srows, stgts, samp_seq, samp_last, samp_lens, samp_slots, total;       // offsets and size, in ints
    PrefillLayout(int M = 0, int B = 0, int nscore = 0, int S = 0) {
        size_t at = 0;
        auto take = [&at](size_t n) { const size_t o = at; at += n; return o; };
        row_src = take(M); row_b = take(M); row_pos = take(M); cu = take((size_t)B + 1); last = take(B); lens = take(B); offs = take(B); slots = take(B);
        raw_ids = take(M); srows = take(nscore); stgts = take(nscore);
        samp_seq = take(S); samp_last = take(S); samp_lens = take(S); samp_slots = take(S);
        total = at;
    }
    template <class T> PrefillMaps<T> maps(T* p) const {
        return {p + row_src, p + row_b, p + row_pos, p + cu, p + last, p + lens, p + offs, p + slots, p + raw_ids, p + srows, p + stgts,
                p + samp_seq, p + samp_last, p + samp_lens, p + samp_slots};
    }
};

// What the maps are built from.  Every pointer but seq_lens may be null.
struct PrefillRows {
    const char* who = "";                            // the entry point, for the messages
    const int* ids = nullptr;                        // [M] token ids (null, pgv_prefill_attention: row_src / raw_ids stay 0, no vocabulary check)
    const int* seq_lens = nullptr; int B = 0;        // rows of every sequence
    const int* start = nullptr;                      // [B] positions already in the cache (null: 0)
    const int* slots = nullptr; int active = 0;      // [B] cache slot of sequence b, each a distinct one of the `active` live slots (null: b)
    const int* counts = nullptr;                     // [B] samples of sequence b, each >= 1 (null: one): `slots` then lists S = sum of the counts slots, those of
                                                     // sequence 0 first; the rows of sequence b go to the FIRST slot of its run, the caller copies them to the others
    const int* vid_pos = nullptr; int Vt = 0;        // [B] row behind which the Vt video rows of sequence b sit, < 0: none (null: no video)
    const int* targets = nullptr;                    // [M] target of every row, < 0: not scored (null: no scoring)
    int vocab = 0, max_seq = 0, hidden = 0;
};

struct PrefillPlan {
    PrefillLayout lo;
    int M = 0, max_len = 0, nscore = 0;
    int S = 0;                   // samples (0: no counts were given)
    double attn_flops = 0;       // causal attention over the new rows and their prefix: 4 * S * (S / 2 + prefix) * H per sequence
};

// Fills `meta` (resized to plan.lo.total ints) and `plan`.  The first refusal is formatted into err and returned as its class: so far every one
// is an invalid argument of the call (PGV_EINVAL in pgv.h).  static: the library exports nothing of it.
enum PrefillPlanStatus { PLAN_OK = 0, PLAN_EINVAL = 1 };
static inline PrefillPlanStatus prefill_plan_build(const PrefillRows& in, std::vector<int>& meta, PrefillPlan& plan, char* err, size_t err_len) {
#define PLAN_CHECK(cond, ...) do { if (!(cond)) { snprintf(err, err_len, __VA_ARGS__); return PLAN_EINVAL; } } while (0)
    const int B = in.B;
    int S = 0;
    if (in.counts) {
        PLAN_CHECK(in.slots != nullptr, "%s: sample counts without a slot list", in.who);
        for (int b = 0; b < B; ++b) {
            PLAN_CHECK(in.counts[b] >= 1, "%s: count %d of sequence %d is below 1", in.who, in.counts[b], b);
            PLAN_CHECK(in.counts[b] <= in.active - S, "%s: %lld samples up to sequence %d for a live group of %d", in.who, (long long)S + in.counts[b], b, in.active);
            S += in.counts[b];
        }
    }
    for (int b = 0; in.slots && b < (in.counts ? S : B); ++b) {
        PLAN_CHECK(in.slots[b] >= 0 && in.slots[b] < in.active, "%s: slot %d outside the %d of the live group", in.who, in.slots[b], in.active);
        for (int c = 0; c < b; ++c) PLAN_CHECK(in.slots[c] != in.slots[b], "%s: slot %d listed twice", in.who, in.slots[b]);
    }
    int M = 0, max_len = 0, nscore = 0;
    for (int b = 0; b < B; ++b) {
        const int off = in.start ? in.start[b] : 0, len = in.seq_lens[b];
        PLAN_CHECK(len >= 1 && off >= 0 && off <= in.max_seq - len, "%s: sequence %d has %d + %d tokens (cache holds %d)", in.who, b, off, len, in.max_seq);
        M += len;
        if (len > max_len) max_len = len;
    }
    for (int r = 0; in.targets && r < M; ++r) {
        PLAN_CHECK(in.targets[r] < in.vocab, "%s: target %d of row %d outside the vocabulary (%d)", in.who, in.targets[r], r, in.vocab);
        nscore += in.targets[r] >= 0;
    }
    plan = PrefillPlan{PrefillLayout(M, B, nscore, S), M, max_len, nscore, S, 0.0};
    meta.assign(plan.lo.total, 0);
    const PrefillMaps<int> h = plan.lo.maps(meta.data());
    for (int i = 0, k = 0; in.targets && i < M; ++i)
        if (in.targets[i] >= 0) { h.srows[k] = i; h.stgts[k++] = in.targets[i]; }
    int r = 0;
    for (int b = 0, j = 0; b < B; ++b) {
        h.cu[b] = r;
        const int slot = !in.slots ? b : in.slots[in.counts ? j : b];       // of the sequence's rows: its (first) slot
        const int off = in.start ? in.start[b] : 0, len = in.seq_lens[b];
        const int vp = in.vid_pos ? in.vid_pos[b] : -1;
        if (vp >= 0) PLAN_CHECK(vp + in.Vt + 1 < len, "%s: video run of sequence %d (start %d, %d rows) overruns its %d tokens", in.who, b, vp, in.Vt, len);
        for (int p = 0; p < len; ++p, ++r) {
            const bool vid = vp >= 0 && p > vp && p <= vp + in.Vt;
            if (in.ids) {
                const int id = in.ids[r];
                if (!vid) PLAN_CHECK(id >= 0 && id < in.vocab, "%s: token id %d at row %d outside the vocabulary (%d)", in.who, id, r, in.vocab);
                h.row_src[r] = vid ? -(b * in.Vt + (p - vp - 1) + 1) : id;
                h.raw_ids[r] = id;
            }
            h.row_b[r] = slot; h.row_pos[r] = off + p;
        }
        h.last[b] = r - 1; h.lens[b] = off + len; h.offs[b] = off; h.slots[b] = slot;
        for (int c = 0; in.counts && c < in.counts[b]; ++c, ++j) { h.samp_seq[j] = b; h.samp_last[j] = r - 1; h.samp_lens[j] = off + len; h.samp_slots[j] = in.slots[j]; }
        plan.attn_flops += 2.0 * (double)len * (len + 2.0 * off) * in.hidden;
    }
    h.cu[B] = r;
    return PLAN_OK;
#undef PLAN_CHECK
}
