// Constrained decoding on the device: HF's PrefixConstrainedLogitsProcessor (generation/logits_process.py; generate(prefix_allowed_tokens_fn=...))
// with the callback replaced by a deterministic token automaton that the device follows -- one kernel between the lm_head and the pick, at the
// place of logit_ban_kernel, and the per-slot record of the automaton's state by cache position.  The rule is stated in include/pgv.h
// (pgv_kv_set_allowed) and, in Python, in video_llava_amd/allowed.py (allowed_ids): the kernel is tested against the latter, the latter against HF.
#include <cstring>

#include "llm_internal.h"

namespace {

constexpr int kAllowMaxVocab = 65536;    // the allowed set of a row is a bitmap in LDS (8 KB), as the ban set of logit_ban_kernel

// ---------------------------------------------------------------------------------------------
// One workgroup per logits row.  Phase 0 (a cache row only): the state the row is in.  With `inc` (the pick of a decode step) the token the step
// consumed, cur[b], belongs at position at = lens[b]: the workgroup looks cur up among the edges of the state before it -- the root when at is the
// prompt length, else state[at - 1] -- and the one thread whose edge carries cur (tokens are distinct within a state) publishes the edge's target
// through LDS; no thread finds it: DEAD.  A state of up to 1024 edges is one load per thread; a wider one is searched in two levels, which its
// sorted tokens allow: every thread owns a run of ceil(n / 1024) edges and compares cur with the run's first and last token, then the workgroup
// reads the one run that brackets cur -- two dependent loads instead of n / 1024 passes.  Thread 0 stores the new state at state[at] for the steps
// to come; no thread of this launch reads that entry.  Without `inc` (a re-pick, the first pick on prefill logits) the state is read and nothing
// is stored.
// Phase 1: the threads mark the tokens of the state's edges in an LDS bitmap (integer LDS atomics: order-free; run-wise, see there), plus eos when
// the state accepts, or when nothing else is allowed (DEAD, a state without edges).  Phase 2: the row is written through the bitmap, every entry by
// exactly one thread with a plain store: dst = allowed ? src : -inf (src == dst: only the entries outside the set are stored).  Entries inside the
// set keep their bits, NaN and -inf included.  A row whose done flag is set is copied as it is.
// The state is found through a chain of dependent loads (length, state, row_ptr, edge, row_ptr, edges): the row itself depends on none of them, so a
// copying launch loads its first kRowRegs x 1024 entries into registers before the chain starts and the two latencies overlap.
// Every index read from memory is checked against the automaton's sizes before it is used: a stale state entry (a cache whose prompt ran before
// the feature was switched on) is DEAD, never an address.
// ---------------------------------------------------------------------------------------------
constexpr int kRowRegs = 32;             // 32 x 1024 entries: LLaMA's 32003 in one go; a larger vocabulary's tail is loaded behind the chain

__global__ __launch_bounds__(1024) void logit_allow_kernel(AllowArgs p) {
    __shared__ unsigned bits[kAllowMaxVocab / 32];
    __shared__ int s_next, s_run;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int V = p.V, words = (V + 31) >> 5, S = p.au.n_states;
    const float* src = p.src + (size_t)b * V;
    float* dst = p.dst + (size_t)b * V;
    const bool copy = src != dst;
    float val[kRowRegs];
    if (copy) {                                        // straight-line loads (an index beyond the row reads its last entry, which is never stored)
#pragma unroll
        for (int k = 0; k < kRowRegs; ++k) {
            const int i = tid + k * 1024;
            val[k] = src[i < V ? i : V - 1];
        }
    }
    int st;
    if (p.direct) {
        st = p.direct[b];
    } else {
        const int slot = p.slot_map ? p.slot_map[b] : b;
        const int at = p.lens[b], plen = p.prompt_lens[slot];
        int* row = p.state + (size_t)slot * p.state_stride;
        const int prev = (at <= plen || at < 1) ? p.root[slot] : (at - 1 < p.state_stride ? row[at - 1] : -1);
        if (p.inc) {                                   // (uniform over the workgroup, as is everything read above: the barriers below are met by all)
            const int cur = p.cur[b];
            if (tid == 0) { s_next = -1; s_run = -1; }
            int e0 = 0, n = 0;
            if (prev >= 0 && prev < S) { e0 = p.au.row_ptr[prev]; n = p.au.row_ptr[prev + 1] - e0; }
            const int run = (n + 1023) >> 10;          // edges per thread of the first level (1: the state fits one pass)
            __syncthreads();
            if (run == 1) {
                if (tid < n && p.au.edge_token[e0 + tid] == cur) s_next = p.au.edge_next[e0 + tid];
            } else if (run > 1) {
                const int lo = tid * run, hi = lo + run < n ? lo + run : n;
                if (lo < n && p.au.edge_token[e0 + lo] <= cur && cur <= p.au.edge_token[e0 + hi - 1]) s_run = lo;      // strictly rising tokens: at most one run
            }
            __syncthreads();
            if (run > 1) {
                const int lo = s_run;
                if (lo >= 0) {
                    const int hi = lo + run < n ? lo + run : n;
                    for (int e = lo + tid; e < hi; e += 1024)
                        if (p.au.edge_token[e0 + e] == cur) s_next = p.au.edge_next[e0 + e];
                }
                __syncthreads();
            }
            st = s_next;
            if (tid == 0 && at >= 0 && at < p.state_stride) row[at] = (st >= 0 && st < S) ? st : -1;
        } else {
            st = prev;
        }
    }
    if (st < 0 || st >= S) st = -1;
    const bool live = !(p.done && p.done[b]);
    for (int i = tid; i < words; i += 1024) bits[i] = live ? 0u : ~0u;       // a finished row: everything passes
    __syncthreads();
    if (live) {
        int e0 = 0, e1 = 0;
        bool accept = false;
        if (st >= 0) { e0 = p.au.row_ptr[st]; e1 = p.au.row_ptr[st + 1]; accept = p.au.accept[st] != 0; }
        // The tokens of a state rise, so neighbouring edges fall into the same bitmap word: a thread takes a RUN of consecutive edges (the runs of the
        // lookup above), gathers the bits of one word in a register and issues one atomic per word -- lanes striding over sorted edges would send the
        // 64 atomics of a wave to two or three words.
        const int n = e1 - e0, run = (n + 1023) >> 10;
        const int lo = tid * run, hi = lo + run < n ? lo + run : n;
        unsigned acc = 0u;
        int w = 0;
        for (int e = lo; e < hi; ++e) {
            const int t = p.au.edge_token[e0 + e];
            if (t < 0 || t >= V) continue;
            if ((t >> 5) != w) {
                if (acc) atomicOr(&bits[w], acc);
                w = t >> 5; acc = 0u;
            }
            acc |= 1u << (t & 31);
        }
        if (acc) atomicOr(&bits[w], acc);
        if (tid == 0 && (accept || e1 <= e0) && p.eos >= 0 && p.eos < V) atomicOr(&bits[p.eos >> 5], 1u << (p.eos & 31));
    }
    __syncthreads();
    if (copy) {
        // every loaded value is consumed here, in straight-line code, before the first store: a store behind a branch would otherwise wait for
        // the store before it (loads and stores share one counter on this target), 32 round trips one after the other
#pragma unroll
        for (int k = 0; k < kRowRegs; ++k) {
            const int i = tid + k * 1024;              // i >> 5 < 1024: inside `bits` whatever V is
            val[k] = ((bits[i >> 5] >> (i & 31)) & 1u) ? val[k] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < kRowRegs; ++k) {
            const int i = tid + k * 1024;
            if (i < V) dst[i] = val[k];
        }
        for (int i = tid + kRowRegs * 1024; i < V; i += 1024) dst[i] = ((bits[i >> 5] >> (i & 31)) & 1u) ? src[i] : -INFINITY;
    } else {
        for (int i = tid; i < V; i += 1024)
            if (!((bits[i >> 5] >> (i & 31)) & 1u)) dst[i] = -INFINITY;
    }
}

// pgv_llm_prefill_slots / _slots_n: the slots a refill fills start at root 0 -- one launch over the device list of the filled slots
__global__ __launch_bounds__(64) void allow_root_zero_kernel(const int* __restrict__ slots, int n, int* __restrict__ root) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n) root[slots[t]] = 0;
}

}  // namespace

int pgv_launch_allow_root_zero(const int* slots, int n, int* root, hipStream_t s) {
    PGV_CHECK(slots && root && n >= 1, "allow_root_zero: bad arguments");
    hipLaunchKernelGGL(allow_root_zero_kernel, dim3((n + 63) / 64), dim3(64), 0, s, slots, n, root);
    return PGV_OK;
}

int pgv_launch_logit_allow(const AllowArgs& a, int B, hipStream_t s) {
    PGV_CHECK(a.V >= 1 && a.V <= kAllowMaxVocab, "logit_allow: vocabulary %d outside [1, %d]", a.V, kAllowMaxVocab);
    PGV_CHECK(a.src && a.dst && B >= 1 && a.au.n_states >= 1 && a.au.row_ptr && a.au.accept, "logit_allow: bad arguments");
    PGV_CHECK(a.au.n_edges == 0 || (a.au.edge_token && a.au.edge_next), "logit_allow: %d edges without their arrays", a.au.n_edges);
    PGV_CHECK(a.direct || (a.state && a.root && a.lens && a.prompt_lens && a.state_stride >= 1), "logit_allow: a cache row needs the state record");
    PGV_CHECK(!a.inc || (!a.direct && a.cur), "logit_allow: a stepping pick needs the record and the current tokens");
    hipLaunchKernelGGL(logit_allow_kernel, dim3(B), dim3(1024), 0, s, a);
    return PGV_OK;
}

// The limits of pgv.h, then the shape of the CSR arrays: row_ptr rises from 0 to n_edges, every edge token lies in the vocabulary, the tokens of a
// state rise strictly (sorted and distinct), every target is a state, every root is a state.  After this the kernel's reads stay inside the arrays.
int pgv_allow_check(const char* who, const pgv_allow_config* c, int V, int n_roots) {
    PGV_CHECK(c != nullptr, "%s: null configuration", who);
    PGV_CHECK(c->n_states >= 1 && c->n_states <= PGV_ALLOW_MAX_STATES, "%s: %d states outside [1, %d]", who, c->n_states, PGV_ALLOW_MAX_STATES);
    PGV_CHECK(c->n_edges >= 0 && c->n_edges <= PGV_ALLOW_MAX_EDGES, "%s: %d edges outside [0, %d]", who, c->n_edges, PGV_ALLOW_MAX_EDGES);
    PGV_CHECK(c->h_row_ptr && c->h_accept && (c->n_edges == 0 || (c->h_edge_token && c->h_edge_next)), "%s: null automaton array", who);
    PGV_CHECK(V >= 1 && V <= kAllowMaxVocab, "%s: vocabulary %d outside [1, %d] (the allowed set is an LDS bitmap)", who, V, kAllowMaxVocab);
    PGV_CHECK(c->eos_id >= 0 && c->eos_id < V, "%s: eos_id %d outside the vocabulary [0, %d) (the rule ends an answer with it)", who, c->eos_id, V);
    PGV_CHECK(c->h_row_ptr[0] == 0 && c->h_row_ptr[c->n_states] == c->n_edges, "%s: row_ptr runs from %d to %d, not from 0 to the %d edges", who,
              c->h_row_ptr[0], c->h_row_ptr[c->n_states], c->n_edges);
    for (int s = 0; s < c->n_states; ++s) {
        const int e0 = c->h_row_ptr[s], e1 = c->h_row_ptr[s + 1];
        PGV_CHECK(e0 >= 0 && e0 <= e1 && e1 <= c->n_edges, "%s: row_ptr of state %d (%d, %d) does not rise inside [0, %d]", who, s, e0, e1, c->n_edges);
        for (int e = e0; e < e1; ++e) {
            PGV_CHECK(c->h_edge_token[e] >= 0 && c->h_edge_token[e] < V, "%s: edge token %d of state %d outside the vocabulary [0, %d)", who, c->h_edge_token[e], s, V);
            PGV_CHECK(e == e0 || c->h_edge_token[e - 1] < c->h_edge_token[e], "%s: the edge tokens of state %d are not sorted and distinct (%d before %d)", who, s,
                      c->h_edge_token[e - 1], c->h_edge_token[e]);
            PGV_CHECK(c->h_edge_next[e] >= 0 && c->h_edge_next[e] < c->n_states, "%s: edge target %d of state %d outside the %d states", who, c->h_edge_next[e], s, c->n_states);
        }
    }
    for (int b = 0; c->h_roots && b < n_roots; ++b)
        PGV_CHECK(c->h_roots[b] >= 0 && c->h_roots[b] < c->n_states, "%s: root %d of sequence %d outside the %d states", who, c->h_roots[b], b, c->n_states);
    return PGV_OK;
}

void pgv_allow_pack(const pgv_allow_config* c, std::vector<int>& blob) {
    const size_t S = (size_t)c->n_states, E = (size_t)c->n_edges;
    blob.assign(allow_words(c->n_states, c->n_edges), 0);
    std::memcpy(blob.data(), c->h_row_ptr, (S + 1) * 4);
    if (E) {
        std::memcpy(blob.data() + S + 1, c->h_edge_token, E * 4);
        std::memcpy(blob.data() + S + 1 + E, c->h_edge_next, E * 4);
    }
    std::memcpy(blob.data() + S + 1 + 2 * E, c->h_accept, S);
}

extern "C" int pgv_allow_logits(pgv_ctx* ctx, float* d_logits, int V, int B, const int32_t* d_states, int eos_id, const pgv_allow_config* cfg, void* stream) {
    return pgv_allow_logits_copy(ctx, d_logits, d_logits, V, B, d_states, eos_id, cfg, stream);
}

// the out-of-place form: what kv_pick launches (the raw row in, the pick's copy out); d_dst == d_src is pgv_allow_logits
extern "C" int pgv_allow_logits_copy(pgv_ctx* ctx, const float* d_src, float* d_dst, int V, int B, const int32_t* d_states, int eos_id,
                                     const pgv_allow_config* cfg, void* stream) {
    PGV_CHECK(ctx && d_src && d_dst && d_states && B >= 1, "pgv_allow_logits: bad arguments");
    PGV_CHECK(cfg != nullptr, "pgv_allow_logits: null configuration");
    const size_t bytes = (size_t)B * V * 4;
    PGV_CHECK(d_src == d_dst || (const char*)d_src + bytes <= (const char*)d_dst || (const char*)d_dst + bytes <= (const char*)d_src,
              "pgv_allow_logits_copy: source and destination overlap without being equal");
    pgv_allow_config c = *cfg;
    c.eos_id = eos_id; c.h_roots = nullptr;                   // eos as an argument (cfg->eos_id is not read); the rows' states are given
    PGV_TRY(pgv_allow_check("pgv_allow_logits", &c, V, 0));
    std::vector<int> blob;
    pgv_allow_pack(&c, blob);
    hipStream_t s = (hipStream_t)stream;
    PGV_TRY(pgv_ws_reserve(ctx, pgv_align(blob.size() * 4), s));
    int* d_blob = (int*)pgv_ws_alloc(ctx, blob.size() * 4);
    PGV_CHECK(d_blob != nullptr, "pgv_allow_logits: workspace exhausted");
    PGV_HIP(hipMemcpyAsync(d_blob, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, s));
    AllowArgs a;
    a.src = d_src; a.dst = d_dst; a.V = V;
    a.au = allow_auto(d_blob, c.n_states, c.n_edges);
    a.direct = d_states; a.eos = eos_id;
    PGV_TRY(pgv_launch_logit_allow(a, B, s));
    PGV_HIP(hipGetLastError());
    PGV_TRY(pgv_ws_release(ctx, s));
    PGV_HIP(hipStreamSynchronize(s));                          // `blob` is host staging of this call
    return PGV_OK;
}
