// What a KV cache has switched on, as far as it matters to a captured decode step and to which calls exclude which.  Host-only, plain C++ without
// HIP headers, like pick_params.h: llm.hip includes it, and tests/test_host_cpu.py compiles it on its own.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include "pick_params.h"

// A value snapshot of the switches (llm.hip: kv_features is the one place that reads them off a cache).
struct KvFeatures {
    bool logprobs = false;                          // pgv_kv_set_logprobs
    int bans = 0, allowed = 0;                      // generation counters of the ban configuration / the token automaton; 0: off
    int guide_pairs = 0; float guide_scale = 1.f;   // pgv_kv_set_guidance (0, 1: off)
    int lookup_D = 0, lookup_n = 0;                 // pgv_kv_set_lookup (D 0: off)
    int beams = 0;                                  // width of the beam run in flight (0: none)
    float penalty = 1.f;                            // repetition penalty of pgv_kv_set_warpers (1: none)
};

// The key of the decode graphs a cache in state f captures for this call.  lookup: the steps are lookup steps, and only then do D and n join the key.
// What a run does not read stays out of it (pick_params.h: default PickParams without AM_SAMPLE, beams 0 without AM_BEAM, scale 1 without pairs).
inline DecodeGraphKey decode_graph_key(const KvFeatures& f, int B, int eos, int flags, int generation, const PickParams& in_flight, bool lookup) {
    return decode_graph_key(B, eos, flags, generation, f.logprobs, in_flight, f.beams, f.bans, lookup ? f.lookup_D : 0, lookup ? f.lookup_n : 0, f.guide_pairs,
                            f.guide_scale, f.allowed);
}

// Which call refuses which state: THE table.  A call reports the first row of its operation and phase whose feature is on.
enum KvOp { KV_SET_ALLOWED, KV_SET_LOGPROBS, KV_SET_GUIDANCE, KV_SET_LOOKUP, KV_PREFILL_SLOTS, KV_FORK, KV_BEAM_BEGIN, KV_LOOKUP_RUN };
enum KvFeature { KF_LOGPROBS, KF_BANS, KF_ALLOWED, KF_GUIDANCE, KF_LOOKUP, KF_BEAM, KF_PENALTY };
inline bool kv_feature_on(const KvFeatures& f, KvFeature x) {
    const bool on[] = {f.logprobs, f.bans > 0, f.allowed > 0, f.guide_pairs > 0, f.lookup_D > 0, f.beams > 0, f.penalty != 1.f};      // in KvFeature's order
    return on[x];
}
// phase 0: before the operation's own state checks (live group, id record); phase 1: behind them.  fmt takes the caller's name, then what a lookup
// step verifies against ("the plain arg-max" / "the plain pick without them").  set_* rows hold for the call that switches its feature ON.
struct KvRule { KvOp op; int phase; KvFeature on; const char* fmt; };
#define KV_GUIDED "%s: guidance is on in this cache (pgv_kv_set_guidance(kv, 1, 0) turns it off)"
static const KvRule kKvRules[] = {
    {KV_SET_ALLOWED, 0, KF_BEAM, "%s: a beam run is in flight in this cache (the beam pick applies no logits processor)"},
    {KV_SET_ALLOWED, 0, KF_LOOKUP, "%s: pgv_kv_set_lookup is on in this cache (lookup steps verify drafts against the unconstrained pick)"},
    {KV_SET_LOGPROBS, 0, KF_GUIDANCE, "%s: guidance is on in this cache (a guided pick records no log-probabilities)"},
    {KV_SET_GUIDANCE, 0, KF_LOGPROBS, "%s: pgv_kv_set_logprobs is on in this cache (a guided pick records no log-probabilities)"},
    {KV_SET_GUIDANCE, 0, KF_BEAM, "%s: a beam run is in flight in this cache"},
    {KV_SET_GUIDANCE, 0, KF_LOOKUP, "%s: pgv_kv_set_lookup is on in this cache (lookup steps verify drafts against the unguided pick)"},
    {KV_SET_LOOKUP, 0, KF_GUIDANCE, KV_GUIDED},
    {KV_SET_LOOKUP, 0, KF_ALLOWED, "%s: a token automaton is set on this cache (pgv_kv_set_allowed); lookup steps verify drafts against the unconstrained pick"},
    {KV_PREFILL_SLOTS, 0, KF_GUIDANCE, KV_GUIDED},
    {KV_FORK, 0, KF_GUIDANCE, KV_GUIDED},
    {KV_BEAM_BEGIN, 0, KF_GUIDANCE, KV_GUIDED},
    {KV_BEAM_BEGIN, 1, KF_BANS, "%s: logit bans are set on this cache (pgv_kv_set_bans); the beam pick applies no logits processor"},
    {KV_BEAM_BEGIN, 1, KF_ALLOWED, "%s: a token automaton is set on this cache (pgv_kv_set_allowed); the beam pick applies no logits processor"},
    {KV_LOOKUP_RUN, 0, KF_GUIDANCE, KV_GUIDED},
    {KV_LOOKUP_RUN, 1, KF_PENALTY, "%s: a repetition penalty is set on this cache (pgv_kv_set_warpers); lookup steps verify %s"},
    {KV_LOOKUP_RUN, 1, KF_BANS, "%s: logit bans are set on this cache (pgv_kv_set_bans); lookup steps verify %s"},
    {KV_LOOKUP_RUN, 1, KF_ALLOWED, "%s: a token automaton is set on this cache (pgv_kv_set_allowed); lookup steps verify %s"},
    {KV_LOOKUP_RUN, 1, KF_LOGPROBS, "%s: log-probabilities are on (pgv_kv_set_logprobs); lookup steps record none"},
    {KV_LOOKUP_RUN, 1, KF_BEAM, "%s: a beam run is in flight on this cache"},
};
#undef KV_GUIDED
// The first refusal of (op, phase) in state f, written to msg [n]; false: none.  Every refusal is a PGV_ESTATE of the caller.
inline bool kv_refusal(KvOp op, int phase, const KvFeatures& f, const char* who, const char* verifies, char* msg, size_t n) {
    for (const KvRule& r : kKvRules) {
        if (r.op != op || r.phase != phase || !kv_feature_on(f, r.on)) continue;
        snprintf(msg, n, r.fmt, who, verifies);
        return true;
    }
    return false;
}
