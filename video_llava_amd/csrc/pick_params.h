// The parameters of a token pick and the key of the captured decode graphs that bake them in.  Host-only, plain C++ without HIP headers:
// llm_internal.h includes it, and tests/test_host_cpu.py compiles it on its own.
#pragma once

enum { AM_INC_POS = 1, AM_RECORD = 2, AM_SAMPLE = 4, AM_BEAM = 8 };      // bookkeeping flags of a pick (sampling.hip); AM_SAMPLE: a stepping run picks with PickParams;
                                                                         // AM_BEAM: the step ends in the beam pick and the in-group cache gather (beam.hip)

// HF's processors in HF's order: repetition penalty, temperature, top-k, top-p (the defaults: none of them).  greedy: the pick is the arg-max of
// the penalised logits and its log-probability their log-softmax over the WHOLE vocabulary, as HF's greedy loop has it.
// min_p, typical_p, epsilon, eta: HF's four remaining sampling warpers, the tail behind top-p (pgv.h: pgv_kv_set_filters; neutral: 0, 1, 0, 0).  A greedy
// pick ignores them, as it ignores top_p.
struct PickParams {
    float temperature = 1.f; int top_k = 0; float top_p = 1.f, penalty = 1.f; bool greedy = false;
    float min_p = 0.f, typical_p = 1.f, epsilon = 0.f, eta = 0.f;
    bool filtered() const { return !greedy && (min_p > 0.f || typical_p < 1.f || epsilon > 0.f || eta > 0.f); }
    bool operator==(const PickParams& o) const {
        return temperature == o.temperature && top_k == o.top_k && top_p == o.top_p && penalty == o.penalty && greedy == o.greedy && min_p == o.min_p &&
               typical_p == o.typical_p && epsilon == o.epsilon && eta == o.eta;
    }
};
// Greedy under a repetition penalty: the arg-max candidates of the lm_head GEMV know no penalty, so the pick is the sampled one over the penalised
// logits with temperature 1, top_k = 1, no nucleus and a uniform of 0 (pgv_zero_uniforms) -- the largest value, the first index on ties.
inline PickParams pick_greedy(float penalty) { return {1.f, 1, 1.f, penalty, true}; }

// What a captured decode step bakes in besides fixed device addresses (generation: pgv_llm::generation; logprobs: pgv_kv_set_logprobs).  A run
// without AM_SAMPLE picks from the lm_head candidates and reads no PickParams: its key holds the defaults, whatever an earlier run left in flight.
struct DecodeGraphKey {
    int B = 0, eos = 0, flags = 0, generation = -1; bool logprobs = false; PickParams pick;
    int beams = 0;          // AM_BEAM: the group width K of the run (the grid of the gather and the slots a pick writes); every other beam parameter lives in device memory
    int bans = 0;           // pgv_kv_set_bans: the generation counter of the cache's ban configuration (0: none) -- the ban kernel's launch and its list lengths are baked in
    int lookup_D = 0, lookup_n = 0;      // pgv_llm_decode_lookup: drafts per slot and ngram size of the captured lookup steps (0: plain token steps)
    int guide_pairs = 0; float guide_scale = 1.f;      // pgv_kv_set_guidance: the mix and follow launches bake in the pair count and the scale (0, 1: off)
    int allowed = 0;        // pgv_kv_set_allowed: the generation counter of the cache's token automaton (0: none) -- the allow kernel's launch and the automaton's addresses are baked in
    bool operator==(const DecodeGraphKey& o) const {
        return B == o.B && eos == o.eos && flags == o.flags && generation == o.generation && logprobs == o.logprobs && pick == o.pick && beams == o.beams && bans == o.bans &&
               lookup_D == o.lookup_D && lookup_n == o.lookup_n && guide_pairs == o.guide_pairs && guide_scale == o.guide_scale && allowed == o.allowed;
    }
};
inline DecodeGraphKey decode_graph_key(int B, int eos, int flags, int generation, bool logprobs, const PickParams& in_flight, int beams = 0, int bans = 0,
                                       int lookup_D = 0, int lookup_n = 0, int guide_pairs = 0, float guide_scale = 1.f, int allowed = 0) {
    return {B, eos, flags, generation, logprobs, (flags & AM_SAMPLE) ? in_flight : PickParams{}, (flags & AM_BEAM) ? beams : 0, bans, lookup_D, lookup_n,
            guide_pairs, guide_pairs > 0 ? guide_scale : 1.f, allowed};
}
