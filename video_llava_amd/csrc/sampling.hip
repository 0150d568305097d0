// LLaMA decoder, token pick on the device: greedy (argmax over the lm_head GEMV's per-workgroup candidates) and the reference's sampling mode
// (temperature, top-k 50, multinomial: video_chatgpt/inference.py:106-112 -> HF generation/logits_process.py:238-302,542-593), plus the
// per-sequence bookkeeping (position, step, token history, EOS stickiness) that keeps a token step's kernel arguments constant.
#include <type_traits>

#include "llm_internal.h"

namespace {

__device__ __forceinline__ void lp_store(const PickLp& lp, int b, int step, int advance, float model, float pick) {
    const int o = lp.slot ? lp.slot[b] : b;
    if (lp.last_model) lp.last_model[o] = model;
    if (lp.last_pick) lp.last_pick[o] = pick;
    if (advance & 2) {
        lp.hist_model[(size_t)b * lp.hist_stride + step] = model;
        lp.hist_pick[(size_t)b * lp.hist_stride + step] = pick;
    }
}

// ---------------------------------------------------------------------------------------------
// greedy pick (first index wins ties, like torch.argmax on CPU) + bookkeeping: advance bit 0 does pos[b]++, bit 1 does
// hist[b][step[b]++] = token and EOS stickiness.
// ---------------------------------------------------------------------------------------------
// greedy pick from the lm_head GEMV's per-workgroup candidates (GemvArgs::amax_*): same result as a scan of the full logits
// (largest value, smallest index on ties, NaN never), 16x fewer values to scan.
// LP (pgv_kv_set_logprobs, argmax_parts_lp_kernel): thread 0 also stores x[tok] - logsumexp(x) from the row statistics of row_lse_kernel (PickLp), as
// both values.  argmax_parts_kernel keeps the argument record and the code it has always had.
template <bool LP>
__device__ __forceinline__ void argmax_parts_body(const float* __restrict__ val, const int* __restrict__ idx, int nblk, int amax_ts, int V, int* __restrict__ next,
                                                  int* __restrict__ pos, int* __restrict__ step, int* __restrict__ hist, int hist_stride,
                                                  int* __restrict__ done, int eos, int advance, const float* __restrict__ logits, const PickLp& lp) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    val += (size_t)(b >> 4) * amax_ts; idx += (size_t)(b >> 4) * amax_ts;          // tile-major [B / 16][nblk][16]
    for (int i = tid; i < nblk; i += 256) {
        const float v = val[(size_t)i * 16 + (b & 15)];
        const int j = idx[(size_t)i * 16 + (b & 15)];
        if (v > best || (v == best && j < bi)) { best = v; bi = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 4; ++i)
            if (sv[i] > best || (sv[i] == best && si[i] < bi)) { best = sv[i]; bi = si[i]; }
        int tok = bi < V ? bi : 0;
        [[maybe_unused]] int lp_step = 0;
        [[maybe_unused]] bool lp_sticky = false;               // the state BEFORE this pick: the step that emits EOS still carries its values
        if constexpr (LP) {
            if (advance & 2) { lp_step = step[b]; lp_sticky = done[b] != 0; }
        }
        // flags (llm.hip AM_*): 1 = advance the position, 2 = record (token history + EOS stickiness).  A plain pgv_llm_decode step passes 1
        // only: it must neither append to the history nor look at a `done` flag a previous decode_greedy / decode_sample run left set
        // (tok = eos = -1 would index embed[-H] on the next step).
        if (advance & 2) {
            if (done[b]) tok = eos;
            else if (eos >= 0 && tok == eos) done[b] = 1;
            hist[(size_t)b * hist_stride + step[b]] = tok;
            step[b] += 1;
        }
        if (advance & 1) pos[b] += 1;
        next[b] = tok;
        if constexpr (LP) {
            const float v = lp_sticky ? 0.f : (logits[(size_t)b * V + tok] - lp.stat[2 * b]) - lp.stat[2 * b + 1];
            lp_store(lp, b, lp_step, advance, v, v);
        }
    }
}

__global__ __launch_bounds__(256) void argmax_parts_kernel(const float* __restrict__ val, const int* __restrict__ idx, int nblk, int amax_ts, int V, int* __restrict__ next,
                                                           int* __restrict__ pos, int* __restrict__ step, int* __restrict__ hist, int hist_stride,
                                                           int* __restrict__ done, int eos, int advance) {
    argmax_parts_body<false>(val, idx, nblk, amax_ts, V, next, pos, step, hist, hist_stride, done, eos, advance, nullptr, PickLp{});
}

__global__ __launch_bounds__(256) void argmax_parts_lp_kernel(const float* __restrict__ val, const int* __restrict__ idx, int nblk, int amax_ts, int V, int* __restrict__ next,
                                                              int* __restrict__ pos, int* __restrict__ step, int* __restrict__ hist, int hist_stride,
                                                              int* __restrict__ done, int eos, int advance, const float* __restrict__ logits, PickLp lp) {
    argmax_parts_body<true>(val, idx, nblk, amax_ts, V, next, pos, step, hist, hist_stride, done, eos, advance, logits, lp);
}

// ---------------------------------------------------------------------------------------------
// Sampling pick (the reference's default decode mode, video_chatgpt/inference.py:106-112: do_sample=True, temperature=0.2; HF's
// sample loop = logits / temperature -> top-k mask (k = 50 from the default GenerationConfig; `scores < kth` keeps ties) -> softmax ->
// multinomial).  The multinomial draw is an inverse-CDF pick with a caller-supplied uniform u: the first vocabulary index whose
// cumulative (unnormalised) weight exceeds u * total.  One workgroup of 16 waves per sequence; wave w owns the contiguous index range
// [w * seg, (w + 1) * seg) so the cumulative sum can be walked hierarchically in vocabulary order: 16 wave totals -> the rounds of 64
// inside the selected wave -> an inclusive scan of the selected round.  Everything is a fixed-order reduction: same logits + same u ->
// same token, on any launch.  The k-th largest logit comes from a 4-pass radix select on order-preserving integer keys (LDS histogram).
// The logits (128 KB per sequence) are re-read from L2 per pass instead of living in registers.
//
// sample_kernel<true> adds the two HF processors around that chain (generation/logits_process.py, RepetitionPenaltyLogitsProcessor and
// TopPLogitsWarper), in HF's order:
//  * repetition penalty, on the raw logits: x = x < 0 ? x * penalty : x / penalty for every id of the row's seen-set.  The set is a
//    bitmap in LDS (8 KB at the 65536-entry limit), loaded from the cache slot's bitmap or built from an id list with integer LDS atomics;
//    every later pass reads the logits through it.  With a slot bitmap the pick sets the bit of the token it returns.
//  * nucleus: HF sorts ascending and removes a token iff its cumulative probability is <= 1 - top_p, i.e. a token stays iff the mass of the
//    tokens ranked above it is < top_p.  Tie rule: equal (penalised) logits share one rank -- a value v stays iff the mass of the values
//    strictly greater than v is < top_p, so equal logits are kept or removed together (as `scores < kth` does for top-k) and the maximum
//    always stays.  The smallest kept key comes from a second 4-pass radix select, over weight MASS instead of counts: a 256-bin LDS
//    histogram of the summed weights per key byte.  The weights enter it as 64-bit fixed point (e * 2^40, e in (0, 1]; 65536 of them fit
//    2^56) through integer LDS atomics, so the sums do not depend on the order in which lanes arrive.  With 0 < top_k the survivors of
//    the top-k mask (k plus ties) are first compacted into LDS and the four passes walk that list; the whole-vocabulary case walks the
//    logits, adding a wave's weights with ONE atomic when all its lanes fall into the same bin (the two leading bytes nearly always).
// sample_kernel<false> is the kernel as it was: with top_p >= 1 and penalty == 1 that is the one launched.
//
// sample_kernel<true, true> (pgv_kv_set_logprobs) also stores the two log-probabilities of the token it returns (PickLp):
//  * pick = (x'[t] - M) / T - ln S: the lane that holds the chosen entry has its (penalised) logit x', thread 0 publishes the total S of the kept
//    weights through LDS.  From the logit, not as the log of the rounded weight.
//  * greedy under a penalty: S is the sum over the WHOLE vocabulary of the penalised weights instead (one more pass, fixed order), not the sum
//    above the top-1 threshold -- HF's greedy loop normalises the processed scores over everything.  Without a penalty the value is `model`,
//    unless the row went through logit_ban_kernel (PickLp::banned): then it is the whole-vocabulary sum of the banned row, -inf entries weight 0.
//  * model = (x[t] - max x) - ln sum exp(x - max x) on the raw logits, the two statistics taken from row_lse_kernel (score.hip).
// The seen-set it reads is the LDS copy made before the pick; the bit of the returned token is set in global memory afterwards.
//
// sample_kernel<true, LP, true> (pgv_kv_set_filters) adds HF's remaining sampling warpers, the tail behind top-p in HF's order: MinPLogitsWarper,
// TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper.  Each stage recomputes the softmax over what the stage before left, so each is one
// statistics pass over the current survivors (S = sum e, A = sum e * t with t = (x - M) c = log2 e, and the largest surviving e: lane, wave, then
// the 16 wave totals in order) followed by a tighter bound.  The survivor predicate becomes `key >= thr && key != 0 && e_lo <= e <= e_hi` on the
// weight e the kernel computes anyway; the two bounds are row-uniform (every thread derives the same floats from the same LDS partials).  M stays the
// row maximum: the weights stay <= 1.  With p = e / S, ln e = t ln 2, m = (A / S) ln 2 (the mean of ln e) and H = ln S - m:
//  * min_p:    keep e >= min_p * e_max (independent of the normaliser).  It is the first stage, so e_max is the weight of the row maximum, 1: no pass.
//  * typical:  d = |(-ln p) - H| = |t ln 2 - m|.  The smallest d* with mass{d <= d*} >= ceil(typical_p * S_fx) comes from a 4-pass radix select like
//              the nucleus one -- ascending, keyed by the bits of the non-negative float d, over 2^40 fixed-point masses added with integer LDS
//              atomics (order-free).  Entries with d <= d* stay: equal d are kept together (HF: `sorted_scores > threshold` removes), the entry that
//              crosses the mass is kept, the smallest d always stays.  One more pass takes the smallest and largest weight among them: they become
//              [e_lo, e_hi] -- a BAND in the logit, the row's largest logit is routinely outside.
//  * epsilon:  keep e >= epsilon * S, or the largest CURRENT survivor: e_lo = max(e_lo, min(epsilon * S, e_max)).
//  * eta:      the same with min(eta, sqrt(eta) * exp(-H)) in place of epsilon.
// A row without a positive total skips the stages.  The final weight pass, the kept count, the CDF walk and the log-probability read the same
// predicate: `pick` is normalised over the final survivors.  Greedy picks never take this form.
// ---------------------------------------------------------------------------------------------
struct SampleArgs {
    const float* logits; int V;
    float c;                 // log2(e) / temperature
    int top_k;
    const float* u; int u_stride; int u_by_step;     // uniform of sequence b: u[(u_by_step ? step[b] : 0) * u_stride + b]
    int* next; int* pos; int* step; int* hist; int hist_stride; int* done; int eos; int advance;
    SampleWarp w;            // sample_kernel<true> only
};
struct SampleArgsLp : SampleArgs { PickLp lp; };     // sample_kernel<true, true>: the other two keep the argument record they have always had
// sample_kernel<true, LP, true>: HF's tail behind top-p (see below).  kept_range [B][2] (optional): the smallest and the largest kept (penalised) logit.
struct SampleFilt { float min_p = 0.f, typical_p = 1.f, epsilon = 0.f, eta = 0.f; float* kept_range = nullptr; };
struct SampleArgsF : SampleArgsLp { SampleFilt f; };

__device__ __forceinline__ unsigned float_key(float x) {          // larger float <-> larger key; NaN -> 0 (below every number)
    if (x != x) return 0u;
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr int SAMPLE_MAXR = 64;     // rounds of 64 per wave: V <= 16 * 64 * 64 = 65536
constexpr int SAMPLE_CAND = 1024;   // top-k survivors the nucleus select compacts into LDS (more: it walks the logits instead)
constexpr float SAMPLE_FX = 1099511627776.f;     // 2^40: fixed-point scale of a weight in the mass histogram

__device__ __forceinline__ unsigned long long weight_fx(float e) { return e > 0.f ? (unsigned long long)(e * SAMPLE_FX) : 0ull; }     // NaN -> 0

template <bool WARP, bool LP = false, bool FILT = false>
__global__ __launch_bounds__(1024) void sample_kernel(std::conditional_t<FILT, SampleArgsF, std::conditional_t<LP, SampleArgsLp, SampleArgs>> p) {
    static_assert(WARP || !LP, "the log-probability form is built on the kernel with both processors");
    static_assert(WARP || !FILT, "the filter tail is built on the kernel with both processors");
    __shared__ float fred[FILT ? 3 : 1][16];   // FILT: per-wave partials of a statistics pass (S, A, e_max) or of the band pass (min e, max e)
    __shared__ float lp_red[LP ? 17 : 1];      // LP: the 16 wave totals of the whole-vocabulary sum, then the total the pick value is normalised by
    __shared__ int hist[256];
    __shared__ unsigned sbits[WARP ? 16 * 64 * SAMPLE_MAXR / 32 : 1];      // seen-set of the row
    __shared__ unsigned long long mass[WARP ? 256 : 1];
    __shared__ unsigned ckey[WARP ? SAMPLE_CAND : 1];
    __shared__ unsigned long long cfx[WARP ? SAMPLE_CAND : 1];
    __shared__ int ccount[1];
    __shared__ unsigned long long sel_q[2];
    __shared__ int kc[16];
    __shared__ float R[16][SAMPLE_MAXR];
    __shared__ float Wt[16];
    __shared__ float red[16];
    __shared__ int sel_i[4];        // chosen bin / wave / round / pick-last flag
    __shared__ float sel_f[1];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int V = p.V;
    const float* lg = p.logits + (size_t)b * V;
    const int seg = (((V + 15) / 16) + 63) / 64 * 64, rounds = seg / 64;
    const int base = w * seg;
    // ---- seen-set -> LDS; `load` = the logit every later pass sees (penalised when its id is in the set) ----------
    const bool pen_on = WARP && p.w.penalty != 1.f;
    const int slot = (WARP && p.w.seen_slot) ? p.w.seen_slot[b] : b;
    if constexpr (WARP) {
        if (pen_on) {
            const int words = (V + 31) >> 5;
            const unsigned* gb = p.w.seen_bits ? p.w.seen_bits + (size_t)slot * p.w.seen_words : nullptr;
            for (int i = tid; i < words; i += 1024) sbits[i] = gb ? gb[i] : 0u;
            __syncthreads();
            if (p.w.seen_ids) {
                const int* ids = p.w.seen_ids + (size_t)b * p.w.seen_stride;
                const int n = p.w.seen_lens[b];
                for (int j = tid; j < n; j += 1024) {
                    const int id = ids[j];
                    if (id >= 0 && id < V) atomicOr(&sbits[id >> 5], 1u << (id & 31));
                }
                __syncthreads();
            }
        }
    }
    auto load = [&](int i) -> float {
        float x = lg[i];
        if constexpr (WARP) {
            if (pen_on && ((sbits[i >> 5] >> (i & 31)) & 1u)) x = x < 0.f ? __fmul_rn(x, p.w.penalty) : __fdiv_rn(x, p.w.penalty);
        }
        return x;
    };
    // ---- pass 1: maximum over the finite entries --------------------------------------------------
    float mx = -INFINITY;
    for (int r = 0; r < rounds; ++r) {
        const int i = base + r * 64 + lane;
        const float x = i < V ? load(i) : -INFINITY;
        mx = fmaxf(mx, x);                       // fmaxf drops NaN operands
    }
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    float M = red[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) M = fmaxf(M, red[i]);
    // ---- k-th largest key (radix select, most significant byte first) -----------------------------------
    unsigned thr = 0u;                           // keep keys >= thr
    if (p.top_k > 0 && p.top_k < V) {
        unsigned prefix = 0u, mask = 0u;
        int k = p.top_k;
        for (int pass = 3; pass >= 0; --pass) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int r = 0; r < rounds; ++r) {
                const int i = base + r * 64 + lane;
                if (i < V) {
                    const unsigned key = float_key(load(i));
                    if ((key & mask) == prefix) atomicAdd(&hist[(key >> (8 * pass)) & 255u], 1);
                }
            }
            __syncthreads();
            if (tid == 0) {
                int cum = 0, bin = 0;
                for (int q = 255; q >= 0; --q) {
                    const int h = hist[q];
                    if (cum + h >= k) { bin = q; k -= cum; break; }
                    cum += h;
                }
                sel_i[0] = bin; sel_i[1] = k;
            }
            __syncthreads();
            prefix |= (unsigned)sel_i[0] << (8 * pass);
            mask |= 0xffu << (8 * pass);
            k = sel_i[1];
            __syncthreads();
        }
        thr = prefix;
    }
    // ---- nucleus: the smallest key whose strictly-greater weight mass is < top_p * total (radix select over fixed-point mass) ----
    if constexpr (WARP) {
        if (p.w.top_p < 1.f) {
            auto cand_fx = [&](int i, unsigned& key) -> unsigned long long {      // fixed-point weight of a top-k survivor, 0 for everything else
                if (i >= V) return 0ull;
                const float x = load(i);
                key = float_key(x);
                return (key >= thr && key != 0u) ? weight_fx(__builtin_amdgcn_exp2f((x - M) * p.c)) : 0ull;
            };
            bool compact = false;
            if (p.top_k > 0 && p.top_k < V) {
                if (tid == 0) ccount[0] = 0;
                __syncthreads();
                for (int r = 0; r < rounds; ++r) {
                    unsigned key = 0u;
                    const unsigned long long q = cand_fx(base + r * 64 + lane, key);
                    if (q != 0ull) {
                        const int at = atomicAdd(&ccount[0], 1);       // the list's order is arbitrary: only order-free integer sums read it
                        if (at < SAMPLE_CAND) { ckey[at] = key; cfx[at] = q; }
                    }
                }
                __syncthreads();
                compact = ccount[0] <= SAMPLE_CAND;
            }
            unsigned prefix = 0u, mask = 0u;
            if (tid == 0) { sel_q[0] = 0ull; sel_q[1] = 0ull; }          // mass above the prefix; the limit top_p * total (set in the first pass)
            for (int pass = 3; pass >= 0; --pass) {
                if (tid < 256) mass[tid] = 0ull;
                __syncthreads();
                if (compact) {
                    if (tid < ccount[0] && (ckey[tid] & mask) == prefix) atomicAdd(&mass[(ckey[tid] >> (8 * pass)) & 255u], cfx[tid]);
                } else {
                    for (int r = 0; r < rounds; ++r) {
                        unsigned key = 0u;
                        unsigned long long q = cand_fx(base + r * 64 + lane, key);
                        if ((key & mask) != prefix) q = 0ull;
                        const int bin = (int)((key >> (8 * pass)) & 255u);
                        const unsigned long long act = __ballot(q != 0ull);
                        if (act == 0ull) continue;
                        const int bin0 = __shfl(bin, __builtin_ctzll(act), 64);
                        if (__ballot(q != 0ull && bin != bin0) == 0ull) {   // one bin for the whole wave: one atomic (integer adds: any order, same sum)
#pragma unroll
                            for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
                            if (lane == 0) atomicAdd(&mass[bin0], q);
                        } else if (q != 0ull) {
                            atomicAdd(&mass[bin], q);
                        }
                    }
                }
                __syncthreads();
                if (tid == 0) {
                    if (pass == 3) {
                        unsigned long long S = 0ull;
                        for (int q = 0; q < 256; ++q) S += mass[q];
                        sel_q[1] = (unsigned long long)ceil((double)p.w.top_p * (double)S);     // integer D: D < top_p * S  <=>  D < ceil(top_p * S)
                    }
                    // the lowest non-empty bin whose LARGEST key is kept (mass above it < limit): the boundary key lies in it
                    const unsigned long long limit = sel_q[1];
                    unsigned long long cum = sel_q[0];
                    int bin = -1;
                    for (int q = 255; q >= 0; --q) {
                        const unsigned long long h = mass[q];
                        if (h == 0ull) continue;
                        if (cum >= limit) break;
                        bin = q; sel_q[0] = cum;
                        cum += h;
                    }
                    sel_i[0] = bin;
                }
                __syncthreads();
                const int bin = sel_i[0];
                __syncthreads();
                if (bin < 0) { mask = 0u; break; }                        // no finite weight in the row: keep what top-k kept
                prefix |= (unsigned)bin << (8 * pass);
                mask |= 0xffu << (8 * pass);
            }
            if (mask == 0xffffffffu) thr = prefix;                        // >= the top-k threshold: every candidate passed it
        }
    }
    // ---- weights e_i = exp2((x_i - M) c) of the kept entries; round and wave totals -------------------------
    [[maybe_unused]] float e_lo = 0.f, e_hi = INFINITY;      // FILT: the bounds of the filter tail on a kept weight (row-uniform)
    auto weight = [&](int i) -> float {
        if (i >= V) return 0.f;
        const float x = load(i);
        const unsigned key = float_key(x);
        if constexpr (FILT) {
            const float e = (key >= thr && key != 0u) ? __builtin_amdgcn_exp2f((x - M) * p.c) : 0.f;
            return (e >= e_lo && e <= e_hi) ? e : 0.f;
        }
        return (key >= thr && key != 0u) ? __builtin_amdgcn_exp2f((x - M) * p.c) : 0.f;
    };
    // ---- filter tail: min_p -> typical_p -> epsilon -> eta, each over the survivors of the stage before (header comment) ----------------
    if constexpr (FILT) {
        constexpr float LN2 = 0.6931471805599453f;
        // a current survivor's weight (0: none) and its exponent t = log2 e
        auto weight_t = [&](int i, float& t) -> float {
            t = 0.f;
            if (i >= V) return 0.f;
            const float x = load(i);
            const unsigned key = float_key(x);
            if (!(key >= thr && key != 0u)) return 0.f;
            t = (x - M) * p.c;
            const float e = __builtin_amdgcn_exp2f(t);
            return (e >= e_lo && e <= e_hi) ? e : 0.f;
        };
        float S = 0.f, A = 0.f, E = 0.f;
        auto stats = [&]() {       // S, A and the largest weight of the current survivors: lane, wave, the 16 wave totals in order
            float s = 0.f, a = 0.f, m = 0.f;
            for (int r = 0; r < rounds; ++r) {
                float t;
                const float e = weight_t(base + r * 64 + lane, t);
                if (e > 0.f) { s += e; a = __fmaf_rn(e, t, a); m = fmaxf(m, e); }
            }
            s = wave_sum(s); a = wave_sum(a); m = wave_max(m);
            __syncthreads();                                  // the partials of the pass before have been read
            if (lane == 0) { fred[0][w] = s; fred[1][w] = a; fred[2][w] = m; }
            __syncthreads();
            S = 0.f; A = 0.f; E = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { S += fred[0][i]; A += fred[1][i]; E = fmaxf(E, fred[2][i]); }
        };
        // min_p is the first stage: the largest survivor of top-k / top-p is the row maximum itself, whose weight is exp2(0) = 1 -- no pass needed
        // (a row without a finite entry has M = -inf and keeps nothing either way).  min_p <= 1: the top passes its own bound.
        if (p.f.min_p > 0.f && M > -INFINITY) e_lo = p.f.min_p;
        if (p.f.typical_p < 1.f) {
            stats();
            if (S > 0.f) {
                const float mean = (A / S) * LN2;                         // the mean of ln e under p: H = ln S - mean, (-ln p_i) - H = mean - t_i ln 2
                auto dist = [&](float t) -> unsigned { return __float_as_uint(fabsf(__fmaf_rn(t, LN2, -mean))); };      // non-negative float: its bits order it
                unsigned prefix = 0u, mask = 0u;
                if (tid == 0) { sel_q[0] = 0ull; sel_q[1] = 0ull; }      // mass below the prefix; the limit ceil(typical_p * total) (set in the first pass)
                for (int pass = 3; pass >= 0; --pass) {
                    if (tid < 256) mass[tid] = 0ull;
                    __syncthreads();
                    for (int r = 0; r < rounds; ++r) {
                        float t;
                        const float e = weight_t(base + r * 64 + lane, t);
                        const unsigned key = dist(t);
                        unsigned long long q = (key & mask) == prefix ? weight_fx(e) : 0ull;
                        const int bin = (int)((key >> (8 * pass)) & 255u);
                        const unsigned long long act = __ballot(q != 0ull);
                        if (act == 0ull) continue;
                        const int bin0 = __shfl(bin, __builtin_ctzll(act), 64);
                        if (__ballot(q != 0ull && bin != bin0) == 0ull) {   // one bin for the whole wave: one atomic (integer adds: any order, same sum)
#pragma unroll
                            for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
                            if (lane == 0) atomicAdd(&mass[bin0], q);
                        } else if (q != 0ull) {
                            atomicAdd(&mass[bin], q);
                        }
                    }
                    __syncthreads();
                    if (tid == 0) {
                        if (pass == 3) {
                            unsigned long long T = 0ull;
                            for (int q = 0; q < 256; ++q) T += mass[q];
                            sel_q[1] = (unsigned long long)ceil((double)p.f.typical_p * (double)T);     // <= T: some bin reaches it in every pass
                        }
                        // the lowest bin at which the mass of everything up to and including it reaches the limit: d* lies in it
                        const unsigned long long limit = sel_q[1];
                        unsigned long long cum = sel_q[0];
                        int bin = -1;
                        for (int q = 0; q < 256 && limit != 0ull; ++q) {
                            const unsigned long long h = mass[q];
                            if (h != 0ull && cum + h >= limit) { bin = q; sel_q[0] = cum; break; }
                            cum += h;
                        }
                        sel_i[0] = bin;
                    }
                    __syncthreads();
                    const int bin = sel_i[0];
                    __syncthreads();
                    if (bin < 0) { mask = 0u; break; }                    // no weight of 2^-40 or more among the survivors: the stage keeps them
                    prefix |= (unsigned)bin << (8 * pass);
                    mask |= 0xffu << (8 * pass);
                }
                if (mask == 0xffffffffu) {        // prefix = the bits of d*: the band of weights with d <= d*
                    float lo = INFINITY, hi = 0.f;
                    for (int r = 0; r < rounds; ++r) {
                        float t;
                        const float e = weight_t(base + r * 64 + lane, t);
                        if (e > 0.f && dist(t) <= prefix) { lo = fminf(lo, e); hi = fmaxf(hi, e); }
                    }
                    lo = -wave_max(-lo); hi = wave_max(hi);
                    __syncthreads();
                    if (lane == 0) { fred[0][w] = lo; fred[1][w] = hi; }
                    __syncthreads();
                    lo = INFINITY; hi = 0.f;
#pragma unroll
                    for (int i = 0; i < 16; ++i) { lo = fminf(lo, fred[0][i]); hi = fmaxf(hi, fred[1][i]); }
                    if (hi > 0.f) { e_lo = fmaxf(e_lo, lo); e_hi = hi; }
                }
            }
        }
        if (p.f.epsilon > 0.f) {
            stats();
            if (S > 0.f) e_lo = fmaxf(e_lo, fminf(p.f.epsilon * S, E));     // the largest current survivor always stays
        }
        if (p.f.eta > 0.f) {
            stats();
            if (S > 0.f) {
                const float H = logf(S) - (A / S) * LN2;
                e_lo = fmaxf(e_lo, fminf(fminf(p.f.eta, sqrtf(p.f.eta) * expf(-H)) * S, E));
            }
        }
        __syncthreads();            // the last partials have been read before the passes below reuse LDS
    }
    [[maybe_unused]] bool lp_whole = false;
    if constexpr (LP) {
        lp_whole = p.lp.greedy && (pen_on || p.lp.banned);      // banned: the -inf entries of the row carry weight 0, like NaN
        if (lp_whole) {        // whole-vocabulary sum of the penalised weights (NaN: weight 0): lane, wave, then the 16 wave totals in order
            float a = 0.f;
            for (int r = 0; r < rounds; ++r) {
                const int i = base + r * 64 + lane;
                if (i < V) {
                    const float x = load(i);
                    a += x == x ? __builtin_amdgcn_exp2f((x - M) * p.c) : 0.f;
                }
            }
            a = wave_sum(a);
            if (lane == 0) lp_red[w] = a;
        }
    }
    int nkept = 0;
    [[maybe_unused]] float x_lo = INFINITY, x_hi = -INFINITY;      // FILT: the smallest / largest kept (penalised) logit
    for (int r = 0; r < rounds; ++r) {
        const float e = weight(base + r * 64 + lane);
        const float t = wave_sum(e);
        if (lane == 0) R[w][r] = t;
        if constexpr (WARP) nkept += __popcll(__ballot(e > 0.f));
        if constexpr (FILT) {
            if (p.f.kept_range && e > 0.f) { const float x = load(base + r * 64 + lane); x_lo = fminf(x_lo, x); x_hi = fmaxf(x_hi, x); }
        }
    }
    if constexpr (WARP) { if (lane == 0) kc[w] = nkept; }
    if constexpr (FILT) {
        if (p.f.kept_range) {
            x_lo = -wave_max(-x_lo); x_hi = wave_max(x_hi);
            if (lane == 0) { fred[0][w] = x_lo; fred[1][w] = x_hi; }
        }
    }
    __syncthreads();
    if (tid < 16) {
        float t = 0.f;
        for (int r = 0; r < rounds; ++r) t += R[tid][r];
        Wt[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        float S = 0.f;
        for (int i = 0; i < 16; ++i) S += Wt[i];
        if constexpr (WARP) {
            if (p.w.kept) { int n = 0; for (int i = 0; i < 16; ++i) n += kc[i]; p.w.kept[b] = n; }
        }
        if constexpr (FILT) {
            if (p.f.kept_range) {       // an empty row: (+inf, -inf)
                float lo = INFINITY, hi = -INFINITY;
                for (int i = 0; i < 16; ++i) { lo = fminf(lo, fred[0][i]); hi = fmaxf(hi, fred[1][i]); }
                p.f.kept_range[2 * b] = lo; p.f.kept_range[2 * b + 1] = hi;
            }
        }
        if constexpr (LP) {
            float G = S;
            if (lp_whole) { G = 0.f; for (int i = 0; i < 16; ++i) G += lp_red[i]; }
            lp_red[16] = G;
        }
        const float uu = p.u[(size_t)(p.u_by_step ? p.step[b] : 0) * p.u_stride + b];
        float T = uu * S;
        int ws = -1, last = 0; float acc = 0.f;
        for (int i = 0; i < 16; ++i) {
            if (Wt[i] > 0.f) { last = i; if (T < acc + Wt[i]) { ws = i; break; } acc += Wt[i]; }
        }
        int pick_last = 0;
        if (ws < 0) { ws = last; pick_last = 1; }            // u * S rounded past the total: the last kept entry
        T -= acc;
        int rs = -1, lastr = 0; acc = 0.f;
        for (int r = 0; r < rounds; ++r) {
            const float t = R[ws][r];
            if (t > 0.f) { lastr = r; if (!pick_last && T < acc + t) { rs = r; break; } acc += t; }
        }
        if (rs < 0) { rs = lastr; pick_last = 1; }
        sel_i[1] = ws; sel_i[2] = rs; sel_i[3] = pick_last; sel_f[0] = T - acc;
    }
    __syncthreads();
    if (w != sel_i[1]) return;
    const int i0 = base + sel_i[2] * 64;
    const float e = weight(i0 + lane);
    float cs = e;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(cs, o, 64);
        if (lane >= o) cs += t;
    }
    const unsigned long long hit = __ballot(e > 0.f && cs > sel_f[0]);
    const unsigned long long any = __ballot(e > 0.f);
    int sl = 0;
    if (hit != 0ull && !sel_i[3]) sl = __builtin_ctzll(hit);
    else if (any != 0ull) sl = 63 - __builtin_clzll(any);
    [[maybe_unused]] float lp_x = 0.f;                       // the (penalised) logit of the chosen entry
    if constexpr (LP) lp_x = __shfl(i0 + lane < V ? load(i0 + lane) : 0.f, sl, 64);
    if (lane == 0) {
        int tok = (any != 0ull) ? i0 + sl : 0;               // all-NaN / empty rows: token 0 rather than an out-of-range id
        [[maybe_unused]] int lp_step = 0;
        [[maybe_unused]] bool lp_sticky = false;              // the state BEFORE this pick: the step that emits EOS still carries its values
        if constexpr (LP) {
            if (p.advance & 2) { lp_step = p.step[b]; lp_sticky = p.done[b] != 0; }
        }
        if (p.advance & 2) {                                  // AM_RECORD (see argmax_parts_kernel)
            if (p.done[b]) tok = p.eos;
            else if (p.eos >= 0 && tok == p.eos) p.done[b] = 1;
            p.hist[(size_t)b * p.hist_stride + p.step[b]] = tok;
            p.step[b] += 1;
        }
        if (p.advance & 1) p.pos[b] += 1;
        p.next[b] = tok;
        if constexpr (LP) {
            float model = 0.f, pick = 0.f;
            if (!lp_sticky) {
                model = (lg[tok] - p.lp.stat[2 * b]) - p.lp.stat[2 * b + 1];
                pick = ((lp_x - M) * p.c - __builtin_amdgcn_logf(lp_red[16])) * 0.6931471805599453f;        // v_log_f32 is log2; c = log2(e) / T
                if (p.lp.greedy && !pen_on && !p.lp.banned) pick = model;
            }
            lp_store(p.lp, b, lp_step, p.advance, model, pick);
        }
        if constexpr (WARP) {                                 // the returned token joins the slot's seen-set (one workgroup per slot: a plain update)
            if (p.w.seen_bits && tok >= 0 && tok < V) p.w.seen_bits[(size_t)slot * p.w.seen_words + (tok >> 5)] |= 1u << (tok & 31);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Seen-set of a prefill: sequence b's ids (placeholder ids included, ids outside the vocabulary ignored) are set in the bitmap of its slot;
// `clear` first empties it (a new prompt; an appended turn keeps what the slot has seen).  One workgroup per sequence -- or, with `seq`, per sample:
// workgroup b marks the ids of sequence seq[b] in slot slots[b] (pgv_llm_prefill_slots_n: every sample's set is built from the prompt's ids alone).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seen_mark_kernel(const int* __restrict__ ids, const int* __restrict__ cu, const int* __restrict__ slots, int V,
                                                        unsigned* __restrict__ bits, int words, int clear, const int* __restrict__ seq) {
    const int tid = threadIdx.x;
    unsigned* row = bits + (size_t)(slots ? slots[blockIdx.x] : blockIdx.x) * words;
    const int b = seq ? seq[blockIdx.x] : blockIdx.x;
    if (clear) {
        for (int i = tid; i < words; i += 256) row[i] = 0u;
        __syncthreads();
    }
    for (int r = cu[b] + tid; r < cu[b + 1]; r += 256) {
        const int id = ids[r];
        if (id >= 0 && id < V) atomicOr(&row[id >> 5], 1u << (id & 31));
    }
}

// ---------------------------------------------------------------------------------------------
// pgv_llm_prefill_slots: the picks of the n refilled sequences (computed in rows [0, n) of the cache's scratch) become the state of their slots;
// every other slot's position, current token, step counter and done flag stays as it is.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void slot_scatter_kernel(const int* __restrict__ slots, const int* __restrict__ pick, const int* __restrict__ lens, int n,
                                                          int* __restrict__ cur, int* __restrict__ pos, int* __restrict__ step, int* __restrict__ done) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int sl = slots[i];
    cur[sl] = pick[i];
    pos[sl] = lens[i];
    step[sl] = 0;
    done[sl] = 0;
}

}  // namespace

int pgv_launch_slot_scatter(const int* slots, const int* pick, const int* lens, int n, int* cur, int* pos, int* step, int* done, hipStream_t s) {
    hipLaunchKernelGGL(slot_scatter_kernel, dim3((n + 63) / 64), dim3(64), 0, s, slots, pick, lens, n, cur, pos, step, done);
    return PGV_OK;
}

static int check_lp(const char* who, const PickLp& lp, int advance) {
    PGV_CHECK(!(advance & AM_RECORD) || (lp.hist_model && lp.hist_pick && lp.hist_stride > 0), "%s: a recording pick needs the log-probability history", who);
    return PGV_OK;
}

int pgv_launch_argmax_parts(const float* val, const int* idx, int nblk, int amax_ts, int V, int B, const PickState& st, hipStream_t s, const float* logits, const PickLp* lp) {
    if (lp && lp->stat) {
        PGV_CHECK(logits != nullptr, "argmax: the log-probabilities need the logits");
        PGV_TRY(check_lp("argmax", *lp, st.advance));
        hipLaunchKernelGGL(argmax_parts_lp_kernel, dim3(B), dim3(256), 0, s, val, idx, nblk, amax_ts, V, st.next, st.pos, st.step, st.hist, st.hist_stride, st.done, st.eos,
                           st.advance, logits, *lp);
    } else
        hipLaunchKernelGGL(argmax_parts_kernel, dim3(B), dim3(256), 0, s, val, idx, nblk, amax_ts, V, st.next, st.pos, st.step, st.hist, st.hist_stride, st.done, st.eos, st.advance);
    return PGV_OK;
}

int pgv_launch_seen_mark(const int* ids, const int* cu, const int* slots, int B, int V, unsigned* bits, int words, int clear, hipStream_t s, const int* seq) {
    hipLaunchKernelGGL(seen_mark_kernel, dim3(B), dim3(256), 0, s, ids, cu, slots, V, bits, words, clear, seq);
    return PGV_OK;
}

int pgv_check_warpers(const char* who, float top_p, float penalty) {
    // HF's wording: generation/logits_process.py, TopPLogitsWarper / RepetitionPenaltyLogitsProcessor constructors (top_p == 0 is refused here:
    // an empty nucleus has no meaning beyond min_tokens_to_keep)
    PGV_CHECK(top_p > 0.f && top_p <= 1.f, "%s: `top_p` has to be a float > 0 and <= 1, but is %g", who, (double)top_p);
    PGV_CHECK(penalty > 0.f, "%s: `penalty` has to be a strictly positive float, but is %g", who, (double)penalty);
    return PGV_OK;
}

int pgv_check_filters(const char* who, float min_p, float typical_p, float epsilon, float eta) {
    // HF's wording: generation/logits_process.py, the constructors of MinPLogitsWarper / TypicalLogitsWarper / EpsilonLogitsWarper / EtaLogitsWarper
    // (here typical_p == 1 and a cutoff of 0 are the neutral values HF's generate() builds no warper for)
    PGV_CHECK(min_p >= 0.f && min_p <= 1.f, "%s: `min_p` has to be a float in the [0, 1] interval, but is %g", who, (double)min_p);
    PGV_CHECK(typical_p > 0.f && typical_p <= 1.f, "%s: `typical_p` has to be a float > 0 and < 1, but is %g", who, (double)typical_p);
    PGV_CHECK(epsilon >= 0.f && epsilon < 1.f, "%s: `epsilon_cutoff` has to be a float > 0 and < 1, but is %g", who, (double)epsilon);
    PGV_CHECK(eta >= 0.f && eta < 1.f, "%s: `eta_cutoff` has to be a float > 0 and < 1, but is %g", who, (double)eta);
    return PGV_OK;
}

int pgv_launch_sample(const float* logits, int V, int B, const PickParams& p, const float* u, int u_stride, int u_by_step, const PickState& st, hipStream_t s,
                      const SampleWarp* warp, const PickLp* lp, float* kept_range) {
    PGV_CHECK(V >= 1 && V <= 16 * 64 * SAMPLE_MAXR, "sample: vocabulary %d outside [1, %d]", V, 16 * 64 * SAMPLE_MAXR);
    PGV_CHECK(p.temperature > 0.f, "sample: temperature must be positive (got %g); use the greedy path for temperature 0", (double)p.temperature);
    SampleArgsLp a;
    const SampleArgs& plain = a;      // what the two kernels without log-probabilities take
    a.logits = logits; a.V = V; a.c = 1.4426950408889634f / p.temperature; a.top_k = p.top_k; a.u = u; a.u_stride = u_stride; a.u_by_step = u_by_step;
    a.next = st.next; a.pos = st.pos; a.step = st.step; a.hist = st.hist; a.hist_stride = st.hist_stride; a.done = st.done; a.eos = st.eos; a.advance = st.advance;
    a.w = warp ? *warp : SampleWarp{};
    a.w.top_p = p.top_p; a.w.penalty = p.penalty;
    a.lp = (lp && lp->stat) ? *lp : PickLp{};
    a.lp.greedy = p.greedy;
    if (a.lp.stat) PGV_TRY(check_lp("sample", a.lp, st.advance));
    // the filter tail (min_p / typical_p / epsilon / eta) runs in an instantiation of its own, launched only when one of the four is on (or the
    // kept range is asked for): with all four neutral everything below launches what it has always launched
    if (p.filtered() || kept_range) {
        PGV_TRY(pgv_check_warpers("sample", p.top_p, p.penalty));
        PGV_TRY(pgv_check_filters("sample", p.min_p, p.typical_p, p.epsilon, p.eta));
        PGV_CHECK(a.w.seen_bits == nullptr || a.w.seen_words * 32 >= V, "sample: seen-set bitmap of %d words for a vocabulary of %d", a.w.seen_words, V);
        SampleArgsF f;
        static_cast<SampleArgsLp&>(f) = a;
        if (p.filtered()) { f.f.min_p = p.min_p; f.f.typical_p = p.typical_p; f.f.epsilon = p.epsilon; f.f.eta = p.eta; }      // a greedy pick ignores them
        f.f.kept_range = kept_range;
        if (a.lp.stat) hipLaunchKernelGGL((sample_kernel<true, true, true>), dim3(B), dim3(1024), 0, s, f);
        else hipLaunchKernelGGL((sample_kernel<true, false, true>), dim3(B), dim3(1024), 0, s, f);
        return PGV_OK;
    }
    // the neutral values run the kernel without the two extra processors: bit for bit the tokens of the temperature / top-k chain alone
    if (p.top_p < 1.f || p.penalty != 1.f || a.w.kept) {
        PGV_TRY(pgv_check_warpers("sample", p.top_p, p.penalty));
        PGV_CHECK(a.w.seen_bits == nullptr || a.w.seen_words * 32 >= V, "sample: seen-set bitmap of %d words for a vocabulary of %d", a.w.seen_words, V);
        if (a.lp.stat) hipLaunchKernelGGL((sample_kernel<true, true>), dim3(B), dim3(1024), 0, s, a);
        else hipLaunchKernelGGL(sample_kernel<true>, dim3(B), dim3(1024), 0, s, plain);
    } else if (a.lp.stat) {        // neutral processors: the same weights, total and token as sample_kernel<false>
        hipLaunchKernelGGL((sample_kernel<true, true>), dim3(B), dim3(1024), 0, s, a);
    } else {
        hipLaunchKernelGGL(sample_kernel<false>, dim3(B), dim3(1024), 0, s, plain);
    }
    return PGV_OK;
}

// the pick of the three building blocks: the seen-set as id lists (none: no penalty applies), the token to d_next and nothing advanced
static int sample_ids(const float* d_logits, int V, int B, const PickParams& p, const int32_t* d_seen_ids, int seen_stride, const int32_t* d_seen_lens, const float* d_u,
                      int32_t* d_next, int32_t* d_kept, const PickLp* lp, hipStream_t s, float* d_kept_range = nullptr) {
    SampleWarp w;
    w.seen_ids = d_seen_ids; w.seen_stride = seen_stride; w.seen_lens = d_seen_lens; w.kept = d_kept;
    PGV_TRY(pgv_launch_sample(d_logits, V, B, p, d_u, B, 0, PickState{d_next}, s, &w, lp, d_kept_range));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

extern "C" int pgv_sample_logits_ex(pgv_ctx* ctx, const float* d_logits, int V, int B, float temperature, int top_k, float top_p, float repetition_penalty,
                                    const int32_t* d_seen_ids, int seen_stride, const int32_t* d_seen_lens, const float* d_u, int32_t* d_next, int32_t* d_kept,
                                    void* stream) {
    PGV_CHECK(ctx && d_logits && d_u && d_next && B >= 1, "pgv_sample_logits_ex: bad arguments");
    PGV_CHECK((d_seen_ids == nullptr) == (d_seen_lens == nullptr) && seen_stride >= 0, "pgv_sample_logits_ex: d_seen_ids and d_seen_lens go together");
    PGV_TRY(pgv_check_warpers("pgv_sample_logits_ex", top_p, repetition_penalty));
    return sample_ids(d_logits, V, B, {temperature, top_k, top_p, repetition_penalty}, d_seen_ids, seen_stride, d_seen_lens, d_u, d_next, d_kept, nullptr, (hipStream_t)stream);
}

// pgv_sample_logits_lp and, with a filter record / a kept-range output, pgv_sample_logits_filtered
static int sample_logits_lp(const char* who, pgv_ctx* ctx, const float* d_logits, int V, int B, float temperature, int top_k, float top_p, float repetition_penalty,
                            const int32_t* d_seen_ids, int seen_stride, const int32_t* d_seen_lens, const float* d_u, int32_t* d_next, int32_t* d_kept,
                            int greedy, float* d_lp_model, float* d_lp_pick, const pgv_filter_config* cfg, float* d_kept_range, void* stream) {
    PGV_CHECK(ctx && d_logits && (d_u || greedy) && d_next && B >= 1, "%s: bad arguments", who);
    PGV_CHECK((d_seen_ids == nullptr) == (d_seen_lens == nullptr) && seen_stride >= 0, "%s: d_seen_ids and d_seen_lens go together", who);
    PickParams p = greedy ? pick_greedy(repetition_penalty) : PickParams{temperature, top_k, top_p, repetition_penalty};
    PGV_TRY(pgv_check_warpers(who, p.top_p, p.penalty));
    if (cfg) {
        PGV_TRY(pgv_check_filters(who, cfg->min_p, cfg->typical_p, cfg->epsilon_cutoff, cfg->eta_cutoff));
        p.min_p = cfg->min_p; p.typical_p = cfg->typical_p; p.epsilon = cfg->epsilon_cutoff; p.eta = cfg->eta_cutoff;
    }
    hipStream_t s = (hipStream_t)stream;
    // row statistics [B][2] and, for the greedy form, its B uniforms
    PGV_TRY(pgv_ws_reserve(ctx, 2 * pgv_align((size_t)B * 8), s));
    float* stat = (float*)pgv_ws_alloc(ctx, (size_t)B * 8);
    float* zero = (float*)pgv_ws_alloc(ctx, (size_t)B * 4);
    PGV_CHECK(stat && zero, "%s: workspace exhausted", who);
    if (greedy) PGV_TRY(pgv_zero_uniforms(zero, B, s));
    PGV_TRY(pgv_launch_row_lse(d_logits, V, V, B, stat, s));
    PickLp lp;
    lp.stat = stat; lp.last_model = d_lp_model; lp.last_pick = d_lp_pick;
    PGV_TRY(sample_ids(d_logits, V, B, p, d_seen_ids, seen_stride, d_seen_lens, greedy ? zero : d_u, d_next, d_kept, &lp, s, d_kept_range));
    PGV_TRY(pgv_ws_release(ctx, s));
    return PGV_OK;
}

extern "C" int pgv_sample_logits_lp(pgv_ctx* ctx, const float* d_logits, int V, int B, float temperature, int top_k, float top_p, float repetition_penalty,
                                    const int32_t* d_seen_ids, int seen_stride, const int32_t* d_seen_lens, const float* d_u, int32_t* d_next, int32_t* d_kept,
                                    int greedy, float* d_lp_model, float* d_lp_pick, void* stream) {
    return sample_logits_lp("pgv_sample_logits_lp", ctx, d_logits, V, B, temperature, top_k, top_p, repetition_penalty, d_seen_ids, seen_stride, d_seen_lens, d_u, d_next,
                            d_kept, greedy, d_lp_model, d_lp_pick, nullptr, nullptr, stream);
}

extern "C" int pgv_sample_logits_filtered(pgv_ctx* ctx, const float* d_logits, int V, int B, float temperature, int top_k, float top_p, float repetition_penalty,
                                          const int32_t* d_seen_ids, int seen_stride, const int32_t* d_seen_lens, const float* d_u, int32_t* d_next, int32_t* d_kept,
                                          int greedy, float* d_lp_model, float* d_lp_pick, const pgv_filter_config* cfg, float* d_kept_range, void* stream) {
    return sample_logits_lp("pgv_sample_logits_filtered", ctx, d_logits, V, B, temperature, top_k, top_p, repetition_penalty, d_seen_ids, seen_stride, d_seen_lens, d_u,
                            d_next, d_kept, greedy, d_lp_model, d_lp_pick, cfg, d_kept_range, stream);
}

extern "C" int pgv_sample_logits(pgv_ctx* ctx, const float* d_logits, int V, int B, float temperature, int top_k, const float* d_u, int32_t* d_next,
                                 void* stream) {
    PGV_CHECK(ctx && d_logits && d_u && d_next && B >= 1, "pgv_sample_logits: bad arguments");
    return sample_ids(d_logits, V, B, {temperature, top_k}, nullptr, 0, nullptr, d_u, d_next, nullptr, nullptr, (hipStream_t)stream);
}
