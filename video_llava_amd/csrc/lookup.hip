// Prompt-lookup speculative decoding, the two small kernels around the row-wise decode step (llm.hip: pgv_llm_decode_lookup): drafting by n-gram
// lookup in the slot's own ids, and acceptance of the longest draft prefix the model agrees with.  A lookup step emits exactly the tokens
// consecutive plain steps would: the rows are picked by arg-max, or (sampled form) each with the uniform the plain run draws for its token.
// The drafting rule is HF's PromptLookupCandidateGenerator.get_candidates (transformers/generation/candidate_generator.py);
// video_llava_amd/lookup_reference.py states it and the step trace in numpy, and the kernels reproduce those.
#include "llm_internal.h"

namespace {

// One workgroup per slot b.  Stores cur[b] at record position pos[b] (the slot's sequence is then rec[0 .. L), L = pos[b] + 1), then for ngram size
// min(n, L - 1) down to 1 finds the LEFTMOST window equal to the last ngram that has a token behind it, takes the up to D tokens behind it, cuts them
// before the first eos and caps them: at most budget[b] - step[b] - 1 (the step emits one token more than it accepts drafts), none past the
// cache's last row.  Rows r = b * (1 + D) + j: j = 0 consumes cur, j >= 1 draft j; rows beyond the drafts, and every row of a finished slot (done
// flag, or the budget is spent), get slot -1 and are skipped by the attention.  Their token stays a valid id: the GEMVs run over all rows.
__global__ __launch_bounds__(256) void lookup_draft_kernel(LookupArgs a) {
    __shared__ int s_best;
    const int b = blockIdx.x, tid = threadIdx.x, W = 1 + a.D;
    const int pos = a.pos[b], cur = a.cur[b], left = a.budget[b] - a.step[b];
    int* rec = a.rec + (size_t)b * a.max_seq;
    const bool live = !a.done[b] && left > 0 && pos < a.max_seq;
    if (tid == 0) s_best = 0x7fffffff;
    if (live && tid == 0) rec[pos] = cur;
    __syncthreads();
    const int L = pos + 1;
    int cap = a.D;
    cap = min(cap, left - 1);
    cap = min(cap, a.max_seq - 1 - pos);
    int g = 0;
    if (live && cap > 0) {
        for (g = min(a.n, L - 1); g >= 1; --g) {
            int mine = 0x7fffffff;
            for (int idx = tid; idx < L - g; idx += 256) {       // idx = L - g is the last ngram itself: nothing behind it
                bool eq = true;
                for (int i = 0; i < g; ++i) eq = eq && rec[idx + i] == rec[L - g + i];
                if (eq) { mine = idx; break; }
            }
            if (mine != 0x7fffffff) atomicMin(&s_best, mine);
            __syncthreads();
            if (s_best != 0x7fffffff) break;                    // uniform: every thread reads the same word behind the barrier
            __syncthreads();
        }
    }
    const int best = s_best;
    int nd = 0, start = 0;
    if (live && cap > 0 && best != 0x7fffffff) {
        start = best + g;
        const int len = min(start + a.D, L) - start;
        while (nd < len && rec[start + nd] != a.eos) ++nd;      // eos < 0 matches no id
        nd = min(nd, cap);
    }
    if (tid == 0) a.n_draft[b] = nd;
    if (tid < W) {
        const int r = b * W + tid;
        const bool row = live && tid <= nd;
        a.row_slot[r] = row ? b : -1;
        a.row_j[r] = tid;
        a.tok[r] = (row && tid > 0) ? rec[start + tid - 1] : cur;
        // sampled: a live row j has step + j < budget (nd <= left - 1), so its uniform lies inside the rows the entry checked
        if (a.u) a.u_row[r] = row ? a.u[(size_t)(a.u_base[b] + a.step[b] + tid) * a.u_stride + b] : 0.f;
    }
}

// One thread per slot b behind the row-wise pick t[r] (arg-max, or the sampled pick).  a = the leading drafts j = 1 .. n_draft with
// draft_j == t[row j - 1]; the slot emits t[row 0 .. a] with the bookkeeping of a recording pick, token by token: history and step++, an eos raises done and ends the emission, the
// budget ends it too.  pos += emitted, cur = the last emitted token, the emitted tokens go into the id record behind cur, counts[k][b] = emitted
// with k the run's step counter (advanced here).  Cache rows at or beyond the new pos are stale: never read, overwritten by later steps.
__global__ __launch_bounds__(64) void lookup_accept_kernel(LookupArgs a, int B) {
    const int b = threadIdx.x, W = 1 + a.D;
    const int k = *a.k;
    __syncthreads();
    if (b == 0) *a.k = k + 1;
    if (b >= B) return;
    int emitted = 0;
    if (a.row_slot[b * W] >= 0) {
        const int nd = a.n_draft[b], pos = a.pos[b];
        int acc = 0;
        while (acc < nd && a.tok[b * W + 1 + acc] == a.t[b * W + acc]) ++acc;
        int st = a.step[b], last = a.cur[b];
        for (int j = 0; j <= acc && st < a.budget[b]; ++j) {
            last = a.t[b * W + j];
            a.hist[(size_t)b * a.hist_stride + st++] = last;
            if (pos + 1 + j < a.max_seq) a.rec[(size_t)b * a.max_seq + pos + 1 + j] = last;
            if (a.seen && last >= 0 && last < a.vocab) a.seen[(size_t)b * a.seen_words + (last >> 5)] |= 1u << (last & 31);
            ++emitted;
            if (a.eos >= 0 && last == a.eos) { a.done[b] = 1; break; }
        }
        a.step[b] = st; a.pos[b] = pos + emitted; a.cur[b] = last;
    }
    a.counts[(size_t)k * a.counts_stride + b] = emitted;
}

}  // namespace

int pgv_launch_lookup_draft(const LookupArgs& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(lookup_draft_kernel, dim3(B), dim3(256), 0, s, a);
    return PGV_OK;
}

int pgv_launch_lookup_accept(const LookupArgs& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(lookup_accept_kernel, dim3(1), dim3(64), 0, s, a, B);
    return PGV_OK;
}
