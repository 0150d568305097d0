// Beam search, device side (pgv.h: pgv_beam_begin / pgv_llm_decode_beam / pgv_kv_gather / pgv_beam_pick_logits).
//   kv_gather_kernel : the cache reorder of a beam step, in place and inside groups of K consecutive slots -- slot g0 + i receives the rows
//                      [row0, len) of slot g0 + src[i].  All K beams of a prompt share the prompt's rows [0, row0) bit for bit (pgv_kv_fork made
//                      them), so only the rows generated since the fork move.
//   beam_pick_kernel : the token pick of a beam step, HF's GenerationMixin._beam_search steps b-g for one prompt per workgroup.
#include <math.h>

#include "llm_internal.h"

namespace {

constexpr int kMaxBeams = 8;
constexpr int kGatherThreads = 256, kGatherBlocksX = 4;

// Grid (kGatherBlocksX, nrun [+ 1], groups), fixed: it does not depend on the lengths, which the kernel reads from device memory.
// Row y < nrun of the grid is run y = (plane, head); a block sweeps 16 rows x 16 pieces of 16 bytes per iteration, grid-stride over the rows
// [row0, len).  ONE LANE owns one piece index of one (plane, head, row) for all K slots of the group: it loads the pieces of the K sources into
// registers (K <= 8: 32 VGPRs), then stores them.  No other lane of the launch touches those K addresses, so the effect is "every read precedes
// every write" although the copy runs in place (a slot may be a source and another source's destination).
// The map is the same for every lane of a block (scalar loads).  An entry outside [0, K) never becomes an index: its slot keeps what it holds.
// A destination whose source is itself is not stored; a group whose map is the identity returns after reading the map.  Rows [0, row0) and
// [len, max_seq) are neither read nor written.  The last grid row (only when `cur` is given) moves the slots' current tokens the same way.
__global__ __launch_bounds__(kGatherThreads) void kv_gather_kernel(KvGatherArgs a) {
    const int g = blockIdx.z, g0 = g * a.K, run = blockIdx.y;
    int src[kMaxBeams];
    bool ident = true;
#pragma unroll
    for (int i = 0; i < kMaxBeams; ++i) {
        src[i] = i;
        if (i < a.K) {
            const int m = a.map[g0 + i];
            if (m >= 0 && m < a.K) src[i] = m;
            ident = ident && src[i] == i;
        }
    }
    if (ident) return;
    if (run >= a.nrun) {
        if (a.cur && blockIdx.x == 0 && threadIdx.x == 0) {
            int v[kMaxBeams];
#pragma unroll
            for (int i = 0; i < kMaxBeams; ++i) v[i] = (i < a.K) ? a.cur[g0 + src[i]] : 0;
#pragma unroll
            for (int i = 0; i < kMaxBeams; ++i)
                if (i < a.K && src[i] != i) a.cur[g0 + i] = v[i];
        }
        return;
    }
    int row0 = a.row0[g], len = a.len[g0];
    if (row0 < 0) row0 = 0;
    if (len > a.max_seq) len = a.max_seq;
    const int plane = run / a.heads, h = run - plane * a.heads;
    char* base = a.cache + (size_t)plane * a.plane_stride + (size_t)h * a.head_stride + (size_t)g0 * a.slot_stride;
    const int piece = threadIdx.x & 15, r_in = threadIdx.x >> 4;
    for (int row = row0 + blockIdx.x * (kGatherThreads / 16) + r_in; row < len; row += gridDim.x * (kGatherThreads / 16)) {
        const size_t off = (size_t)row * (kHD * 2) + (size_t)piece * 16;
        u32x4_t v[kMaxBeams];
#pragma unroll
        for (int i = 0; i < kMaxBeams; ++i) {
            v[i] = u32x4_t{0u, 0u, 0u, 0u};
            if (i < a.K && src[i] != i) v[i] = *(const u32x4_t*)(base + (size_t)src[i] * a.slot_stride + off);
        }
#pragma unroll
        for (int i = 0; i < kMaxBeams; ++i)
            if (i < a.K && src[i] != i) *(u32x4_t*)(base + (size_t)i * a.slot_stride + off) = v[i];
    }
}

constexpr int kPickThreads = 512, kPickWaves = kPickThreads / 64;
constexpr float kBeamNeg = -1.0e9f;

// The order of every selection: higher score first, then the lower index.
__device__ __forceinline__ bool beam_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// One workgroup per prompt p.  State words (PGV_BEAM_STATE_WORDS): run [K] f32 | fin score [K] f32 | fin length [K] | fin parent [K] | fin last
// token [K] | fin flag [K] | unsat | open.
//  b/c. acc[k * V + v] = ((x[k][v] - max_k) - lnsum_k) + run[k] (a NaN ranks as -inf) and its top 2K in the order (score down, flat index up): 2K
//       successive maximum reductions, round j over the candidates that come AFTER winner j - 1 in that order -- a total order, so the exclusion is
//       one comparison and a maximum under it does not depend on the order of the reduction: same logits, same state -> same result on any launch.
//       The rows are re-read from L2 every round.
//  d-g. by lane 0 on the 2K winners, in LDS (no dynamically indexed private arrays: nothing goes to scratch).
__global__ __launch_bounds__(kPickThreads) void beam_pick_kernel(BeamPickArgs a) {
    __shared__ float s_val[2][kPickWaves];
    __shared__ int s_idx[2][kPickWaves];
    __shared__ float s_run[kMaxBeams], s_M[kMaxBeams], s_ls[kMaxBeams];
    __shared__ float s_top[2 * kMaxBeams], s_r[2 * kMaxBeams];
    __shared__ int s_topi[2 * kMaxBeams], s_hit[2 * kMaxBeams], s_used[3 * kMaxBeams];
    __shared__ float s_ms[3 * kMaxBeams];
    __shared__ int s_mlen[3 * kMaxBeams], s_mpar[3 * kMaxBeams], s_mtok[3 * kMaxBeams], s_mflag[3 * kMaxBeams];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = a.K, V = a.V, g0 = p * K;
    unsigned* st = a.state + (size_t)p * a.state_stride;
    if (tid < K) {
        s_run[tid] = __builtin_bit_cast(float, st[tid]);
        s_M[tid] = a.stat[2 * (g0 + tid)];
        s_ls[tid] = a.stat[2 * (g0 + tid) + 1];
    }
    __syncthreads();
    float prev_s = INFINITY;
    int prev_i = -1;                       // every candidate comes after (+inf, -1)
    for (int j = 0; j < 2 * K; ++j) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int k = 0; k < K; ++k) {
            const float* lg = a.logits + (size_t)(g0 + k) * a.ld;
            const float M = s_M[k], ls = s_ls[k], run = s_run[k];
            for (int c = tid; c < V; c += kPickThreads) {
                float acc = ((lg[c] - M) - ls) + run;
                if (!(acc == acc)) acc = -INFINITY;
                const int fi = k * V + c;
                if (beam_before(prev_s, prev_i, acc, fi) && beam_before(acc, fi, best, bi)) { best = acc; bi = fi; }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (beam_before(ov, oi, best, bi)) { best = ov; bi = oi; }
        }
        const int buf = j & 1;
        if (lane == 0) { s_val[buf][w] = best; s_idx[buf][w] = bi; }
        __syncthreads();
        best = s_val[buf][0]; bi = s_idx[buf][0];
#pragma unroll
        for (int i = 1; i < kPickWaves; ++i)
            if (beam_before(s_val[buf][i], s_idx[buf][i], best, bi)) { best = s_val[buf][i]; bi = s_idx[buf][i]; }
        prev_s = best; prev_i = bi;
        if (tid == 0) { s_top[j] = best; s_topi[j] = bi; }
    }
    if (tid != 0) return;

    const BeamParams prm = a.prm_dev ? *a.prm_dev : a.prm_val;
    const int N = prm.max_new, t = a.t_dev ? a.t_dev[p] : a.t_val;
    int ti = t < 0 ? 0 : t, ni = N - 1;
    if (ni < 0) ni = 0;
    if (ti > ni) ti = ni;
    const float den_t = a.denom ? a.denom[ti] : a.den_t;
    const float den_h = (prm.early == 2 && prm.length_penalty > 0.f) ? (a.denom ? a.denom[ni] : a.den_n) : den_t;
    const bool unsat = st[6 * K] != 0u, open = st[6 * K + 1] != 0u;
    // d. which of the 2K continuations end their sequence
    bool all_hit = true;
    for (int j = 0; j < 2 * K; ++j) {
        const int tok = s_topi[j] % V;
        const bool hit = (prm.eos >= 0 && tok == prm.eos) || t + 1 >= N;
        s_hit[j] = hit;
        s_r[j] = s_top[j] + (hit ? kBeamNeg : 0.f);
        s_used[j] = 0;
        all_hit = all_hit && hit;
    }
    // e. the next running beams: the top K of r, ties to the lower j
    for (int i = 0; i < K; ++i) {
        int bj = -1;
        for (int j = 0; j < 2 * K; ++j)
            if (!s_used[j] && (bj < 0 || s_r[j] > s_r[bj])) bj = j;
        s_used[bj] = 1;
        const int tok = s_topi[bj] % V, par = s_topi[bj] / V;
        st[i] = __builtin_bit_cast(unsigned, s_r[bj]);
        a.cur[g0 + i] = tok;
        a.map[g0 + i] = par;
        if (a.hist_tok && t >= 0 && t < a.hist_steps) {
            a.hist_tok[(size_t)t * a.hist_stride + g0 + i] = tok;
            a.hist_par[(size_t)t * a.hist_stride + g0 + i] = par;
        }
        if (a.advance) a.pos[g0 + i] += 1;
    }
    const float run0 = __builtin_bit_cast(float, st[0]);
    if (a.t_dev) a.t_dev[p] = t + 1;
    if (!open) return;                     // a closed prompt keeps stepping with its group; its finished set stands
    // f. merge the K finished entries with the 2K new ones, keep the top K (ties: the earlier position)
    bool all_fin = true;
    for (int i = 0; i < K; ++i) {
        s_ms[i] = __builtin_bit_cast(float, st[K + i]);
        s_mlen[i] = (int)st[2 * K + i]; s_mpar[i] = (int)st[3 * K + i]; s_mtok[i] = (int)st[4 * K + i]; s_mflag[i] = (int)st[5 * K + i];
        all_fin = all_fin && s_mflag[i] != 0;
    }
    for (int j = 0; j < 2 * K; ++j) {
        const bool did = s_hit[j] && j < K;
        float s = s_top[j] / den_t;
        if (all_fin && prm.early == 1) s += kBeamNeg;
        if (!unsat) s += kBeamNeg;
        if (!did) s += kBeamNeg;
        s_ms[K + j] = s;
        s_mlen[K + j] = t + 1; s_mpar[K + j] = s_topi[j] / V; s_mtok[K + j] = s_topi[j] % V; s_mflag[K + j] = did;
    }
    for (int j = 0; j < 3 * K; ++j) s_used[j] = 0;
    bool all_fin2 = true, any_fin2 = false;
    float min_fin = INFINITY;
    for (int i = 0; i < K; ++i) {
        int bj = -1;
        for (int j = 0; j < 3 * K; ++j)
            if (!s_used[j] && (bj < 0 || s_ms[j] > s_ms[bj])) bj = j;
        s_used[bj] = 1;
        st[K + i] = __builtin_bit_cast(unsigned, s_ms[bj]);
        st[2 * K + i] = (unsigned)s_mlen[bj]; st[3 * K + i] = (unsigned)s_mpar[bj]; st[4 * K + i] = (unsigned)s_mtok[bj]; st[5 * K + i] = (unsigned)s_mflag[bj];
        all_fin2 = all_fin2 && s_mflag[bj] != 0;
        any_fin2 = any_fin2 || s_mflag[bj] != 0;
        min_fin = fminf(min_fin, s_ms[bj]);
    }
    // g. can a running beam still beat the worst finished one?  (torch.where(finished, min, -1e9) per entry: all K finished -> the minimum)
    const float best = run0 / den_h;
    const bool any = (any_fin2 && best > min_fin) || (!all_fin2 && best > kBeamNeg);
    const bool unsat2 = unsat && any;
    st[6 * K] = unsat2 ? 1u : 0u;
    st[6 * K + 1] = (unsat2 && !(all_fin2 && prm.early == 1) && !all_hit) ? 1u : 0u;
}

}  // namespace

int pgv_launch_kv_gather(const KvGatherArgs& a, hipStream_t s) {
    PGV_CHECK(a.cache && a.map && a.row0 && a.len && a.K >= 1 && a.K <= kMaxBeams && a.groups >= 1 && a.groups <= kMaxBatch && a.nrun >= 0 && a.nrun < 65535 &&
              a.heads >= 1 && a.max_seq >= 1, "kv gather: bad launch arguments");
    const int ny = a.nrun + (a.cur ? 1 : 0);
    if (ny < 1) return PGV_OK;
    hipLaunchKernelGGL(kv_gather_kernel, dim3(kGatherBlocksX, ny, a.groups), dim3(kGatherThreads), 0, s, a);
    return PGV_OK;
}

int pgv_launch_beam_pick(const BeamPickArgs& a, int P, hipStream_t s) {
    PGV_CHECK(a.logits && a.stat && a.state && a.cur && a.map && P >= 1 && P <= kMaxBatch && a.K >= 1 && a.K <= kMaxBeams && a.V >= 2 * a.K && a.ld >= a.V &&
              (long long)a.K * a.V < 0x7fffffffLL && a.state_stride >= 6 * a.K + 2 && (!a.advance || a.pos) && (!a.hist_tok || a.hist_par),
              "beam pick: bad launch arguments");
    hipLaunchKernelGGL(beam_pick_kernel, dim3(P), dim3(kPickThreads), 0, s, a);
    return PGV_OK;
}
