// pgv_kv_fork, device side: one cache slot becomes a run of slots (sample N answers from one prefill; the first half of a beam search's cache
// handling -- the per-step reorder inside a run of slots is kv_gather_kernel, beam.hip).
//   kv_fork_kernel : slot `src` -> slots [d0, d0 + nd) except itself -- the cache rows [0, len) of every layer, K / V plane and head, and the
//                    short per-slot state a decode step does not rebuild (position, current token, done flag, seen-set bitmap, logits row, the
//                    two latest log-probabilities).  HBM-bound: every 16-byte piece of the source is read once and stored nd times.
//   kv_fork_list_kernel : slot `src` -> the nd slots of a device list, the cache rows only (pgv_llm_prefill_slots_n: the freed slots of a live group
//                    lie anywhere in it, and the tail of the prefill sets every sample's state itself).  The same copy scheme.
// The host (llm.hip) launches either once per source; pgv_kv_fork in DESCENDING order of its sources: see there for why that order is safe in place.
#include "llm_internal.h"

namespace {

constexpr int kForkThreads = 256;
constexpr int kForkPieces = 4;          // 16-byte pieces a lane has in flight: 4 loads, then 4 stores per destination

// The bytes of run y = (plane, head) in slot 0: the run of slot d sits d * slot_stride bytes further on.
__device__ __forceinline__ char* fork_run_base(const KvForkArgs& a, int run) {
    const int plane = run / a.heads, h = run - plane * a.heads;
    return a.cache + (size_t)plane * a.plane_stride + (size_t)h * a.head_stride;
}
// This lane's kForkPieces pieces of the source slot's run (zeros beyond piece run_pieces), and their store into slot d
__device__ __forceinline__ void fork_load(const KvForkArgs& a, const char* base, u32x4_t (&v)[kForkPieces]) {
    const u32x4_t* s = (const u32x4_t*)(base + (size_t)a.src * a.slot_stride);
    const unsigned i0 = blockIdx.x * (kForkThreads * kForkPieces) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kForkPieces; ++k) {
        const unsigned i = i0 + k * kForkThreads;
        v[k] = u32x4_t{0u, 0u, 0u, 0u};
        if (i < a.run_pieces) v[k] = s[i];
    }
}
__device__ __forceinline__ void fork_store(const KvForkArgs& a, char* base, int d, const u32x4_t (&v)[kForkPieces]) {
    u32x4_t* t = (u32x4_t*)(base + (size_t)d * a.slot_stride);
    const unsigned i0 = blockIdx.x * (kForkThreads * kForkPieces) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kForkPieces; ++k) {
        const unsigned i = i0 + k * kForkThreads;
        if (i < a.run_pieces) t[i] = v[k];
    }
}

// Grid (ceil(run_pieces / (kForkThreads * kForkPieces)), nrun + 1).  Row y < nrun of the grid copies run y = (plane, head): the len * 256 contiguous
// bytes of the source slot's rows [0, len) in that plane and head.  The last row copies the per-slot state, 4 bytes per lane.
// Nothing beyond piece run_pieces of a run is touched: rows [len, max_seq) of a destination keep what they held.  No lane reads a byte another
// lane of the launch writes (the source slot is no destination), so the launch needs no ordering inside itself.
__global__ __launch_bounds__(kForkThreads) void kv_fork_kernel(KvForkArgs a) {
    const int run = blockIdx.y;
    if (run < a.nrun) {
        char* base = fork_run_base(a, run);
        u32x4_t v[kForkPieces];
        fork_load(a, base, v);
        for (int d = a.d0; d < a.d0 + a.nd; ++d)
            if (d != a.src) fork_store(a, base, d, v);
        return;
    }
    // per-slot state as one list of 32-bit words: seen-set bitmap | logits row | position, current token, done flag, lp model, lp pick
    const int n_words = a.seen_words + a.vocab + 5;
    for (int i = blockIdx.x * kForkThreads + threadIdx.x; i < n_words; i += gridDim.x * kForkThreads) {
        unsigned* p;                    // the word of slot 0
        size_t stride;                  // words from one slot to the next
        if (i < a.seen_words) { p = a.seen + i; stride = (size_t)a.seen_words; }
        else if (i < a.seen_words + a.vocab) { p = (unsigned*)a.logits + (i - a.seen_words); stride = (size_t)a.vocab; }
        else {
            const int j = i - a.seen_words - a.vocab;
            p = j == 0 ? (unsigned*)a.pos : j == 1 ? (unsigned*)a.cur : j == 2 ? (unsigned*)a.done : (unsigned*)a.lp_last + (size_t)(j - 3) * a.lp_stride;
            stride = 1;
        }
        const unsigned v = p[(size_t)a.src * stride];
        for (int d = a.d0; d < a.d0 + a.nd; ++d)
            if (d != a.src) p[(size_t)d * stride] = v;
    }
}

// Grid (ceil(run_pieces / (kForkThreads * kForkPieces)), nrun): the cache rows of kv_fork_kernel, stored to slots dst[0 .. nd) -- distinct slots, none
// of them the source (prefill_plan_build refuses a slot listed twice), so here too no lane reads a byte the launch writes.  dst[j] is the same
// address for every lane: one scalar load per destination.
__global__ __launch_bounds__(kForkThreads) void kv_fork_list_kernel(KvForkArgs a) {
    char* base = fork_run_base(a, blockIdx.y);
    u32x4_t v[kForkPieces];
    fork_load(a, base, v);
    for (int j = 0; j < a.nd; ++j) fork_store(a, base, a.dst[j], v);
}

}  // namespace

int pgv_launch_kv_fork_list(const KvForkArgs& a, hipStream_t s) {
    PGV_CHECK(a.src >= 0 && a.dst && a.nd >= 1 && a.nrun >= 1 && a.nrun < 65535 && a.heads >= 1 && a.run_pieces >= 1, "kv fork to a slot list: bad launch arguments");
    const unsigned per_block = kForkThreads * kForkPieces;
    hipLaunchKernelGGL(kv_fork_list_kernel, dim3((a.run_pieces + per_block - 1) / per_block, a.nrun), dim3(kForkThreads), 0, s, a);
    return PGV_OK;
}

int pgv_launch_kv_fork(const KvForkArgs& a, hipStream_t s) {
    PGV_CHECK(a.src >= 0 && a.d0 >= 0 && a.nd >= 1 && a.nrun >= 0 && a.nrun < 65535 && a.heads >= 1, "kv fork: bad launch arguments");
    const unsigned per_block = kForkThreads * kForkPieces;
    unsigned gx = (a.run_pieces + per_block - 1) / per_block;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(kv_fork_kernel, dim3(gx, a.nrun + 1), dim3(kForkThreads), 0, s, a);
    return PGV_OK;
}
