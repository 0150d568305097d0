// Encoder of the lossless 12-bit weight stream (format: w12.h).  One workgroup per row block of 16 rows (all K columns), three passes:
// a histogram of the 7-bit exponents per row (LDS) -> the row bases; the unit planes, exceptions counted and collected in LDS; the
// exception list sorted (rank by comparison: the order does not depend on which thread found an entry) and written.  Vector stores only.
#include "w12.h"

namespace {

constexpr int kEncThreads = 256;

__global__ __launch_bounds__(kEncThreads) void encode_w12_kernel(const unsigned short* __restrict__ w16, unsigned char* __restrict__ out,
                                                                 int* __restrict__ counts, long long N, long long K) {
    __shared__ unsigned hist[16][128];
    __shared__ unsigned base_s[16];
    __shared__ unsigned exc_s[kW12MaxExc];
    __shared__ unsigned nexc;
    const int tid = threadIdx.x;
    const long long rb = blockIdx.x;
    const long long G = K >> 6;
    const unsigned short* src = w16 + (size_t)rb * 16 * K;      // the row block's 16 x K elements are contiguous in the blocked layout
    for (int i = tid; i < 16 * 128; i += kEncThreads) (&hist[0][0])[i] = 0u;
    if (tid == 0) nexc = 0u;
    __syncthreads();
    // pass 1: exponent histogram.  16-byte chunk c of the row block = row c % 16 (k-group (c / 16) % 4, k-block c / 64): with a stride of
    // 256 chunks a thread always sees the same row
    const long long nchunks = 2 * K;
    for (long long c = tid; c < nchunks; c += kEncThreads) {
        const u32x4_t v = *(const u32x4_t*)(src + c * 8);
        const int r = (int)(c & 15);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            atomicAdd(&hist[r][(v[e] >> 8) & 0x7f], 1u);
            atomicAdd(&hist[r][(v[e] >> 24) & 0x7f], 1u);
        }
    }
    __syncthreads();
    if (tid < 16) {
        unsigned best = 0, bestc = 0, win = 0;
        for (int b = 0; b < 128; ++b) {                         // window [b - 7, b]; the first maximum wins
            win += hist[tid][b];
            if (b >= 8) win -= hist[tid][b - 8];
            if (win > bestc) { bestc = win; best = (unsigned)b; }
        }
        base_s[tid] = best;
        out[pgv_w12_units_bytes(N, K) + pgv_w12_exc_bytes(N) + (size_t)rb * 16 + tid] = (unsigned char)best;
    }
    __syncthreads();
    // pass 2: unit planes.  Work item (group g, lane l): 16 weights of row l % 16, columns g * 64 + h * 32 + (l / 16) * 8 + e
    unsigned char* units = out + (size_t)rb * G * 1536;
    for (long long i = tid; i < G * 64; i += kEncThreads) {
        const long long g = i >> 6;
        const int l = (int)(i & 63), r = l & 15, kg = l >> 4;
        const unsigned base = base_s[r];
        u32x4_t lo;
        u32x2_t code;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4_t v = *(const u32x4_t*)(src + ((2 * g + h) * 512 + (kg * 16 + r) * 8));
            unsigned lw[2] = {0u, 0u}, cw = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned x = (v[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
                const unsigned hb = x >> 8, e7 = hb & 0x7f, s = hb >> 7;
                lw[e >> 2] |= (x & 0xffu) << ((e & 3) * 8);
                unsigned cd = 0u;
                if (e7 <= base && base - e7 <= 7u) cd = (s << 3) | (base - e7);
                else {
                    const unsigned slot = atomicAdd(&nexc, 1u);
                    if (slot < (unsigned)kW12MaxExc) exc_s[slot] = ((unsigned)g << 18) | ((unsigned)l << 12) | ((unsigned)(h * 8 + e) << 8) | hb;
                }
                cw |= cd << ((e & 3) * 8 + (e >> 2) * 4);
            }
            lo[2 * h] = lw[0]; lo[2 * h + 1] = lw[1];
            code[h] = cw;
        }
        *(u32x4_t*)(units + g * 1536 + l * 16) = lo;
        *(u32x2_t*)(units + g * 1536 + 1024 + l * 8) = code;
    }
    __syncthreads();
    // pass 3: the exception list in ascending order (entries are distinct: rank = number of smaller entries)
    const unsigned n = nexc < (unsigned)kW12MaxExc ? nexc : (unsigned)kW12MaxExc;
    if (tid < kW12MaxExc) {
        unsigned* exc = (unsigned*)(out + pgv_w12_units_bytes(N, K)) + (size_t)rb * kW12MaxExc;
        if ((unsigned)tid < n) {
            const unsigned e = exc_s[tid];
            unsigned rank = 0;
            for (unsigned j = 0; j < n; ++j) rank += exc_s[j] < e ? 1u : 0u;
            exc[rank] = e;
        } else {
            exc[tid] = kW12NoExc;
        }
        if (tid == 0) counts[rb] = (int)nexc;
    }
}

}  // namespace

int pgv_launch_encode_w12(const void* w16_blocked, void* w12, int* counts, long long N, long long K, hipStream_t s) {
    PGV_CHECK(N > 0 && N % 16 == 0 && K > 0 && K % 64 == 0, "encode_w12: need N %% 16 == 0 and K %% 64 == 0 (got %lld x %lld)", N, K);
    PGV_CHECK(K / 64 < 0x3fff, "encode_w12: K = %lld exceeds the 14-bit group index of an exception entry", K);
    hipLaunchKernelGGL(encode_w12_kernel, dim3((unsigned)(N / 16)), dim3(kEncThreads), 0, s, (const unsigned short*)w16_blocked, (unsigned char*)w12, counts, N, K);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

extern "C" size_t pgv_w12_bytes(int N, int K) { return (N > 0 && K > 0) ? pgv_w12_total_bytes(N, K) : 0; }

extern "C" int pgv_encode_w12_blocked(pgv_ctx* ctx, int dtype, const void* d_w16_blocked, void* d_w12, int* d_counts, int N, int K, void* stream) {
    PGV_CHECK(ctx && d_w16_blocked && d_w12 && d_counts, "pgv_encode_w12_blocked: null argument");
    PGV_CHECK(dtype == PGV_BF16, "pgv_encode_w12_blocked: the 12-bit stream codes bf16 weights (dtype %d)", dtype);
    return pgv_launch_encode_w12(d_w16_blocked, d_w12, d_counts, N, K, (hipStream_t)stream);
}
