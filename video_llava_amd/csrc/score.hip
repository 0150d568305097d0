// Teacher-forced scoring: per-row log-probability of a GIVEN token from fp32 logits -- what the reference's forward(labels=...) feeds its
// CrossEntropyLoss with (video_chatgpt/model/video_chatgpt.py:228-239: shift, flatten, CrossEntropyLoss), one row at a time.
//   logprob[r] = x[t] - logsumexp(x[0:V]),  lse[r] = logsumexp(x[0:V]),  argmax[r] = first index of the largest entry (the greedy pick's rule)
#include "llm_internal.h"

namespace {

struct LogprobArgs {
    const float* logits; int ld, V;
    const int* targets;
    const int* out_rows;     // row r writes its results at index out_rows[r] (null: r) -- pgv_llm_score scatters a chunk to the batch's rows
    float* logprob; float* lse; int* argmax;
};

// One workgroup of 4 waves per row, TWO passes over the row: maximum + argmax, then the sum of exp(x - max).  The second pass is served from
// L2 (a row is 128 KB at the 32003-entry vocabulary), as in sample_kernel; the maximum is then exact and final before the first exponential,
// so no term is ever rescaled.  Loads are 16 bytes per lane (ld % 4 == 0, row base 16-byte aligned); the reduction covers columns [0, V) only:
// the lanes of the last vector that fall at or beyond V are replaced before they are used (the lm_head GEMM writes ceil16(vocab) columns and
// the spare ones hold logit 0).
// Fixed order (batch invariance): lane `tid` sums the columns 4 (tid + 256 k) + e in (k, e) order, then a fixed tree -- xor
// butterfly inside a wave, (w0 + w1) + (w2 + w3) across the waves.  A row's result depends on its V columns alone: not on R, the row's index or
// the launch.
// exp and log are the raw v_exp_f32 / v_log_f32 on the max-subtracted argument (1 ulp each, whatever the magnitude of the logits).
// -inf entries add exp2(-inf) = 0; a target on -inf gives -inf.  NaN never wins the maximum (it then poisons the sum, as in torch).
__global__ __launch_bounds__(256) void logprob_rows_kernel(LogprobArgs p) {
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    __shared__ float s_sum[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int V = p.V, nv = (V + 3) >> 2;
    const float* lg = p.logits + (size_t)r * p.ld;
    // ---- pass 1: maximum, first index on ties -------------------------------------------------------
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int q = tid; q < nv; q += 256) {
        const f32x4_t v = *(const f32x4_t*)(lg + 4 * (size_t)q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            const float x = c < V ? v[e] : -INFINITY;
            if (x > best) { best = x; bi = c; }          // a lane's columns ascend: strict > keeps the first
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { s_val[w] = best; s_idx[w] = bi; }
    __syncthreads();
    best = s_val[0]; bi = s_idx[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (s_val[i] > best || (s_val[i] == best && s_idx[i] < bi)) { best = s_val[i]; bi = s_idx[i]; }
    const float M = best;
    // ---- pass 2: sum of exp(x - M) ---------------------------------------------------------------------
    float sum = 0.f;
    for (int q = tid; q < nv; q += 256) {
        const f32x4_t v = *(const f32x4_t*)(lg + 4 * (size_t)q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = __builtin_amdgcn_exp2f((v[e] - M) * 1.4426950408889634f);
            sum += (4 * q + e < V) ? t : 0.f;
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) s_sum[w] = sum;
    __syncthreads();
    if (tid == 0) {
        const float total = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        const float ls = __builtin_amdgcn_logf(total) * 0.6931471805599453f;          // v_log_f32 is log2
        const int o = p.out_rows ? p.out_rows[r] : r;
        if (p.lse) p.lse[o] = M + ls;
        if (p.argmax) p.argmax[o] = bi < V ? bi : 0;       // nothing above -inf in the row: index 0, as torch.argmax
        if (p.logprob) {
            const int t = p.targets[r];
            // (x[t] - M) - log(sum), not x[t] - lse: the first difference is the small one.  A target at or beyond V has no probability: NaN
            p.logprob[o] = t < 0 ? 0.f : t < V ? (lg[t] - M) - ls : __builtin_nanf("");
        }
    }
}

// The sibling that runs in front of a token pick (pgv_kv_set_logprobs): the row's maximum and ln sum exp(x - maximum), for the pick kernel to turn
// into x[t] - logsumexp(x) once it knows t.  Same two passes, same lane -> column map and the same reduction trees as logprob_rows_kernel, so the value
// is bit for bit what that kernel gives for the same row and token; but the rows of the decode logits are `vocab` floats apart (32003: odd), so
// every column is one guarded 4-byte load (a lane's four loads hit the same 16 bytes; the row is served from L2 right behind the lm_head GEMV).
__global__ __launch_bounds__(256) void row_lse_kernel(const float* __restrict__ logits, int ld, int V, float* __restrict__ stat) {
    __shared__ float s_val[4];
    __shared__ float s_sum[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nv = (V + 3) >> 2;
    const float* lg = logits + (size_t)r * ld;
    float best = -INFINITY;
    for (int q = tid; q < nv; q += 256) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            const float x = c < V ? lg[c] : -INFINITY;
            if (x > best) best = x;                        // NaN never wins
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        if (ov > best) best = ov;
    }
    if (lane == 0) s_val[w] = best;
    __syncthreads();
    float M = s_val[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (s_val[i] > M) M = s_val[i];
    float sum = 0.f;
    for (int q = tid; q < nv; q += 256) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            const float t = __builtin_amdgcn_exp2f(((c < V ? lg[c] : 0.f) - M) * 1.4426950408889634f);
            sum += c < V ? t : 0.f;
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) s_sum[w] = sum;
    __syncthreads();
    if (tid == 0) {
        const float total = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        stat[2 * r] = M;
        stat[2 * r + 1] = __builtin_amdgcn_logf(total) * 0.6931471805599453f;
    }
}

}  // namespace

int pgv_launch_row_lse(const float* logits, int ld, int V, int R, float* stat, hipStream_t s) {
    PGV_CHECK(logits && stat && V >= 1 && ld >= V && R >= 1, "row_lse: bad arguments");
    hipLaunchKernelGGL(row_lse_kernel, dim3(R), dim3(256), 0, s, logits, ld, V, stat);
    return PGV_OK;
}

int pgv_launch_logprob_rows(pgv_ctx* ctx, const float* logits, int ld, int V, int R, const int* targets, const int* out_rows, float* logprob, float* lse,
                            int* argmax, hipStream_t s) {
    PGV_CHECK(logits && targets, "logprob_rows: null logits / targets");
    PGV_CHECK(V >= 1 && ld >= V && ld % 4 == 0, "logprob_rows: V %d must be positive and ld %d a multiple of 4 that is at least V", V, ld);
    PGV_CHECK(((uintptr_t)logits & 15) == 0, "logprob_rows: the logits must be 16-byte aligned");
    PGV_CHECK(R >= 0, "logprob_rows: negative row count %d", R);
    if (R == 0) return PGV_OK;
    LogprobArgs a{logits, ld, V, targets, out_rows, logprob, lse, argmax};
    pgv_prof_begin(ctx, 6, s);
    hipLaunchKernelGGL(logprob_rows_kernel, dim3(R), dim3(256), 0, s, a);
    pgv_prof_end(ctx, 6, s, 0.0, 2.0 * (double)R * V * 4);
    return PGV_OK;
}

extern "C" int pgv_logprob_rows(pgv_ctx* ctx, const float* d_logits, int ld, int V, int R, const int32_t* d_targets, float* d_logprob, float* d_lse,
                                int32_t* d_argmax, void* stream) {
    PGV_CHECK(ctx != nullptr, "pgv_logprob_rows: null context");
    PGV_TRY(pgv_launch_logprob_rows(ctx, d_logits, ld, V, R, d_targets, nullptr, d_logprob, d_lse, d_argmax, (hipStream_t)stream));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}
