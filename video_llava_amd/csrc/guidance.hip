// Classifier-free guidance between the lm_head and the pick (pgv.h: pgv_kv_set_guidance): HF's UnbatchedClassifierFreeGuidanceLogitsProcessor,
//   guided = scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond)
// on the logits rows of a conditional sequence and of its unconditional twin, and the step that keeps the twin's slot behind the conditional one.
#include "llm_internal.h"

namespace {

struct GuidanceArgs {
    const float* cond; const float* uncond; int ld, V;
    float scale;
    float* out; int ld_out;
};

// One workgroup of 8 waves per PAIR, three passes over its two rows: the maxima, the sums of exp(x - maximum), the mix.  Waves 0 - 3 take the
// conditional row's statistics, waves 4 - 7 the unconditional row's, side by side; all eight write the mix.  The rows come straight from the lm_head
// GEMV (128 KB each at the 32003-entry vocabulary), so passes two and three are served from L2.  A pure stream: two reads and one write of V floats
// per pair, LDS only for the cross-wave reductions.
// Alignment: the rows of the decode logits are `vocab` floats apart (32003: odd), so row p and row P + p sit at different offsets inside a 16-byte
// line and no vector width suits both.  Every access is one 4-byte load or store; in passes one and two a lane's four loads hit the same 16 bytes
// (row_lse_kernel's map), in pass three consecutive lanes touch consecutive floats.
// Fixed order (batch invariance): each row's statistics are row_lse_kernel's, operation for operation -- lane t of the row's 256 covers the
// columns 4 (t + 256 k) + e in (k, e) order, xor butterfly inside a wave, (w0 + w1) + (w2 + w3) across the row's four waves -- so (x[v] - M) - ls is
// bit for bit the value pgv_logprob_rows gives for target v, and a pair's result depends on its two rows alone: not on P, the pair's index or the launch.
// The mix is written without contraction, in the order pgv.h states: lc = (xc - Mc) - lsc, lu = (xu - Mu) - lsu, out = scale * (lc - lu) + lu.
// IEEE results stand: a -inf in the conditional row gives -inf under a positive scale and NaN under scale 0 (0 * inf), as HF's tensor arithmetic does.
__global__ __launch_bounds__(512) void guidance_mix_kernel(GuidanceArgs a) {
    __shared__ float s_val[2][4];
    __shared__ float s_sum[2][4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, t = tid & 255;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = wave >> 2, w = wave & 3;             // which row this wave reduces, and its place among the row's four waves
    const int V = a.V, nv = (V + 3) >> 2;
    const float* xc = a.cond + (size_t)p * a.ld;
    const float* xu = a.uncond + (size_t)p * a.ld;
    const float* x = half ? xu : xc;
    // ---- pass 1: the row's maximum (NaN never wins) -------------------------------------------------------
    float best = -INFINITY;
    for (int q = t; q < nv; q += 256) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            const float v = c < V ? x[c] : -INFINITY;
            if (v > best) best = v;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(best, off, 64);
        if (o > best) best = o;
    }
    if (lane == 0) s_val[half][w] = best;
    __syncthreads();
    float Mc = s_val[0][0], Mu = s_val[1][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        if (s_val[0][i] > Mc) Mc = s_val[0][i];
        if (s_val[1][i] > Mu) Mu = s_val[1][i];
    }
    // ---- pass 2: the row's sum of exp(x - M) ---------------------------------------------------------------
    const float M = half ? Mu : Mc;
    float sum = 0.f;
    for (int q = t; q < nv; q += 256) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            const float ex = __builtin_amdgcn_exp2f(((c < V ? x[c] : 0.f) - M) * 1.4426950408889634f);
            sum += c < V ? ex : 0.f;
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) s_sum[half][w] = sum;
    __syncthreads();
    const float lsc = __builtin_amdgcn_logf((s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3])) * 0.6931471805599453f;      // v_log_f32 is log2
    const float lsu = __builtin_amdgcn_logf((s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3])) * 0.6931471805599453f;
    // ---- pass 3: the mix --------------------------------------------------------------------------------------
    float* out = a.out + (size_t)p * a.ld_out;
    const float scale = a.scale;
    for (int c = tid; c < V; c += 512) {
        const float lc = __fsub_rn(__fsub_rn(xc[c], Mc), lsc);
        const float lu = __fsub_rn(__fsub_rn(xu[c], Mu), lsu);
        out[c] = __fadd_rn(__fmul_rn(scale, __fsub_rn(lc, lu)), lu);
    }
}

// The follow step behind the pick on rows [0, P): the twin slot P + p takes the conditional slot's token and done flag, and advances exactly as the
// pick advanced slot p (AM_INC_POS: position + 1; AM_RECORD: the token joins the twin's history, so rows [P, 2P) of d_tokens repeat rows [0, P)).
__global__ void guidance_follow_kernel(int P, int* __restrict__ cur, int* __restrict__ done, int* __restrict__ pos, int* __restrict__ step,
                                       int* __restrict__ hist, int hist_stride, int advance) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int t = p + P, tok = cur[p];
    cur[t] = tok;
    done[t] = done[p];
    if (advance & AM_RECORD) {
        hist[(size_t)t * hist_stride + step[t]] = tok;
        step[t] += 1;
    }
    if (advance & AM_INC_POS) pos[t] += 1;
}

}  // namespace

int pgv_launch_guidance_mix(const float* cond, const float* uncond, int ld, int V, int P, float scale, float* out, int ld_out, hipStream_t s) {
    PGV_CHECK(cond && uncond && out, "guidance_mix: null pointer");
    PGV_CHECK(V >= 1 && ld >= V && ld_out >= V && P >= 1, "guidance_mix: V %d, ld %d, ld_out %d, pairs %d: need V >= 1, both strides >= V, pairs >= 1", V, ld, ld_out, P);
    const GuidanceArgs a{cond, uncond, ld, V, scale, out, ld_out};
    hipLaunchKernelGGL(guidance_mix_kernel, dim3(P), dim3(512), 0, s, a);
    return PGV_OK;
}

int pgv_launch_guidance_follow(int P, const PickState& st, hipStream_t s) {
    PGV_CHECK(P >= 1 && st.next && st.done && st.pos && st.step && st.hist, "guidance_follow: the cache's pick state is incomplete");
    hipLaunchKernelGGL(guidance_follow_kernel, dim3((P + 63) / 64), dim3(64), 0, s, P, st.next, st.done, st.pos, st.step, st.hist, st.hist_stride, st.advance);
    return PGV_OK;
}

extern "C" int pgv_guidance_logits(pgv_ctx* ctx, const float* d_cond, const float* d_uncond, int ld, int V, int P, float scale, float* d_out, int ld_out,
                                   void* stream) {
    PGV_CHECK(ctx != nullptr, "pgv_guidance_logits: null context");
    PGV_CHECK(d_cond && d_uncond && d_out, "pgv_guidance_logits: null pointer");
    PGV_CHECK(V >= 1, "pgv_guidance_logits: V %d must be positive", V);
    PGV_CHECK(ld >= V && ld_out >= V, "pgv_guidance_logits: row strides %d / %d below V %d", ld, ld_out, V);
    PGV_CHECK(P >= 0, "pgv_guidance_logits: negative pair count %d", P);
    PGV_CHECK(scale == scale && scale - scale == 0.f, "pgv_guidance_logits: scale %g is not finite", (double)scale);
    PGV_CHECK((((uintptr_t)d_cond | (uintptr_t)d_uncond | (uintptr_t)d_out) & 3) == 0, "pgv_guidance_logits: the buffers must be 4-byte aligned");
    if (P == 0) return PGV_OK;
    PGV_TRY(pgv_launch_guidance_mix(d_cond, d_uncond, ld, V, P, scale, d_out, ld_out, (hipStream_t)stream));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}
