// Lab: what binds the 12-bit residual producers (gemv_mfma_kernel, MODE 5, TL 1, W12) at the two 7B shapes, N = 4096 with K = 4096 (o_proj) and
// K = 11008 (down_proj).  Chains of 64 launches over 16 HBM-cold copies of one encoded matrix, captured in a hipGraph, against the bare
// read-only chain of scripts/lab/tail_prefetch.hip at the same bytes (25.2 / 67.6 MB).  With a lab library (build.build(lab=True) or
// build_variant(name, ["PGV_LAB", ...])) the ablations of GV_ABL are timed too: 2 = no decode VALU / MFMA, 1 = no x loads, 4 = no weight loads.
// The library is loaded by path, so one binary times every variant build (-DPGV_W12_PRODUCER_PU=1 .. 4).  Not product code.
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/w12_producer_chain scripts/lab/w12_producer_chain.hip -ldl
//   /tmp/w12_producer_chain video_llava_amd/libpgv.so [B]            the producer against the bare chain at B sequences (default 8, at most 16)
//   /tmp/w12_producer_chain video_llava_amd/libpgv_lab.so B lab      ... and the ablations
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/pgv.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)
#define PK(x) do { int e = (x); if (e) { printf("%s: %s\n", #x, p_last_error()); exit(1); } } while (0)
typedef __attribute__((ext_vector_type(4))) unsigned int u4;

static decltype(&pgv_ctx_create) p_ctx_create;
static decltype(&pgv_last_error) p_last_error;
static decltype(&pgv_pack_blocked) p_pack_blocked;
static decltype(&pgv_w12_bytes) p_w12_bytes;
static decltype(&pgv_encode_w12_blocked) p_encode;
static decltype(&pgv_gemv_ex) p_gemv_ex;

// the bare chain: 256 workgroups x 8 waves, two buffers of 4 x 1 KiB wave-loads, LDS reduce + 1 KiB store (tail_prefetch.hip without the prefetch)
__global__ __launch_bounds__(512) void chain_kernel(const char* cur, size_t bytes, float* out) {
    __shared__ u4 red[8][64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t per_wg = bytes / gridDim.x;
    const char* p = cur + (size_t)blockIdx.x * per_wg + lane * 16;
    const int nblk = (int)(per_wg / 1024);
    const int nb = (nblk - w + 7) / 8;
    u4 acc = {0, 0, 0, 0};
    u4 a[4], b[4];
    auto load = [&](u4 (&v)[4], int i0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load((const u4*)(p + (size_t)(w + 8 * min(i0 + u, nb - 1)) * 1024));
    };
    auto use = [&](u4 (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) acc ^= v[u];
    };
    load(a, 0);
    int i = 0;
    for (; i + 8 < nb; i += 8) {
        load(b, i + 4);
        __builtin_amdgcn_sched_barrier(0);
        use(a);
        __builtin_amdgcn_sched_barrier(0);
        load(a, i + 8);
        __builtin_amdgcn_sched_barrier(0);
        use(b);
        __builtin_amdgcn_sched_barrier(0);
    }
    load(b, i + 4);
    use(a);
    use(b);
    red[w][lane] = acc;
    __syncthreads();
    if (w != 0) return;
    u4 t = red[0][lane];
#pragma unroll
    for (int k = 1; k < 8; ++k) t ^= red[k][lane];
    out[(size_t)blockIdx.x * 64 + lane] = (float)(t[0] ^ t[1] ^ t[2] ^ t[3]);
}

constexpr int kCopies = 16;          // matrices in rotation: 400 MB / 1.1 GB, beyond the 256 MB Infinity Cache

template <typename F>
static double time_chain(const char* name, double bytes, F launch) {
    hipStream_t s; CK(hipStreamCreate(&s));
    const int n = 64;
    hipGraph_t g; hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    for (int i = 0; i < n; ++i) launch(i % kCopies, s);
    CK(hipStreamEndCapture(s, &g));
    CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    float best = 1e9f, sum = 0.f;
    for (int r = 0; r < 8; ++r) {
        CK(hipEventRecord(a, s)); CK(hipGraphLaunch(ge, s)); CK(hipEventRecord(b, s)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (r > 0) { sum += ms; if (ms < best) best = ms; }
    }
    printf("  %-40s %6.2f us per launch (best %6.2f)   %.2f TB/s\n", name, sum / 7 * 1e3 / n, best * 1e3 / n, bytes / (sum / 7 * 1e-3 / n) / 1e12);
    CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g)); CK(hipStreamDestroy(s));
    return sum / 7 * 1e3 / n;
}

static uint16_t bf16_of(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IONBF, 0);
    if (argc < 2) { printf("usage: %s libpgv[_variant].so [B [lab]]\n", argv[0]); return 2; }
    const int B = argc > 2 ? atoi(argv[2]) : 8;
    if (B < 1 || B > 16) { printf("B = %d outside [1, 16] (the 12-bit copy serves one column tile)\n", B); return 2; }
    void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!h) { printf("dlopen: %s\n", dlerror()); return 1; }
#define SYM(v, n) do { v = (decltype(v))dlsym(h, n); if (!v) { printf("missing %s\n", n); return 1; } } while (0)
    SYM(p_ctx_create, "pgv_ctx_create"); SYM(p_last_error, "pgv_last_error"); SYM(p_pack_blocked, "pgv_pack_blocked"); SYM(p_w12_bytes, "pgv_w12_bytes");
    SYM(p_encode, "pgv_encode_w12_blocked"); SYM(p_gemv_ex, "pgv_gemv_ex");
    pgv_ctx* ctx; PK(p_ctx_create(0, &ctx));
    const int N = 4096, NM = kCopies;
    float* resid; CK(hipMalloc(&resid, (size_t)B * N * 4)); CK(hipMemset(resid, 0, (size_t)B * N * 4));
    float* gamma; CK(hipMalloc(&gamma, N * 4)); CK(hipMemset(gamma, 0, N * 4));
    char* xg; CK(hipMalloc(&xg, (size_t)B * N * 2));
    float* ssq; CK(hipMalloc(&ssq, N * 4));
    float* out; CK(hipMalloc(&out, 256 * 64 * 4));
    for (int K : {4096, 11008}) {
        // one matrix like the bench's (normal-ish, sigma 0.02), blocked, encoded, 16 copies
        std::vector<uint16_t> hw((size_t)N * K);
        uint64_t st = 0x9E3779B97F4A7C15ull + (uint64_t)K;
        for (auto& v : hw) {
            float a = 0.f;
            for (int q = 0; q < 4; ++q) { st = st * 6364136223846793005ull + 1442695040888963407ull; a += (float)(st >> 40) * (1.0f / 16777216.0f) - 0.5f; }
            v = bf16_of(a * 0.02f * 1.7320508f);
        }
        uint16_t *w16, *wb; CK(hipMalloc(&w16, hw.size() * 2)); CK(hipMalloc(&wb, hw.size() * 2));
        CK(hipMemcpy(w16, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
        PK(p_pack_blocked(ctx, PGV_BF16, w16, N, K, wb, nullptr));
        const size_t nb12 = p_w12_bytes(N, K), slot = (nb12 + 4095) & ~(size_t)4095;
        char* w12; CK(hipMalloc(&w12, slot * NM)); CK(hipMemset(w12, 0, slot * NM));
        int* counts; CK(hipMalloc(&counts, N / 16 * 4));
        PK(p_encode(ctx, PGV_BF16, wb, w12, counts, N, K, nullptr));
        CK(hipDeviceSynchronize());
        std::vector<int> hc(N / 16); CK(hipMemcpy(hc.data(), counts, hc.size() * 4, hipMemcpyDeviceToHost));
        int cmax = 0; for (int c : hc) cmax = c > cmax ? c : cmax;
        if (cmax > 64) { printf("K = %d: %d exceptions in a row block\n", K, cmax); return 1; }
        for (int m = 1; m < NM; ++m) CK(hipMemcpy(w12 + slot * m, w12, nb12, hipMemcpyDeviceToDevice));
        std::vector<uint16_t> hx((size_t)B * K);
        for (auto& v : hx) { st = st * 6364136223846793005ull + 1442695040888963407ull; v = bf16_of((float)(st >> 40) * (2.0f / 16777216.0f) - 1.0f); }
        char* x; CK(hipMalloc(&x, hx.size() * 2)); CK(hipMemcpy(x, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
        const double bytes = 1.5 * N * K;
        printf("== N = %d, K = %d, B = %d: %.1f MB of 12-bit weights (%d exceptions at most per row block) ==\n", N, K, B, bytes / 1e6, cmax);
        pgv_gemv_shape shp = {};
        auto gemv = [&](int m, hipStream_t s) {
            pgv_gemv_desc d = {};
            d.mode = 5; d.d_W12 = w12 + slot * m; d.d_x = x; d.ldx = K; d.d_out = resid; d.ldo = N; d.N = N; d.K = K; d.B = B;
            d.d_gamma = gamma; d.d_xg = xg; d.d_ssq_out = ssq; d.ssq_ts = N; d.hidden = N; d.shape = &shp;
            PK(p_gemv_ex(ctx, PGV_BF16, &d, s));
        };
        const size_t cb = (size_t)bytes / (256 * 8192) * (256 * 8192);
        auto bare = [&](int m, hipStream_t s) { hipLaunchKernelGGL(chain_kernel, dim3(256), dim3(512), 0, s, w12 + slot * m, cb, out); };
        const double t_bare = time_chain("bare read-only chain", (double)cb, bare);
        unsetenv("PGV_GEMV_ABLATE");
        const double t_full = time_chain("producer", bytes, gemv);
        printf("  (ran: wfmt %d, tl %d, ct %d, x2 %d, k8 %d)   producer / bare chain = %.3f\n", shp.wfmt, shp.tl, shp.ct, shp.x2, shp.k8, t_full / t_bare);
        if (argc > 3) {          // lab library: the ablations (a release library ignores the variable)
            setenv("PGV_GEMV_ABLATE", "2", 1); time_chain("  no decode VALU / MFMA (abl 2)", bytes, gemv);
            setenv("PGV_GEMV_ABLATE", "1", 1); time_chain("  no x loads (abl 1)", bytes, gemv);
            setenv("PGV_GEMV_ABLATE", "3", 1); time_chain("  neither (abl 3)", bytes, gemv);
            setenv("PGV_GEMV_ABLATE", "4", 1); time_chain("  no weight loads (abl 4)", bytes, gemv);
            unsetenv("PGV_GEMV_ABLATE");
            time_chain("producer (again)", bytes, gemv);
        }
        time_chain("bare read-only chain (again)", (double)cb, bare);
        CK(hipFree(w16)); CK(hipFree(wb)); CK(hipFree(w12)); CK(hipFree(counts)); CK(hipFree(x));
    }
    return 0;
}
