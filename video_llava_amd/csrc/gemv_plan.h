// The launch plan of a decode GEMV (gemv.hip): the quantities derived from the batch, the list of kernel instantiations, the choice among them,
// the weight format a launch streams and the argument checks.  Host-only, plain C++ without HIP headers: gemv.hip and llm.hip include it, and
// tests/test_host_cpu.py compiles it on its own.  Nothing here depends on anything but the model shape, the batch and the chip's CU count, and
// every shape computes bit-identical results per batch column (tests/test_gpu_llm.py), so the choice is performance only.
#pragma once
#include <stddef.h>
#include <stdio.h>

enum { GV_STORE16 = 0, GV_RESID = 1, GV_SWIGLU = 2, GV_F32 = 3, GV_RESIDNORM = 5 };     // gemv.hip epilogues
enum { WF_16 = 0, WF_FP8 = 1, WF_12 = 2 };                                              // weight formats of the decode GEMVs
constexpr int kMaxBatch = 64;        // decode GEMVs: up to 4 MFMA column tiles of 16 sequences per weight fragment
constexpr int kGemvWaves = 8;        // waves per workgroup = K phases of a row block (the arithmetic of every launch shape is defined on these 8 chains)
// float4 chunks of sum-of-squares partials a consumer workgroup loads (3 per thread): >= 4 x hidden / 16 up to hidden 6144
constexpr int kGemvSsqChunks = 3 * kGemvWaves * 64;

// Column tiles of 16 sequences a batch of B runs with, and those of the blocked activation layout (0: row-major -- up to 8 sequences the merged
// row loads of the narrow kernels, one full line per sequence and group, are cheaper).  The ONE place that decides it: producers and consumers,
// the side arrays of a cache and the 8-phase scratch must agree.
constexpr int gemv_col_tiles(int B) { return B <= 16 ? 1 : (B <= 32 ? 2 : 4); }
constexpr int gemv_xblk_tiles(int B) { return B <= 8 ? 0 : gemv_col_tiles(B); }
// What a launch is counted in: row blocks of 16, for SwiGLU (gate, up) pairs of them; and the workgroups for tl row blocks each (a ragged last
// workgroup clamps its row blocks and stores nothing for those past the matrix)
constexpr int gemv_units(int mode, int N) { return mode == GV_SWIGLU ? N / 32 : (N + 15) / 16; }
constexpr int gemv_units_per_wg(int mode, int tl) { return mode == GV_SWIGLU ? tl / 2 : tl; }
constexpr int gemv_grid(int mode, int units, int tl) { return (units + gemv_units_per_wg(mode, tl) - 1) / gemv_units_per_wg(mode, tl); }
// 8-phase residual producers: the phase tiles [row blocks][8][column tiles][64] float4, and the LDS of the x slice of one pass -- every group
// (64 columns) of the longest phase, or as many whole groups as fit 96 KiB
constexpr size_t gemv_k8_part_bytes(int nrb, int ct) { return (size_t)nrb * 8 * ct * 1024; }
constexpr unsigned kGemvK8LdsMax = 96u * 1024u;
constexpr unsigned gemv_k8_lds_bytes(int K, int ct) {
    const unsigned budget = kGemvK8LdsMax, per_group = (unsigned)ct * 16u * 128u, all = (unsigned)(((K / 32 + 1) / 2 + 7) / 8) * per_group;
    return all > budget ? budget / per_group * per_group : all;
}

// The kernel instantiations, written once: ROW(epilogue, row blocks per workgroup, column tiles) of the 16-row kernel, K8(column tiles, row blocks
// = waves per workgroup) of the 8-phase producer.  gemv.hip generates the launch lookup and the per-device configure loop from it.
#define GEMV_KERNELS(ROW, K8)                                                                                                                        \
    /* one MFMA tile of sequences (B <= 16) */                                                                                                       \
    ROW(GV_STORE16, 1, 1) ROW(GV_STORE16, 3, 1) ROW(GV_STORE16, 4, 1) ROW(GV_RESID, 1, 1) ROW(GV_SWIGLU, 2, 1) ROW(GV_F32, 1, 1) ROW(GV_F32, 8, 1)    \
    ROW(GV_RESIDNORM, 1, 1)                                                                                                                          \
    /* 2 / 4 column tiles (B <= 32 / 64) */                                                                                                          \
    ROW(GV_STORE16, 1, 2) ROW(GV_STORE16, 3, 2) ROW(GV_STORE16, 4, 2) ROW(GV_RESID, 1, 2) ROW(GV_SWIGLU, 2, 2) ROW(GV_SWIGLU, 4, 2)                  \
    ROW(GV_SWIGLU, 6, 2) ROW(GV_SWIGLU, 8, 2) ROW(GV_F32, 1, 2) ROW(GV_F32, 8, 2) ROW(GV_RESIDNORM, 1, 2)                                            \
    ROW(GV_STORE16, 1, 4) ROW(GV_STORE16, 3, 4) ROW(GV_STORE16, 4, 4) ROW(GV_RESID, 1, 4) ROW(GV_SWIGLU, 2, 4) ROW(GV_SWIGLU, 4, 4)                  \
    ROW(GV_SWIGLU, 6, 4) ROW(GV_SWIGLU, 8, 4) ROW(GV_F32, 1, 4) ROW(GV_F32, 8, 4) ROW(GV_RESIDNORM, 1, 4)                                            \
    K8(1, 8) K8(1, 10) K8(2, 8) K8(2, 10) K8(4, 8) K8(4, 10)
#define GEMV_NONE(...)
// Every ROW entry exists with 16-bit and with fp8 weights.  The merged x load (x2, B <= 8) uses the lanes of batch columns 8..15: one column tile
// only, and not the half-group pipeline of six row blocks and more.  The 12-bit copy (bf16, never fp8) is streamed at one column tile.
constexpr bool gemv_variant_ok(int tl, int ct, int wf, bool x2) { return (!x2 || (ct == 1 && tl < 6)) && (wf != WF_12 || ct == 1); }
constexpr bool gemv_has_kernel(int mode, int tl, int ct, int wf, bool x2) {
#define GEMV_ROW(M, TL, CT) if (mode == M && tl == TL && ct == CT) return gemv_variant_ok(tl, ct, wf, x2);
    GEMV_KERNELS(GEMV_ROW, GEMV_NONE)
#undef GEMV_ROW
    return false;
}
constexpr bool gemv_has_k8_kernel(int ct, int nwb) {
#define GEMV_K8(CT, NWB) if (ct == CT && nwb == NWB) return true;
    GEMV_KERNELS(GEMV_NONE, GEMV_K8)
#undef GEMV_K8
    return false;
}

// Launch-shape A/B switches, the defaults being the product's.  gemv.hip fills them from the environment in the lab library only (-DPGV_LAB, never
// loaded by the product): PGV_GEMV_X2, _K8, _K8_NWB10, _K8_NARROW_MINK (below 0: 4096 with 10 row blocks per workgroup, 12288 with 8), _TL3,
// _TL4, _WIDE_QKV4, _WIDE_TL4, _WIDE_TL6, _WIDE_TL8, _WIDE_FP8, _WIDE_HEAD8.
struct GemvLab { int x2 = 1, k8 = 1, k8_nwb10 = 1, k8_narrow_mink = -1, tl3 = 1, tl4 = 1, wide_qkv4 = 1, wide_tl4 = 1, wide_tl6 = 1, wide_tl8 = 1, wide_fp8 = 1, wide_head8 = 1; };

struct GemvChoice { int tl = 1, ct = 1; bool x2 = false, k8 = false; int nwb = 8; };

// TL = row blocks per workgroup (they share the x fragments), CT = column tiles, x2 = merged x load, k8 = the 8-phase residual producer.
// units = gemv_units(mode, N).
static inline GemvChoice choose_gemv(int mode, bool w8, int B, int units, int K, int num_cu, bool have_k8_scratch, const GemvLab& lab = GemvLab()) {
    const int grid = units;
    GemvChoice c{1, gemv_col_tiles(B), B <= 8 && lab.x2 != 0, false, 8};
    // row blocks (= waves) per 8-phase workgroup: 8, or 10 where that makes (row groups x 8 phases) exactly one workgroup per CU (13B: 320 row
    // blocks -> 32 groups x 8 = 256 workgroups of 10 waves instead of 320 of 8 = 1 1/4 rounds).  The (row block, phase) partition and the phase
    // order of the sums do not depend on it: bitwise the same result.
    // (13B fp8, 8 sequences, same box: 6.53 -> 6.64 videos/s with down_proj alone in that shape, 6.71 with o_proj as well.)
    if (lab.k8_nwb10 != 0 && grid % 10 == 0 && grid / 10 * 8 == num_cu) c.nwb = 10;
    const bool k8_ok = have_k8_scratch && lab.k8 != 0 && grid % c.nwb == 0;
    if (B > 16) {
        // Wide batches re-read 2 - 4 x the activation lines per workgroup, so the row blocks that share them matter more: qkv 3, gate/up two
        // (gate, up) pairs when the block counts divide.
        if (mode == GV_STORE16 && grid % 3 == 0) c.tl = 3;
        // ... four where three leave a ragged second round and four fill one (13B qkv: 960 row blocks -> 320 workgroups = 1 1/4 rounds with three,
        // 240 with four -- the choice the narrow batches make below, for the same reason)
        if (mode == GV_STORE16 && lab.wide_qkv4 != 0 && grid % 4 == 0 && grid / 4 <= num_cu && (grid % 3 != 0 || grid / 3 > num_cu)) c.tl = 4;
        // (four column tiles: 228 VGPRs once the sum-of-squares partials are requested after the weight loop, SSQ_LATE)
        if (mode == GV_SWIGLU) c.tl = (grid % 2 == 0 && (B <= 32 || lab.wide_tl4 != 0)) ? 4 : 2;
        // A wide workgroup holds a CU to itself (its registers and the LDS of its partial tiles), so the launch runs in ROUNDS of num_cu workgroups
        // and every workgroup moves the whole activation operand through its CU: 7B gate/up = 688 (gate, up) pairs -> 344 workgroups of two pairs =
        // two rounds (88 CUs run a second workgroup, the others wait: 50.9 us at 64 sequences), 230 workgroups of THREE pairs = one round and a third
        // fewer reads of x (LAB.md round 6).  Taken when three pairs per workgroup fit one round and two do not.
        if (mode == GV_SWIGLU && (!w8 || lab.wide_fp8 != 0) && lab.wide_tl6 != 0 && (grid + 2) / 3 <= num_cu && (grid + 1) / 2 > num_cu) c.tl = 6;
        // ... four pairs where three still need a second round (13B gate/up: 864 pairs -> 288 workgroups of three, 216 of four)
        else if (mode == GV_SWIGLU && (!w8 || lab.wide_fp8 != 0) && lab.wide_tl8 != 0 && (grid + 3) / 4 <= num_cu && (grid + 1) / 2 > num_cu) c.tl = 8;
        // lm_head: 2001 row blocks; one per workgroup means 2001 passes over the activation operand (512 KB each against 128 KB of weights: 102 us at
        // 64 sequences).  Eight per workgroup: 251 workgroups, one round.
        if (mode == GV_F32 && (!w8 || lab.wide_fp8 != 0) && lab.wide_head8 != 0 && (grid + 7) / 8 <= num_cu) c.tl = 8;
        // narrow matrices (o_proj, down_proj): 8 row blocks x K phase per workgroup + a finish launch where it pays (kernel trace at 32 clips:
        // down_proj 32.0 -> 22.4 + 4.9 us (finish), o_proj 13.3 -> 9.6 + 4.9: the short-K matrix only gains once the batch spans four tiles)
        if (mode == GV_RESIDNORM) c.k8 = k8_ok && (K / 64) >= 16 && (B > 32 || K >= 8192);
        return c;
    }
    switch (mode) {
        case GV_STORE16:
            // three row blocks per workgroup when that puts at most ~one workgroup on every CU and nothing is left over (7B qkv: 768 -> 256;
            // 13B: 960 -> 320 workgroups, two resident per CU -- with fp8 weights a 16-row workgroup requests as many activation lines as weight
            // lines: qkv 20.7 -> 18.7 us; with 16-bit weights the same launch shape LOSES 4 us per layer, so the relaxed bound is for fp8 only)
            if (lab.tl3 != 0 && grid % 3 == 0 && grid / 3 <= (w8 ? 2 : 1) * num_cu && grid / 3 >= num_cu / 2) c.tl = 3;
            // ... unless three blocks leave a ragged second round and FOUR give one round that nearly fills the chip (13B qkv: 960 row blocks ->
            // 320 workgroups = 1 1/4 rounds with three, 240 workgroups on 256 CUs with four: same box, fp8 weights 6.68 -> 6.92 videos/s and the
            // GEMV family 0.539 -> 0.570 of 8 TB/s; 16-bit weights 4.79 -> 4.84)
            if (lab.tl4 != 0 && grid % 4 == 0 && grid / 4 <= num_cu && grid / 4 >= num_cu - num_cu / 8 && !(grid % 3 == 0 && grid / 3 == num_cu)) c.tl = 4;
            break;
        case GV_SWIGLU: c.tl = 2; break;
        case GV_F32:
            // lm_head at 9 .. 16 sequences: 2001 workgroups of one row block each read the whole activation operand (128 KB against 128 KB of
            // weights); eight row blocks per workgroup as at the wide batches (251 workgroups, one round)
            if ((!w8 || lab.wide_fp8 != 0) && B > 8 && lab.wide_head8 != 0 && (grid + 7) / 8 <= num_cu) c.tl = 8;
            break;
        case GV_RESIDNORM:
            // fp8 down_proj of the 13B shapes (K = 13 824, 320 row blocks): a 16-row workgroup requests as many activation lines as weight lines
            // (LAB.md "what the activation operand costs"); the 8-phase form reads 1/8 of x per workgroup and is bitwise the same result
            // With 10 row blocks per workgroup (13B) the short-K producer (o_proj, K = 5120) gains too: one workgroup per CU, 1/8 of x each.
            c.k8 = w8 && k8_ok && K >= (lab.k8_narrow_mink >= 0 ? lab.k8_narrow_mink : (c.nwb == 10 ? 4096 : 12288));
            break;
        default: break;
    }
    return c;
}

// The weight format a launch streams.  The 12-bit copy (w12.h) replaces W at one column tile, not with fp8 and not in the 8-phase form; beyond,
// the 16-bit matrix is streamed (the same products in the same order).  pgv_llm_weight_stream_bytes counts with the same predicate.
constexpr int gemv_weight_format(bool w8, bool have12, const GemvChoice& c) { return have12 && !w8 && c.ct == 1 && !c.k8 ? WF_12 : (w8 ? WF_FP8 : WF_16); }

// A launch as plain shapes and "is this pointer present" flags.  norm: a GemvNorm is given, the fields behind it are read from it.
struct GemvCall {
    int mode = 0, N = 0, K = 0, B = 0, num_cu = 256;
    bool w8 = false, bf16 = false, W = false;          // fp8 matrix with per-row scales; the activations are bf16; the 16-bit / fp8 matrix is present
    bool w12 = false; long long rows12 = 0;            // a 12-bit copy is present; the row count it was encoded with
    bool norm = false;
    int nparts_in = 0, ssq_ts = 0, amax_ts = 0;
    bool amax_val = false, gamma = false, xg = false, ssq_out = false, k8_part = false, x_blocked = false;
};
// What the launch runs: the shape as pgv_gemv_shape reports it (x2 as launched, nwb 0 outside the 8-phase form), the unit count and the workgroups
// of the 16-row kernel, and whether x is read / xg is written in the blocked activation layout.
struct GemvPlan { int tl = 1, ct = 1, x2 = 0, k8 = 0, nwb = 0, wf = WF_16, units = 0, grid = 0; bool xblk = false, xgblk = false; };

// The first refusal is formatted into err and returned as its class: every one is an invalid argument of the call (PGV_EINVAL in pgv.h).
enum GemvPlanStatus { GEMV_PLAN_OK = 0, GEMV_PLAN_EINVAL = 1 };
#define GEMV_PLAN_CHECK(cond, ...) do { if (!(cond)) { snprintf(err, err_len, __VA_ARGS__); return GEMV_PLAN_EINVAL; } } while (0)
static inline GemvPlanStatus gemv_plan_build(const GemvCall& in, GemvPlan& plan, char* err, size_t err_len, const GemvLab& lab = GemvLab()) {
    const int mode = in.mode, N = in.N, K = in.K, B = in.B;
    GEMV_PLAN_CHECK(B >= 1 && B <= 64, "gemv: batch %d outside [1,64]", B);
    GEMV_PLAN_CHECK(K % 32 == 0, "gemv: K=%d must be a multiple of 32", K);
    GEMV_PLAN_CHECK(mode == GV_STORE16 || mode == GV_RESID || mode == GV_SWIGLU || mode == GV_F32 || mode == GV_RESIDNORM, "gemv: bad mode %d", mode);
    GEMV_PLAN_CHECK(B <= 16 || !in.norm || (in.ssq_ts > 0 && (!in.amax_val || in.amax_ts > 0)), "gemv: batches beyond 16 need the tile strides of the side arrays");
    plan = GemvPlan();
    if (in.norm) {
        if (in.x_blocked && gemv_xblk_tiles(B) > 0) {          // consumers read x blocked, producers write xg blocked
            if (mode == GV_RESIDNORM) { GEMV_PLAN_CHECK(N % 32 == 0, "gemv: a blocked xg needs N in multiples of 32"); plan.xgblk = true; }
            else plan.xblk = true;                              // (K % 32 == 0 is checked above)
        }
        GEMV_PLAN_CHECK(in.nparts_in * 4 <= kGemvSsqChunks, "gemv: %d sum-of-squares partials exceed what a consumer workgroup loads (hidden <= 6144)", in.nparts_in);
    }
    GEMV_PLAN_CHECK(mode != GV_RESIDNORM || (in.norm && in.gamma && in.xg && in.ssq_out), "gemv: the residual+norm producer needs gamma / xg / ssq_out");
    if (in.w8) GEMV_PLAN_CHECK(K % 64 == 0, "gemv fp8: K=%d must be a multiple of 64", K);
    // W must be in the fragment-blocked layout with its row count padded to a multiple of 16 (zero rows)
    if (mode == GV_SWIGLU) GEMV_PLAN_CHECK(N % 64 == 0, "gemv swiglu: N=%d must be a multiple of 64", N);
    else if (mode != GV_F32) GEMV_PLAN_CHECK(N % 16 == 0, "gemv: N=%d must be a multiple of 16", N);
    plan.units = gemv_units(mode, N);
    const GemvChoice c = choose_gemv(mode, in.w8, B, plan.units, K, in.num_cu, in.norm && in.k8_part, lab);
    plan.wf = gemv_weight_format(in.w8, in.w12, c);
    if (in.w12) {
        GEMV_PLAN_CHECK(!in.w8 && in.bf16 && K % 64 == 0 && in.rows12 % 16 == 0 && in.rows12 >= ((N + 15) & ~15), "gemv: bad 12-bit weight copy (%lld rows for N = %d, K = %d)",
                        in.rows12, N, K);
        GEMV_PLAN_CHECK(plan.wf == WF_12 || in.W, "gemv: %d sequences need the 16-bit matrix (the 12-bit copy serves one column tile)", B);
    }
    plan.tl = c.tl; plan.ct = c.ct; plan.x2 = !c.k8 && c.x2 && c.ct == 1; plan.k8 = c.k8; plan.nwb = c.k8 ? c.nwb : 0;
    plan.grid = gemv_grid(mode, plan.units, c.tl);
    // the table holds every shape choose_gemv returns (tests/test_host_cpu.py sweeps it); the launch lookup in gemv.hip refuses what it does not
    return GEMV_PLAN_OK;
}

// The test entry pgv_gemv_ex: what a wrong test argument could turn into a stray write, checked in front of gemv_plan_build.
struct GemvDescShape {
    int mode = 0, N = 0, K = 0, B = 0, ldx = 0, ldo = 0, ssq_ts = 0, amax_ts = 0, nparts_in = 0, hidden = 0; size_t k8_part_bytes = 0;
    bool W = false, W12 = false, x = false, out = false, ssq_in = false, gamma = false, xg = false, ssq_out = false, amax_val = false, amax_idx = false, k8_part = false,
         x_blocked = false;
};
static inline GemvPlanStatus gemv_check_desc(const GemvDescShape& d, char* err, size_t err_len) {
    GEMV_PLAN_CHECK((d.W || d.W12) && d.x && d.out, "pgv_gemv_ex: null W / x / out");
    const int mode = d.mode, N = d.N, K = d.K, B = d.B;
    GEMV_PLAN_CHECK((mode >= GV_STORE16 && mode <= GV_F32) || mode == GV_RESIDNORM, "pgv_gemv_ex: mode %d is none of 0..3, 5", mode);
    GEMV_PLAN_CHECK(B >= 1 && B <= kMaxBatch && N >= 1 && K >= 32, "pgv_gemv_ex: bad shape N = %d, K = %d, B = %d", N, K, B);
    const int nrb = (N + 15) / 16;
    const size_t k8_bytes = gemv_k8_part_bytes(nrb, gemv_col_tiles(B));
    const bool producer = mode == GV_RESIDNORM, consumer = mode == GV_STORE16 || mode == GV_SWIGLU || mode == GV_F32;
    const bool blocked = d.x_blocked && gemv_xblk_tiles(B) > 0;
    GEMV_PLAN_CHECK((blocked && !producer) || (d.ldx >= K && d.ldx % 8 == 0), "pgv_gemv_ex: ldx = %d for K = %d (row-major x: 16-byte rows)", d.ldx, K);
    GEMV_PLAN_CHECK(d.ldo >= (mode == GV_SWIGLU ? N / 2 : N) && (mode == GV_F32 || d.ldo % 4 == 0), "pgv_gemv_ex: ldo = %d for N = %d, mode %d", d.ldo, N, mode);
    GEMV_PLAN_CHECK(d.ssq_ts >= 0 && d.amax_ts >= 0 && d.nparts_in >= 0, "pgv_gemv_ex: negative stride or count");
    GEMV_PLAN_CHECK(!d.ssq_in || (consumer && d.nparts_in >= 1 && d.hidden >= 1 && d.ssq_ts >= 16 * d.nparts_in),
                    "pgv_gemv_ex: ssq_in needs a consumer mode, nparts_in >= 1, hidden >= 1 and ssq_ts >= 16 nparts_in (mode %d, %d parts, ssq_ts %d)", mode, d.nparts_in, d.ssq_ts);
    GEMV_PLAN_CHECK(producer == (d.gamma || d.xg || d.ssq_out), "pgv_gemv_ex: gamma / xg / ssq_out belong to mode 5, and mode 5 needs all three");
    if (producer) GEMV_PLAN_CHECK(d.gamma && d.xg && d.ssq_out && d.ssq_ts >= N, "pgv_gemv_ex: a producer needs gamma, xg, ssq_out and ssq_ts >= N (%d < %d)", d.ssq_ts, N);
    GEMV_PLAN_CHECK(d.amax_val == d.amax_idx && (!d.amax_val || (mode == GV_F32 && d.amax_ts >= 16 * nrb)),
                    "pgv_gemv_ex: the candidates need mode 3, both arrays and amax_ts >= 16 ceil(N / 16) (%d < %d)", d.amax_ts, 16 * nrb);
    GEMV_PLAN_CHECK(!d.k8_part || (producer && d.k8_part_bytes >= k8_bytes),
                    "pgv_gemv_ex: k8_part belongs to mode 5 and holds (N / 16) * 8 * ct * 1024 = %zu bytes (%zu given)", k8_bytes, d.k8_part_bytes);
    return GEMV_PLAN_OK;
}
#undef GEMV_PLAN_CHECK
