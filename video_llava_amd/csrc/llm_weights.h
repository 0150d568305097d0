// The decoder's weight matrices in one place: their shapes, the HF keys that land in them (row offset, gate / up interleave) and where
// each of their copies sits in its blob.  Host-only, plain C++ without HIP headers: llm.hip includes it, and tests/test_host_cpu.py
// compiles it on its own against the offsets and key mappings written out independently.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "pgv_sizes.h"

constexpr int kMaxPos = 4096;   // max_position_embeddings of LLaVA-1.5 / Vicuna-1.5

// pgv_llm::mats holds lm_head first, then the four matrices of each layer in this order
enum { MAT_QKV = 0, MAT_O = 1, MAT_GU = 2, MAT_DOWN = 3, MAT_PER_LAYER = 4 };
constexpr int llm_mat_index(int layer, int kind) { return 1 + layer * MAT_PER_LAYER + kind; }

// HF keys `model.layers.<i>.<suffix>` of the matrices: checkpoint rows [0, rows) go to matrix row
// (r / row_blk) * blk_stride + r % row_blk + row_off (row_blk 0: r + row_off) -- PackDst in weights.h.
// A row count or offset is h * hidden + i * intermediate + c.
struct LlmDim { int h, i, c; };
constexpr long long llm_dim(LlmDim d, long long H, long long I) { return d.h * H + d.i * I + d.c; }
struct LlmMatKey { const char* suffix; int kind; LlmDim row_off, rows; int row_blk, blk_stride; };
constexpr LlmMatKey kLlmMatKeys[] = {
    {"self_attn.q_proj.weight", MAT_QKV, {0, 0, 0}, {1, 0, 0}, 0, 0},
    {"self_attn.k_proj.weight", MAT_QKV, {1, 0, 0}, {1, 0, 0}, 0, 0},
    {"self_attn.v_proj.weight", MAT_QKV, {2, 0, 0}, {1, 0, 0}, 0, 0},
    {"self_attn.o_proj.weight", MAT_O, {0, 0, 0}, {1, 0, 0}, 0, 0},
    {"mlp.gate_proj.weight", MAT_GU, {0, 0, 0}, {0, 1, 0}, 32, 64},       // [32 gate | 32 up] per 64 rows
    {"mlp.up_proj.weight", MAT_GU, {0, 0, 32}, {0, 1, 0}, 32, 64},
    {"mlp.down_proj.weight", MAT_DOWN, {0, 0, 0}, {1, 0, 0}, 0, 0},
};

enum LlmKeyStatus {
    LLM_KEY_NOT_LAYER,      // does not start with "model.layers.": `rest` is empty
    LLM_KEY_BAD_INDEX,      // no number, no '.' behind it, or a layer the model does not have: `rest` is empty
    LLM_KEY_OTHER,          // a layer's key, but none of the matrices: `rest` is the suffix (norm vectors, rotary_emb.inv_freq, unknown ones)
    LLM_KEY_MATRIX,         // `mat` is its row of kLlmMatKeys
};
struct LlmLayerKey { LlmKeyStatus status; int layer; const char* rest; const LlmMatKey* mat; };
inline LlmLayerKey llm_parse_layer_key(const char* name, int layers) {
    if (strncmp(name, "model.layers.", 13) != 0) return {LLM_KEY_NOT_LAYER, -1, "", nullptr};
    char* end = nullptr;
    const long li = strtol(name + 13, &end, 10);
    if (end == name + 13 || *end != '.' || li < 0 || li >= layers) return {LLM_KEY_BAD_INDEX, -1, "", nullptr};
    for (const LlmMatKey& t : kLlmMatKeys)
        if (!strcmp(end + 1, t.suffix)) return {LLM_KEY_MATRIX, (int)li, end + 1, &t};
    return {LLM_KEY_OTHER, (int)li, end + 1, nullptr};
}

// Where every item sits in the 16-bit blob, the fp8 blob (pgv_llm_quantize_fp8) and the 12-bit blob (w12.h): byte offsets, every item padded
// to pgv_align.  One pass over the lm_head and then each layer's four matrices lays out all three, each in its own order:
//   16-bit: embed, lm_head, final norm, RoPE table, then per layer in_g, post_g and its four matrices
//   fp8:    the lm_head's codes and per-row fp32 scales first; a layer's four code matrices come before its four scale vectors
//   12-bit: one buffer of pgv_w12_total_bytes per matrix
struct LlmDims { long long H, I, Vcap; int L; };       // hidden, intermediate, ALLOCATED rows of embed / lm_head, layers
struct LlmMatSlot {
    long long N, K;                             // rows as ALLOCATED (the lm_head's live row count is the vocabulary, which pgv_llm_resize_vocab changes), columns
    size_t w16, w8, scale, w12;                 // byte offsets: 16-bit matrix, fp8 codes, fp8 scales, 12-bit buffer
};
struct LlmLayout {
    std::vector<LlmMatSlot> mat;                // indexed like pgv_llm::mats
    size_t embed, norm_g, rope;                 // the other items of the 16-bit blob
    std::vector<size_t> in_g, post_g;
    size_t total16 = 0, total8 = 0, total12 = 0;
};
inline size_t llm_take(size_t& total, size_t bytes) { const size_t o = total; total += pgv_align(bytes); return o; }
inline LlmLayout llm_layout(const LlmDims& d) {
    const LlmMatSlot layer[MAT_PER_LAYER] = {{3 * d.H, d.H}, {d.H, d.H}, {2 * d.I, d.H}, {d.H, d.I}};       // q, k, v rows stacked; o; gate / up; down
    LlmLayout lo;
    lo.mat.resize(1 + d.L * MAT_PER_LAYER);
    lo.embed = llm_take(lo.total16, (size_t)d.Vcap * d.H * 2);
    for (int g0 = 0, g1 = 1; g0 < (int)lo.mat.size(); g0 = g1, g1 += MAT_PER_LAYER) {
        if (g0 > 0) { lo.in_g.push_back(llm_take(lo.total16, (size_t)d.H * 4)); lo.post_g.push_back(llm_take(lo.total16, (size_t)d.H * 4)); }
        for (int i = g0; i < g1; ++i) {
            LlmMatSlot& x = lo.mat[i] = g0 == 0 ? LlmMatSlot{d.Vcap, d.H} : layer[i - g0];
            x.w16 = llm_take(lo.total16, (size_t)x.N * x.K * 2);
            x.w8 = llm_take(lo.total8, (size_t)x.N * x.K);
            x.w12 = llm_take(lo.total12, pgv_w12_total_bytes(x.N, x.K));
        }
        for (int i = g0; i < g1; ++i) lo.mat[i].scale = llm_take(lo.total8, (size_t)lo.mat[i].N * 4);
        if (g0 == 0) { lo.norm_g = llm_take(lo.total16, (size_t)d.H * 4); lo.rope = llm_take(lo.total16, (size_t)kMaxPos * 64 * 8); }
    }
    return lo;
}
