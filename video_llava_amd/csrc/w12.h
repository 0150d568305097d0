// Lossless 12-bit stream of a bf16 matrix for the decode GEMVs (w12.hip encodes, gemv.hip decodes in registers).
//
// A bf16 weight is a high byte (sign + exponent bits 7..1) and a low byte (exponent bit 0 + 7 mantissa bits).  The low byte is kept as it
// is; the 7 exponent bits of the high byte are coded as a 3-bit offset d = base - e7 below a per-row base, next to the sign: one 4-bit code.
// A weight whose offset does not fit 0..7 is an exception: its code is 0 and its true high byte sits in the row block's exception list,
// patched into the register before the weight reaches the MFMA -- the MFMAs see exactly the 16-bit operands, in the same order.
//
// Matrix W[N, K] (N % 16 == 0, K % 64 == 0), G = K / 64 groups, one buffer of pgv_w12_bytes(N, K) bytes:
//   units   [N / 16][G] x 1536 B   unit (row block, 64-column group) = what one wave consumes per step:
//             [0, 1024)     low bytes, lane ((k % 32) / 8) * 16 + n % 16 holds 16 B: byte ((k / 32) % 2) * 8 + k % 8 (the fp8 copy's layout)
//             [1024, 1536)  codes, lane holds 8 B: byte h * 4 + j = element h * 8 + j (low nibble) and h * 8 + j + 4 (high nibble) of k-block h
//   except  [N / 16][64] u32       per row block, ascending, unused entries 0xffffffff:
//                                  group << 18 | lane << 12 | byte << 8 | high byte  (lane / byte as in the low-byte plane)
//   base    [N] u8                 per-row base: the e7 whose window [base - 7, base] holds the most weights of the row (first such)
// The encoder reports the exception count of every row block; a matrix with more than kW12MaxExc in some row block is not used (the
// 16-bit copy is streamed instead).
#pragma once
#include "pgv_common.h"

constexpr unsigned kW12NoExc = 0xffffffffu;   // kW12MaxExc and the pgv_w12_*_bytes sizes: pgv_sizes.h

#if defined(__HIPCC__)
// High bytes of the 16 weights of a lane in one unit from its two code dwords and the row base replicated in four bytes (b4):
// hi[h * 2 + 0] = elements 0..3 of k-block h, hi[h * 2 + 1] = elements 4..7.  Packed byte arithmetic: base - d never borrows (d <= base).
__device__ __forceinline__ void w12_high_bytes(u32x2_t code, unsigned b4, unsigned (&hi)[4]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const unsigned c = code[h];
        hi[2 * h] = (b4 - (c & 0x07070707u)) | ((c << 4) & 0x80808080u);
        hi[2 * h + 1] = (b4 - ((c >> 4) & 0x07070707u)) | (c & 0x80808080u);
    }
}

// The 8 bf16 weights of k-block h: low byte / high byte interleaved, two weights per v_perm_b32.
template <typename V8>
__device__ __forceinline__ V8 w12_kblock(u32x4_t lo, const unsigned (&hi)[4], int h) {
    u32x4_t r;
    r[0] = __builtin_amdgcn_perm(hi[2 * h], lo[2 * h], 0x05010400u);
    r[1] = __builtin_amdgcn_perm(hi[2 * h], lo[2 * h], 0x07030602u);
    r[2] = __builtin_amdgcn_perm(hi[2 * h + 1], lo[2 * h + 1], 0x05010400u);
    r[3] = __builtin_amdgcn_perm(hi[2 * h + 1], lo[2 * h + 1], 0x07030602u);
    return __builtin_bit_cast(V8, r);
}

// Patch the exceptions of group g into the high bytes (wave-uniform: taken only when an entry of the row block belongs to g).
// ex = this lane's entry of the row block's list, exg = ex >> 18 (kept in a register: one compare per unit).
__device__ __forceinline__ void w12_patch(unsigned ex, unsigned exg, unsigned g, int lane, unsigned (&hi)[4]) {
    unsigned long long m = __builtin_amdgcn_ballot_w64(exg == g);
    while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const unsigned e = __builtin_amdgcn_readlane(ex, j);
        const unsigned byte = (e >> 8) & 15u, sh = (byte & 3u) * 8u;
        const bool mine = lane == (int)((e >> 12) & 63u);
        const unsigned val = (e & 0xffu) << sh;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned msk = (mine && (byte >> 2) == (unsigned)q) ? (0xffu << sh) : 0u;
            hi[q] = (hi[q] & ~msk) | (val & msk);
        }
    }
}
#endif
