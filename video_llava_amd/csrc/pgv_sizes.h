// Byte-size arithmetic that host-only headers (llm_weights.h) share with the HIP translation units: plain C++, no HIP headers.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define PGV_HD __host__ __device__
#else
#define PGV_HD
#endif

inline size_t pgv_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// 12-bit weight stream (w12.h): bytes of the three parts of one matrix's buffer
constexpr int kW12MaxExc = 64;               // exceptions per row block: one entry per lane of a wave
inline PGV_HD size_t pgv_w12_units_bytes(long long N, long long K) { return (size_t)N * (size_t)K / 2 * 3; }
inline PGV_HD size_t pgv_w12_exc_bytes(long long N) { return (size_t)(N / 16) * kW12MaxExc * 4; }
inline PGV_HD size_t pgv_w12_total_bytes(long long N, long long K) { return pgv_w12_units_bytes(N, K) + pgv_w12_exc_bytes(N) + (size_t)N; }
