// lbvh_core.hpp -- the arithmetic of the LBVH build that the host twin
// (lbvh_builder.cpp) and the HIP kernels (rt_lbvh.hip) share: cells, Morton keys and the binary
// radix tree node of Karras 2012.  Plain inline functions, no HIP types; the kernels compile them
// for the device through LBVH_HD.  Float arithmetic here is single IEEE operations (both sides are
// built with -ffp-contract=off, the device with correctly rounded division).
#pragma once
#include <cstdint>

#ifndef LBVH_HD
#if defined(__HIPCC__)
#define LBVH_HD __host__ __device__ inline
#else
#define LBVH_HD inline
#endif
#endif

namespace lbvh {

constexpr int kCellBits = 13;                      // per axis: a 39-bit Morton code
constexpr int kIndexBits = 25;                     // the triangle index below it: n <= 2^25
constexpr int32_t kMaxTris = 1 << kIndexBits;
constexpr uint64_t kIndexMask = (1ull << kIndexBits) - 1;

// cell = min(8191, (int)((c2 - cmin) * (8192 / (cmax - cmin)))), 0 on an axis without extent.
// The comparisons also give a NaN (non-finite vertices) a defined cell.
LBVH_HD uint32_t cell(float c2, float cmin, float cmax) {
    if (cmax == cmin) return 0u;
    const float scale = 8192.0f / (cmax - cmin);
    const float f = (c2 - cmin) * scale;
    if (f >= 8191.0f) return 8191u;
    return f > 0.0f ? (uint32_t)(int32_t)f : 0u;
}

// the 13 bits of v, bit i at position 3 * i
LBVH_HD uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1FFFu;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// key = morton39(x, y, z) << 25 | t, x in the most significant place of every bit triple
LBVH_HD uint64_t key(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t t) {
    const uint64_t m = (spread3(cx) << 2) | (spread3(cy) << 1) | spread3(cz);
    return (m << kIndexBits) | (uint64_t)t;
}

// length of the common prefix of the keys at i and j; -1 for j outside [0, n).  Keys are unique.
LBVH_HD int delta(const uint64_t* k, int32_t n, int32_t i, int32_t j) {
    if (j < 0 || j >= n) return -1;
    return __builtin_clzll(k[i] ^ k[j]);
}

// Radix node i (0 <= i < n - 1) over the sorted keys: it covers positions [a, b] and splits after
// s: children [a, s] and [s + 1, b]; an inner left child is node s, an inner right child s + 1.
LBVH_HD void node(const uint64_t* k, int32_t n, int32_t i, int32_t& a, int32_t& b, int32_t& s) {
    const int d = delta(k, n, i, i + 1) > delta(k, n, i, i - 1) ? 1 : -1;
    const int dmin = delta(k, n, i, i - d);
    int32_t lmax = 2;
    while (delta(k, n, i, i + lmax * d) > dmin) lmax *= 2;
    int32_t l = 0;
    for (int32_t t = lmax / 2; t >= 1; t /= 2)
        if (delta(k, n, i, i + (l + t) * d) > dmin) l += t;
    const int32_t j = i + l * d;
    const int dnode = delta(k, n, i, j);
    int32_t q = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(k, n, i, i + (q + t) * d) > dnode) q += t;
    } while (t > 1);
    s = i + q * d + (d < 0 ? -1 : 0);
    a = d > 0 ? i : j;
    b = d > 0 ? j : i;
}

}  // namespace lbvh
