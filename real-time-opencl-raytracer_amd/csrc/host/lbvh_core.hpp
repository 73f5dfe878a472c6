// lbvh_core.hpp -- the arithmetic of the LBVH build that the host twin
// (lbvh_builder.cpp) and the HIP kernels (rt_lbvh.hip) share: the key plan, cells, Morton keys and
// the binary radix tree node of Karras 2012.  Plain inline functions, no HIP types; the kernels
// compile them for the device through LBVH_HD.  Float arithmetic here is single IEEE operations
// (both sides are built with -ffp-contract=off, the device with correctly rounded division).
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

constexpr int kCellBits = 13;                      // per axis with the per-axis keys
constexpr int kMortonBits = 3 * kCellBits;         // a 39-bit Morton code
constexpr int kAxisBitsMax = 20;                   // most bits one axis takes with the extent-aware keys
constexpr int kIndexBits = 25;                     // the triangle index below it: n <= 2^25
constexpr int32_t kMaxTris = 1 << kIndexBits;
constexpr uint64_t kIndexMask = (1ull << kIndexBits) - 1;
constexpr int32_t kExtentKeys = 0x100;             // RT_BUILD_EXTENT_KEYS, ORed into max_leaf

// The builders' max_leaf argument: 1 .. 8 in the low byte, kExtentKeys above it, nothing else.
inline bool split_max_leaf(int32_t arg, int32_t& max_leaf, bool& extent_keys) {
    max_leaf = arg & 0xFF;
    extent_keys = (arg & kExtentKeys) != 0;
    return (arg & ~(0xFF | kExtentKeys)) == 0 && max_leaf >= 1 && max_leaf <= 8;
}

// Which axis gives Morton bit 38 - k, and how many bits each axis gives in all.  A plain struct:
// the host computes it once per build and key_kernel takes it as a kernel argument.
struct KeyPlan {
    uint8_t axis[kMortonBits];
    uint8_t bits[3];
};

// The per-axis keys: x, y, z in turn, 13 bits each.
inline KeyPlan axis_plan() {
    KeyPlan p{};
    for (int k = 0; k < kMortonBits; ++k) p.axis[k] = (uint8_t)(k % 3);
    p.bits[0] = p.bits[1] = p.bits[2] = (uint8_t)kCellBits;
    return p;
}

// The extent-aware keys: every bit halves the axis whose cells are the widest, so
// cells come out as near cubes as 39 bits allow.  w = extent, 0 where it is not a positive finite
// number; a tie goes to the lowest axis; no axis takes more than 20 bits (3 * 20 >= 39: every bit
// is placed).  Three equal extents give axis_plan().  Host only: the halving may run into
// subnormals, which a device may flush.
inline KeyPlan extent_plan(const float cmin[3], const float cmax[3]) {
    float w[3];
    for (int a = 0; a < 3; ++a) {
        w[a] = cmax[a] - cmin[a];
        if (!(w[a] > 0.0f) || !(w[a] <= 3.402823466e+38f)) w[a] = 0.0f;
    }
    KeyPlan p{};
    for (int k = 0; k < kMortonBits; ++k) {
        int best = -1;
        for (int a = 0; a < 3; ++a)
            if (p.bits[a] < kAxisBitsMax && (best < 0 || w[a] > w[best])) best = a;
        p.axis[k] = (uint8_t)best;
        ++p.bits[best];
        w[best] *= 0.5f;
    }
    return p;
}

// cell = min(2^bits - 1, (int)((c2 - cmin) * (2^bits / (cmax - cmin)))), 0 on an axis without
// extent or without bits.  The comparisons also give a NaN (non-finite vertices) a defined cell.
LBVH_HD uint32_t cell(float c2, float cmin, float cmax, int bits) {
    if (cmax == cmin || bits == 0) return 0u;
    const float scale = (float)(1 << bits) / (cmax - cmin);
    const float f = (c2 - cmin) * scale;
    const uint32_t top = (1u << bits) - 1u;
    if (f >= (float)top) return top;
    return f > 0.0f ? (uint32_t)(int32_t)f : 0u;
}

// key = morton39 << 25 | t: Morton bit 38 - k is the next most significant unused bit of the
// cell of axis plan.axis[k]
LBVH_HD uint64_t key(const KeyPlan& plan, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t t) {
    int lx = plan.bits[0], ly = plan.bits[1], lz = plan.bits[2];
    uint64_t m = 0;
    for (int k = 0; k < kMortonBits; ++k) {
        const int a = plan.axis[k];
        const uint32_t bit = a == 0 ? cx >> --lx : a == 1 ? cy >> --ly : cz >> --lz;
        m = (m << 1) | (bit & 1u);
    }
    return (m << kIndexBits) | (uint64_t)t;
}

// the whole step: c2 of triangle t -> its key
LBVH_HD uint64_t key_of(const KeyPlan& plan, const float c[3], const float cmin[3], const float cmax[3], uint32_t t) {
    return key(plan, cell(c[0], cmin[0], cmax[0], plan.bits[0]), cell(c[1], cmin[1], cmax[1], plan.bits[1]),
               cell(c[2], cmin[2], cmax[2], plan.bits[2]), t);
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
