// Drives csrc/host/lbvh_builder.cpp with RT_BUILD_EXTENT_KEYS alone under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_lbvh_keys.py): the meshes on which the
// key plan degenerates -- a single triangle, no extent at all, one axis without extent, an axis
// 2^22 times the others (the 20-bit cap), non-finite vertices -- and the refused values.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "lbvh_core.hpp"
#include "rt_abi.h"
#include "scene.hpp"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

struct Mesh {
    std::vector<rt_float4> verts;
    std::vector<int32_t> idx;
};

void tri(Mesh& m, float cx, float cy, float cz, float r) {
    const int32_t b = (int32_t)m.verts.size();
    m.verts.push_back(rt_float4{cx - r, cy, cz + r, 1.0f});
    m.verts.push_back(rt_float4{cx + r, cy - r, cz, 1.0f});
    m.verts.push_back(rt_float4{cx, cy + r, cz - r, 1.0f});
    for (int k = 0; k < 3; ++k) m.idx.push_back(b + k);
}

int build(const Mesh& m, int max_leaf, rtamd::Bvh& out, std::string& err) {
    return rtamd::build_lbvh(m.verts.data(), (int32_t)m.verts.size(), m.idx.data(), (int32_t)m.idx.size(), max_leaf, out, err);
}

// structure: 2K + 1 nodes, kept nodes first; leaves of 1..max_leaf tiling [0, n); every triangle once; depth <= 64
void check(const Mesh& m, int max_leaf, const char* what) {
    rtamd::Bvh b;
    std::string err;
    EXPECT(build(m, max_leaf | RT_BUILD_EXTENT_KEYS, b, err) == RT_OK);
    const int32_t n = (int32_t)m.idx.size() / 3, nn = (int32_t)b.nodes.size();
    EXPECT(nn % 2 == 1 && (int32_t)b.tri_indices.size() == n);
    const int32_t K = nn / 2;
    std::vector<int> seen((size_t)n, 0);
    for (int32_t r : b.tri_indices) {
        EXPECT(r >= 0 && r % 3 == 0 && r / 3 < n);
        if (r >= 0 && r / 3 < n) ++seen[r / 3];
    }
    for (int s : seen) EXPECT(s == 1);
    int32_t next = 0;
    for (int32_t i = 0; i < nn; ++i) {
        const rt_bvh_node& nd = b.nodes[i];
        if (i < K) {
            EXPECT(nd.offset_left > 0 && nd.offset_left < nn && nd.offset_right > 0 && nd.offset_right < nn);
        } else {
            EXPECT(nd.offset_left == -1 && nd.offset_right == -1);
            EXPECT(nd.offset_tris == next && nd.num_tris >= 1 && nd.num_tris <= max_leaf);
            next += nd.num_tris;
        }
    }
    EXPECT(next == n);
    EXPECT(b.max_depth <= 64 && b.num_leaves == K + 1);
    std::printf("%s (max_leaf %d): ok, %d nodes, depth %d\n", what, max_leaf, nn, b.max_depth);
}

bool plan_bits(const float lo[3], const float hi[3], int bx, int by, int bz) {
    const lbvh::KeyPlan p = lbvh::extent_plan(lo, hi);
    int count[3] = {0, 0, 0};
    for (int k = 0; k < lbvh::kMortonBits; ++k) {
        if (p.axis[k] > 2) return false;
        ++count[p.axis[k]];
    }
    return p.bits[0] == bx && p.bits[1] == by && p.bits[2] == bz && count[0] == bx && count[1] == by && count[2] == bz;
}

}  // namespace

int main() {
    {   // the plan itself: equal extents, none, one missing, the cap, not finite, subnormal
        const float o[3] = {0, 0, 0};
        const float cube[3] = {3, 3, 3}, flat[3] = {5, 0, 5}, thin[3] = {4194304.0f, 1, 1};
        const float inf[3] = {INFINITY, 2, 1}, nan[3] = {NAN, NAN, NAN}, tiny[3] = {1e-44f, 3e-45f, 1e-45f};
        EXPECT(plan_bits(o, cube, 13, 13, 13));
        EXPECT(plan_bits(o, o, 20, 19, 0));
        EXPECT(plan_bits(o, flat, 20, 0, 19));
        EXPECT(plan_bits(o, thin, 20, 10, 9));
        EXPECT(plan_bits(o, inf, 0, 20, 19));    // an infinite extent counts as none
        EXPECT(plan_bits(o, nan, 20, 19, 0));
        EXPECT(plan_bits(cube, o, 20, 19, 0));   // cmax < cmin
        const lbvh::KeyPlan t = lbvh::extent_plan(o, tiny);
        EXPECT(t.bits[0] + t.bits[1] + t.bits[2] == lbvh::kMortonBits && t.bits[0] <= 20);
        const lbvh::KeyPlan a = lbvh::extent_plan(o, cube), b = lbvh::axis_plan();
        for (int k = 0; k < lbvh::kMortonBits; ++k) EXPECT(a.axis[k] == b.axis[k]);
        std::printf("plans: ok\n");
    }
    {   // n = 1: a root leaf
        Mesh m;
        tri(m, 1.0f, 2.0f, 3.0f, 0.5f);
        check(m, 1, "single");
        check(m, 8, "single");
    }
    {   // 70 copies of one triangle: no axis has extent, the cap alone decides the plan
        Mesh m;
        tri(m, 1.0f, 2.0f, 3.0f, 0.5f);
        for (int c = 1; c < 70; ++c)
            for (int k = 0; k < 3; ++k) m.idx.push_back(k);
        for (int ml : {1, 4, 8}) check(m, ml, "coincident");
    }
    {   // a flat grid: y gets no bit
        Mesh m;
        for (int x = 0; x < 16; ++x)
            for (int z = 0; z < 16; ++z) {
                const int32_t b = (int32_t)m.verts.size();
                m.verts.push_back(rt_float4{2.5f * x, 0.0f, 2.5f * z, 1.0f});
                m.verts.push_back(rt_float4{2.5f * x + 2.5f, 0.0f, 2.5f * z, 1.0f});
                m.verts.push_back(rt_float4{2.5f * x, 0.0f, 2.5f * z + 2.5f, 1.0f});
                for (int k = 0; k < 3; ++k) m.idx.push_back(b + k);
            }
        for (int ml : {1, 4}) check(m, ml, "flat");
    }
    {   // x extent 2^22 times the others: the 20-bit cap binds
        Mesh m;
        uint32_t s = 777u;
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
        tri(m, 0.0f, 0.0f, 0.0f, 0.0625f);
        tri(m, 4194304.0f, 1.0f, 1.0f, 0.0625f);
        for (int t = 0; t < 400; ++t) tri(m, rnd() * 4194304.0f, rnd(), rnd(), 0.0625f);
        for (int ml : {1, 4}) check(m, ml, "needle");
    }
    {   // a pseudo-random mesh, then non-finite vertices (defined plan and cells, no trap)
        Mesh m;
        uint32_t s = 12345u;
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f * 200.0f - 100.0f; };
        for (int t = 0; t < 3000; ++t) tri(m, rnd(), 0.1f * rnd(), rnd(), 1.5f);
        for (int ml : {1, 3, 8}) check(m, ml, "random");
        m.verts[10].x = INFINITY;
        check(m, 4, "one infinite vertex");
        m.verts[50].y = NAN;
        m.verts[90].z = -3.0e38f;
        m.verts[91].z = 3.0e38f;
        rtamd::Bvh b;
        std::string err;
        EXPECT(build(m, 4 | RT_BUILD_EXTENT_KEYS, b, err) == RT_OK && b.nodes.size() % 2 == 1);
        std::printf("non-finite: ok\n");
    }
    {   // refusals
        Mesh m;
        tri(m, 0, 0, 0, 1);
        tri(m, 5, 0, 0, 1);
        rtamd::Bvh b;
        std::string err;
        EXPECT(build(m, RT_BUILD_EXTENT_KEYS | 0, b, err) == RT_ERR_INVALID_ARG && !err.empty());
        EXPECT(build(m, RT_BUILD_EXTENT_KEYS | 9, b, err) == RT_ERR_INVALID_ARG);
        EXPECT(build(m, 0x200 | 4, b, err) == RT_ERR_INVALID_ARG);
        EXPECT(build(m, -1, b, err) == RT_ERR_INVALID_ARG);
        EXPECT(build(m, RT_BUILD_EXTENT_KEYS | 4, b, err) == RT_OK && b.nodes.size() == 1);
        std::printf("refusals: ok\n");
    }
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
