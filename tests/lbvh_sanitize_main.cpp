// Drives csrc/host/lbvh_builder.cpp (rtamd::build_lbvh, the host twin of rt_build_bvh) alone under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_lbvh.py): a single triangle, coincident
// centroids, a deep one-sided tree, a random mesh, the refusals, and two of tests/mesh_edge_common.py's
// meshes: chain52 (depth 52) and a mesh with a NaN coordinate, an all-NaN axis and an overflowing c2.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

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

// mesh_edge_common.lattice: (p, p + (0.25, 0, 0), p + (0, 0.25, 0))
void lattice_tri(Mesh& m, float x, float y, float z) {
    const int32_t b = (int32_t)m.verts.size();
    m.verts.push_back(rt_float4{x, y, z, 1.0f});
    m.verts.push_back(rt_float4{x + 0.25f, y, z, 1.0f});
    m.verts.push_back(rt_float4{x, y + 0.25f, z, 1.0f});
    for (int k = 0; k < 3; ++k) m.idx.push_back(b + k);
}

int build(const Mesh& m, int max_leaf, rtamd::Bvh& out, std::string& err) {
    return rtamd::build_lbvh(m.verts.data(), (int32_t)m.verts.size(), m.idx.data(), (int32_t)m.idx.size(), max_leaf, out, err);
}

// structure: 2K + 1 nodes, kept nodes first; leaves of 1..max_leaf tiling [0, n); every triangle
// once; every box the min / max of what lies below it; depth <= 64
// (the union is checked on min.x and max.z: a mesh with NaNs keeps them off those two)
int check(const Mesh& m, int max_leaf, const char* what, int flags = 0) {
    rtamd::Bvh b;
    std::string err;
    EXPECT(build(m, max_leaf | flags, b, err) == RT_OK);
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
        EXPECT(nd.min.w == 1.0f && nd.max.w == 1.0f);
        if (i < K) {
            EXPECT(nd.offset_left > 0 && nd.offset_left < nn && nd.offset_right > 0 && nd.offset_right < nn);
            EXPECT(nd.offset_tris == -1 && nd.num_tris == 0);
            if (nd.offset_left > 0 && nd.offset_left < nn && nd.offset_right > 0 && nd.offset_right < nn) {
                const rt_bvh_node &L = b.nodes[nd.offset_left], &R = b.nodes[nd.offset_right];
                EXPECT(nd.min.x == std::fmin(L.min.x, R.min.x) && nd.max.z == std::fmax(L.max.z, R.max.z));
            }
        } else {
            EXPECT(nd.offset_left == -1 && nd.offset_right == -1);
            EXPECT(nd.offset_tris == next && nd.num_tris >= 1 && nd.num_tris <= max_leaf);
            next += nd.num_tris;
        }
    }
    EXPECT(next == n);
    EXPECT(b.max_depth <= 64 && b.num_leaves == K + 1);
    std::printf("%s (max_leaf %d): ok, %d nodes, depth %d\n", what, max_leaf, nn, b.max_depth);
    return b.max_depth;
}

}  // namespace

int main() {
    {   // n = 1: a root leaf
        Mesh m;
        tri(m, 1.0f, 2.0f, 3.0f, 0.5f);
        check(m, 1, "single");
        check(m, 8, "single");
    }
    {   // 70 copies of one triangle: no axis has extent
        Mesh m;
        tri(m, 1.0f, 2.0f, 3.0f, 0.5f);
        for (int c = 1; c < 70; ++c)
            for (int k = 0; k < 3; ++k) m.idx.push_back(k);
        for (int ml : {1, 4, 8}) check(m, ml, "coincident");
    }
    {   // centroids at 100 * 2^-k: a one-sided tree
        Mesh m;
        for (int k = 0; k < 40; ++k) {
            const float c = std::ldexp(100.0f, -k);
            tri(m, c, c, c, std::ldexp(1.0f, -k - 4));
        }
        for (int ml : {1, 4}) check(m, ml, "deep");
    }
    {   // a pseudo-random mesh, and non-finite vertices (defined cells, no trap)
        Mesh m;
        uint32_t s = 12345u;
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f * 200.0f - 100.0f; };
        for (int t = 0; t < 3000; ++t) tri(m, rnd(), rnd(), rnd(), 1.5f);
        for (int ml : {1, 3, 8}) check(m, ml, "random");
        m.verts[10].x = INFINITY;
        m.verts[50].y = NAN;
        m.verts[90].z = -3.0e38f;
        m.verts[91].z = 3.0e38f;
        rtamd::Bvh b;
        std::string err;
        EXPECT(build(m, 4, b, err) == RT_OK && b.nodes.size() % 2 == 1);
        std::printf("non-finite: ok\n");
    }
    {   // chain52: triangles 0, 1, 2, 4, ..., 4096 at the origin, the next 39 free indices at the
        // single-bit cells, the rest at the far corner: a Morton chain of 39 levels into an index-bit chain of 13
        Mesh m;
        const int n = (1 << 12) + 40;
        int j = 0;
        for (int t = 0; t < n; ++t) {
            float p[3] = {8192.0f, 8192.0f, 8192.0f};
            if ((t & (t - 1)) == 0) {
                p[0] = p[1] = p[2] = 0.0f;
            } else if (j < 39) {
                p[0] = p[1] = p[2] = 0.0f;
                p[j % 3] = (float)(1 << (12 - j / 3));
                ++j;
            }
            lattice_tri(m, p[0], p[1], p[2]);
        }
        EXPECT(check(m, 1, "chain52") == 52);
        check(m, 4, "chain52");
        EXPECT(check(m, 1, "chain52 extent keys", RT_BUILD_EXTENT_KEYS) == 52);
    }
    {   // non-finite coordinates on y: one NaN; finite +-3e38 whose lo + hi overflows; the whole axis NaN
        Mesh m;
        uint32_t s = 777u;
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f * 200.0f - 100.0f; };
        for (int t = 0; t < 512; ++t) tri(m, rnd(), rnd(), rnd(), 1.5f);
        Mesh a = m;
        a.verts[22].y = NAN;
        for (int ml : {1, 4}) { check(a, ml, "nan coordinate"); check(a, ml, "nan coordinate extent keys", RT_BUILD_EXTENT_KEYS); }
        Mesh e = m;
        for (int k = 0; k < 3; ++k) { e.verts[60 + k].y = 3.0e38f; e.verts[63 + k].y = -3.0e38f; }
        e.verts[66].y = 3.0e38f;
        e.verts[67].y = -3.0e38f;
        for (int ml : {1, 4}) { check(e, ml, "overflowing c2"); check(e, ml, "overflowing c2 extent keys", RT_BUILD_EXTENT_KEYS); }
        Mesh c = m;
        for (rt_float4& v : c.verts) v.y = NAN;
        for (int ml : {1, 4}) { check(c, ml, "nan axis"); check(c, ml, "nan axis extent keys", RT_BUILD_EXTENT_KEYS); }
    }
    {   // refusals
        Mesh m;
        tri(m, 0, 0, 0, 1);
        tri(m, 5, 0, 0, 1);
        rtamd::Bvh b;
        std::string err;
        EXPECT(build(m, 0, b, err) == RT_ERR_INVALID_ARG && !err.empty());
        EXPECT(build(m, 9, b, err) == RT_ERR_INVALID_ARG);
        EXPECT(rtamd::build_lbvh(m.verts.data(), 6, m.idx.data(), 4, 4, b, err) == RT_ERR_INVALID_ARG);
        EXPECT(rtamd::build_lbvh(m.verts.data(), 6, m.idx.data(), 0, 4, b, err) == RT_ERR_INVALID_ARG);
        EXPECT(rtamd::build_lbvh(nullptr, 6, m.idx.data(), 6, 4, b, err) == RT_ERR_INVALID_ARG);
        EXPECT(rtamd::build_lbvh(m.verts.data(), 6, nullptr, 6, 4, b, err) == RT_ERR_INVALID_ARG);
        m.idx[4] = 6;   // == nv
        EXPECT(build(m, 4, b, err) == RT_ERR_BAD_SCENE);
        m.idx[4] = -1;
        EXPECT(build(m, 4, b, err) == RT_ERR_BAD_SCENE);
        std::printf("refusals: ok\n");
    }
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
