// Drives csrc/host/closest_points.cpp (rt_closest_points_host) with scene_encode.cpp under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_closest.py): the edge set of the rule
// (non-finite coordinates; r NaN, 0, -0, -1, subnormal, 1e-30, 1e30, +inf; a degenerate triangle;
// coordinates at 2^64) into buffers of exactly n records, a root leaf, an empty leaf, a malformed
// node, a 70-level comb whose every query overflows the 65-entry stack and the same comb at 40
// levels, and hostile sizes, which must be refused before a byte is read or written.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_abi.h"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

const float kInf = std::numeric_limits<float>::infinity();
const float kNan = std::numeric_limits<float>::quiet_NaN();
const float kSub = std::numeric_limits<float>::denorm_min();

struct Scene {
    std::vector<rt_float4> verts;
    std::vector<int32_t> idx;
    std::vector<rt_bvh_node> nodes;
    std::vector<int32_t> refs;
};

rt_bvh_node node(const float lo[3], const float hi[3], int32_t l, int32_t r, int32_t off, int32_t cnt) {
    rt_bvh_node n{};
    n.min = rt_float4{lo[0], lo[1], lo[2], 1.0f};
    n.max = rt_float4{hi[0], hi[1], hi[2], 1.0f};
    n.offset_left = l; n.offset_right = r; n.offset_tris = off; n.num_tris = cnt;
    return n;
}

void add_tri(Scene& s, float x, float y, float z, float size) {
    const int32_t b = (int32_t)s.verts.size();
    s.verts.push_back(rt_float4{x, y, z, 1.0f});
    s.verts.push_back(rt_float4{x + size, y, z, 1.0f});
    s.verts.push_back(rt_float4{x, y + size, z + 0.25f * size, 1.0f});
    for (int k = 0; k < 3; ++k) s.idx.push_back(b + k);
}

// a comb `depth` levels deep over as many triangles: inner k -> {inner k + 1, leaf k}, every box the whole scene
Scene comb(int depth) {
    Scene s;
    for (int k = 0; k < depth; ++k) add_tri(s, (float)(k % 7), (float)(k % 5), (float)k * 0.5f, 1.0f);
    const float lo[3] = {-1, -1, -1}, hi[3] = {9, 7, 0.5f * depth + 1};
    for (int k = 0; k < depth; ++k) {
        const int32_t next = k + 1 < depth ? 2 * (k + 1) : 2 * k + 1;
        s.nodes.push_back(node(lo, hi, next, 2 * k + 1, -1, 0));
        s.nodes.push_back(node(lo, hi, -1, -1, k, 1));
        s.refs.push_back(3 * k);
    }
    return s;
}

int query(const Scene& s, const std::vector<rt_point>& pts, std::vector<rt_closest>& out, uint64_t* st) {
    out.assign(pts.size(), rt_closest{});   // exactly n: one record more is out of bounds
    return rt_closest_points_host(s.verts.data(), (int32_t)s.verts.size(), s.idx.data(), (int32_t)s.idx.size(), s.nodes.data(),
                                  (int32_t)s.nodes.size(), s.refs.empty() ? nullptr : s.refs.data(), (int32_t)s.refs.size(),
                                  pts.data(), (int64_t)pts.size(), out.data(), st);
}

bool is_miss(const rt_closest& c) {
    uint32_t w[8];
    std::memcpy(w, &c, 32);
    return w[0] == 0xFFFFFFFFu && w[1] == 0x7F800000u && !(w[2] | w[3] | w[4] | w[5] | w[6] | w[7]);
}

}  // namespace

int main() {
    uint64_t st[3];
    std::vector<rt_closest> out;
    {   // two leaves, one of them empty, plus the edge set
        Scene s;
        add_tri(s, 0, 0, 0, 2.0f);
        add_tri(s, 5, 5, 5, 0.0f);   // three equal vertices
        s.verts.push_back(rt_float4{8, 0, 0, 1}); s.verts.push_back(rt_float4{9, 0, 0, 1}); s.verts.push_back(rt_float4{10, 0, 0, 1});
        for (int k = 6; k < 9; ++k) s.idx.push_back(k);   // collinear vertices
        const float lo[3] = {0, 0, 0}, hi[3] = {10, 5, 5};
        s.nodes = {node(lo, hi, 1, 2, -1, 0), node(lo, hi, -1, -1, 0, 3), node(lo, hi, -1, -1, 0, 0)};
        s.refs = {0, 3, 6};
        std::vector<rt_point> pts;
        for (float bad : {kNan, kInf, -kInf}) {
            pts.push_back(rt_point{bad, 0, 0, kInf});
            pts.push_back(rt_point{0, bad, 0, kInf});
            pts.push_back(rt_point{0, 0, bad, kInf});
        }
        for (float r : {kNan, 0.0f, -0.0f, -1.0f, kSub, 1e-30f}) pts.push_back(rt_point{0.5f, 0.5f, 3.0f, r});
        const size_t n_miss = pts.size();
        for (float r : {1e30f, kInf, 100.0f}) pts.push_back(rt_point{0.5f, 0.5f, 3.0f, r});
        pts.push_back(rt_point{5, 5, 5.5f, kInf});       // nearest the point triangle
        pts.push_back(rt_point{9.5f, 0.5f, 0, kInf});    // nearest the collinear one
        EXPECT(query(s, pts, out, st) == RT_OK);
        for (size_t i = 0; i < n_miss; ++i) EXPECT(is_miss(out[i]));
        for (size_t i = n_miss; i < pts.size(); ++i) EXPECT(out[i].id >= 0 && out[i].d2 == out[i].d2 && out[i].reserved == 0u);
        EXPECT(st[0] == 0 && st[2] == 3 * (pts.size() - n_miss + 2));   // r subnormal and 1e-30 are valid: best = 0, the box at distance 0 is visited
        const float big = 0x1p64f;   // (at 2^60 the squares still fit: 3 * 2^120)
        std::vector<rt_point> far = {rt_point{big, big, big, kInf}, rt_point{-big, 0, 0, kInf}};
        EXPECT(query(s, far, out, st) == RT_OK);
        EXPECT(is_miss(out[0]) && is_miss(out[1]));      // d2 overflows to +inf: never below best
        std::printf("edge set: ok\n");
    }
    {   // a root leaf, and exact sizes around the wave's group
        Scene s;
        add_tri(s, 0, 0, 0, 1.0f);
        const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 0.25f};
        s.nodes = {node(lo, hi, -1, -1, 0, 1)};
        s.refs = {0};
        for (int n : {0, 1, 63, 64, 65, 129}) {
            std::vector<rt_point> pts;
            for (int i = 0; i < n; ++i) pts.push_back(rt_point{std::sin((float)i), std::cos((float)i), 0.1f * i, kInf});
            EXPECT(query(s, pts, out, st) == RT_OK);
            for (int i = 0; i < n; ++i) EXPECT(out[(size_t)i].id == 0);
            EXPECT(st[1] == 0 && st[2] == (uint64_t)n);
        }
        std::printf("root leaf: ok\n");
    }
    {   // a malformed inner node: the right child of the root points outside the array
        Scene s;
        add_tri(s, 0, 0, 0, 1.0f);
        const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
        s.nodes = {node(lo, hi, 1, 2, -1, 0), node(lo, hi, -1, -1, 0, 1), node(lo, hi, 7, 9, -1, 0)};
        s.refs = {0};
        std::vector<rt_point> pts = {rt_point{0.2f, 0.2f, 0.2f, kInf}};
        EXPECT(query(s, pts, out, st) == RT_OK);
        EXPECT(is_miss(out[0]) && st[0] == 0);
        std::printf("malformed node: ok\n");
    }
    {   // the combs
        std::vector<rt_point> pts;
        for (int i = 0; i < 200; ++i) pts.push_back(rt_point{0.37f * (i % 19), 0.21f * (i % 23), 0.3f * (i % 31), kInf});
        const Scene deep = comb(70);
        EXPECT(query(deep, pts, out, st) == RT_OK);
        EXPECT(st[0] == pts.size());
        for (const rt_closest& c : out) EXPECT(is_miss(c));
        const Scene mid = comb(40);
        EXPECT(query(mid, pts, out, st) == RT_OK);
        EXPECT(st[0] == 0 && st[2] == 41 * pts.size());   // the last inner node holds its leaf twice
        for (const rt_closest& c : out) EXPECT(c.id >= 0 && c.id < 120);
        std::printf("combs: ok\n");
    }
    {   // hostile sizes and bad scenes: refused with one-record buffers untouched
        Scene s;
        add_tri(s, 0, 0, 0, 1.0f);
        const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
        s.nodes = {node(lo, hi, -1, -1, 0, 1)};
        s.refs = {0};
        std::vector<rt_point> p1 = {rt_point{0, 0, 0, 1}};
        std::vector<rt_closest> o1(1);
        std::memset(o1.data(), 0x5A, sizeof(rt_closest));
        auto call = [&](const rt_float4* v, int32_t nv, const int32_t* ix, int32_t nidx, const rt_bvh_node* nd, int32_t nn,
                        const int32_t* rf, int32_t nref, const rt_point* p, int64_t n, rt_closest* o) {
            return rt_closest_points_host(v, nv, ix, nidx, nd, nn, rf, nref, p, n, o, nullptr);
        };
        const int64_t bad_n[] = {-1, (1ll << 30) + 1, 1ll << 40, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()};
        for (int64_t n : bad_n)
            EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), n, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(nullptr, 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, nullptr, 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, nullptr, 1, s.refs.data(), 1, p1.data(), 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, nullptr, 1, p1.data(), 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, nullptr, 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, nullptr) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 2, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 0, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 2, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, o1.data()) == RT_ERR_BAD_SCENE);
        const int32_t bad_ref[1] = {3};
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, bad_ref, 1, p1.data(), 1, o1.data()) == RT_ERR_BAD_SCENE);
        for (size_t b = 0; b < sizeof(rt_closest); ++b) EXPECT(((const unsigned char*)o1.data())[b] == 0x5A);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, nullptr, 0, nullptr) == RT_OK);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, o1.data()) == RT_OK);
        EXPECT(o1[0].id == 0 && o1[0].d2 == 0.0f && o1[0].reserved == 0u);
        std::printf("arguments: ok\n");
    }
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
