// Drives csrc/host/closest_points.cpp (rt_nearest_k_host) with scene_encode.cpp under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_nearest_k.py): for every k in 1 .. 8, into
// buffers of exactly k * n records, the edge set of the rule (non-finite coordinates; r NaN, 0, -0, -1,
// subnormal, 1e-30, 1e30, +inf; degenerate triangles; coordinates at 2^64), a duplicate set (a tree
// that references every triangle from two leaves), a root leaf at the sizes around a wave's group, a
// malformed node, a 70-level comb whose every query overflows and the same comb at 40 levels, and
// hostile sizes, which must be refused before a byte is read or written.
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

int query(const Scene& s, const std::vector<rt_point>& pts, int k, std::vector<rt_closest>& out, uint64_t* st) {
    out.assign(pts.size() * (size_t)k, rt_closest{});   // exactly k * n: one record more is out of bounds
    return rt_nearest_k_host(s.verts.data(), (int32_t)s.verts.size(), s.idx.data(), (int32_t)s.idx.size(), s.nodes.data(),
                             (int32_t)s.nodes.size(), s.refs.empty() ? nullptr : s.refs.data(), (int32_t)s.refs.size(),
                             pts.data(), (int64_t)pts.size(), k, out.data(), st);
}

bool is_miss(const rt_closest& c) {
    uint32_t w[8];
    std::memcpy(w, &c, 32);
    return w[0] == 0xFFFFFFFFu && w[1] == 0x7F800000u && !(w[2] | w[3] | w[4] | w[5] | w[6] | w[7]);
}

// plane j of point i
const rt_closest& at(const std::vector<rt_closest>& out, size_t n, int j, size_t i) { return out[(size_t)j * n + i]; }

// a row is sorted by (d2, id), holds no id twice, and its misses come last
bool row_ok(const std::vector<rt_closest>& out, size_t n, int k, size_t i) {
    for (int j = 0; j + 1 < k; ++j) {
        const rt_closest &a = at(out, n, j, i), &b = at(out, n, j + 1, i);
        if (is_miss(a) && !is_miss(b)) return false;
        if (!is_miss(b) && !(a.d2 < b.d2 || (a.d2 == b.d2 && a.id < b.id))) return false;
    }
    return true;
}

}  // namespace

int main() {
    uint64_t st[3];
    std::vector<rt_closest> out;
    for (int k = 1; k <= RT_NEAREST_MAX_K; ++k) {
        {   // two leaves, one of them empty, plus the edge set
            Scene s;
            add_tri(s, 0, 0, 0, 2.0f);
            add_tri(s, 5, 5, 5, 0.0f);   // three equal vertices
            s.verts.push_back(rt_float4{8, 0, 0, 1}); s.verts.push_back(rt_float4{9, 0, 0, 1}); s.verts.push_back(rt_float4{10, 0, 0, 1});
            for (int v = 6; v < 9; ++v) s.idx.push_back(v);   // collinear vertices
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
            pts.push_back(rt_point{5, 5, 5.5f, kInf});
            pts.push_back(rt_point{9.5f, 0.5f, 0, kInf});
            const size_t n = pts.size();
            EXPECT(query(s, pts, k, out, st) == RT_OK);
            for (size_t i = 0; i < n_miss; ++i)
                for (int j = 0; j < k; ++j) EXPECT(is_miss(at(out, n, j, i)));   // a miss is k miss records
            for (size_t i = n_miss; i < n; ++i) {
                EXPECT(row_ok(out, n, k, i));
                EXPECT(!is_miss(at(out, n, 0, i)));
                for (int j = 3; j < k; ++j) EXPECT(is_miss(at(out, n, j, i)));   // the scene has three triangles
            }
            EXPECT(st[0] == 0);
            const float big = 0x1p64f;
            std::vector<rt_point> far = {rt_point{big, big, big, kInf}, rt_point{-big, 0, 0, kInf}};
            EXPECT(query(s, far, k, out, st) == RT_OK);
            for (const rt_closest& c : out) EXPECT(is_miss(c));   // d2 overflows to +inf: never below the bound
        }
        {   // the duplicate set: 12 triangles, each referenced from both leaves
            Scene s;
            for (int t = 0; t < 12; ++t) add_tri(s, (float)(t % 4), (float)(t / 4), 0.1f * t, 1.0f);
            const float lo[3] = {0, 0, 0}, hi[3] = {5, 4, 2};
            s.nodes = {node(lo, hi, 1, 2, -1, 0), node(lo, hi, -1, -1, 0, 12), node(lo, hi, -1, -1, 12, 12)};
            for (int rep = 0; rep < 2; ++rep)
                for (int t = 0; t < 12; ++t) s.refs.push_back(3 * (rep ? 11 - t : t));
            std::vector<rt_point> pts;
            for (int i = 0; i < 130; ++i) pts.push_back(rt_point{0.04f * i, 0.03f * (i % 97), 0.02f * (i % 31), kInf});
            const size_t n = pts.size();
            EXPECT(query(s, pts, k, out, st) == RT_OK);
            EXPECT(st[0] == 0 && st[1] == n && st[2] == 24 * n);
            for (size_t i = 0; i < n; ++i) {
                EXPECT(row_ok(out, n, k, i));
                for (int j = 0; j < k; ++j) EXPECT(!is_miss(at(out, n, j, i)) && at(out, n, j, i).reserved == 0u);
            }
        }
        {   // a root leaf, and exact sizes around the wave's group: one found, k - 1 misses
            Scene s;
            add_tri(s, 0, 0, 0, 1.0f);
            const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 0.25f};
            s.nodes = {node(lo, hi, -1, -1, 0, 1)};
            s.refs = {0};
            for (int n : {0, 1, 63, 64, 65, 129}) {
                std::vector<rt_point> pts;
                for (int i = 0; i < n; ++i) pts.push_back(rt_point{std::sin((float)i), std::cos((float)i), 0.1f * i, kInf});
                EXPECT(query(s, pts, k, out, st) == RT_OK);
                for (int i = 0; i < n; ++i) {
                    EXPECT(at(out, (size_t)n, 0, (size_t)i).id == 0);
                    for (int j = 1; j < k; ++j) EXPECT(is_miss(at(out, (size_t)n, j, (size_t)i)));
                }
                EXPECT(st[1] == 0 && st[2] == (uint64_t)n);
            }
        }
        {   // a malformed inner node: the right child of the root points outside the array
            Scene s;
            add_tri(s, 0, 0, 0, 1.0f);
            const float lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
            s.nodes = {node(lo, hi, 1, 2, -1, 0), node(lo, hi, -1, -1, 0, 1), node(lo, hi, 7, 9, -1, 0)};
            s.refs = {0};
            std::vector<rt_point> pts = {rt_point{0.2f, 0.2f, 0.2f, kInf}};
            EXPECT(query(s, pts, k, out, st) == RT_OK);
            for (const rt_closest& c : out) EXPECT(is_miss(c));
            EXPECT(st[0] == 0);
        }
        {   // the combs
            std::vector<rt_point> pts;
            for (int i = 0; i < 200; ++i) pts.push_back(rt_point{0.37f * (i % 19), 0.21f * (i % 23), 0.3f * (i % 31), kInf});
            const Scene deep = comb(70);
            EXPECT(query(deep, pts, k, out, st) == RT_OK);
            EXPECT(st[0] == pts.size());   // once per query, not per record
            for (const rt_closest& c : out) EXPECT(is_miss(c));
            const Scene mid = comb(40);
            EXPECT(query(mid, pts, k, out, st) == RT_OK);
            EXPECT(st[0] == 0 && st[2] == 41 * pts.size());   // the last inner node holds its leaf twice
            for (size_t i = 0; i < pts.size(); ++i) {
                EXPECT(row_ok(out, pts.size(), k, i));
                for (int j = 0; j < k; ++j) EXPECT(at(out, pts.size(), j, i).id >= 0 && at(out, pts.size(), j, i).id < 120);
            }
        }
        std::printf("k = %d: ok\n", k);
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
                        const int32_t* rf, int32_t nref, const rt_point* p, int64_t n, int32_t k, rt_closest* o) {
            return rt_nearest_k_host(v, nv, ix, nidx, nd, nn, rf, nref, p, n, k, o, nullptr);
        };
        const int64_t bad_n[] = {-1, (1ll << 30) + 1, 1ll << 40, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()};
        for (int64_t n : bad_n)
            for (int32_t k : {1, 8})
                EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), n, k, o1.data()) == RT_ERR_INVALID_ARG);
        const int32_t bad_k[] = {0, 9, -1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};
        for (int32_t k : bad_k)
            for (int64_t n : {(int64_t)0, (int64_t)1})
                EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), n, k, o1.data()) == RT_ERR_INVALID_ARG);
        // n * k over 2^30 with n itself legal
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), (1ll << 27) + 1, 8, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), (1ll << 29) + 1, 2, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(nullptr, 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, nullptr, 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, nullptr, 1, s.refs.data(), 1, p1.data(), 1, 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, nullptr, 1, p1.data(), 1, 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, nullptr, 1, 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, 1, nullptr) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 2, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, 1, o1.data()) == RT_ERR_INVALID_ARG);
        EXPECT(call(s.verts.data(), 2, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, 1, o1.data()) == RT_ERR_BAD_SCENE);
        for (size_t b = 0; b < sizeof(rt_closest); ++b) EXPECT(((const unsigned char*)o1.data())[b] == 0x5A);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, nullptr, 0, 8, nullptr) == RT_OK);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, 1, o1.data()) == RT_OK);
        EXPECT(o1[0].id == 0 && o1[0].d2 == 0.0f && o1[0].reserved == 0u);
        std::printf("arguments: ok\n");
    }
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
