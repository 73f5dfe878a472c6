// Drives csrc/host/multihit.cpp (rt_trace_rays_k_host) with scene_encode.cpp under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_multihit.py): for every k in 1 .. 8, into buffers of exactly
// k * n records, the edge set of the rule (non-finite origins and directions, a zero direction; tmax NaN,
// 0, -1, 0.001f, +inf), a stack of parallel triangles with an empty leaf and degenerate triangles, a
// duplicate set (a tree that references every triangle from two leaves), a root leaf at the sizes around
// a wave's group, a malformed node, a 70-level comb whose every ray overflows and the same comb at 40
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

// a triangle in the plane z = const that covers [x, x + size / 2]^2 well
void add_tri(Scene& s, float x, float y, float z, float size) {
    const int32_t b = (int32_t)s.verts.size();
    s.verts.push_back(rt_float4{x, y, z, 1.0f});
    s.verts.push_back(rt_float4{x + size, y, z, 1.0f});
    s.verts.push_back(rt_float4{x, y + size, z, 1.0f});
    for (int k = 0; k < 3; ++k) s.idx.push_back(b + k);
}

// a comb `depth` levels deep over as many parallel triangles: inner k -> {inner k + 1, leaf k}, every box the whole scene
Scene comb(int depth) {
    Scene s;
    for (int k = 0; k < depth; ++k) add_tri(s, 0.0f, 0.0f, (float)k, 8.0f);
    const float lo[3] = {-1, -1, -1}, hi[3] = {9, 9, (float)depth + 1};
    for (int k = 0; k < depth; ++k) {
        const int32_t next = k + 1 < depth ? 2 * (k + 1) : 2 * k + 1;
        s.nodes.push_back(node(lo, hi, next, 2 * k + 1, -1, 0));
        s.nodes.push_back(node(lo, hi, -1, -1, k, 1));
        s.refs.push_back(3 * k);
    }
    return s;
}

rt_ray ray(float ox, float oy, float oz, float dx, float dy, float dz, float tmax) {
    return rt_ray{ox, oy, oz, tmax, dx, dy, dz, 0u};
}

int query(const Scene& s, const std::vector<rt_ray>& rays, int k, std::vector<rt_hit_uv>& out, uint64_t* st) {
    out.assign(rays.size() * (size_t)k, rt_hit_uv{});   // exactly k * n: one record more is out of bounds
    return rt_trace_rays_k_host(s.verts.data(), (int32_t)s.verts.size(), s.idx.data(), (int32_t)s.idx.size(), s.nodes.data(),
                                (int32_t)s.nodes.size(), s.refs.empty() ? nullptr : s.refs.data(), (int32_t)s.refs.size(),
                                rays.data(), (int64_t)rays.size(), k, out.data(), st);
}

bool is_miss(const rt_hit_uv& c, const rt_ray& r) {
    uint32_t w[4], tw;
    std::memcpy(w, &c, 16);
    std::memcpy(&tw, &r.tmax, 4);
    return w[0] == 0xFFFFFFFFu && w[1] == tw && !(w[2] | w[3]);
}

// plane j of ray i
const rt_hit_uv& at(const std::vector<rt_hit_uv>& out, size_t n, int j, size_t i) { return out[(size_t)j * n + i]; }

// a row is sorted by (t, id), holds no id twice, and its misses come last
bool row_ok(const std::vector<rt_hit_uv>& out, const std::vector<rt_ray>& rays, int k, size_t i) {
    const size_t n = rays.size();
    for (int j = 0; j + 1 < k; ++j) {
        const rt_hit_uv &a = at(out, n, j, i), &b = at(out, n, j + 1, i);
        if (is_miss(a, rays[i]) && !is_miss(b, rays[i])) return false;
        if (!is_miss(b, rays[i]) && !(a.t < b.t || (a.t == b.t && a.id < b.id))) return false;
    }
    return true;
}

}  // namespace

int main() {
    uint64_t st[3];
    std::vector<rt_hit_uv> out;
    for (int k = 1; k <= RT_TRACE_MAX_K; ++k) {
        {   // five parallel triangles and two degenerate ones in one leaf, an empty leaf beside it, plus the edge set
            Scene s;
            for (int t = 0; t < 5; ++t) add_tri(s, 0, 0, (float)(t + 1), 4.0f);
            add_tri(s, 1, 1, 7, 0.0f);   // three equal vertices
            s.verts.push_back(rt_float4{0, 0, 8, 1}); s.verts.push_back(rt_float4{1, 1, 8, 1}); s.verts.push_back(rt_float4{2, 2, 8, 1});
            for (int v = 18; v < 21; ++v) s.idx.push_back(v);   // collinear vertices
            const float lo[3] = {0, 0, 1}, hi[3] = {4, 4, 8};
            s.nodes = {node(lo, hi, 1, 2, -1, 0), node(lo, hi, -1, -1, 0, 7), node(lo, hi, -1, -1, 0, 0)};
            s.refs = {0, 3, 6, 9, 12, 15, 18};
            std::vector<rt_ray> rays;
            for (float bad : {kNan, kInf, -kInf}) {
                rays.push_back(ray(bad, 1, 0, 0, 0, 1, kInf));
                rays.push_back(ray(1, bad, 0, 0, 0, 1, kInf));
                rays.push_back(ray(1, 1, bad, 0, 0, 1, kInf));
                rays.push_back(ray(1, 1, 0, bad, 0, 1, kInf));
                rays.push_back(ray(1, 1, 0, 0, bad, 1, kInf));
                rays.push_back(ray(1, 1, 0, 0, 0, bad, kInf));
            }
            rays.push_back(ray(1, 1, 0, 0, 0, 0, kInf));
            rays.push_back(ray(1, 1, 0, -0.0f, 0, -0.0f, kInf));
            for (float tmax : {kNan, 0.0f, -0.0f, -1.0f, -kInf, 0.001f}) rays.push_back(ray(1, 1, 0, 0, 0, 1, tmax));
            const size_t n_miss = rays.size();
            rays.push_back(ray(1, 1, 0, 0, 0, 1, kInf));      // 5 hits at t = 1 .. 5
            rays.push_back(ray(1, 1, 0, 0, 0, 2.5f, 1e30f));  // the same, the direction not unit length
            rays.push_back(ray(1, 1, 0, 0, 0, 1, 3.0f));      // tmax equal to a hit's t excludes it: t = 1, 2
            const size_t n = rays.size();
            EXPECT(query(s, rays, k, out, st) == RT_OK);
            for (size_t i = 0; i < n_miss; ++i)
                for (int j = 0; j < k; ++j) EXPECT(is_miss(at(out, n, j, i), rays[i]));   // an invalid ray is k miss records
            for (size_t i = n_miss; i < n; ++i) {
                EXPECT(row_ok(out, rays, k, i));
                const int want = i + 1 == n ? 2 : 5;
                for (int j = 0; j < k; ++j) {
                    if (j < want) EXPECT(at(out, n, j, i).id == 3 * j && at(out, n, j, i).t == (float)(j + 1));
                    else EXPECT(is_miss(at(out, n, j, i), rays[i]));
                }
            }
            EXPECT(st[0] == 0);
        }
        {   // the duplicate set: 12 parallel triangles, each referenced from both leaves
            Scene s;
            for (int t = 0; t < 12; ++t) add_tri(s, 0, 0, 0.5f * (float)(t + 1), 8.0f);
            const float lo[3] = {0, 0, 0}, hi[3] = {8, 8, 7};
            s.nodes = {node(lo, hi, 1, 2, -1, 0), node(lo, hi, -1, -1, 0, 12), node(lo, hi, -1, -1, 12, 12)};
            for (int rep = 0; rep < 2; ++rep)
                for (int t = 0; t < 12; ++t) s.refs.push_back(3 * (rep ? 11 - t : t));
            std::vector<rt_ray> rays;
            for (int i = 0; i < 130; ++i) rays.push_back(ray(0.5f + 0.01f * i, 0.5f + 0.01f * (i % 97), -1.0f, 0.001f * (i % 7), 0, 1, kInf));
            const size_t n = rays.size();
            EXPECT(query(s, rays, k, out, st) == RT_OK);
            EXPECT(st[0] == 0 && st[1] == n && st[2] == 24 * n);
            for (size_t i = 0; i < n; ++i) {
                EXPECT(row_ok(out, rays, k, i));
                for (int j = 0; j < k; ++j) EXPECT(at(out, n, j, i).id == 3 * j);
            }
        }
        {   // a root leaf, and exact sizes around the wave's group: one found, k - 1 misses
            Scene s;
            add_tri(s, 0, 0, 1, 4.0f);
            const float lo[3] = {0, 0, 1}, hi[3] = {4, 4, 1};
            s.nodes = {node(lo, hi, -1, -1, 0, 1)};
            s.refs = {0};
            for (int n : {0, 1, 63, 64, 65, 129}) {
                std::vector<rt_ray> rays;
                for (int i = 0; i < n; ++i) rays.push_back(ray(0.5f + 0.005f * i, 0.5f, 0, 0, 0, 1, kInf));
                EXPECT(query(s, rays, k, out, st) == RT_OK);
                for (int i = 0; i < n; ++i) {
                    EXPECT(at(out, (size_t)n, 0, (size_t)i).id == 0 && at(out, (size_t)n, 0, (size_t)i).t == 1.0f);
                    for (int j = 1; j < k; ++j) EXPECT(is_miss(at(out, (size_t)n, j, (size_t)i), rays[(size_t)i]));
                }
                EXPECT(st[1] == 0 && st[2] == (uint64_t)n);
            }
        }
        {   // a malformed inner node: the right child of the root points outside the array
            Scene s;
            add_tri(s, 0, 0, 1, 4.0f);
            const float lo[3] = {0, 0, 0}, hi[3] = {4, 4, 2};
            s.nodes = {node(lo, hi, 1, 2, -1, 0), node(lo, hi, -1, -1, 0, 1), node(lo, hi, 7, 9, -1, 0)};
            s.refs = {0};
            std::vector<rt_ray> rays = {ray(1, 1, -1, 0, 0, 1, kInf)};
            EXPECT(query(s, rays, k, out, st) == RT_OK);
            for (const rt_hit_uv& c : out) EXPECT(is_miss(c, rays[0]));
            EXPECT(st[0] == 0);
        }
        {   // the combs
            std::vector<rt_ray> rays;
            for (int i = 0; i < 200; ++i) rays.push_back(ray(0.5f + 0.01f * (i % 19), 0.5f + 0.01f * (i % 23), -0.5f, 0, 0, 1, kInf));
            const Scene deep = comb(70);
            EXPECT(query(deep, rays, k, out, st) == RT_OK);
            EXPECT(st[0] == rays.size());   // once per ray, not per record
            for (size_t i = 0; i < out.size(); ++i) EXPECT(is_miss(out[i], rays[i % rays.size()]));
            const Scene mid = comb(40);
            EXPECT(query(mid, rays, k, out, st) == RT_OK);
            EXPECT(st[0] == 0);
            for (size_t i = 0; i < rays.size(); ++i) {
                EXPECT(row_ok(out, rays, k, i));
                for (int j = 0; j < k; ++j) EXPECT(at(out, rays.size(), j, i).id == 3 * j);
            }
        }
        std::printf("k = %d: ok\n", k);
    }
    {   // hostile sizes and bad scenes: refused with one-record buffers untouched
        Scene s;
        add_tri(s, 0, 0, 1, 4.0f);
        const float lo[3] = {0, 0, 1}, hi[3] = {4, 4, 1};
        s.nodes = {node(lo, hi, -1, -1, 0, 1)};
        s.refs = {0};
        std::vector<rt_ray> p1 = {ray(1, 1, 0, 0, 0, 1, kInf)};
        std::vector<rt_hit_uv> o1(1);
        std::memset(o1.data(), 0x5A, sizeof(rt_hit_uv));
        auto call = [&](const rt_float4* v, int32_t nv, const int32_t* ix, int32_t nidx, const rt_bvh_node* nd, int32_t nn,
                        const int32_t* rf, int32_t nref, const rt_ray* p, int64_t n, int32_t k, rt_hit_uv* o) {
            return rt_trace_rays_k_host(v, nv, ix, nidx, nd, nn, rf, nref, p, n, k, o, nullptr);
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
        for (size_t b = 0; b < sizeof(rt_hit_uv); ++b) EXPECT(((const unsigned char*)o1.data())[b] == 0x5A);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, nullptr, 0, 8, nullptr) == RT_OK);
        EXPECT(call(s.verts.data(), 3, s.idx.data(), 3, s.nodes.data(), 1, s.refs.data(), 1, p1.data(), 1, 1, o1.data()) == RT_OK);
        EXPECT(o1[0].id == 0 && o1[0].t == 1.0f && o1[0].u == 0.25f && o1[0].v == 0.25f);
        std::printf("arguments: ok\n");
    }
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
