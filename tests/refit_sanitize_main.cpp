// Drives csrc/host/refit.cpp (rt_refit_nodes and its plan) alone under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_refit.py): well-formed trees, and malformed ones that
// must be refused with RT_ERR_BAD_SCENE without a write or a read out of bounds; and a tree of
// tests/mesh_edge_common.py's chain52 shape (52 heights, the first of 2,039 nodes), with finite
// vertices, a NaN coordinate, an all-NaN axis and +-3e38.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "refit.hpp"
#include "rt_abi.h"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

struct Scene {
    std::vector<rt_float4> verts;
    std::vector<int32_t> idx, refs;
    std::vector<rt_bvh_node> nodes;
};

rt_bvh_node node(int32_t l, int32_t r, int32_t off, int32_t cnt) {
    rt_bvh_node n{};
    n.min = rt_float4{-1, -1, -1, 1};
    n.max = rt_float4{1, 1, 1, 1};
    n.offset_left = l; n.offset_right = r; n.offset_tris = off; n.num_tris = cnt;
    return n;
}

void triangles(Scene& s, int ntri) {
    for (int t = 0; t < ntri; ++t) {
        for (int k = 0; k < 3; ++k) {
            const float a = (float)(t * 3 + k);
            s.verts.push_back(rt_float4{std::sin(a) * 50.0f, std::cos(a * 0.7f) * 40.0f, a * 0.25f - 20.0f, 1.0f});
            s.idx.push_back(t * 3 + k);
        }
        s.refs.push_back(3 * t);
    }
}

Scene comb(int inner) {   // inner i = node 2i {leaf 2i+1, inner i+1}; the last right child is a leaf
    Scene s;
    triangles(s, inner + 1);
    for (int i = 0; i < inner; ++i) {
        s.nodes.push_back(node(2 * i + 1, 2 * i + 2, -1, 0));
        s.nodes.push_back(node(-1, -1, i, 1));
    }
    s.nodes.push_back(node(-1, -1, inner, 1));
    return s;
}

Scene bigleaf() {   // leaves of 40, 3, 0 and 35 triangles
    Scene s;
    triangles(s, 78);
    s.nodes = {node(1, 2, -1, 0), node(3, 4, -1, 0), node(5, 6, -1, 0), node(-1, -1, 0, 40),
               node(-1, -1, 40, 3), node(-1, -1, -1, 0), node(-1, -1, 43, 35)};
    return s;
}

// A tree over triangles [first, first + count): `chain` one-sided levels (one triangle to the left),
// then halves.  span[node] = its range.
int grow(Scene& s, std::vector<std::pair<int, int>>& span, int first, int count, int chain) {
    const int me = (int)s.nodes.size();
    s.nodes.push_back(node(-1, -1, first, count));
    span.push_back({first, first + count});
    if (count == 1) return me;
    const int nl = chain > 0 ? 1 : count / 2;
    const int l = grow(s, span, first, nl, 0);
    const int r = grow(s, span, first + nl, count - nl, chain > 0 ? chain - 1 : 0);
    s.nodes[me] = node(l, r, -1, 0);
    return me;
}

int refit(Scene& s) {
    return rt_refit_nodes(s.verts.data(), (int32_t)s.verts.size(), s.idx.data(), (int32_t)s.idx.size(), s.nodes.data(),
                          (int32_t)s.nodes.size(), s.refs.data(), (int32_t)s.refs.size());
}

// a refused scene: the status, a message, and not one byte of the nodes changed
void expect_refused(Scene s, const char* what) {
    const std::vector<rt_bvh_node> before = s.nodes;
    EXPECT(refit(s) == RT_ERR_BAD_SCENE);
    EXPECT(!rtrefit::last_error().empty());
    EXPECT(std::memcmp(before.data(), s.nodes.data(), before.size() * sizeof(rt_bvh_node)) == 0);
    std::printf("%s: refused (%s)\n", what, rtrefit::last_error().c_str());
}

void box_of(const Scene& s, int t0, int t1, float mn[3], float mx[3]) {
    for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
    for (int v = 3 * t0; v < 3 * t1; ++v) {
        const float p[3] = {s.verts[v].x, s.verts[v].y, s.verts[v].z};
        for (int a = 0; a < 3; ++a) { mn[a] = std::fmin(mn[a], p[a]); mx[a] = std::fmax(mx[a], p[a]); }
    }
}

bool box_is(const rt_bvh_node& n, const float mn[3], const float mx[3]) {
    return n.min.x == mn[0] && n.min.y == mn[1] && n.min.z == mn[2] && n.max.x == mx[0] && n.max.y == mx[1] &&
           n.max.z == mx[2] && n.min.w == 1.0f && n.max.w == 1.0f;
}

bool same(float a, float b) { return a == b || (std::isnan(a) && std::isnan(b)); }

// every node's box is fmin / fmax over its range, which ignores a NaN unless all operands are one
void check_spans(const Scene& s, const std::vector<std::pair<int, int>>& span, const char* what) {
    float mn[3], mx[3];
    int bad = 0;
    for (size_t n = 0; n < s.nodes.size(); ++n) {
        box_of(s, span[n].first, span[n].second, mn, mx);
        const rt_bvh_node& nd = s.nodes[n];
        const float gmn[3] = {nd.min.x, nd.min.y, nd.min.z}, gmx[3] = {nd.max.x, nd.max.y, nd.max.z};
        for (int a = 0; a < 3; ++a) {
            const bool all_nan = std::isinf(mn[a]) && mn[a] > 0 && std::isinf(mx[a]) && mx[a] < 0;   // box_of's seeds survived
            if (all_nan ? !(std::isnan(gmn[a]) && std::isnan(gmx[a])) : !(same(gmn[a], mn[a]) && same(gmx[a], mx[a]))) ++bad;
        }
    }
    EXPECT(bad == 0);
    rtrefit::Plan plan;
    std::string err;
    EXPECT(rtrefit::plan_build(s.nodes.data(), (int32_t)s.nodes.size(), (int32_t)s.refs.size(), nullptr, plan, err) == RT_OK);
    std::printf("%s: ok, %u heights, %u nodes of height 1\n", what, plan.heights(), plan.level_begin[1] - plan.level_begin[0]);
}

}  // namespace

int main() {
    float mn[3], mx[3];
    {   // chain52's shape: 39 one-sided levels into 13 balanced ones; then its vertices at the edges
        Scene s;
        std::vector<std::pair<int, int>> span;
        triangles(s, (1 << 12) + 40);
        grow(s, span, 0, (1 << 12) + 40, 39);
        EXPECT(refit(s) == RT_OK);
        check_spans(s, span, "chain52");
        Scene a = s;
        a.verts[22].y = NAN;
        EXPECT(refit(a) == RT_OK);
        check_spans(a, span, "nan coordinate");
        Scene e = s;
        for (int k = 0; k < 3; ++k) { e.verts[60 + k].y = 3.0e38f; e.verts[63 + k].y = -3.0e38f; }
        EXPECT(refit(e) == RT_OK);
        check_spans(e, span, "overflowing c2");
        Scene c = s;
        for (rt_float4& v : c.verts) v.y = NAN;
        EXPECT(refit(c) == RT_OK);
        check_spans(c, span, "nan axis");
    }
    {   // the comb: 60 heights, one node each; every inner node i bounds triangles i..60
        Scene s = comb(60);
        EXPECT(refit(s) == RT_OK);
        EXPECT(rtrefit::last_error().empty());
        for (int i = 0; i < 60; ++i) {
            box_of(s, i, 61, mn, mx);
            EXPECT(box_is(s.nodes[2 * i], mn, mx));
            box_of(s, i, i + 1, mn, mx);
            EXPECT(box_is(s.nodes[2 * i + 1], mn, mx));
        }
        rtrefit::Plan plan;
        std::string err;
        EXPECT(rtrefit::plan_build(s.nodes.data(), (int32_t)s.nodes.size(), (int32_t)s.refs.size(), nullptr, plan, err) == RT_OK);
        EXPECT(plan.heights() == 60 && plan.ids.size() == 60 && plan.order.size() == 121);
        for (uint32_t h = 0; h < plan.heights(); ++h) {   // height h + 1 holds inner node 59 - h alone
            EXPECT(plan.level_begin[h + 1] - plan.level_begin[h] == 1);
            EXPECT(plan.ids[plan.level_begin[h]] == 2 * (59 - h));
        }
        std::printf("comb: ok\n");
    }
    {   // big leaves and an empty one, which keeps its box
        Scene s = bigleaf();
        EXPECT(refit(s) == RT_OK);
        box_of(s, 0, 40, mn, mx);  EXPECT(box_is(s.nodes[3], mn, mx));
        box_of(s, 40, 43, mn, mx); EXPECT(box_is(s.nodes[4], mn, mx));
        box_of(s, 43, 78, mn, mx); EXPECT(box_is(s.nodes[6], mn, mx));
        box_of(s, 0, 43, mn, mx);  EXPECT(box_is(s.nodes[1], mn, mx));
        const float e0[3] = {-1, -1, -1}, e1[3] = {1, 1, 1};
        EXPECT(box_is(s.nodes[5], e0, e1));
        box_of(s, 43, 78, mn, mx);   // node 2 = the empty leaf's kept box + leaf 6
        for (int a = 0; a < 3; ++a) { mn[a] = std::fmin(mn[a], -1.0f); mx[a] = std::fmax(mx[a], 1.0f); }
        EXPECT(box_is(s.nodes[2], mn, mx));
        std::printf("bigleaf: ok\n");
    }
    {   // a root that is a leaf; and one without triangles
        Scene s;
        triangles(s, 2);
        s.nodes = {node(-1, -1, 0, 2)};
        EXPECT(refit(s) == RT_OK);
        box_of(s, 0, 2, mn, mx);
        EXPECT(box_is(s.nodes[0], mn, mx));
        s.nodes = {node(-1, -1, -1, 0)};
        s.refs.clear();
        EXPECT(rt_refit_nodes(s.verts.data(), 6, s.idx.data(), 6, s.nodes.data(), 1, nullptr, 0) == RT_OK);
        std::printf("rootleaf: ok\n");
    }
    {   // cycles: a node that is its own ancestor
        Scene s = comb(4);
        s.nodes[6].offset_right = 2;
        expect_refused(s, "cycle");
        s = comb(4);
        s.nodes[0].offset_left = 0;
        expect_refused(s, "self loop");
        s = comb(4);
        s.nodes[2].offset_left = 7;   // node 7 now has two parents
        expect_refused(s, "shared node");
    }
    {   // children out of range
        Scene s = comb(4);
        s.nodes[2].offset_right = 1000;
        expect_refused(s, "child too large");
        s = comb(4);
        s.nodes[2].offset_right = -1;   // offset_left >= 0: an inner node with one child
        expect_refused(s, "missing child");
        s = comb(4);
        s.nodes[4].offset_left = 0x7FFFFFFF;
        expect_refused(s, "child INT_MAX");
    }
    {   // leaf ranges and references out of range
        Scene s = bigleaf();
        s.nodes[6].num_tris = 36;
        expect_refused(s, "range past the end");
        s = bigleaf();
        s.nodes[4].offset_tris = -2;
        expect_refused(s, "negative range start");
        s = bigleaf();
        s.nodes[3].offset_tris = 0x7FFFFFF0;
        expect_refused(s, "range overflow");
        s = bigleaf();
        s.refs[10] = 3 * 78;
        expect_refused(s, "reference past the indices");
        s = bigleaf();
        s.refs[10] = 4;
        expect_refused(s, "reference not a multiple of 3");
        s = bigleaf();
        s.idx[17] = 1 << 20;
        expect_refused(s, "vertex index out of range");
    }
    {   // argument checks
        Scene s = comb(2);
        const int32_t nv = (int32_t)s.verts.size(), ni = (int32_t)s.idx.size(), nn = (int32_t)s.nodes.size(),
                      nr = (int32_t)s.refs.size();
        EXPECT(rt_refit_nodes(nullptr, nv, s.idx.data(), ni, s.nodes.data(), nn, s.refs.data(), nr) == RT_ERR_INVALID_ARG);
        EXPECT(rt_refit_nodes(s.verts.data(), nv, nullptr, ni, s.nodes.data(), nn, s.refs.data(), nr) == RT_ERR_INVALID_ARG);
        EXPECT(rt_refit_nodes(s.verts.data(), nv, s.idx.data(), ni, nullptr, nn, s.refs.data(), nr) == RT_ERR_INVALID_ARG);
        EXPECT(rt_refit_nodes(s.verts.data(), nv, s.idx.data(), ni, s.nodes.data(), nn, nullptr, nr) == RT_ERR_INVALID_ARG);
        EXPECT(rt_refit_nodes(s.verts.data(), nv, s.idx.data(), ni - 1, s.nodes.data(), nn, s.refs.data(), nr) == RT_ERR_INVALID_ARG);
        EXPECT(rt_refit_nodes(s.verts.data(), 0, s.idx.data(), ni, s.nodes.data(), nn, s.refs.data(), nr) == RT_ERR_INVALID_ARG);
        EXPECT(rt_refit_nodes(s.verts.data(), nv, s.idx.data(), ni, s.nodes.data(), 0, s.refs.data(), nr) == RT_ERR_INVALID_ARG);
        EXPECT(rt_refit_nodes(s.verts.data(), nv, s.idx.data(), ni, s.nodes.data(), nn, s.refs.data(), -1) == RT_ERR_INVALID_ARG);
        std::printf("arguments: ok\n");
    }
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
