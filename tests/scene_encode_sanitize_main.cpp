// Drives csrc/host/scene_encode.cpp (rt_upload_scene's host half; with csrc/host/refit.cpp for the
// plan that takes its inner ids) alone under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_scene_encode.py): well-formed trees, trees that must be refused with
// RT_ERR_BAD_SCENE, and the malformed inner node that must encode as the error reference.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "refit.hpp"
#include "rt_abi.h"
#include "rt_records.h"
#include "scene_encode.hpp"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

struct Mesh {
    std::vector<rt_float4> verts, normals;
    std::vector<int32_t> idx, normal_idx, refs, tri_to_mat;
    std::vector<rt_material> mats;
    std::vector<rt_bvh_node> nodes;
};

rt_bvh_node node(int32_t l, int32_t r, int32_t off, int32_t cnt, float lo = -1.0f, float hi = 1.0f) {
    rt_bvh_node n{};
    n.min = rt_float4{lo, lo, lo, 1};
    n.max = rt_float4{hi, hi, hi, 1};
    n.offset_left = l; n.offset_right = r; n.offset_tris = off; n.num_tris = cnt;
    return n;
}

// ntri triangles of their own vertices, one normal per vertex, two materials, references in order
Mesh triangles(int ntri) {
    Mesh m;
    for (int t = 0; t < ntri; ++t) {
        for (int k = 0; k < 3; ++k) {
            const float a = (float)(t * 3 + k);
            m.verts.push_back(rt_float4{a * 1.5f - 7.0f, (float)((t * 5 + k * 3) % 11) - 4.0f, a * 0.25f + (float)k, 1.0f});
            m.normals.push_back(rt_float4{0.0f, (float)k, 1.0f, 0.0f});
            m.idx.push_back(t * 3 + k);
            m.normal_idx.push_back(t * 3 + k);
        }
        m.refs.push_back(3 * t);
        m.tri_to_mat.push_back(t % 2);
    }
    m.mats.resize(2);
    m.mats[0].diffuse = rt_float4{0.25f, 0.5f, 0.75f, 1.0f};
    m.mats[1].diffuse = rt_float4{1.0f, 0.125f, 0.0f, 1.0f};
    return m;
}

int encode(const Mesh& m, rtamd::EncodedScene& e, std::string& err) {
    return rtamd::encode_scene(m.verts.data(), (int32_t)m.verts.size(), m.idx.data(), (int32_t)m.idx.size(), m.nodes.data(),
                               (int32_t)m.nodes.size(), m.refs.data(), (int32_t)m.refs.size(), m.normals.data(),
                               (int32_t)m.normals.size(), m.normal_idx.data(), m.mats.data(), (int32_t)m.mats.size(),
                               m.tri_to_mat.data(), e, err);
}

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// the counts every encoded scene has, and every record word against the definition
void expect_layout(const Mesh& m, const rtamd::EncodedScene& e) {
    const size_t nref = m.refs.size(), ntri = m.idx.size() / 3;
    EXPECT(e.wnodes.size() == 4 * (size_t)std::max<uint32_t>(e.n_inner, 1u));
    EXPECT(e.tris.size() == 3 * std::max<size_t>(nref, 1) + 1);
    EXPECT(e.shade.size() == 7 * ntri);
    EXPECT(!e.leaf_table.empty());
    EXPECT(e.inner_id.size() == m.nodes.size());
    for (size_t i = 0; i < nref && 3 * i + 2 < e.tris.size(); ++i) {
        const int32_t t = m.refs[i];
        const rt_float4 v0 = m.verts[m.idx[t]], v1 = m.verts[m.idx[t + 1]], v2 = m.verts[m.idx[t + 2]];
        const rt_float4 *r = &e.tris[3 * i];
        EXPECT(r[0].x == v0.x && r[0].y == v0.y && r[0].z == v0.z && bits(r[0].w) == (uint32_t)t);
        EXPECT(r[1].x == v1.x - v0.x && r[1].y == v1.y - v0.y && r[1].z == v1.z - v0.z && r[1].w == 0.0f);
        EXPECT(r[2].x == v2.x - v0.x && r[2].y == v2.y - v0.y && r[2].z == v2.z - v0.z && r[2].w == 0.0f);
    }
    const rt_float4 pad = e.tris.back();
    EXPECT(pad.x == 0.0f && pad.y == 0.0f && pad.z == 0.0f && pad.w == 0.0f);
    for (size_t t = 0; t < ntri && 7 * t + 6 < e.shade.size(); ++t) {
        const rt_float4* s = &e.shade[7 * t];
        for (int k = 0; k < 3; ++k) {
            const rt_float4 v = m.verts[m.idx[3 * t + k]], n = m.normals[m.normal_idx[3 * t + k]];
            EXPECT(s[k].x == v.x && s[k].y == v.y && s[k].z == v.z && s[k].w == 0.0f);
            EXPECT(s[3 + k].x == n.x && s[3 + k].y == n.y && s[3 + k].z == n.z && s[3 + k].w == 0.0f);
        }
        const rt_float4 d = m.mats[m.tri_to_mat[t]].diffuse;
        EXPECT(s[6].x == d.x && s[6].y == d.y && s[6].z == d.z && s[6].w == 0.0f);
    }
}

// a valid scene: encodes, has the layout, and its inner ids feed the refit plan
rtamd::EncodedScene expect_ok(const Mesh& m, const char* what, bool refittable = true) {
    rtamd::EncodedScene e;
    std::string err;
    const int rc = encode(m, e, err);
    EXPECT(rc == RT_OK);
    if (rc != RT_OK) { std::printf("%s: %s\n", what, err.c_str()); return e; }
    expect_layout(m, e);
    rtrefit::Plan plan;
    std::string why;
    const int prc = rtrefit::plan_build(m.nodes.data(), (int32_t)m.nodes.size(), (int32_t)m.refs.size(), e.inner_id.data(),
                                        plan, why);
    EXPECT((prc == RT_OK) == refittable);
    if (prc == RT_OK) EXPECT(plan.ids.size() == e.n_inner);
    std::printf("%s: ok\n", what);
    return e;
}

void expect_refused(const Mesh& m, const char* message, const char* what) {
    rtamd::EncodedScene e;
    std::string err;
    EXPECT(encode(m, e, err) == RT_ERR_BAD_SCENE);
    EXPECT(err == message);
    if (err != message) std::printf("%s: got \"%s\"\n", what, err.c_str());
    else std::printf("%s: refused\n", what);
}

Mesh two_leaves(int left, int right) {
    Mesh m = triangles(left + right);
    m.nodes = {node(1, 2, -1, 0), node(-1, -1, 0, left), node(-1, -1, left, right)};
    return m;
}

void valid_scenes() {
    {   // the root is a leaf: no inner record, four zero float4s in its place
        Mesh m = triangles(1);
        m.nodes = {node(-1, -1, 0, 1)};
        const rtamd::EncodedScene e = expect_ok(m, "root leaf");
        EXPECT(e.n_inner == 0 && e.root == rtrec::leaf_ref(1, 0) && e.clean == 1 && e.fast_div == 1);
        EXPECT(e.inner_id[0] == -1);
        for (const rt_float4& q : e.wnodes) EXPECT(q.x == 0.0f && q.y == 0.0f && q.z == 0.0f && q.w == 0.0f);
        EXPECT(e.leaf_table.size() == 1 && e.leaf_table[0].first == 0 && e.leaf_table[0].second == 0);
    }
    {
        Mesh m = two_leaves(2, 3);
        m.nodes[1] = node(-1, -1, 0, 2, -3.0f, 0.5f);
        m.nodes[2] = node(-1, -1, 2, 3, 0.25f, 4.0f);
        const rtamd::EncodedScene e = expect_ok(m, "two leaves");
        EXPECT(e.n_inner == 1 && e.root == 0 && e.inner_id[0] == 0 && e.clean == 1 && e.fast_div == 1);
        for (int k = 0; k < 3; ++k) {   // axis-major {L.min, R.min, L.max, R.max}
            const float* q = &e.wnodes[k].x;
            EXPECT(q[0] == -3.0f && q[1] == 0.25f && q[2] == 0.5f && q[3] == 4.0f);
        }
        EXPECT(bits(e.wnodes[3].x) == rtrec::leaf_ref(2, 0) && bits(e.wnodes[3].y) == rtrec::leaf_ref(3, 2));
        EXPECT(e.wnodes[3].z == 0.0f && e.wnodes[3].w == 0.0f);
    }
    {   // 30 references fit the count field; 31 and 40 take the escape table
        Mesh m = triangles(101);
        m.nodes = {node(1, 2, -1, 0), node(3, 4, -1, 0), node(-1, -1, 0, 30), node(-1, -1, 30, 31), node(-1, -1, 61, 40)};
        const rtamd::EncodedScene e = expect_ok(m, "escape leaves");
        EXPECT(e.n_inner == 2 && e.leaf_table.size() == 2);
        EXPECT(e.leaf_table[0].first == 30 && e.leaf_table[0].second == 31);
        EXPECT(e.leaf_table[1].first == 61 && e.leaf_table[1].second == 40);
        EXPECT(bits(e.wnodes[3].x) == 1u && bits(e.wnodes[3].y) == rtrec::leaf_ref(30, 0));
        EXPECT(bits(e.wnodes[7].x) == rtrec::leaf_ref(rtrec::kCntEscape, 0));
        EXPECT(bits(e.wnodes[7].y) == rtrec::leaf_ref(rtrec::kCntEscape, 1));
        EXPECT(rtrec::ref_count(bits(e.wnodes[7].y)) == rtrec::kCntEscape && rtrec::ref_offset(bits(e.wnodes[7].y)) == 1u);
    }
    {   // an empty leaf and one with a negative count: count 0, offset 0, whatever the offset says
        Mesh m = two_leaves(1, 1);
        m.nodes[1] = node(-1, -1, -1, 0);
        m.nodes[2] = node(-1, -1, 1 << 30, -5);
        const rtamd::EncodedScene e = expect_ok(m, "empty and negative leaves");
        EXPECT(bits(e.wnodes[3].x) == rtrec::leaf_ref(0, 0) && bits(e.wnodes[3].y) == rtrec::leaf_ref(0, 0));
        EXPECT(e.leaf_table.size() == 1 && e.clean == 1);
    }
    {   // no references at all: the triangle records keep their minimum size
        Mesh m = two_leaves(1, 1);
        m.refs.clear();
        m.nodes[1] = node(-1, -1, 0, 0);
        m.nodes[2] = node(-1, -1, 0, 0);
        const rtamd::EncodedScene e = expect_ok(m, "no references");
        EXPECT(e.tris.size() == 4);
    }
}

void fast_quotient_domain() {
    for (int big = 0; big < 2; ++big) {
        Mesh m = two_leaves(1, 1);
        m.nodes[2].max.y = big ? 0x1p61f : 0x1p60f;
        const rtamd::EncodedScene e = expect_ok(m, big ? "2^61" : "2^60");
        EXPECT(e.fast_div == (big ? 0 : 1));
    }
    Mesh m = two_leaves(1, 1);
    m.nodes[1].min.x = -0x1p-67f;
    EXPECT(expect_ok(m, "2^-67").fast_div == 0);
    m.nodes[1].min.x = -0x1p-66f;
    m.nodes[1].min.z = -0.0f;
    EXPECT(expect_ok(m, "2^-66 and a negative zero").fast_div == 1);
}

void refusals() {
    {
        Mesh m = two_leaves(1, 1);
        m.nodes = {node(1, 2, -1, 0), node(0, 2, -1, 0), node(-1, -1, 0, 2)};   // node 1's left child is the root
        expect_refused(m, "BVH has a cycle", "cycle through the root");
        m.nodes = {node(1, 2, -1, 0), node(1, 2, -1, 0), node(-1, -1, 0, 2)};   // node 1 is its own child
        expect_refused(m, "BVH has a cycle", "self loop");
    }
    {
        Mesh m = two_leaves(2, 2);
        m.idx[4] = (int32_t)m.verts.size();
        expect_refused(m, "mesh_indices out of range", "vertex index == nv");
        m.idx[4] = -1;
        expect_refused(m, "mesh_indices out of range", "vertex index -1");
    }
    {
        Mesh m = two_leaves(2, 2);
        m.normal_idx[11] = (int32_t)m.normals.size();
        expect_refused(m, "mesh_normals_indices out of range", "normal index == nnorm");
        m.normal_idx[11] = -7;
        expect_refused(m, "mesh_normals_indices out of range", "normal index -7");
    }
    {
        Mesh m = two_leaves(2, 2);
        m.tri_to_mat[3] = 2;
        expect_refused(m, "tri_to_material out of range", "material index == nmat");
        m.tri_to_mat[3] = -1;
        expect_refused(m, "tri_to_material out of range", "material index -1");
    }
    {
        Mesh m = two_leaves(2, 2);
        for (int32_t bad : {4, 12, 10, -3, 0x7FFFFFFF, 0x7FFFFFFE}) {   // no multiple of 3; at or past the indices
            m.refs[1] = bad;
            expect_refused(m, "bvh_tris_indices entry out of range", "reference");
        }
    }
    {
        Mesh m = two_leaves(2, 2);
        m.nodes[2] = node(-1, -1, 2, 3);
        expect_refused(m, "leaf triangle range out of bounds", "leaf range past nref");
        m.nodes[2] = node(-1, -1, -1, 1);
        expect_refused(m, "leaf triangle range out of bounds", "negative leaf offset");
        m.nodes[2] = node(-1, -1, 0x7FFFFFFF, 0x7FFFFFFF);
        expect_refused(m, "leaf triangle range out of bounds", "leaf range that overflows 32 bits");
    }
}

// tests/golden/bad_node.npz's shape: a reachable inner node with a child offset outside [0, nn)
void malformed_inner_node() {
    for (int32_t bad : {5, 1 << 30, -1}) {   // == nn, far past it, negative
        Mesh m = triangles(3);
        m.nodes = {node(1, 2, -1, 0), node(3, bad, -1, 0), node(-1, -1, 0, 1), node(-1, -1, 1, 1), node(-1, -1, 2, 1)};
        const rtamd::EncodedScene e = expect_ok(m, "malformed inner node", false);
        EXPECT(e.clean == 0 && e.n_inner == 1 && e.inner_id[1] == -1);
        EXPECT(bits(e.wnodes[3].x) == rtrec::kRefError);   // the parent's slot of the malformed node
        EXPECT(bits(e.wnodes[3].y) == rtrec::leaf_ref(1, 0));
    }
    Mesh m = triangles(1);   // the root itself
    m.nodes = {node(0, 7, -1, 0)};
    const rtamd::EncodedScene e = expect_ok(m, "malformed root", false);
    EXPECT(e.clean == 0 && e.n_inner == 0 && e.root == rtrec::kRefError);
}

}  // namespace

int main() {
    valid_scenes();
    fast_quotient_domain();
    refusals();
    malformed_inner_node();
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
