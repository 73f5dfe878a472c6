// Drives rtamd::derive_walk (csrc/host/scene_encode.cpp, the host twin of rt_render.hip's
// derive_walk_kernel) on encoded scenes, alone under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_walk_refs.py): leaves of 1, 2, 15, 16 and 17 references, an empty leaf, escape leaves
// (refit_common's tree of 40, 3, 0 and 35), a root that is a leaf, a kRefError child.  Every walk
// reference must decode back to the (offset, count) of the reference it stands for, and a scene
// has walk references exactly when every leaf has at most 16 and no child is kRefError.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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

rt_bvh_node node(int32_t l, int32_t r, int32_t off, int32_t cnt) {
    rt_bvh_node n{};
    n.min = rt_float4{-1, -1, -1, 1};
    n.max = rt_float4{1, 1, 1, 1};
    n.offset_left = l; n.offset_right = r; n.offset_tris = off; n.num_tris = cnt;
    return n;
}

Mesh triangles(int ntri) {
    Mesh m;
    for (int t = 0; t < ntri; ++t) {
        for (int k = 0; k < 3; ++k) {
            const float a = (float)(t * 3 + k);
            m.verts.push_back(rt_float4{a * 0.5f - 7.0f, (float)((t * 5 + k * 3) % 11) - 4.0f, a * 0.25f + (float)k, 1.0f});
            m.normals.push_back(rt_float4{0.0f, (float)k, 1.0f, 0.0f});
            m.idx.push_back(t * 3 + k);
            m.normal_idx.push_back(t * 3 + k);
        }
        m.refs.push_back(3 * t);
        m.tri_to_mat.push_back(0);
    }
    m.mats.resize(1);
    m.mats[0].diffuse = rt_float4{0.25f, 0.5f, 0.75f, 1.0f};
    return m;
}

// a comb whose leaves have the given reference counts, in order: inner nodes 0, 2, 4, ... each with
// a leaf on the left and the rest on the right
Mesh comb(const std::vector<int>& counts) {
    int total = 0;
    for (int c : counts) total += c;
    Mesh m = triangles(total > 0 ? total : 1);
    if (total == 0) m.refs.clear();
    const int n = (int)counts.size();
    int off = 0;
    if (n == 1) {
        m.nodes = {node(-1, -1, 0, counts[0])};
        return m;
    }
    for (int i = 0; i < n - 1; ++i) {
        const int me = 2 * i;   // its leaf follows it; then the next inner node, or the last leaf
        m.nodes.push_back(node(me + 1, me + 2, -1, 0));
        m.nodes.push_back(node(-1, -1, counts[i] ? off : 0, counts[i]));
        off += counts[i];
    }
    m.nodes.push_back(node(-1, -1, counts[n - 1] ? off : 0, counts[n - 1]));
    return m;
}

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// the present reference's (offset, count), escape table resolved
void present(const rtamd::EncodedScene& e, uint32_t ref, int64_t& off, int64_t& cnt) {
    off = rtrec::ref_offset(ref);
    cnt = rtrec::ref_count(ref);
    if (cnt == rtrec::kCntEscape) {
        cnt = e.leaf_table[off].second;
        off = e.leaf_table[off].first;
    }
}

void check_one(const rtamd::EncodedScene& e, uint32_t ref, uint32_t w, uint32_t tri_unit, uint32_t n_refs, bool& all) {
    if (!(ref & rtrec::kLeafBit)) {
        if (ref == rtrec::kRefError) { EXPECT(w == rtrec::kWalkNone); all = false; return; }
        EXPECT(w == 4 * ref);   // the unit offset of a 64-B record
        return;
    }
    int64_t off, cnt;
    present(e, ref, off, cnt);
    if (cnt > 16) { EXPECT(w == rtrec::kWalkNone); all = false; return; }
    EXPECT(w != rtrec::kWalkNone && (w & rtrec::kLeafBit));
    if (cnt == 0) {   // the pad record, one trip
        EXPECT(rtrec::walk_unit(w) == tri_unit + 3 * n_refs && rtrec::walk_count(w) == 1);
        EXPECT(w < rtrec::kWalkLastBelow);
        return;
    }
    EXPECT((int64_t)rtrec::walk_unit(w) == (int64_t)tri_unit + 3 * off);
    EXPECT((int64_t)rtrec::walk_count(w) == cnt);
    // the cursor's walk: cnt records 48 B apart, the last one (and only it) below kWalkLastBelow
    uint32_t c = w;
    for (int64_t k = 0; k < cnt; ++k) {
        EXPECT((rtrec::walk_unit(c) << 4) == (uint32_t)(16 * tri_unit + 48 * (off + k)));
        EXPECT((c < rtrec::kWalkLastBelow) == (k == cnt - 1));
        c += rtrec::kWalkNext;
    }
}

// -> whether the scene has walk references
bool check_scene(const Mesh& m, const char* what, bool want_walk) {
    rtamd::EncodedScene e;
    std::string err;
    const int rc = rtamd::encode_scene(m.verts.data(), (int32_t)m.verts.size(), m.idx.data(), (int32_t)m.idx.size(), m.nodes.data(),
                                       (int32_t)m.nodes.size(), m.refs.data(), (int32_t)m.refs.size(), m.normals.data(),
                                       (int32_t)m.normals.size(), m.normal_idx.data(), m.mats.data(), (int32_t)m.mats.size(),
                                       m.tri_to_mat.data(), e, err);
    EXPECT(rc == RT_OK);
    if (rc != RT_OK) { std::printf("%s: %s\n", what, err.c_str()); return false; }
    const size_t n_rec = e.wnodes.size() / 4;
    const uint32_t tri_unit = (uint32_t)e.wnodes.size(), n_refs = (uint32_t)((e.tris.size() - 1) / 3);
    std::vector<uint32_t> walk;
    uint32_t walk_root = 0;
    const bool ok = rtamd::derive_walk(e.wnodes.data(), n_rec, e.leaf_table.data(), e.leaf_table.size(), tri_unit, n_refs, e.root,
                                       walk, walk_root);
    EXPECT(walk.size() == 2 * n_rec);
    bool all = true;
    for (size_t i = 0; i < n_rec && 2 * i + 1 < walk.size(); ++i) {
        check_one(e, bits(e.wnodes[4 * i + 3].x), walk[2 * i], tri_unit, n_refs, all);
        check_one(e, bits(e.wnodes[4 * i + 3].y), walk[2 * i + 1], tri_unit, n_refs, all);
    }
    check_one(e, e.root, walk_root, tri_unit, n_refs, all);
    EXPECT(ok == all);
    EXPECT(ok == want_walk);
    std::printf("%s: %s\n", what, ok ? "walk" : "no walk");
    return ok;
}

}  // namespace

int main() {
    check_scene(comb({1, 2, 15, 16}), "leaves of 1 2 15 16", true);
    check_scene(comb({1, 2, 15, 16, 17}), "a leaf of 17", false);
    check_scene(comb({16, 17}), "17 last", false);
    check_scene(comb({3, 0, 5}), "an empty leaf", true);
    check_scene(comb({0, 0}), "no references", true);
    check_scene(comb({40, 3, 0, 35}), "escape leaves 40 and 35", false);
    check_scene(comb({1}), "root leaf of 1", true);
    check_scene(comb({16}), "root leaf of 16", true);
    check_scene(comb({17}), "root leaf of 17", false);
    check_scene(comb({31}), "root escape leaf of 31", false);
    {   // a reachable malformed inner node: kRefError in its parent's record
        Mesh m = triangles(3);
        m.nodes = {node(1, 2, -1, 0), node(3, 99, -1, 0), node(-1, -1, 0, 1), node(-1, -1, 1, 1), node(-1, -1, 2, 1)};
        check_scene(m, "kRefError child", false);
        Mesh r = triangles(1);
        r.nodes = {node(0, 7, -1, 0)};
        check_scene(r, "kRefError root", false);
    }
    {   // hostile tables and references straight into walk_ref: no read outside the table, no wrap
        const int32_t table[4] = {0, 5, -3, 2};
        EXPECT(rtrec::walk_ref(rtrec::leaf_ref(rtrec::kCntEscape, 0), table, 2, 1, 4, 10) == (rtrec::kLeafBit | (4u << 27) | 4u));
        EXPECT(rtrec::walk_ref(rtrec::leaf_ref(rtrec::kCntEscape, 1), table, 2, 1, 4, 10) == rtrec::kWalkNone);   // negative offset
        EXPECT(rtrec::walk_ref(rtrec::leaf_ref(rtrec::kCntEscape, 2), table, 2, 1, 4, 10) == rtrec::kWalkNone);   // past the table
        EXPECT(rtrec::walk_ref(rtrec::leaf_ref(4, 8), table, 2, 1, 4, 10) == rtrec::kWalkNone);                    // range past the records
        EXPECT(rtrec::walk_ref(rtrec::leaf_ref(2, 8), table, 2, 1, 4, 10) == (rtrec::kLeafBit | (1u << 27) | 28u));
        EXPECT(rtrec::walk_ref(1u, table, 2, 1, 4, 10) == rtrec::kWalkNone);                                       // inner id past the records
        EXPECT(rtrec::walk_ref(rtrec::leaf_ref(1, 0), table, 2, 1, 0x07FFFFFEu, 10) == rtrec::kWalkNone);           // unit offset past 27 bits
        std::printf("hostile references: ok\n");
    }
    if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
