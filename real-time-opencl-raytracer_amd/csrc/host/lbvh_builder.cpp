// lbvh_builder.cpp -- the host twin of the on-GPU LBVH build (rt_build_bvh, csrc/rt_lbvh.hip;
// DESIGN.md 15).  No HIP, no GPU: the same definition, stage by stage, and the same bytes.
//
//   boxes    lo / hi of every triangle (fminf / fmaxf over its vertices), c2 = lo + hi
//   bounds   cmin / cmax of c2 over all triangles
//   keys     cells per axis -> morton39 << 25 | triangle (lbvh_core.hpp); sorted ascending.  The
//            key plan says which axis gives which Morton bit: 13 bits per axis in turn, or with
//            RT_BUILD_EXTENT_KEYS in max_leaf the extent-aware plan of DESIGN.md 17
//   tree     the binary radix tree over the sorted keys (Karras 2012), node by node
//   collapse a radix node is kept iff its range holds more than max_leaf positions; a child of a
//            kept node that is not kept is ONE leaf over its range
//   output   kept nodes by Karras number (root = node 0), then leaves by first position;
//            tri_indices[p] = 3 * triangle at position p
//   boxes    leaf = min / max over its triangles' vertices, inner = union of its children
//            (rt_refit_nodes' semantics: a refit of the output with the same vertices is a no-op)
//
// The node order is the builder's own, not pre-order: everything downstream follows child offsets.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <new>

#include "lbvh_core.hpp"
#include "rt_handles.hpp"

static_assert(lbvh::kExtentKeys == RT_BUILD_EXTENT_KEYS, "lbvh_core.hpp restates the ABI's flag");

namespace rtamd {

namespace {

struct Fit {
    const rt_float4* verts;
    const int32_t* idx;
    Bvh& out;
    int32_t max_depth = 0;

    void leaf_box(rt_bvh_node& nd) const {
        float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
        bool first = true;
        for (int32_t r = nd.offset_tris; r < nd.offset_tris + nd.num_tris; ++r)
            for (int k = 0; k < 3; ++k) {
                const rt_float4& v = verts[idx[out.tri_indices[r] + k]];
                const float p[3] = {v.x, v.y, v.z};
                for (int a = 0; a < 3; ++a) {
                    mn[a] = first ? p[a] : fminf(mn[a], p[a]);
                    mx[a] = first ? p[a] : fmaxf(mx[a], p[a]);
                }
                first = false;
            }
        nd.min = rt_float4{mn[0], mn[1], mn[2], 1.0f};
        nd.max = rt_float4{mx[0], mx[1], mx[2], 1.0f};
    }

    // bottom-up; the tree is at most 64 deep (64-bit unique keys)
    void fit(int32_t n, int32_t depth) {
        rt_bvh_node& nd = out.nodes[n];
        if (nd.offset_left < 0) {
            leaf_box(nd);
            max_depth = std::max(max_depth, depth);
            return;
        }
        fit(nd.offset_left, depth + 1);
        fit(nd.offset_right, depth + 1);
        const rt_bvh_node& L = out.nodes[nd.offset_left];
        const rt_bvh_node& R = out.nodes[nd.offset_right];
        nd.min = rt_float4{fminf(L.min.x, R.min.x), fminf(L.min.y, R.min.y), fminf(L.min.z, R.min.z), 1.0f};
        nd.max = rt_float4{fmaxf(L.max.x, R.max.x), fmaxf(L.max.y, R.max.y), fmaxf(L.max.z, R.max.z), 1.0f};
    }
};

rt_bvh_node leaf_node(int32_t first, int32_t count) {
    rt_bvh_node nd{};
    nd.offset_left = nd.offset_right = -1;
    nd.offset_tris = first;
    nd.num_tris = count;
    return nd;
}

}  // namespace

int build_lbvh(const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx, int max_leaf_arg, Bvh& out,
               std::string& err) {
    const auto t0 = std::chrono::steady_clock::now();
    out = Bvh();
    if (!verts || nv <= 0 || !idx || nidx <= 0 || nidx % 3 != 0 || nidx / 3 > lbvh::kMaxTris) {
        err = "lbvh: needs vertices and 1 .. 2^25 triangles (3 indices each)";
        return RT_ERR_INVALID_ARG;
    }
    int32_t max_leaf = 0;
    bool extent_keys = false;
    if (!lbvh::split_max_leaf(max_leaf_arg, max_leaf, extent_keys)) {
        err = "lbvh: max_leaf must be 1 .. 8 (| RT_BUILD_EXTENT_KEYS)";
        return RT_ERR_INVALID_ARG;
    }
    for (int32_t i = 0; i < nidx; ++i)
        if (idx[i] < 0 || idx[i] >= nv) { err = "lbvh: mesh_indices out of range"; return RT_ERR_BAD_SCENE; }
    const int32_t n = nidx / 3;

    // triangle boxes -> c2 = lo + hi, and its bounds
    std::vector<float> c2((size_t)n * 3);
    float cmin[3] = {0, 0, 0}, cmax[3] = {0, 0, 0};
    for (int32_t t = 0; t < n; ++t) {
        const rt_float4 &v0 = verts[idx[3 * t]], &v1 = verts[idx[3 * t + 1]], &v2 = verts[idx[3 * t + 2]];
        const float p[3][3] = {{v0.x, v0.y, v0.z}, {v1.x, v1.y, v1.z}, {v2.x, v2.y, v2.z}};
        for (int a = 0; a < 3; ++a) {
            const float lo = fminf(fminf(p[0][a], p[1][a]), p[2][a]);
            const float hi = fmaxf(fmaxf(p[0][a], p[1][a]), p[2][a]);
            const float c = lo + hi;
            c2[(size_t)t * 3 + a] = c;
            cmin[a] = t ? fminf(cmin[a], c) : c;
            cmax[a] = t ? fmaxf(cmax[a], c) : c;
        }
    }
    const lbvh::KeyPlan plan = extent_keys ? lbvh::extent_plan(cmin, cmax) : lbvh::axis_plan();
    std::vector<uint64_t> keys((size_t)n);
    for (int32_t t = 0; t < n; ++t) keys[t] = lbvh::key_of(plan, &c2[(size_t)t * 3], cmin, cmax, (uint32_t)t);
    std::sort(keys.begin(), keys.end());
    out.tri_indices.resize((size_t)n);
    for (int32_t p = 0; p < n; ++p) out.tri_indices[p] = 3 * (int32_t)(keys[p] & lbvh::kIndexMask);

    if (n <= max_leaf) {   // the root is not kept: one root leaf
        out.nodes.push_back(leaf_node(0, n));
    } else {
        // radix nodes: range and split; kept flags; where leaves start
        struct Radix { int32_t a, b, s; };
        std::vector<Radix> rad((size_t)n - 1);
        std::vector<int32_t> inner_rank((size_t)n, 0), leaf_rank((size_t)n, 0);   // flags, then exclusive sums
        auto kept = [&](int32_t lo, int32_t hi) { return hi - lo + 1 > max_leaf; };
        for (int32_t i = 0; i < n - 1; ++i) {
            Radix& r = rad[i];
            lbvh::node(keys.data(), n, i, r.a, r.b, r.s);
            if (!kept(r.a, r.b)) continue;
            inner_rank[i] = 1;
            if (!kept(r.a, r.s)) leaf_rank[r.a] = 1;
            if (!kept(r.s + 1, r.b)) leaf_rank[r.s + 1] = 1;
        }
        int32_t K = 0, leaves = 0;
        for (int32_t p = 0; p < n; ++p) {
            const int32_t fi = inner_rank[p], fl = leaf_rank[p];
            inner_rank[p] = K;
            leaf_rank[p] = leaves;
            K += fi;
            leaves += fl;
        }
        out.nodes.resize((size_t)K + leaves);
        for (int32_t i = 0; i < n - 1; ++i) {
            const Radix& r = rad[i];
            if (!kept(r.a, r.b)) continue;
            rt_bvh_node nd{};
            nd.offset_tris = -1;
            nd.num_tris = 0;
            const int32_t lo[2] = {r.a, r.s + 1}, hi[2] = {r.s, r.b};
            int32_t child[2];
            for (int c = 0; c < 2; ++c) {
                if (kept(lo[c], hi[c])) {
                    child[c] = inner_rank[c ? r.s + 1 : r.s];   // Karras: inner children are nodes s and s + 1
                } else {
                    child[c] = K + leaf_rank[lo[c]];
                    out.nodes[child[c]] = leaf_node(lo[c], hi[c] - lo[c] + 1);
                }
            }
            nd.offset_left = child[0];
            nd.offset_right = child[1];
            out.nodes[inner_rank[i]] = nd;
        }
    }
    Fit f{verts, idx, out};
    f.fit(0, 0);
    out.max_depth = f.max_depth;
    out.num_leaves = (int32_t)(out.nodes.size() + 1) / 2;
    out.build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}

}  // namespace rtamd

extern "C" int rt_bvh_build_lbvh(const rt_mesh* mh, int32_t max_leaf, rt_bvh** out) {
    if (!mh || !out) return RT_ERR_INVALID_ARG;
    rt_bvh* b = new (std::nothrow) rt_bvh();
    if (!b) return RT_ERR_OUT_OF_MEMORY;
    std::string err;
    const rtamd::Mesh& m = mh->m;
    const int rc = rtamd::build_lbvh(m.vertices.data(), (int32_t)m.vertices.size(), m.indices.data(),
                                     (int32_t)m.indices.size(), max_leaf, b->b, err);
    if (rc != RT_OK) { delete b; return rc; }
    *out = b;
    return RT_OK;
}
