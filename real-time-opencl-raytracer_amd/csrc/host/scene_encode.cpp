// scene_encode.cpp -- see scene_encode.hpp.  Every float operation is a single one, as written
// (-ffp-contract=off): rt_refit.hip and rt_scene_build.hip make the same ones on the device.
#include "scene_encode.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_records.h"

namespace rtamd {

int encode_scene(const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx, const rt_bvh_node* nodes, int32_t nn,
                 const int32_t* refs, int32_t nref, const rt_float4* normals, int32_t nnorm, const int32_t* normal_idx,
                 const rt_material* mats, int32_t nmat, const int32_t* tri_to_mat, EncodedScene& out, std::string& err) {
    auto refuse = [&err](const char* why) { err = why; return (int)RT_ERR_BAD_SCENE; };
    const int32_t ntri = nidx / 3;
    for (int32_t i = 0; i < nidx; ++i) {
        if (idx[i] < 0 || idx[i] >= nv) return refuse("mesh_indices out of range");
        if (normal_idx[i] < 0 || normal_idx[i] >= nnorm) return refuse("mesh_normals_indices out of range");
    }
    for (int32_t t = 0; t < ntri; ++t)
        if (tri_to_mat[t] < 0 || tri_to_mat[t] >= nmat) return refuse("tri_to_material out of range");
    for (int32_t i = 0; i < nref; ++i)
        if (refs[i] < 0 || refs[i] % 3 != 0 || refs[i] > nidx - 3) return refuse("bvh_tris_indices entry out of range");

    // --- reference encoding of every node (traverse_bvh semantics, volumeRender.cl:829-856) ---
    std::vector<int32_t>& inner_id = out.inner_id;
    inner_id.assign(nn, -1);
    out.leaf_table.clear();
    std::vector<uint32_t> ref_of(nn, 0);
    // inner ids in pre-order of reachability from the root; detect cycles (the
    // reference would spin forever on some of them).
    std::vector<uint8_t> state(nn, 0);  // 0 new, 1 on path, 2 done
    {
        std::vector<std::pair<int32_t, int>> stk;
        int32_t next = 0;
        stk.push_back({0, 0});
        while (!stk.empty()) {
            auto& top = stk.back();
            const int32_t n = top.first;
            const rt_bvh_node& nd = nodes[n];
            if (top.second == 0) {
                if (state[n] == 2) { stk.pop_back(); continue; }
                if (state[n] == 1) return refuse("BVH has a cycle");
                state[n] = 1;
                bool valid_inner = nd.offset_left >= 0 && nd.offset_right >= 0 && nd.offset_left < nn && nd.offset_right < nn;
                if (nd.offset_left >= 0 && valid_inner) inner_id[n] = next++;
            }
            const bool is_inner = nd.offset_left >= 0 && inner_id[n] >= 0;
            if (is_inner && top.second < 2) {
                int32_t child = top.second == 0 ? nd.offset_left : nd.offset_right;
                top.second++;
                if (state[child] == 1) return refuse("BVH has a cycle");
                if (state[child] == 0) stk.push_back({child, 0});
                continue;
            }
            state[n] = 2;
            stk.pop_back();
        }
        // the first kBfsTop inner nodes in breadth-first order from the root get ids
        // 0..kBfsTop-1 (the top of the tree, which every ray walks, in 64 KB); the rest
        // keep their pre-order
        constexpr int32_t kBfsTop = 1024;
        std::vector<int32_t> bfs;
        std::vector<uint8_t> seen(nn, 0);
        if (inner_id[0] >= 0) { bfs.push_back(0); seen[0] = 1; }
        for (size_t i = 0; i < bfs.size() && (int32_t)bfs.size() < kBfsTop; ++i) {
            const rt_bvh_node& nd = nodes[bfs[i]];
            for (int32_t ch : {nd.offset_left, nd.offset_right})
                if (inner_id[ch] >= 0 && !seen[ch] && (int32_t)bfs.size() < kBfsTop) {
                    seen[ch] = 1;
                    bfs.push_back(ch);
                }
        }
        std::vector<int32_t> by_old(next, -1);
        for (int32_t n = 0; n < nn; ++n)
            if (inner_id[n] >= 0) by_old[inner_id[n]] = n;
        int32_t id = 0;
        for (int32_t n : bfs) inner_id[n] = id++;
        for (int32_t o = 0; o < next; ++o)
            if (!seen[by_old[o]]) inner_id[by_old[o]] = id++;
    }
    bool clean = true;
    for (int32_t n = 0; n < nn; ++n)
        if (state[n] != 0 && nodes[n].offset_left >= 0 && inner_id[n] < 0) clean = false;
    int32_t n_inner = 0;
    for (int32_t n = 0; n < nn; ++n) {
        const rt_bvh_node& nd = nodes[n];
        if (inner_id[n] >= 0) ++n_inner;
        if (nd.offset_left >= 0) {
            ref_of[n] = inner_id[n] >= 0 ? (uint32_t)inner_id[n] : rtrec::kRefError;
        } else {
            int32_t off = nd.offset_tris, cnt = nd.num_tris < 0 ? 0 : nd.num_tris;
            if (cnt > 0 && (off < 0 || (int64_t)off + cnt > nref)) return refuse("leaf triangle range out of bounds");
            if (cnt == 0) off = 0;
            if (cnt < (int32_t)rtrec::kCntEscape && off < (int32_t)rtrec::kOffLimit) {
                ref_of[n] = rtrec::leaf_ref((uint32_t)cnt, (uint32_t)off);
            } else {
                if (out.leaf_table.size() >= rtrec::kOffLimit) return refuse("too many escape leaves");
                ref_of[n] = rtrec::leaf_ref(rtrec::kCntEscape, (uint32_t)out.leaf_table.size());
                out.leaf_table.push_back({off, cnt});
            }
        }
    }
    out.wnodes.assign((size_t)std::max(n_inner, 1) * 4, rt_float4{0, 0, 0, 0});
    bool fast_ok = true;  // slab-test fast quotient domain (rt_kernel_body.inc axis_ok)
    for (int32_t n = 0; n < nn; ++n) {
        if (inner_id[n] < 0) continue;
        const rt_bvh_node& L = nodes[nodes[n].offset_left];
        const rt_bvh_node& R = nodes[nodes[n].offset_right];
        rt_float4* q = &out.wnodes[(size_t)inner_id[n] * 4];
        // axis-major: {L.min, R.min, L.max, R.max} per axis (rt_kernel_body.inc slab2_pk)
        q[0] = rt_float4{L.min.x, R.min.x, L.max.x, R.max.x};
        q[1] = rt_float4{L.min.y, R.min.y, L.max.y, R.max.y};
        q[2] = rt_float4{L.min.z, R.min.z, L.max.z, R.max.z};
        uint32_t r0 = ref_of[nodes[n].offset_left], r1 = ref_of[nodes[n].offset_right];
        float f0, f1;
        std::memcpy(&f0, &r0, 4);
        std::memcpy(&f1, &r1, 4);
        q[3] = rt_float4{f0, f1, 0.0f, 0.0f};
        for (int k = 0; k < 3; ++k) {
            const float* qf = &q[k].x;
            for (int j = 0; j < 4; ++j) {
                const float a = std::fabs(qf[j]);
                if (!(a == 0.0f || (a >= 0x1p-66f && a <= 0x1p60f))) fast_ok = false;
            }
            // the octant loops (slab2_pk's OCT) name near and far by the ray's sign: both children's
            // min <= max.  An inverted box sends the scene to the division form, as a coordinate
            // outside the domain does.  (The device builds, rt_refit.hip and rt_scene_build.hip,
            // make every box as min / max over finite data, so theirs are ordered.)
            if (!(qf[0] <= qf[2] && qf[1] <= qf[3])) fast_ok = false;
        }
    }
    // triangle reference records {v0|id, e1, e2} (volumeRender.cl:965-974), layout of tri_rec
    out.tris.assign((size_t)std::max(nref, 1) * 3 + 1, rt_float4{0, 0, 0, 0});
    for (int32_t i = 0; i < nref; ++i) {
        const int32_t tri1 = refs[i];
        const rt_float4 v0 = verts[idx[tri1]], v1 = verts[idx[tri1 + 1]], v2 = verts[idx[tri1 + 2]];
        float idf;
        std::memcpy(&idf, &tri1, 4);
        out.tris[(size_t)i * 3 + 0] = rt_float4{v0.x, v0.y, v0.z, idf};
        out.tris[(size_t)i * 3 + 1] = rt_float4{v1.x - v0.x, v1.y - v0.y, v1.z - v0.z, 0.0f};
        out.tris[(size_t)i * 3 + 2] = rt_float4{v2.x - v0.x, v2.y - v0.y, v2.z - v0.z, 0.0f};
    }
    // per-triangle shading records (volumeRender.cl:1306-1374)
    out.shade.assign((size_t)ntri * 7, rt_float4{0, 0, 0, 0});
    for (int32_t t = 0; t < ntri; ++t) {
        rt_float4* s = &out.shade[(size_t)t * 7];
        for (int k = 0; k < 3; ++k) {
            const rt_float4 v = verts[idx[3 * t + k]];
            const rt_float4 n = normals[normal_idx[3 * t + k]];
            s[k] = rt_float4{v.x, v.y, v.z, 0.0f};
            s[3 + k] = rt_float4{n.x, n.y, n.z, 0.0f};
        }
        const rt_float4 d = mats[tri_to_mat[t]].diffuse;
        s[6] = rt_float4{d.x, d.y, d.z, 0.0f};
    }
    if (out.leaf_table.empty()) out.leaf_table.push_back({0, 0});
    out.root = ref_of[0];
    out.n_inner = (uint32_t)n_inner;
    out.fast_div = fast_ok ? 1 : 0;
    out.clean = clean ? 1 : 0;
    return RT_OK;
}

bool derive_walk(const rt_float4* wnodes, size_t n_rec, const std::pair<int32_t, int32_t>* leaf_table, size_t n_leaf,
                 uint32_t tri_unit, uint32_t n_refs, uint32_t root, std::vector<uint32_t>& walk, uint32_t& walk_root) {
    static_assert(sizeof(std::pair<int32_t, int32_t>) == 8, "the escape table is {offset, count} pairs of int32");
    std::vector<int32_t> table(2 * n_leaf);
    for (size_t i = 0; i < n_leaf; ++i) {
        table[2 * i] = leaf_table[i].first;
        table[2 * i + 1] = leaf_table[i].second;
    }
    walk.assign(2 * n_rec, 0u);
    bool ok = true;
    for (size_t i = 0; i < n_rec; ++i) {
        uint32_t r[2];
        std::memcpy(r, &wnodes[4 * i + 3], 8);
        for (int k = 0; k < 2; ++k) {
            const uint32_t w = rtrec::walk_ref(r[k], table.data(), (uint32_t)n_leaf, (uint32_t)n_rec, tri_unit, n_refs);
            walk[2 * i + k] = w;
            ok = ok && w != rtrec::kWalkNone;
        }
    }
    walk_root = rtrec::walk_ref(root, table.data(), (uint32_t)n_leaf, (uint32_t)n_rec, tri_unit, n_refs);
    return ok && walk_root != rtrec::kWalkNone;
}

}  // namespace rtamd
