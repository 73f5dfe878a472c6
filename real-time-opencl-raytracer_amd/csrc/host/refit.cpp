// refit.cpp -- BVH refit: the plan (refittability + bottom-up order) and the CPU refit
// rt_refit_nodes (include/rt_abi.h).  The device path (rt_update_vertices, rt_refit.hip) walks
// the same plan and computes the same boxes; this file is its restatement on the host.
//
// Semantics: a leaf with num_tris > 0 takes, per axis, the min / max over the
// three vertices of every triangle of its range (the whole triangle, also where an SBVH leaf
// held a clipped reference: conservative); a leaf with num_tris <= 0 keeps its box; an inner
// node takes the union of its children's boxes.  fminf / fmaxf: a NaN operand is ignored.
// Only min.xyz / max.xyz of reachable nodes are written.
#include "refit.hpp"

#include <algorithm>
#include <cmath>

namespace rtrefit {

namespace {
std::string g_refit_err;

inline bool is_inner(const rt_bvh_node& nd) { return nd.offset_left >= 0; }
}  // namespace

const std::string& last_error() { return g_refit_err; }
void clear_error() { g_refit_err.clear(); }

int plan_build(const rt_bvh_node* nodes, int32_t nn, int32_t nref, const int32_t* inner_id, Plan& plan,
               std::string& err) {
    plan = Plan{};
    if (!nodes || nn <= 0 || nref < 0) { err = "refit: no nodes"; return RT_ERR_INVALID_ARG; }
    std::vector<uint8_t> seen((size_t)nn, 0);
    std::vector<int32_t>& order = plan.order;
    std::vector<int32_t> stk;
    stk.push_back(0);
    seen[0] = 1;
    while (!stk.empty()) {
        const int32_t n = stk.back();
        stk.pop_back();
        order.push_back(n);
        const rt_bvh_node& nd = nodes[n];
        if (is_inner(nd)) {
            if (nd.offset_right < 0 || nd.offset_left >= nn || nd.offset_right >= nn) {
                err = "refit: node " + std::to_string(n) + " is a malformed inner node (child out of range)";
                return RT_ERR_BAD_SCENE;
            }
            // right pushed first: the left subtree comes first in `order` (pre-order)
            for (int32_t ch : {nd.offset_right, nd.offset_left}) {
                if (seen[ch]) {   // a shared node, or a cycle: some node is reached twice
                    err = "refit: node " + std::to_string(ch) + " has more than one parent";
                    return RT_ERR_BAD_SCENE;
                }
                seen[ch] = 1;
                stk.push_back(ch);
            }
        } else if (nd.num_tris > 0 && (nd.offset_tris < 0 || (int64_t)nd.offset_tris + nd.num_tris > nref)) {
            err = "refit: leaf " + std::to_string(n) + " has a triangle range out of bounds";
            return RT_ERR_BAD_SCENE;
        }
    }
    // heights bottom-up: in a tree every child comes after its parent in pre-order
    std::vector<uint32_t> height((size_t)nn, 0);
    uint32_t top = 0;
    for (size_t i = order.size(); i-- > 0;) {
        const rt_bvh_node& nd = nodes[order[i]];
        if (!is_inner(nd)) continue;
        const uint32_t h = 1u + std::max(height[nd.offset_left], height[nd.offset_right]);
        height[order[i]] = h;
        top = std::max(top, h);
    }
    plan.level_begin.assign((size_t)top + 1, 0);
    for (int32_t n : order)
        if (is_inner(nodes[n])) ++plan.level_begin[height[n]];
    uint32_t sum = 0;   // counts per height -> start offsets (level_begin[h-1] = start of height h)
    for (uint32_t h = 1; h <= top; ++h) {
        const uint32_t cnt = plan.level_begin[h];
        plan.level_begin[h - 1] = sum;
        sum += cnt;
    }
    plan.level_begin[top] = sum;
    plan.ids.resize(sum);
    std::vector<uint32_t> cursor(plan.level_begin.begin(), plan.level_begin.end());
    for (int32_t n : order)
        if (is_inner(nodes[n])) plan.ids[cursor[height[n] - 1]++] = (uint32_t)(inner_id ? inner_id[n] : n);
    return RT_OK;
}

}  // namespace rtrefit

extern "C" int rt_refit_nodes(const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx, rt_bvh_node* nodes,
                              int32_t nn, const int32_t* refs, int32_t nref) {
    std::string& err = rtrefit::g_refit_err;
    err.clear();
    if (!verts || nv <= 0 || !idx || nidx <= 0 || nidx % 3 || !nodes || nn <= 0 || nref < 0 || (!refs && nref > 0)) {
        err = "rt_refit_nodes: missing or empty array";
        return RT_ERR_INVALID_ARG;
    }
    for (int32_t i = 0; i < nidx; ++i)
        if (idx[i] < 0 || idx[i] >= nv) { err = "rt_refit_nodes: mesh_indices out of range"; return RT_ERR_BAD_SCENE; }
    for (int32_t i = 0; i < nref; ++i)
        if (refs[i] < 0 || refs[i] % 3 != 0 || refs[i] + 2 >= nidx) {
            err = "rt_refit_nodes: bvh_tris_indices entry out of range";
            return RT_ERR_BAD_SCENE;
        }
    rtrefit::Plan plan;
    const int rc = rtrefit::plan_build(nodes, nn, nref, nullptr, plan, err);
    if (rc != RT_OK) return rc;   // nothing written so far
    for (size_t i = plan.order.size(); i-- > 0;) {   // children before parents
        rt_bvh_node& nd = nodes[plan.order[i]];
        if (nd.offset_left >= 0) {
            const rt_bvh_node& L = nodes[nd.offset_left];
            const rt_bvh_node& R = nodes[nd.offset_right];
            nd.min.x = fminf(L.min.x, R.min.x); nd.min.y = fminf(L.min.y, R.min.y); nd.min.z = fminf(L.min.z, R.min.z);
            nd.max.x = fmaxf(L.max.x, R.max.x); nd.max.y = fmaxf(L.max.y, R.max.y); nd.max.z = fmaxf(L.max.z, R.max.z);
        } else if (nd.num_tris > 0) {
            float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
            bool first = true;
            for (int32_t r = nd.offset_tris; r < nd.offset_tris + nd.num_tris; ++r)
                for (int k = 0; k < 3; ++k) {
                    const rt_float4& v = verts[idx[refs[r] + k]];
                    const float p[3] = {v.x, v.y, v.z};
                    for (int a = 0; a < 3; ++a) {
                        mn[a] = first ? p[a] : fminf(mn[a], p[a]);
                        mx[a] = first ? p[a] : fmaxf(mx[a], p[a]);
                    }
                    first = false;
                }
            nd.min.x = mn[0]; nd.min.y = mn[1]; nd.min.z = mn[2];
            nd.max.x = mx[0]; nd.max.y = mx[1]; nd.max.z = mx[2];
        }
    }
    return RT_OK;
}
