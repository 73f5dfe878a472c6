// closest_points.cpp -- rt_closest_points_host (include/rt_abi.h): the definition of a
// closest-point query in host code.  The caller's arrays go through rt_upload_scene's host encoding
// (scene_encode.cpp), so the traversal walks the records the device holds, and closest_core.hpp is
// the text the kernel (rt_closest.hip) compiles too.  No context, no GPU.  rt_nearest_k_host,
// the k nearest triangles per point, follows it.
#include <cstring>
#include <string>
#include <vector>

#include "closest_core.hpp"
#include "rt_abi.h"
#include "scene_encode.hpp"

namespace {

constexpr int64_t kMaxPoints = 1ll << 30;

struct HostScene {
    const rtamd::EncodedScene& E;
    void inner(uint32_t id, closest::V3& lo0, closest::V3& hi0, closest::V3& lo1, closest::V3& hi1, uint32_t& r0,
               uint32_t& r1) const {
        const rt_float4* q = &E.wnodes[(size_t)id * 4];   // axis-major: {L.min, R.min, L.max, R.max}
        lo0 = closest::V3{q[0].x, q[1].x, q[2].x};
        lo1 = closest::V3{q[0].y, q[1].y, q[2].y};
        hi0 = closest::V3{q[0].z, q[1].z, q[2].z};
        hi1 = closest::V3{q[0].w, q[1].w, q[2].w};
        std::memcpy(&r0, &q[3].x, 4);
        std::memcpy(&r1, &q[3].y, 4);
    }
    void leaf(uint32_t ref, int& off, int& cnt) const {
        const uint32_t c = rtrec::ref_count(ref);
        if (c == rtrec::kCntEscape) {
            const auto& e = E.leaf_table[rtrec::ref_offset(ref)];
            off = e.first;
            cnt = e.second;
        } else {
            off = (int)rtrec::ref_offset(ref);
            cnt = (int)c;
        }
    }
    void tri(int k, closest::V3& p0, closest::V3& e1, closest::V3& e2, int32_t& id) const {
        const rt_float4* t = &E.tris[(size_t)k * 3];
        p0 = closest::V3{t[0].x, t[0].y, t[0].z};
        e1 = closest::V3{t[1].x, t[1].y, t[1].z};
        e2 = closest::V3{t[2].x, t[2].y, t[2].z};
        std::memcpy(&id, &t[0].w, 4);
    }
};

struct HostStack {
    uint32_t* w;
    uint32_t get(int i) const { return w[i]; }
    void put(int i, uint32_t v) const { w[i] = v; }
};

}  // namespace

extern "C" int rt_closest_points_host(const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx,
                                      const rt_bvh_node* nodes, int32_t nn, const int32_t* refs, int32_t nref,
                                      const rt_point* pts, int64_t n, rt_closest* out, uint64_t* stats3) {
    if (n < 0 || n > kMaxPoints) return RT_ERR_INVALID_ARG;
    if (!verts || nv <= 0 || !idx || nidx <= 0 || nidx % 3 || !nodes || nn <= 0 || nref < 0 || (!refs && nref > 0))
        return RT_ERR_INVALID_ARG;
    if (n > 0 && (!pts || !out)) return RT_ERR_INVALID_ARG;
    // the encoding wants shading arrays; a point query reads none of them
    const rt_float4 normal{0.0f, 0.0f, 1.0f, 0.0f};
    const rt_material mat{};
    const std::vector<int32_t> zeros((size_t)nidx, 0);
    rtamd::EncodedScene E;
    std::string err;
    const int rc = rtamd::encode_scene(verts, nv, idx, nidx, nodes, nn, refs, nref, &normal, 1, zeros.data(), &mat, 1,
                                       zeros.data(), E, err);
    if (rc != RT_OK) return rc;
    const HostScene S{E};
    uint32_t words[closest::kStackSize];
    const HostStack st{words};
    uint64_t overflows = 0, inner_visits = 0, tri_tests = 0;
    for (int64_t i = 0; i < n; ++i) {
        const rt_point& p = pts[i];
        closest::State T;
        closest::start(T, E.root, p.r);
        if (closest::point_ok(p.x, p.y, p.z, p.r)) {
            const closest::V3 q{p.x, p.y, p.z};
            while (T.sc > 0) closest::step<true>(T, q, S, st);
        }
        uint32_t w[8];
        closest::result_words(T, w);
        std::memcpy(&out[i], w, sizeof(rt_closest));
        overflows += T.overflow ? 1u : 0u;
        inner_visits += T.inner_visits;
        tri_tests += T.tri_tests;
    }
    if (stats3) {
        stats3[0] = overflows;
        stats3[1] = inner_visits;
        stats3[2] = tri_tests;
    }
    return RT_OK;
}

// ---- rt_nearest_k_host: the same with closest_core.hpp's list of K entries ----
namespace {

template <int K>
void nearest_all(const rtamd::EncodedScene& E, const rt_point* pts, int64_t n, rt_closest* out, uint64_t st3[3]) {
    const HostScene S{E};
    uint32_t words[closest::kStackSize];
    const HostStack st{words};
    for (int64_t i = 0; i < n; ++i) {
        const rt_point& p = pts[i];
        closest::StateK<K> T;
        closest::start(T, E.root, p.r);
        const closest::V3 q{p.x, p.y, p.z};
        if (closest::point_ok(p.x, p.y, p.z, p.r))
            while (T.sc > 0) closest::step<true>(T, q, S, st);
        for (int j = 0; j < K; ++j) {   // plane j
            uint32_t w[8];
            closest::entry_words(T.id[j], T.at[j], q, S, w);
            std::memcpy(&out[(size_t)j * (size_t)n + (size_t)i], w, sizeof(rt_closest));
        }
        st3[0] += T.overflow ? 1u : 0u;
        st3[1] += T.inner_visits;
        st3[2] += T.tri_tests;
    }
}

}  // namespace

extern "C" int rt_nearest_k_host(const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx,
                                 const rt_bvh_node* nodes, int32_t nn, const int32_t* refs, int32_t nref, const rt_point* pts,
                                 int64_t n, int32_t k, rt_closest* out, uint64_t* stats3) {
    if (n < 0 || n > kMaxPoints || k < 1 || k > RT_NEAREST_MAX_K || n * k > kMaxPoints) return RT_ERR_INVALID_ARG;
    if (!verts || nv <= 0 || !idx || nidx <= 0 || nidx % 3 || !nodes || nn <= 0 || nref < 0 || (!refs && nref > 0))
        return RT_ERR_INVALID_ARG;
    if (n > 0 && (!pts || !out)) return RT_ERR_INVALID_ARG;
    const rt_float4 normal{0.0f, 0.0f, 1.0f, 0.0f};
    const rt_material mat{};
    const std::vector<int32_t> zeros((size_t)nidx, 0);
    rtamd::EncodedScene E;
    std::string err;
    const int rc = rtamd::encode_scene(verts, nv, idx, nidx, nodes, nn, refs, nref, &normal, 1, zeros.data(), &mat, 1,
                                       zeros.data(), E, err);
    if (rc != RT_OK) return rc;
    uint64_t st3[3] = {0, 0, 0};
    switch (k) {
        case 1: nearest_all<1>(E, pts, n, out, st3); break;
        case 2: nearest_all<2>(E, pts, n, out, st3); break;
        case 3: nearest_all<3>(E, pts, n, out, st3); break;
        case 4: nearest_all<4>(E, pts, n, out, st3); break;
        case 5: nearest_all<5>(E, pts, n, out, st3); break;
        case 6: nearest_all<6>(E, pts, n, out, st3); break;
        case 7: nearest_all<7>(E, pts, n, out, st3); break;
        default: nearest_all<8>(E, pts, n, out, st3); break;
    }
    if (stats3) std::memcpy(stats3, st3, sizeof st3);
    return RT_OK;
}
