// multihit.cpp -- rt_trace_rays_k_host (include/rt_abi.h): the definition of a first-k-hits
// ray query in host code, in S_strict.  The caller's arrays go through rt_upload_scene's host encoding
// (scene_encode.cpp), so the traversal walks the records the device holds, and multihit_core.hpp is the
// text the kernels (multihit_kernel<K> of rt_kernel_body.inc) compile too.  The arithmetic is restated
// here for the host from rt_device_math.h's S_strict (RTK_MATH 0) and the division form of the slab test
// (slab2_div): every operation a single IEEE binary32 one, fmaf only where it is written, this unit
// compiled with -ffp-contract=off; rsqrt is (float)(1.0 / sqrt((double)x)).  No context, no GPU.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "multihit_core.hpp"
#include "rt_abi.h"
#include "scene_encode.hpp"

namespace {

constexpr int64_t kMaxRays = 1ll << 30;

struct V3 {
    float x, y, z;
};
inline V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator*(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
inline float dot(V3 a, V3 b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
inline V3 cross(V3 a, V3 b) {
    return V3{std::fmaf(a.y, b.z, b.y * -a.z), std::fmaf(a.z, b.x, b.z * -a.x), std::fmaf(a.x, b.y, b.x * -a.y)};
}
inline float rsqrt_s(float x) { return (float)(1.0 / std::sqrt((double)x)); }

// rt_device_math.h normalize
inline V3 normalize(V3 p) {
    constexpr float inf = std::numeric_limits<float>::infinity();
    if (p.x == 0.0f && p.y == 0.0f && p.z == 0.0f) return p;
    float l2 = dot(p, p);
    if (l2 < 1.17549435e-38f) {
        p = p * 0x1p86f;
        l2 = dot(p, p);
    } else if (l2 == inf) {
        p = p * 0x1p-66f;
        l2 = dot(p, p);
        if (l2 == inf) {
            p = V3{std::copysign(std::isinf(p.x) ? 1.0f : 0.0f, p.x), std::copysign(std::isinf(p.y) ? 1.0f : 0.0f, p.y),
                   std::copysign(std::isinf(p.z) ? 1.0f : 0.0f, p.z)};
            l2 = dot(p, p);
        }
    }
    return p * rsqrt_s(l2);
}

// rt_device_math.h ray_tri, and ray_tri_uv: its u and v by its own lines without its early-outs
inline float ray_tri(V3 o, V3 d, V3 v0, V3 e1, V3 e2) {
    const V3 tvec = o - v0;
    const V3 pvec = cross(d, e2);
    float det = dot(e1, pvec);
    det = 1.0f / det;
    const float u = dot(tvec, pvec) * det;
    if (u < 0.0f || u > 1.0f) return -1.0f;
    const V3 qvec = cross(tvec, e1);
    const float v = dot(d, qvec) * det;
    if (v < 0.0f || (u + v) > 1.0f) return -1.0f;
    return dot(e2, qvec) * det;
}
inline void ray_tri_uv(V3 o, V3 d, V3 v0, V3 e1, V3 e2, float& u, float& v) {
    const V3 tvec = o - v0;
    const V3 pvec = cross(d, e2);
    float det = dot(e1, pvec);
    det = 1.0f / det;
    u = dot(tvec, pvec) * det;
    const V3 qvec = cross(tvec, e1);
    v = dot(d, qvec) * det;
}

// rt_kernel_body.inc query_ray_ok
inline bool ray_ok(const rt_ray& r) {
    constexpr float inf = std::numeric_limits<float>::infinity();
    const bool fin = std::fabs(r.ox) < inf && std::fabs(r.oy) < inf && std::fabs(r.oz) < inf && std::fabs(r.dx) < inf &&
                     std::fabs(r.dy) < inf && std::fabs(r.dz) < inf;
    const bool zero = r.dx == 0.0f && r.dy == 0.0f && r.dz == 0.0f;
    return fin && !zero && r.tmax > multihit::kTmin;   // (false for a NaN tmax too)
}

// The adaptor of multihit_core.hpp: the encoded scene and one ray, o and the normalised d.
struct HostRayScene {
    const rtamd::EncodedScene& E;
    V3 o, d;
    // slab2_div: the IEEE quotient on every plane, the reference's nesting of min and max
    static void axis(const rt_float4& q, float o, float d, float lo[2], float hi[2]) {
        const float a0 = (q.x - o) / d, a1 = (q.y - o) / d, b0 = (q.z - o) / d, b1 = (q.w - o) / d;
        lo[0] = std::fmin(a0, b0);
        hi[0] = std::fmax(a0, b0);
        lo[1] = std::fmin(a1, b1);
        hi[1] = std::fmax(a1, b1);
    }
    void slab(uint32_t cur, float& n0, float& f0, float& n1, float& f1, uint32_t& r0, uint32_t& r1) const {
        const rt_float4* q = &E.wnodes[(size_t)cur * 4];   // axis-major: {L.min, R.min, L.max, R.max}
        float lx[2], hx[2], ly[2], hy[2], lz[2], hz[2];
        axis(q[0], o.x, d.x, lx, hx);
        axis(q[1], o.y, d.y, ly, hy);
        axis(q[2], o.z, d.z, lz, hz);
        n0 = std::fmax(std::fmax(lx[0], ly[0]), lz[0]);
        f0 = std::fmin(std::fmin(hx[0], hy[0]), hz[0]);
        n1 = std::fmax(std::fmax(lx[1], ly[1]), lz[1]);
        f1 = std::fmin(std::fmin(hx[1], hy[1]), hz[1]);
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
    void rec(int k, V3& p0, V3& e1, V3& e2, int32_t& id) const {
        const rt_float4* t = &E.tris[(size_t)k * 3];
        p0 = V3{t[0].x, t[0].y, t[0].z};
        e1 = V3{t[1].x, t[1].y, t[1].z};
        e2 = V3{t[2].x, t[2].y, t[2].z};
        std::memcpy(&id, &t[0].w, 4);
    }
    void tri_t(int k, float& t, int32_t& id) const {
        V3 p0, e1, e2;
        rec(k, p0, e1, e2, id);
        t = ray_tri(o, d, p0, e1, e2);
    }
};

struct HostStack {
    uint32_t* w;
    uint32_t get(int i) const { return w[i]; }
    void put(int i, uint32_t v) const { w[i] = v; }
};

template <int K>
void trace_all(const rtamd::EncodedScene& E, const rt_ray* rays, int64_t n, rt_hit_uv* out, uint64_t st3[3]) {
    uint32_t words[multihit::kStackSize];
    const HostStack st{words};
    for (int64_t i = 0; i < n; ++i) {
        const rt_ray& r = rays[i];
        const HostRayScene S{E, V3{r.ox, r.oy, r.oz}, normalize(V3{r.dx, r.dy, r.dz})};
        multihit::StateK<K> T;
        multihit::start(T, E.root, r.tmax);
        if (ray_ok(r))
            while (T.sc > 0) multihit::step<true>(T, S, st);
        for (int j = 0; j < K; ++j) {   // plane j
            rt_hit_uv h;
            h.id = -1;
            std::memcpy(&h.t, &r.tmax, 4);   // the miss record carries the ray's tmax word
            h.u = h.v = 0.0f;
            if (T.id[j] >= 0) {
                V3 p0, e1, e2;
                S.rec(T.at[j], p0, e1, e2, h.id);
                h.t = T.t[j];
                ray_tri_uv(S.o, S.d, p0, e1, e2, h.u, h.v);
            }
            std::memcpy(&out[(size_t)j * (size_t)n + (size_t)i], &h, sizeof h);
        }
        st3[0] += T.overflow ? 1u : 0u;
        st3[1] += T.inner_visits;
        st3[2] += T.tri_tests;
    }
}

}  // namespace

extern "C" int rt_trace_rays_k_host(const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx, const rt_bvh_node* nodes,
                                    int32_t nn, const int32_t* refs, int32_t nref, const rt_ray* rays, int64_t n, int32_t k,
                                    rt_hit_uv* out, uint64_t* stats3) {
    if (n < 0 || n > kMaxRays || k < 1 || k > RT_TRACE_MAX_K || n * k > kMaxRays) return RT_ERR_INVALID_ARG;
    if (!verts || nv <= 0 || !idx || nidx <= 0 || nidx % 3 || !nodes || nn <= 0 || nref < 0 || (!refs && nref > 0))
        return RT_ERR_INVALID_ARG;
    if (n > 0 && (!rays || !out)) return RT_ERR_INVALID_ARG;
    // the encoding wants shading arrays; this query reads none of them
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
        case 1: trace_all<1>(E, rays, n, out, st3); break;
        case 2: trace_all<2>(E, rays, n, out, st3); break;
        case 3: trace_all<3>(E, rays, n, out, st3); break;
        case 4: trace_all<4>(E, rays, n, out, st3); break;
        case 5: trace_all<5>(E, rays, n, out, st3); break;
        case 6: trace_all<6>(E, rays, n, out, st3); break;
        case 7: trace_all<7>(E, rays, n, out, st3); break;
        default: trace_all<8>(E, rays, n, out, st3); break;
    }
    if (stats3) std::memcpy(stats3, st3, sizeof st3);
    return RT_OK;
}
