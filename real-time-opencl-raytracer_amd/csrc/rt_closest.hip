// rt_closest.hip -- the kernel of rt_closest_points: for every point the nearest
// triangle of the scene as it stands on the GPU, its squared distance, barycentrics and the closest
// point, by a traversal of the inner records by point-to-box distance and Ericson's point-triangle
// test on the triangle reference records.  The arithmetic, the visit order and the acceptance rule
// are csrc/host/closest_core.hpp's, the text the host twin (rt_closest_points_host) runs: both
// compute the same words.
//
//   closest_kernel  a persistent grid; a wave takes 64 consecutive points by one cursor add (the ray
//                   queries' eight cursors), lane = point: one 16-B load in, two 16-B stores out.
//                   Lanes step independently: every trip of the loop a lane makes ONE step of its own
//                   sequence, an inner visit (three 16-B loads + one 8-B) or one triangle test (three
//                   16-B loads), as the fast ray traversal does; the sequence of each lane is the
//                   definition's, only the interleaving of lanes in time differs.
//                   The stack is one word per entry: entries 0 .. 15 in the lane's LDS column,
//                   deeper ones in the lane's global column, [entry][grid lane].
//   nearest_kernel<K>  rt_nearest_k: the same with a list of K answers, below.
// One kernel serves every scene: it addresses inner records, triangle records and the escape table
// by pointer, so split records, malformed nodes and escape leaves need no second instantiation.
#define CLOSEST_HD __host__ __device__ __forceinline__
#include "rt_closest.h"

#include "closest_core.hpp"

#ifndef RTK_CLOSEST_WAVES
#define RTK_CLOSEST_WAVES 8   // waves per SIMD the kernel is bounded to (no scratch: DESIGN.md 22)
#endif

namespace rtclosest {

namespace {

// waves per SIMD nearest_kernel<K> is bounded to: what its 54 .. 88 VGPRs allow without scratch
constexpr int nearest_waves(int k) { return k <= 3 ? 8 : k == 4 ? 7 : k <= 6 ? 6 : 5; }

using closest::V3;
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;

// rt_render.hip's grab_group: cursor c hands out the groups c, c + 8, c + 16, ...; a wave whose
// cursor is used up takes from the next one
__device__ __forceinline__ uint32_t grab_group(uint32_t* cursors, uint32_t ngroups, uint32_t& home) {
    uint32_t g = kNoGroup, h = home;
    if ((threadIdx.x & 63u) == 0) {
        for (uint32_t k = 0; k < kCursors; ++k) {
            const uint32_t c = (h + k) & (kCursors - 1u);
            const uint32_t gg = c + kCursors * atomicAdd(cursors + c * kCursorStride, 1u);
            if (gg < ngroups) {
                g = gg;
                h = c;
                break;
            }
        }
    }
    home = __builtin_amdgcn_readfirstlane(h);
    return __builtin_amdgcn_readfirstlane(g);
}

struct DevScene {
    const float4* __restrict__ wnodes;
    const float4* __restrict__ tris;
    const int2* __restrict__ leaf_table;
    __device__ __forceinline__ void inner(uint32_t id, V3& lo0, V3& hi0, V3& lo1, V3& hi1, uint32_t& r0, uint32_t& r1) const {
        const float4* np = wnodes + (size_t)id * 4;   // axis-major: {L.min, R.min, L.max, R.max}
        const float4 x = np[0], y = np[1], z = np[2];
        const float2 r = *(const float2*)(np + 3);
        lo0 = V3{x.x, y.x, z.x};
        lo1 = V3{x.y, y.y, z.y};
        hi0 = V3{x.z, y.z, z.z};
        hi1 = V3{x.w, y.w, z.w};
        r0 = __float_as_uint(r.x);
        r1 = __float_as_uint(r.y);
    }
    __device__ __forceinline__ void leaf(uint32_t ref, int& off, int& cnt) const {
        const uint32_t c = rtrec::ref_count(ref);
        if (c == rtrec::kCntEscape) {
            const int2 e = leaf_table[rtrec::ref_offset(ref)];
            off = e.x;
            cnt = e.y;
        } else {
            off = (int)rtrec::ref_offset(ref);
            cnt = (int)c;
        }
    }
    __device__ __forceinline__ void tri(int k, V3& p0, V3& e1, V3& e2, int32_t& id) const {
        const float4* tp = tris + (size_t)k * 3;
        const float4 a0 = tp[0], a1 = tp[1], a2 = tp[2];
        p0 = V3{a0.x, a0.y, a0.z};
        e1 = V3{a1.x, a1.y, a1.z};
        e2 = V3{a2.x, a2.y, a2.z};
        id = __float_as_int(a0.w);
    }
};

struct DevStack {
    uint32_t* lds;      // this lane's column: lds[i * 64]
    uint32_t* glb;      // this grid lane's column: glb[(i - kLdsStack) * gstride]
    uint64_t gstride;
    __device__ __forceinline__ uint32_t get(int i) const {
        return i < kLdsStack ? lds[i * 64] : glb[(uint64_t)(i - kLdsStack) * gstride];
    }
    __device__ __forceinline__ void put(int i, uint32_t v) const {
        if (i < kLdsStack) lds[i * 64] = v;
        else glb[(uint64_t)(i - kLdsStack) * gstride] = v;
    }
};

__global__ void __launch_bounds__(kThreads, RTK_CLOSEST_WAVES) closest_kernel(Scene Sc, Launch L) {
    __shared__ uint32_t s_stack[kThreads / 64][kLdsStack][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ngroups = (L.n + 63u) / 64u;
    uint32_t home = blockIdx.x & (kCursors - 1u);
    const DevScene S{Sc.wnodes, Sc.tris, Sc.leaf_table};
    DevStack st;
    st.lds = &s_stack[wave][0][lane];
    st.glb = L.gstack + ((size_t)blockIdx.x * kThreads + threadIdx.x);
    st.gstride = (uint64_t)gridDim.x * kThreads;   // the lanes launched
    for (;;) {
        const uint32_t g = grab_group(L.fetch, ngroups, home);
        if (g == kNoGroup) break;
        const uint32_t i = g * 64u + lane;
        const bool inside = i < L.n;   // (false only in the last group's tail)
        float4 pt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (inside) pt = L.pts[i];
        closest::State T;
        closest::start(T, Sc.root, pt.w);
        if (!(inside && closest::point_ok(pt.x, pt.y, pt.z, pt.w))) T.sc = 0;   // sits the traversal out
        const V3 q{pt.x, pt.y, pt.z};
        while (T.sc > 0) closest::step<false>(T, q, S, st);
        if (inside) {
            uint32_t w[8];
            closest::result_words(T, w);
            float4* o = L.out + (size_t)i * 2;
            o[0] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
            o[1] = make_float4(__uint_as_float(w[4]), __uint_as_float(w[5]), __uint_as_float(w[6]), __uint_as_float(w[7]));
        }
        if (T.overflow) atomicAdd(L.overflow, 1ull);
    }
}

// nearest_kernel<K>: rt_nearest_k, closest_kernel with closest_core.hpp's list of K
// entries in registers in place of the one answer.  An entry is (d2, id, triangle record): at the end a
// lane evaluates tri_point again for the entries it found and writes plane j of its point to
// out[j * n + i], every plane as closest_kernel writes its one.  One instantiation per K, so the list
// is indexed statically only.
template <int K>
__global__ void __launch_bounds__(kThreads, nearest_waves(K)) nearest_kernel(Scene Sc, Launch L) {
    __shared__ uint32_t s_stack[kThreads / 64][kLdsStack][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ngroups = (L.n + 63u) / 64u;
    uint32_t home = blockIdx.x & (kCursors - 1u);
    const DevScene S{Sc.wnodes, Sc.tris, Sc.leaf_table};
    DevStack st;
    st.lds = &s_stack[wave][0][lane];
    st.glb = L.gstack + ((size_t)blockIdx.x * kThreads + threadIdx.x);
    st.gstride = (uint64_t)gridDim.x * kThreads;
    for (;;) {
        const uint32_t g = grab_group(L.fetch, ngroups, home);
        if (g == kNoGroup) break;
        const uint32_t i = g * 64u + lane;
        const bool inside = i < L.n;
        float4 pt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (inside) pt = L.pts[i];
        closest::StateK<K> T;
        closest::start(T, Sc.root, pt.w);
        if (!(inside && closest::point_ok(pt.x, pt.y, pt.z, pt.w))) T.sc = 0;
        const V3 q{pt.x, pt.y, pt.z};
        while (T.sc > 0) closest::step<false>(T, q, S, st);
        if (inside) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                uint32_t w[8];
                closest::entry_words(T.id[j], T.at[j], q, S, w);
                float4* o = L.out + ((size_t)j * L.n + i) * 2;
                o[0] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
                o[1] = make_float4(__uint_as_float(w[4]), __uint_as_float(w[5]), __uint_as_float(w[6]), __uint_as_float(w[7]));
            }
        }
        if (T.overflow) atomicAdd(L.overflow, 1ull);
    }
}

typedef void (*NearestKernel)(Scene, Launch);
const NearestKernel kNearest[closest::kMaxK] = {nearest_kernel<1>, nearest_kernel<2>, nearest_kernel<3>, nearest_kernel<4>,
                                                nearest_kernel<5>, nearest_kernel<6>, nearest_kernel<7>, nearest_kernel<8>};

}  // namespace

const void* kernel(int k) { return k ? (const void*)kNearest[k - 1] : (const void*)closest_kernel; }

hipError_t launch(const Scene& S, const Launch& L, int k, uint32_t grid, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    Scene sc = S;
    Launch la = L;
    void* args[] = {&sc, &la};
    const hipError_t e = hipExtLaunchKernel(kernel(k), dim3(grid), dim3(kThreads), args, 0, s, start, stop, 0);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace rtclosest
