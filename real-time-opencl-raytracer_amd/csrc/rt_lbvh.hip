// rt_lbvh.hip -- the kernels of rt_build_bvh: a linear BVH built on the GPU, byte
// for byte the arrays of the host twin (csrc/host/lbvh_builder.cpp).
//
//   tri_kernel      per triangle: index check, box, c2 = lo + hi; block min / max of c2
//   bounds_kernel   one workgroup: cmin / cmax from the blocks' partial results
//   key_kernel      cells -> morton39 << 25 | triangle, the bits laid out by the key plan the host
//                   made from cmin / cmax (per-axis, or the extent-aware plan of DESIGN.md 17)
//   (rocprim)       device radix sort of the 64-bit keys
//   radix_kernel    one thread per radix node (Karras 2012): range, split, each inner child's
//                   parent, kept flag, where leaves start; tri_indices
//   (rocprim)       one exclusive scan over {kept, leaf start} gives every output index
//   emit_kernel     per kept node: its child words, its leaf children whole (box included), its
//                   depth by a read-only walk up the parent links
//   bucket_kernel   kept nodes grouped by depth
//   fit_level / fit_top   inner boxes bottom-up, ONE LAUNCH PER DEPTH from the deepest upwards
//                   (runs of short depths in one single-workgroup launch, __syncthreads() between
//                   depths).  A parent reads boxes an EARLIER launch wrote: the per-XCD L2s are not
//                   coherent and a CU's L1 is not refreshed by another CU's stores, so nothing is
//                   handed from workgroup to workgroup inside a kernel (as rt_refit.hip).
// Node words are written as whole float4s (a node = 3 of them), vertices gathered as float4s.
#include "rt_lbvh.h"

#include <cstring>   // (rocprim's iterator headers call memset on the host)

#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "lbvh_core.hpp"
#include "rt_abi.h"

namespace rtlbvh {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTopMax = 1024;     // depths with at most this many kept nodes run in the top kernel
constexpr int kDepths = 65;            // a kept node's depth is below 64 (64-bit unique keys)
// control words
constexpr int kBad = 0, kKept = 1, kCmin = 8, kCmax = 12, kHist = 16, kCursor = 96, kCtlWords = 192;

struct Levels { uint32_t begin[kDepths + 1]; };

__global__ void __launch_bounds__(kThreads) tri_kernel(const float4* verts, int32_t nv, const int32_t* idx, int32_t n,
                                                       float4* c2, float4* part, uint32_t* ctl) {
    __shared__ float smn[3][kThreads], smx[3][kThreads];
    const uint32_t tid = threadIdx.x;
    const int32_t t = (int32_t)(blockIdx.x * kThreads + tid);
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (t < n) {
        const int32_t i0 = idx[3 * (size_t)t], i1 = idx[3 * (size_t)t + 1], i2 = idx[3 * (size_t)t + 2];
        const bool ok = (uint32_t)i0 < (uint32_t)nv && (uint32_t)i1 < (uint32_t)nv && (uint32_t)i2 < (uint32_t)nv;
        if (!ok) {
            ctl[kBad] = 1u;   // the host stops after this stage; no vertex is read through a bad index
        } else {
            const float4 v0 = verts[i0], v1 = verts[i1], v2 = verts[i2];
            const float p[3][3] = {{v0.x, v0.y, v0.z}, {v1.x, v1.y, v1.z}, {v2.x, v2.y, v2.z}};
            for (int a = 0; a < 3; ++a) {
                const float lo = fminf(fminf(p[0][a], p[1][a]), p[2][a]);
                const float hi = fmaxf(fmaxf(p[0][a], p[1][a]), p[2][a]);
                mn[a] = mx[a] = lo + hi;
            }
            c2[t] = make_float4(mn[0], mn[1], mn[2], 0.0f);
        }
    }
    for (int a = 0; a < 3; ++a) { smn[a][tid] = mn[a]; smx[a][tid] = mx[a]; }
    __syncthreads();
    for (uint32_t w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int a = 0; a < 3; ++a) {
                smn[a][tid] = fminf(smn[a][tid], smn[a][tid + w]);
                smx[a][tid] = fmaxf(smx[a][tid], smx[a][tid + w]);
            }
        __syncthreads();
    }
    if (tid == 0) {
        part[2 * (size_t)blockIdx.x] = make_float4(smn[0][0], smn[1][0], smn[2][0], 0.0f);
        part[2 * (size_t)blockIdx.x + 1] = make_float4(smx[0][0], smx[1][0], smx[2][0], 0.0f);
    }
}

__global__ void __launch_bounds__(kThreads) bounds_kernel(const float4* part, uint32_t nblocks, uint32_t* ctl) {
    __shared__ float smn[3][kThreads], smx[3][kThreads];
    const uint32_t tid = threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t b = tid; b < nblocks; b += kThreads) {
        const float4 lo = part[2 * (size_t)b], hi = part[2 * (size_t)b + 1];
        mn[0] = fminf(mn[0], lo.x); mn[1] = fminf(mn[1], lo.y); mn[2] = fminf(mn[2], lo.z);
        mx[0] = fmaxf(mx[0], hi.x); mx[1] = fmaxf(mx[1], hi.y); mx[2] = fmaxf(mx[2], hi.z);
    }
    for (int a = 0; a < 3; ++a) { smn[a][tid] = mn[a]; smx[a][tid] = mx[a]; }
    __syncthreads();
    for (uint32_t w = kThreads / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int a = 0; a < 3; ++a) {
                smn[a][tid] = fminf(smn[a][tid], smn[a][tid + w]);
                smx[a][tid] = fmaxf(smx[a][tid], smx[a][tid + w]);
            }
        __syncthreads();
    }
    if (tid < 3) {
        ctl[kCmin + tid] = __float_as_uint(smn[tid][0]);
        ctl[kCmax + tid] = __float_as_uint(smx[tid][0]);
    }
}

__global__ void __launch_bounds__(kThreads) key_kernel(const float4* c2, int32_t n, const uint32_t* ctl, lbvh::KeyPlan plan,
                                                       uint64_t* keys) {
    const int32_t t = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (t >= n) return;
    const float4 c4 = c2[t];
    const float c[3] = {c4.x, c4.y, c4.z};
    const float* cmin = reinterpret_cast<const float*>(ctl + kCmin);
    const float* cmax = reinterpret_cast<const float*>(ctl + kCmax);
    keys[t] = lbvh::key_of(plan, c, cmin, cmax, (uint32_t)t);
}

__device__ __forceinline__ bool kept(int32_t lo, int32_t hi, int32_t max_leaf) { return hi - lo + 1 > max_leaf; }

// flags: per position two 32-bit words, {a leaf starts here, radix node of this number is kept}
// (one 64-bit word to the scan); zeroed before the launch, only ones are stored.
__global__ void __launch_bounds__(kThreads) radix_kernel(const uint64_t* keys, int32_t n, int32_t max_leaf, int4* radix,
                                                         int32_t* parent, uint32_t* flags, int32_t* refs) {
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    refs[i] = 3 * (int32_t)(keys[i] & lbvh::kIndexMask);
    if (i == 0) parent[0] = -1;
    if (i >= n - 1) return;
    int32_t a, b, s;
    lbvh::node(keys, n, i, a, b, s);
    radix[i] = make_int4(a, b, s, 0);
    if (s > a) parent[s] = i;           // an inner left child is node s
    if (s + 1 < b) parent[s + 1] = i;   // an inner right child is node s + 1
    if (!kept(a, b, max_leaf)) return;
    flags[2 * (size_t)i + 1] = 1u;
    if (!kept(a, s, max_leaf)) flags[2 * (size_t)a] = 1u;
    if (!kept(s + 1, b, max_leaf)) flags[2 * (size_t)(s + 1)] = 1u;
}

// One leaf node, whole: box over its triangles' vertices, then the leaf words.
__device__ __forceinline__ void write_leaf(float4* nodes, int32_t id, int32_t first, int32_t count, const uint64_t* keys,
                                           const float4* verts, const int32_t* idx) {
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    bool is_first = true;
    for (int32_t p = first; p < first + count; ++p) {
        const size_t tri1 = 3 * (size_t)(keys[p] & lbvh::kIndexMask);
        for (int k = 0; k < 3; ++k) {
            const float4 v = verts[idx[tri1 + k]];
            const float q[3] = {v.x, v.y, v.z};
            for (int a = 0; a < 3; ++a) {
                mn[a] = is_first ? q[a] : fminf(mn[a], q[a]);
                mx[a] = is_first ? q[a] : fmaxf(mx[a], q[a]);
            }
            is_first = false;
        }
    }
    float4* nd = nodes + 3 * (size_t)id;
    nd[0] = make_float4(mn[0], mn[1], mn[2], 1.0f);
    nd[1] = make_float4(mx[0], mx[1], mx[2], 1.0f);
    nd[2] = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(first), __int_as_float(count));
}

// One kept radix node i (a thread of emit_kernel).
__device__ __forceinline__ void emit_node(int32_t i, const int4* radix, const int32_t* parent, const uint64_t* ranks,
                                          int32_t n, int32_t max_leaf, const uint64_t* keys, const float4* verts,
                                          const int32_t* idx, float4* nodes, int32_t node_cap, uint32_t* depth, uint32_t* ctl,
                                          uint32_t* hist) {
    const int32_t K = (int32_t)(ranks[n - 1] >> 32);   // position n - 1 is no radix node: the sum of all kept flags
    if (i == 0) ctl[kKept] = (uint32_t)K;
    const int4 r = radix[i];
    if (!kept(r.x, r.y, max_leaf)) return;
    const int32_t id = (int32_t)(ranks[i] >> 32);
    const int32_t lo[2] = {r.x, r.z + 1}, hi[2] = {r.z, r.y};
    int32_t child[2];
    for (int c = 0; c < 2; ++c) {
        if (kept(lo[c], hi[c], max_leaf)) {
            child[c] = (int32_t)(ranks[c ? r.z + 1 : r.z] >> 32);
        } else {
            child[c] = K + (int32_t)(ranks[lo[c]] & 0xFFFFFFFFull);
            if (child[c] < node_cap) write_leaf(nodes, child[c], lo[c], hi[c] - lo[c] + 1, keys, verts, idx);
        }
    }
    if (id >= node_cap || child[0] >= node_cap || child[1] >= node_cap) { ctl[kBad] = 2u; return; }   // (cannot happen: 2K + 1 <= 2n - 1)
    nodes[3 * (size_t)id + 2] = make_float4(__int_as_float(child[0]), __int_as_float(child[1]), __int_as_float(-1),
                                            __int_as_float(0));
    uint32_t d = 0;
    for (int32_t j = parent[i]; j >= 0 && d < (uint32_t)kDepths - 1; j = parent[j]) ++d;
    depth[id] = d;
    atomicAdd(&hist[d], 1u);
}

__global__ void __launch_bounds__(kThreads) emit_kernel(const int4* radix, const int32_t* parent, const uint64_t* ranks,
                                                        int32_t n, int32_t max_leaf, const uint64_t* keys,
                                                        const float4* verts, const int32_t* idx, float4* nodes,
                                                        int32_t node_cap, uint32_t* depth, uint32_t* ctl) {
    // depth counts: gathered per block in LDS, one global add per depth and block (a million
    // adds to some forty words would queue up at the L2)
    __shared__ uint32_t hist[kDepths];
    if (threadIdx.x < (uint32_t)kDepths) hist[threadIdx.x] = 0u;
    __syncthreads();
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i < n - 1) emit_node(i, radix, parent, ranks, n, max_leaf, keys, verts, idx, nodes, node_cap, depth, ctl, hist);
    __syncthreads();
    if (threadIdx.x < (uint32_t)kDepths && hist[threadIdx.x]) atomicAdd(&ctl[kHist + threadIdx.x], hist[threadIdx.x]);
}

// n <= max_leaf: the root is not kept, the tree is one leaf
__global__ void rootleaf_kernel(const uint64_t* keys, int32_t n, const float4* verts, const int32_t* idx, float4* nodes,
                                int32_t* refs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int32_t p = 0; p < n; ++p) refs[p] = 3 * (int32_t)(keys[p] & lbvh::kIndexMask);
    write_leaf(nodes, 0, 0, n, keys, verts, idx);
}

// order inside a depth's list does not matter: every node is written by the thread that draws it
__global__ void __launch_bounds__(kThreads) bucket_kernel(const uint32_t* depth, uint32_t K, Levels lv, uint32_t* ctl,
                                                          uint32_t* level_ids) {
    // a block counts its nodes per depth in LDS and draws one run of slots per depth
    __shared__ uint32_t cnt[kDepths], base[kDepths];
    const uint32_t tid = threadIdx.x;
    if (tid < (uint32_t)kDepths) cnt[tid] = 0u;
    __syncthreads();
    const uint32_t id = blockIdx.x * kThreads + tid;
    uint32_t d = 0, local = 0;
    if (id < K) {
        d = min(depth[id], (uint32_t)kDepths - 1);
        local = atomicAdd(&cnt[d], 1u);
    }
    __syncthreads();
    if (tid < (uint32_t)kDepths && cnt[tid]) base[tid] = atomicAdd(&ctl[kCursor + tid], cnt[tid]);
    __syncthreads();
    if (id >= K) return;
    const uint32_t slot = lv.begin[d] + base[d] + local;
    if (slot < lv.begin[d + 1]) level_ids[slot] = id;
}

// K kept nodes, 2K + 1 nodes in all: an id outside them (there is none) is never followed
__device__ __forceinline__ void fit_node(float4* nodes, uint32_t K, uint32_t id) {
    if (id >= K) return;
    float4* nd = nodes + 3 * (size_t)id;
    const float4 w = nd[2];
    const uint32_t l = (uint32_t)__float_as_int(w.x), r = (uint32_t)__float_as_int(w.y);
    if (l > 2 * K || r > 2 * K) return;
    const float4* L = nodes + 3 * (size_t)l;
    const float4* R = nodes + 3 * (size_t)r;
    const float4 lmn = L[0], lmx = L[1], rmn = R[0], rmx = R[1];
    nd[0] = make_float4(fminf(lmn.x, rmn.x), fminf(lmn.y, rmn.y), fminf(lmn.z, rmn.z), 1.0f);
    nd[1] = make_float4(fmaxf(lmx.x, rmx.x), fmaxf(lmx.y, rmx.y), fmaxf(lmx.z, rmx.z), 1.0f);
}

// one depth whose list is long; its children are deeper: leaves (emit_kernel) or earlier launches
__global__ void __launch_bounds__(kThreads) fit_level_kernel(float4* nodes, uint32_t K, const uint32_t* level_ids,
                                                             uint32_t first, uint32_t count) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < count) fit_node(nodes, K, level_ids[first + t]);
}

// depths d_hi, d_hi - 1, ..., d_lo (short lists) in ONE workgroup: its waves share a CU and its
// L1, so __syncthreads() orders a depth's stores before the next depth's loads
__global__ void __launch_bounds__(kThreads) fit_top_kernel(float4* nodes, uint32_t K, const uint32_t* level_ids, Levels lv,
                                                           int d_hi, int d_lo) {
    for (int d = d_hi; d >= d_lo; --d) {
        for (uint32_t t = lv.begin[d] + threadIdx.x; t < lv.begin[d + 1]; t += kThreads) fit_node(nodes, K, level_ids[t]);
        __syncthreads();
    }
}

inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

}  // namespace

hipError_t reserve(Scratch::Buf& b, size_t bytes) {
    if (b.p && bytes <= b.bytes) return hipSuccess;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    const size_t want = std::max<size_t>(bytes, 256);
    const hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { b.p = nullptr; return e; }
    b.bytes = want;
    return hipSuccess;
}

void release(Scratch& s) {
    for (Scratch::Buf* b : {&s.c2, &s.part, &s.keys[0], &s.keys[1], &s.sort_tmp, &s.radix, &s.parent, &s.flags, &s.ranks,
                            &s.scan_tmp, &s.depth, &s.level_ids, &s.ctl, &s.verts, &s.idx, &s.nodes, &s.refs}) {
        if (b->p) (void)hipFree(b->p);
        *b = Scratch::Buf{};
    }
    for (hipEvent_t& e : s.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    s.timed = false;
}

#define LB_HIP(expr)                                                                 \
    do {                                                                             \
        const hipError_t e__ = (expr);                                               \
        if (e__ != hipSuccess) {                                                     \
            err = std::string(#expr) + ": " + hipGetErrorString(e__);                \
            return e__ == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_DEVICE; \
        }                                                                            \
    } while (0)

int build(Scratch& S, hipStream_t s, const float4* d_verts, int32_t nv, const int32_t* d_idx, int32_t n, int32_t max_leaf,
          bool extent_keys, float4* d_nodes, int32_t node_cap, int32_t* d_refs, int32_t* num_nodes, std::string& err) {
    const size_t N = (size_t)n;
    const uint32_t tri_blocks = grid_for(N).x;
    size_t sort_bytes = 0, scan_bytes = 0;
    LB_HIP(rocprim::radix_sort_keys(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, N, 0u, 64u, s));
    LB_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, N,
                                   rocprim::plus<uint64_t>(), s));
    LB_HIP(reserve(S.c2, N * sizeof(float4)));
    LB_HIP(reserve(S.part, 2 * (size_t)tri_blocks * sizeof(float4)));
    LB_HIP(reserve(S.keys[0], N * 8));
    LB_HIP(reserve(S.keys[1], N * 8));
    LB_HIP(reserve(S.sort_tmp, sort_bytes));
    LB_HIP(reserve(S.radix, N * sizeof(int4)));
    LB_HIP(reserve(S.parent, N * 4));
    LB_HIP(reserve(S.flags, N * 8));
    LB_HIP(reserve(S.ranks, N * 8));
    LB_HIP(reserve(S.scan_tmp, scan_bytes));
    LB_HIP(reserve(S.depth, N * 4));
    LB_HIP(reserve(S.level_ids, N * 4));
    LB_HIP(reserve(S.ctl, kCtlWords * 4));
    float4* c2 = (float4*)S.c2.p;
    uint64_t *keys_in = (uint64_t*)S.keys[0].p, *keys = (uint64_t*)S.keys[1].p;
    uint32_t* ctl = (uint32_t*)S.ctl.p;
    uint32_t launches = 0;

    LB_HIP(hipMemsetAsync(ctl, 0, kCtlWords * 4, s));
    hipLaunchKernelGGL(tri_kernel, dim3(tri_blocks), dim3(kThreads), 0, s, d_verts, nv, d_idx, n, c2, (float4*)S.part.p, ctl);
    hipLaunchKernelGGL(bounds_kernel, dim3(1), dim3(kThreads), 0, s, (const float4*)S.part.p, tri_blocks, ctl);
    launches += 2;
    LB_HIP(hipGetLastError());
    uint32_t h_ctl[kCtlWords] = {};
    LB_HIP(hipMemcpyAsync(h_ctl, ctl, kHist * sizeof(uint32_t), hipMemcpyDeviceToHost, s));   // the flag, cmin, cmax
    LB_HIP(hipStreamSynchronize(s));
    if (h_ctl[kBad]) { err = "mesh_indices out of range"; return RT_ERR_BAD_SCENE; }
    lbvh::KeyPlan plan = lbvh::axis_plan();
    if (extent_keys) {   // every float decision of the plan is the host's, as in the twin
        float cmin[3], cmax[3];
        std::memcpy(cmin, h_ctl + kCmin, sizeof cmin);
        std::memcpy(cmax, h_ctl + kCmax, sizeof cmax);
        plan = lbvh::extent_plan(cmin, cmax);
    }

    hipLaunchKernelGGL(key_kernel, dim3(tri_blocks), dim3(kThreads), 0, s, (const float4*)c2, n, (const uint32_t*)ctl, plan,
                       keys_in);
    ++launches;
    LB_HIP(rocprim::radix_sort_keys(S.sort_tmp.p, sort_bytes, keys_in, keys, N, 0u, 64u, s));
    if (n <= max_leaf) {
        hipLaunchKernelGGL(rootleaf_kernel, dim3(1), dim3(64), 0, s, (const uint64_t*)keys, n, d_verts, d_idx, d_nodes, d_refs);
        ++launches;
        LB_HIP(hipGetLastError());
        *num_nodes = 1;
        S.deepest = -1;
        S.launches = launches;
        return RT_OK;
    }
    LB_HIP(hipMemsetAsync(S.flags.p, 0, N * 8, s));
    hipLaunchKernelGGL(radix_kernel, dim3(tri_blocks), dim3(kThreads), 0, s, (const uint64_t*)keys, n, max_leaf,
                       (int4*)S.radix.p, (int32_t*)S.parent.p, (uint32_t*)S.flags.p, d_refs);
    ++launches;
    LB_HIP(rocprim::exclusive_scan(S.scan_tmp.p, scan_bytes, (uint64_t*)S.flags.p, (uint64_t*)S.ranks.p, (uint64_t)0, N,
                                   rocprim::plus<uint64_t>(), s));
    hipLaunchKernelGGL(emit_kernel, grid_for(N - 1), dim3(kThreads), 0, s, (const int4*)S.radix.p, (const int32_t*)S.parent.p,
                       (const uint64_t*)S.ranks.p, n, max_leaf, (const uint64_t*)keys, d_verts, d_idx, d_nodes, node_cap,
                       (uint32_t*)S.depth.p, ctl);
    ++launches;
    LB_HIP(hipGetLastError());
    LB_HIP(hipMemcpyAsync(h_ctl, ctl, kCursor * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LB_HIP(hipStreamSynchronize(s));
    const uint32_t K = h_ctl[kKept];
    if (h_ctl[kBad] || K == 0 || 2 * (size_t)K + 1 > (size_t)node_cap) { err = "rt_build_bvh: inconsistent tree"; return RT_ERR_DEVICE; }
    Levels lv{};
    int deepest = 0;
    uint32_t sum = 0;
    for (int d = 0; d < kDepths; ++d) {
        lv.begin[d] = sum;
        sum += h_ctl[kHist + d];
        if (h_ctl[kHist + d]) deepest = d;
    }
    lv.begin[kDepths] = sum;
    if (sum != K) { err = "rt_build_bvh: depth counts do not cover the kept nodes"; return RT_ERR_DEVICE; }
    hipLaunchKernelGGL(bucket_kernel, grid_for(K), dim3(kThreads), 0, s, (const uint32_t*)S.depth.p, K, lv, ctl,
                       (uint32_t*)S.level_ids.p);
    ++launches;
    const uint32_t* ids = (const uint32_t*)S.level_ids.p;
    for (int d = deepest; d >= 0;) {
        const uint32_t count = lv.begin[d + 1] - lv.begin[d];
        if (count > kTopMax) {
            hipLaunchKernelGGL(fit_level_kernel, grid_for(count), dim3(kThreads), 0, s, d_nodes, K, ids, lv.begin[d], count);
            --d;
        } else {
            int lo = d;
            while (lo > 0 && lv.begin[lo] - lv.begin[lo - 1] <= kTopMax) --lo;
            hipLaunchKernelGGL(fit_top_kernel, dim3(1), dim3(kThreads), 0, s, d_nodes, K, ids, lv, d, lo);
            d = lo - 1;
        }
        ++launches;
    }
    LB_HIP(hipGetLastError());
    *num_nodes = (int32_t)(2 * K + 1);
    static_assert(sizeof S.depth_begin == sizeof lv.begin, "the scratch keeps the whole table");
    std::memcpy(S.depth_begin, lv.begin, sizeof lv.begin);
    S.deepest = deepest;
    S.launches = launches;
    return RT_OK;
}

}  // namespace rtlbvh
