// rt_scene_build.hip -- the kernels of rt_build_scene: rt_upload_scene's device
// records computed on the GPU from the arrays rtlbvh::build leaves on the device, word for word
// what the host loops give for the same tree.
//
//   check_kernel     every vertex, normal and material index against its bound (the first kernel)
//   (rtlbvh::build)  BVH_Node_[] / tri_indices[] into scratch; its radix, parent, rank and depth
//                    arrays are read below
//   pre_kernel       per kept node: its pre-order rank, in closed form (below)
//   bfs_kernel       one workgroup: the first 1,024 kept nodes breadth-first, level by level
//   (rocprim)        one exclusive scan over pre-order positions: nodes the top took
//   assign_kernel    every other kept node: B + its rank among the nodes the top left
//   height_level / height_top   heights bottom-up over the build's depth lists, ONE LAUNCH PER
//                    DEPTH (runs of short depths in one single-workgroup launch)
//   hist_kernel      kept nodes per height  -> host: the refit plan's level_begin
//   bucket_kernel    inner record ids grouped by height
//   inner_kernel     per kept node its 64-B record: the children's boxes axis-major, their
//                    references; the fast-quotient flag; the root box
//   records_kernel   triangle reference records, then shading records, staged through LDS and
//                    stored as contiguous runs of float4s
// A value another workgroup wrote is only ever read in a later launch (rt_lbvh.hip, rt_refit.hip).
//
// Pre-order in closed form.  A radix node over positions [a, b] is numbered a or b (Karras 2012:
// a left child [a, s] is node s, a right child [s + 1, b] is node s + 1, the root is node 0), and
// by induction the inner nodes of its subtree are the numbers [a, b - 1] (it is numbered a) or
// [a + 1, b] (numbered b): the children's runs are [a + 1, s] and [s + 1, b - 1].  Every kept
// node numbered below a is either an ancestor of the node or lies wholly to its left, and what
// lies to its left comes before it in pre-order; so
//     pre(i) = #{kept j < a} + #{ancestors j of i with j >= a},
// the first from the build's kept-rank scan, the second from a read-only walk up the parent links.
#include "rt_scene_build.h"

#include <cstring>   // (rocprim's iterator headers call memset on the host)

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstddef>

#include "rt_abi.h"
#include "rt_records.h"

namespace rtscene {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kBfsTop = 1024;           // rt_upload_scene's breadth-first top
constexpr uint32_t kTopMax = 1024;           // depths with at most this many kept nodes share a launch
constexpr int kHeights = 66;                 // a kept node's height is at most 64
// control words
constexpr int kBad = 0, kTop = 1, kHist = 8, kCursor = 80, kCtlWords = 160;

struct Levels { uint32_t begin[kHeights]; };

__global__ void __launch_bounds__(kThreads) check_kernel(const int32_t* idx, int32_t nv, const int32_t* normal_idx,
                                                         int32_t nnorm, const int32_t* tri_to_mat, int32_t nmat,
                                                         int32_t n, uint32_t* ctl) {
    const int32_t t = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (t >= n) return;
    uint32_t bad = 0;
    for (int k = 0; k < 3; ++k) {
        if ((uint32_t)idx[3 * (size_t)t + k] >= (uint32_t)nv) bad |= kBadVerts;
        if ((uint32_t)normal_idx[3 * (size_t)t + k] >= (uint32_t)nnorm) bad |= kBadNormals;
    }
    if ((uint32_t)tri_to_mat[t] >= (uint32_t)nmat) bad |= kBadMats;
    if (bad) atomicOr(&ctl[kBad], bad);
}

__device__ __forceinline__ bool kept(int32_t lo, int32_t hi, int32_t max_leaf) { return hi - lo + 1 > max_leaf; }

__global__ void __launch_bounds__(kThreads) pre_kernel(const int4* radix, const int32_t* parent, const uint64_t* ranks,
                                                       int32_t n, int32_t max_leaf, uint32_t K, uint32_t* pre_of) {
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n - 1) return;
    const int4 r = radix[i];
    if (!kept(r.x, r.y, max_leaf)) return;
    const uint32_t id = (uint32_t)(ranks[i] >> 32);
    uint32_t above = 0;
    int steps = 0;
    for (int32_t j = parent[i]; j >= 0 && steps < 64; j = parent[j], ++steps)
        if (j >= r.x) ++above;
    if (id < K) pre_of[id] = (uint32_t)(ranks[r.x] >> 32) + above;
}

// The first kBfsTop kept nodes in breadth-first order from the root (node 0), left child before
// right, cut at exactly kBfsTop: position in that order = inner record id.  One workgroup of
// kBfsTop threads; a level is q[lb, le), its kept children are appended in order by a scan.
__global__ void __launch_bounds__(kBfsTop) bfs_kernel(const float4* nodes, uint32_t K, const uint32_t* pre_of,
                                                      uint32_t* seen, uint32_t* inner_id, uint32_t* ctl) {
    __shared__ uint32_t q[kBfsTop], sc[kBfsTop];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) q[0] = 0u;
    __syncthreads();
    uint32_t lb = 0, le = 1;
    while (lb < le && le < kBfsTop) {   // (uniform: lb and le come from shared values)
        const uint32_t m = le - lb;
        uint32_t child[2] = {0, 0}, cnt = 0;
        bool in[2] = {false, false};
        if (tid < m) {
            const float4 w = nodes[3 * (size_t)q[lb + tid] + 2];
            child[0] = (uint32_t)__float_as_int(w.x);
            child[1] = (uint32_t)__float_as_int(w.y);
            in[0] = child[0] < K;
            in[1] = child[1] < K;
            cnt = (in[0] ? 1u : 0u) + (in[1] ? 1u : 0u);
        }
        sc[tid] = cnt;
        __syncthreads();
        for (uint32_t off = 1; off < kBfsTop; off <<= 1) {
            const uint32_t v = tid >= off ? sc[tid - off] : 0u;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const uint32_t total = sc[kBfsTop - 1];
        uint32_t pos = le + sc[tid] - cnt;
        for (int c = 0; c < 2; ++c)
            if (in[c]) {
                if (pos < kBfsTop) q[pos] = child[c];
                ++pos;
            }
        __syncthreads();
        lb = le;
        le = min(kBfsTop, le + total);
    }
    if (tid < le) {
        const uint32_t id = q[tid];
        inner_id[id] = tid;
        const uint32_t p = pre_of[id];
        if (p < K) seen[p] = 1u;
    }
    if (tid == 0) ctl[kTop] = le;
}

__global__ void __launch_bounds__(kThreads) assign_kernel(uint32_t K, const uint32_t* pre_of, const uint32_t* seen,
                                                          const uint32_t* seen_scan, const uint32_t* ctl,
                                                          uint32_t* inner_id) {
    const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
    if (id >= K) return;
    const uint32_t p = pre_of[id];
    if (p >= K) return;   // (cannot happen)
    if (!seen[p]) inner_id[id] = ctl[kTop] + p - seen_scan[p];
}

__device__ __forceinline__ void height_node(const float4* nodes, uint32_t K, uint32_t* height, uint32_t id) {
    if (id >= K) return;
    const float4 w = nodes[3 * (size_t)id + 2];
    const uint32_t l = (uint32_t)__float_as_int(w.x), r = (uint32_t)__float_as_int(w.y);
    const uint32_t hl = l < K ? height[l] : 0u, hr = r < K ? height[r] : 0u;
    height[id] = 1u + max(hl, hr);
}

// one depth whose list is long; its kept children are deeper: earlier launches
__global__ void __launch_bounds__(kThreads) height_level_kernel(const float4* nodes, uint32_t K, const uint32_t* depth_ids,
                                                                uint32_t first, uint32_t count, uint32_t* height) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < count) height_node(nodes, K, height, depth_ids[first + t]);
}

// depths d_hi, d_hi - 1, ..., d_lo (short lists) in ONE workgroup, __syncthreads() between depths
__global__ void __launch_bounds__(kThreads) height_top_kernel(const float4* nodes, uint32_t K, const uint32_t* depth_ids,
                                                              Levels lv, int d_hi, int d_lo, uint32_t* height) {
    for (int d = d_hi; d >= d_lo; --d) {
        for (uint32_t t = lv.begin[d] + threadIdx.x; t < lv.begin[d + 1]; t += kThreads)
            height_node(nodes, K, height, depth_ids[t]);
        __syncthreads();
    }
}

// counts per height: gathered per block in LDS, one global add per height and block
__global__ void __launch_bounds__(kThreads) hist_kernel(const uint32_t* height, uint32_t K, uint32_t* ctl) {
    __shared__ uint32_t hist[kHeights];
    if (threadIdx.x < (uint32_t)kHeights) hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
    if (id < K) atomicAdd(&hist[min(height[id], (uint32_t)kHeights - 1)], 1u);
    __syncthreads();
    if (threadIdx.x < (uint32_t)kHeights && hist[threadIdx.x]) atomicAdd(&ctl[kHist + threadIdx.x], hist[threadIdx.x]);
}

// lv.begin[h - 1] = start of height h's list; order inside a list does not matter
__global__ void __launch_bounds__(kThreads) bucket_kernel(const uint32_t* height, const uint32_t* inner_id, uint32_t K,
                                                          Levels lv, uint32_t* ctl, uint32_t* level_ids) {
    __shared__ uint32_t cnt[kHeights], base[kHeights];
    const uint32_t tid = threadIdx.x;
    if (tid < (uint32_t)kHeights) cnt[tid] = 0u;
    __syncthreads();
    const uint32_t id = blockIdx.x * kThreads + tid;
    uint32_t h = 1, local = 0;
    if (id < K) {
        h = min(max(height[id], 1u), (uint32_t)kHeights - 1);
        local = atomicAdd(&cnt[h], 1u);
    }
    __syncthreads();
    if (tid < (uint32_t)kHeights && cnt[tid]) base[tid] = atomicAdd(&ctl[kCursor + tid], cnt[tid]);
    __syncthreads();
    if (id >= K) return;
    const uint32_t slot = lv.begin[h - 1] + base[h] + local;
    if (slot < lv.begin[h]) level_ids[slot] = inner_id[id];
}

// fast quotient domain of the slab test (rt_upload_scene's fast_ok): 0 or [2^-66, 2^60]
__device__ __forceinline__ bool coord_ok(float v) {
    const float a = fabsf(v);
    return a == 0.0f || (a >= 0x1p-66f && a <= 0x1p60f);
}

__device__ __forceinline__ uint32_t ref_of(const float4* nodes, uint32_t K, const uint32_t* inner_id, uint32_t child) {
    if (child < K) return inner_id[child];
    const float4 w = nodes[3 * (size_t)child + 2];   // a leaf: 1 .. 8 references below 2^25
    return rtrec::leaf_ref((uint32_t)__float_as_int(w.w), (uint32_t)__float_as_int(w.z));
}

__global__ void __launch_bounds__(kThreads) inner_kernel(const float4* nodes, uint32_t K, const uint32_t* inner_id,
                                                         float4* wnodes, uint32_t* out, uint32_t* ctl) {
    const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
    if (id >= K) return;
    const float4* nd = nodes + 3 * (size_t)id;
    const float4 w = nd[2];
    const uint32_t l = (uint32_t)__float_as_int(w.x), r = (uint32_t)__float_as_int(w.y);
    const uint32_t rec_id = inner_id[id];
    if (l > 2 * K || r > 2 * K || rec_id >= K) { ctl[kBad] = 8u; return; }   // (cannot happen)
    const float4 lmn = nodes[3 * (size_t)l], lmx = nodes[3 * (size_t)l + 1];
    const float4 rmn = nodes[3 * (size_t)r], rmx = nodes[3 * (size_t)r + 1];
    float4* rec = wnodes + 4 * (size_t)rec_id;
    // axis-major: {L.min, R.min, L.max, R.max} per axis
    const float4 q[3] = {make_float4(lmn.x, rmn.x, lmx.x, rmx.x), make_float4(lmn.y, rmn.y, lmx.y, rmx.y),
                         make_float4(lmn.z, rmn.z, lmx.z, rmx.z)};
    // S.fast_div also promises min <= max on every axis of every child box (the octant loops,
    // rt_kernel_body.inc slab2_pk): the LBVH's boxes are min / max over at least one triangle's
    // vertices, so a box of finite data is ordered, and a NaN fails coord_ok.
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        rec[k] = q[k];
        ok = ok && coord_ok(q[k].x) && coord_ok(q[k].y) && coord_ok(q[k].z) && coord_ok(q[k].w);
    }
    rec[3] = make_float4(__uint_as_float(ref_of(nodes, K, inner_id, l)), __uint_as_float(ref_of(nodes, K, inner_id, r)),
                         0.0f, 0.0f);
    if (!ok) out[0] = 0u;   // (set to 1 before the launch)
    if (id == 0) {          // the root box
        const float4 mn = nd[0], mx = nd[1];
        out[2] = __float_as_uint(mn.x); out[3] = __float_as_uint(mn.y); out[4] = __float_as_uint(mn.z);
        out[5] = __float_as_uint(mx.x); out[6] = __float_as_uint(mx.y); out[7] = __float_as_uint(mx.z);
    }
}

// Reference records {v0 | id, v1 - v0, v2 - v0}, then shading records {p0..p2, n0..n2, albedo}: a
// block stages 256 records in LDS and stores them as one contiguous run of float4s.
__global__ void __launch_bounds__(kThreads) records_kernel(Args A) {
    __shared__ float4 stage[kThreads * 7];
    const uint32_t tid = threadIdx.x, n = (uint32_t)A.n;
    const uint32_t ref_blocks = (n + kThreads - 1) / kThreads;
    const bool is_ref = blockIdx.x < ref_blocks;
    const uint32_t base = (is_ref ? blockIdx.x : blockIdx.x - ref_blocks) * kThreads, i = base + tid;
    if (base >= n) return;
    const uint32_t per = is_ref ? 3u : 7u;
    if (i < n && is_ref) {
        const int32_t tri1 = A.refs[i];
        const float4 v0 = A.verts[A.idx[tri1]], v1 = A.verts[A.idx[tri1 + 1]], v2 = A.verts[A.idx[tri1 + 2]];
        stage[tid * 3 + 0] = make_float4(v0.x, v0.y, v0.z, __int_as_float(tri1));
        stage[tid * 3 + 1] = make_float4(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z, 0.0f);
        stage[tid * 3 + 2] = make_float4(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z, 0.0f);
    } else if (i < n) {
        for (uint32_t k = 0; k < 3; ++k) {
            const float4 v = A.verts[A.idx[3 * (size_t)i + k]];
            const float4 nm = A.normals[A.normal_idx[3 * (size_t)i + k]];
            stage[tid * 7 + k] = make_float4(v.x, v.y, v.z, 0.0f);
            stage[tid * 7 + 3 + k] = make_float4(nm.x, nm.y, nm.z, 0.0f);
        }
        const float4 d = A.mats[11 * (size_t)A.tri_to_mat[i] + 3];   // rt_material::diffuse
        stage[tid * 7 + 6] = make_float4(d.x, d.y, d.z, 0.0f);
    }
    __syncthreads();
    const uint32_t words = min(kThreads, n - base) * per;
    float4* out = (is_ref ? A.tris : A.shade) + (size_t)base * per;
    for (uint32_t j = tid; j < words; j += kThreads) out[j] = stage[j];
}

inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

}  // namespace

static_assert(sizeof(rt_material) == 11 * sizeof(float4) && offsetof(rt_material, diffuse) == 3 * sizeof(float4),
              "records_kernel reads rt_material::diffuse as float4 3 of 11");

void release(Scratch& w) {
    for (Scratch::Buf* b : {&w.ctl, &w.pre, &w.seen, &w.seen_scan, &w.scan_tmp, &w.inner_id, &w.height, &w.mats,
                            &w.tri_to_mat}) {
        if (b->p) (void)hipFree(b->p);
        *b = Scratch::Buf{};
    }
    for (hipEvent_t& e : w.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    w.timed = false;
}

#define SB_HIP(expr)                                                                 \
    do {                                                                             \
        const hipError_t e__ = (expr);                                               \
        if (e__ != hipSuccess) {                                                     \
            err = std::string(#expr) + ": " + hipGetErrorString(e__);                \
            return e__ == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_DEVICE; \
        }                                                                            \
    } while (0)

int check(Scratch& W, hipStream_t s, const int32_t* d_idx, int32_t nv, const int32_t* d_normal_idx, int32_t nnorm,
          const int32_t* d_tri_to_mat, int32_t nmat, int32_t n, uint32_t* bad, std::string& err) {
    SB_HIP(rtlbvh::reserve(W.ctl, kCtlWords * 4));
    uint32_t* ctl = (uint32_t*)W.ctl.p;
    SB_HIP(hipMemsetAsync(ctl, 0, kCtlWords * 4, s));
    hipLaunchKernelGGL(check_kernel, grid_for((size_t)n), dim3(kThreads), 0, s, d_idx, nv, d_normal_idx, nnorm, d_tri_to_mat,
                       nmat, n, ctl);
    SB_HIP(hipGetLastError());
    SB_HIP(hipMemcpyAsync(bad, ctl + kBad, 4, hipMemcpyDeviceToHost, s));
    SB_HIP(hipStreamSynchronize(s));
    W.launches = 1;
    return RT_OK;
}

int leaf_records(Scratch& W, hipStream_t s, const Args& a, std::string& err) {
    hipLaunchKernelGGL(records_kernel, dim3(2 * grid_for((size_t)a.n).x), dim3(kThreads), 0, s, a);
    SB_HIP(hipGetLastError());
    ++W.launches;
    return RT_OK;
}

int records(Scratch& W, const rtlbvh::Scratch& S, hipStream_t s, const Args& a, std::vector<uint32_t>& level_begin,
            std::string& err) {
    const uint32_t K = a.K;
    const size_t N = (size_t)a.n;
    if (K == 0 || K >= (uint32_t)a.n || S.deepest < 0 || S.deepest >= kHeights - 1 || S.depth_begin[S.deepest + 1] != K) {
        err = "inconsistent tree";
        return RT_ERR_DEVICE;
    }
    size_t scan_bytes = 0;
    SB_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)K,
                                   rocprim::plus<uint32_t>(), s));
    SB_HIP(rtlbvh::reserve(W.pre, (size_t)K * 4));
    SB_HIP(rtlbvh::reserve(W.seen, (size_t)K * 4));
    SB_HIP(rtlbvh::reserve(W.seen_scan, (size_t)K * 4));
    SB_HIP(rtlbvh::reserve(W.scan_tmp, scan_bytes));
    SB_HIP(rtlbvh::reserve(W.inner_id, (size_t)K * 4));
    SB_HIP(rtlbvh::reserve(W.height, (size_t)K * 4));
    uint32_t* ctl = (uint32_t*)W.ctl.p;   // (check() reserved and zeroed it)
    uint32_t *pre = (uint32_t*)W.pre.p, *seen = (uint32_t*)W.seen.p, *seen_scan = (uint32_t*)W.seen_scan.p;
    uint32_t *inner_id = (uint32_t*)W.inner_id.p, *height = (uint32_t*)W.height.p;
    const uint32_t* depth_ids = (const uint32_t*)S.level_ids.p;
    uint32_t launches = W.launches;

    // inner record ids
    SB_HIP(hipMemsetAsync(seen, 0, (size_t)K * 4, s));
    SB_HIP(hipMemsetAsync(inner_id, 0xFF, (size_t)K * 4, s));
    hipLaunchKernelGGL(pre_kernel, grid_for(N - 1), dim3(kThreads), 0, s, (const int4*)S.radix.p, (const int32_t*)S.parent.p,
                       (const uint64_t*)S.ranks.p, a.n, a.max_leaf, K, pre);
    hipLaunchKernelGGL(bfs_kernel, dim3(1), dim3(kBfsTop), 0, s, a.nodes, K, (const uint32_t*)pre, seen, inner_id, ctl);
    launches += 2;
    SB_HIP(hipGetLastError());
    SB_HIP(rocprim::exclusive_scan(W.scan_tmp.p, scan_bytes, seen, seen_scan, 0u, (size_t)K, rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(assign_kernel, grid_for(K), dim3(kThreads), 0, s, K, (const uint32_t*)pre, (const uint32_t*)seen,
                       (const uint32_t*)seen_scan, (const uint32_t*)ctl, inner_id);
    ++launches;

    // heights, bottom-up over the build's depth lists
    Levels dl{};
    std::memcpy(dl.begin, S.depth_begin, sizeof dl.begin);
    for (int d = S.deepest; d >= 0;) {
        const uint32_t count = dl.begin[d + 1] - dl.begin[d];
        if (count > kTopMax) {
            hipLaunchKernelGGL(height_level_kernel, grid_for(count), dim3(kThreads), 0, s, a.nodes, K, depth_ids, dl.begin[d],
                               count, height);
            --d;
        } else {
            int lo = d;
            while (lo > 0 && dl.begin[lo] - dl.begin[lo - 1] <= kTopMax) --lo;
            hipLaunchKernelGGL(height_top_kernel, dim3(1), dim3(kThreads), 0, s, a.nodes, K, depth_ids, dl, d, lo, height);
            d = lo - 1;
        }
        ++launches;
    }
    hipLaunchKernelGGL(hist_kernel, grid_for(K), dim3(kThreads), 0, s, (const uint32_t*)height, K, ctl);
    ++launches;
    SB_HIP(hipGetLastError());

    // the records that need no plan run while the host reads the counts
    const uint32_t out0[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    SB_HIP(hipMemcpyAsync(a.out, out0, sizeof out0, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(inner_kernel, grid_for(K), dim3(kThreads), 0, s, a.nodes, K, (const uint32_t*)inner_id, a.wnodes,
                       a.out, ctl);
    hipLaunchKernelGGL(records_kernel, dim3(2 * grid_for(N).x), dim3(kThreads), 0, s, a);
    launches += 2;
    SB_HIP(hipGetLastError());

    uint32_t h_ctl[kCursor] = {};
    SB_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, s));
    SB_HIP(hipStreamSynchronize(s));   // (out0 and h_ctl are stack objects)
    if (h_ctl[kBad]) { err = "inconsistent tree"; return RT_ERR_DEVICE; }
    int top = 0;
    for (int h = 1; h < kHeights; ++h)
        if (h_ctl[kHist + h]) top = h;
    if (h_ctl[kHist] || top == 0 || top >= kHeights - 1) { err = "heights out of range"; return RT_ERR_DEVICE; }
    // rtrefit::plan_build's table: level_begin[h - 1] = start of height h, level_begin[top] = K
    Levels hl{};
    level_begin.assign((size_t)top + 1, 0u);
    uint32_t sum = 0;
    for (int h = 1; h <= top; ++h) {
        level_begin[h - 1] = hl.begin[h - 1] = sum;
        sum += h_ctl[kHist + h];
    }
    level_begin[top] = hl.begin[top] = sum;
    if (sum != K) { err = "height counts do not cover the inner records"; return RT_ERR_DEVICE; }
    hipLaunchKernelGGL(bucket_kernel, grid_for(K), dim3(kThreads), 0, s, (const uint32_t*)height, (const uint32_t*)inner_id, K,
                       hl, ctl, a.level_ids);
    ++launches;
    SB_HIP(hipGetLastError());
    W.launches = launches;
    return RT_OK;
}

}  // namespace rtscene
