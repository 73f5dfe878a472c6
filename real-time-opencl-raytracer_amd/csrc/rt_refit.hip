// rt_refit.hip -- animated geometry: the kernels of rt_update_vertices.
//
// refit_records_kernel rewrites the triangle reference records {v0|id, v1 - v0, v2 - v0} and
// the positions (and normals) of the shading records from the vertex buffer, with the same
// single subtractions rt_upload_scene makes on the host (-ffp-contract=off).
// The box pass is bottom-up and parent-centric: a thread owns one inner record, gets each
// child's box (a leaf: min / max over its triangles' vertices; an inner child: the union of
// the two slots of that child's own record, written by an EARLIER launch or, in the
// single-workgroup top kernel, before the preceding __syncthreads()), and writes the record's
// three axis float4s whole.  One writer per record, heights ordered by kernel boundaries: no
// hand-off between workgroups inside a kernel (the per-XCD L2s are not coherent and a CU's L1
// is not refreshed by another CU's stores).
#include "rt_refit.h"
#include "rt_records.h"

namespace rtrefit {

namespace {

using rtrec::kCntEscape;
using rtrec::kLeafBit;
constexpr uint32_t kThreads = 256;
constexpr uint32_t kTopMax = 1024;           // heights with at most this many records run in the top kernel

// fast quotient domain of the slab test (rt_upload_scene's fast_ok): 0 or [2^-66, 2^60]
__device__ __forceinline__ bool coord_ok(float v) {
    const float a = fabsf(v);
    return a == 0.0f || (a >= 0x1p-66f && a <= 0x1p60f);
}

// Reference records, then shading records: a block stages 256 records in LDS and stores them
// as one contiguous run of float4s.
__global__ void __launch_bounds__(kThreads) refit_records_kernel(DevArgs A) {
    __shared__ float4 stage[kThreads * 6];
    const uint32_t tid = threadIdx.x;
    const uint32_t ref_blocks = (A.nref + kThreads - 1) / kThreads;
    if (blockIdx.x == 0 && tid == 0) A.out[0] = 1u;   // the box kernels (later launches) clear it
    if (blockIdx.x < ref_blocks) {
        const uint32_t base = blockIdx.x * kThreads, i = base + tid;
        if (i < A.nref) {
            const int32_t tri1 = A.ref_tri[i];
            const float4 v0 = A.verts[A.idx[tri1]], v1 = A.verts[A.idx[tri1 + 1]], v2 = A.verts[A.idx[tri1 + 2]];
            stage[tid * 3 + 0] = make_float4(v0.x, v0.y, v0.z, __int_as_float(tri1));
            stage[tid * 3 + 1] = make_float4(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z, 0.0f);
            stage[tid * 3 + 2] = make_float4(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z, 0.0f);
        }
        __syncthreads();
        const uint32_t n = min(kThreads, A.nref - base) * 3;
        float4* out = A.tris + (size_t)base * 3;
        for (uint32_t j = tid; j < n; j += kThreads) out[j] = stage[j];
    } else {
        const uint32_t base = (blockIdx.x - ref_blocks) * kThreads, t = base + tid;
        if (base >= A.ntri) return;
        const uint32_t per = A.normals ? 6u : 3u;   // float4s rewritten per 7-float4 record
        if (t < A.ntri) {
            for (uint32_t k = 0; k < 3; ++k) {
                const float4 v = A.verts[A.idx[3 * t + k]];
                stage[tid * per + k] = make_float4(v.x, v.y, v.z, 0.0f);
                if (A.normals) {
                    const float4 nm = A.normals[A.normal_idx[3 * t + k]];
                    stage[tid * per + 3 + k] = make_float4(nm.x, nm.y, nm.z, 0.0f);
                }
            }
        }
        __syncthreads();
        const uint32_t n = min(kThreads, A.ntri - base) * per;
        float4* out = A.shade + (size_t)base * 7;
        for (uint32_t j = tid; j < n; j += kThreads) {
            const uint32_t r = j / per, k = j - r * per;
            out[r * 7 + k] = stage[j];
        }
    }
}

// The box of the child behind reference `ref` (slot 0 = left, 1 = right of the record q).
__device__ __forceinline__ void child_box(const DevArgs& A, uint32_t ref, int slot, const float4 q[3], float mn[3],
                                          float mx[3]) {
    if (!(ref & kLeafBit)) {   // an inner child: the union of its record's two slots
        const float4* c = A.wnodes + (size_t)ref * 4;
        for (int k = 0; k < 3; ++k) {
            const float4 b = c[k];
            mn[k] = fminf(b.x, b.y);
            mx[k] = fmaxf(b.z, b.w);
        }
        return;
    }
    int32_t cnt = (int32_t)rtrec::ref_count(ref), off = (int32_t)rtrec::ref_offset(ref);
    if ((uint32_t)cnt == kCntEscape) {
        const int2 e = A.leaf_table[off];
        off = e.x;
        cnt = e.y;
    }
    if (cnt <= 0) {   // an empty leaf keeps the box it was uploaded with
        for (int k = 0; k < 3; ++k) {
            mn[k] = slot ? q[k].y : q[k].x;
            mx[k] = slot ? q[k].w : q[k].z;
        }
        return;
    }
    bool first = true;
    for (int32_t r = off; r < off + cnt; ++r) {
        const int32_t tri1 = A.ref_tri[r];
        for (int k = 0; k < 3; ++k) {
            const float4 v = A.verts[A.idx[tri1 + k]];
            const float p[3] = {v.x, v.y, v.z};
            for (int a = 0; a < 3; ++a) {
                mn[a] = first ? p[a] : fminf(mn[a], p[a]);
                mx[a] = first ? p[a] : fmaxf(mx[a], p[a]);
            }
            first = false;
        }
    }
}

__device__ __forceinline__ void refit_record(const DevArgs& A, uint32_t id, bool is_root) {
    float4* rec = A.wnodes + (size_t)id * 4;
    const float4 q[3] = {rec[0], rec[1], rec[2]};
    const float4 w = rec[3];
    float mnL[3], mxL[3], mnR[3], mxR[3];
    child_box(A, __float_as_uint(w.x), 0, q, mnL, mxL);
    child_box(A, __float_as_uint(w.y), 1, q, mnR, mxR);
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        rec[k] = make_float4(mnL[k], mnR[k], mxL[k], mxR[k]);   // axis-major, as the upload lays it out
        ok = ok && coord_ok(mnL[k]) && coord_ok(mnR[k]) && coord_ok(mxL[k]) && coord_ok(mxR[k]);
        // S.fast_div also promises min <= max (the octant loops, rt_kernel_body.inc slab2_pk).  A box
        // made here is min / max over finite data (a NaN fails coord_ok), hence ordered; only an
        // empty leaf's box, kept as uploaded, can be inverted
        ok = ok && mnL[k] <= mxL[k] && mnR[k] <= mxR[k];
    }
    if (!ok) A.out[0] = 0u;
    if (is_root) {
        float* b = reinterpret_cast<float*>(A.out + 2);
        for (int k = 0; k < 3; ++k) {
            b[k] = fminf(mnL[k], mnR[k]);
            b[3 + k] = fmaxf(mxL[k], mxR[k]);
        }
    }
}

// One height whose list is long: a thread per record.  Its children are of lower heights,
// written by earlier launches.
__global__ void __launch_bounds__(kThreads) refit_level_kernel(DevArgs A, uint32_t first, uint32_t count) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t < count) refit_record(A, A.level_ids[first + t], false);
}

// The top heights [h0, h1) (0-based rows of level_begin; short lists, the last is the root) in
// ONE workgroup: its waves share a CU and its L1, so __syncthreads() orders a height's stores
// before the next height's loads.  A scene whose root is a leaf has no inner record: its bounds
// come from the leaf.
__global__ void __launch_bounds__(kThreads) refit_top_kernel(DevArgs A, uint32_t h0, uint32_t h1) {
    if (A.n_inner == 0) {
        if (threadIdx.x == 0) {
            const float* old = reinterpret_cast<const float*>(A.out + 2);
            float4 q[3];
            for (int k = 0; k < 3; ++k) q[k] = make_float4(old[k], 0.0f, old[3 + k], 0.0f);
            float mn[3], mx[3];
            child_box(A, A.root, 0, q, mn, mx);
            float* b = reinterpret_cast<float*>(A.out + 2);
            for (int k = 0; k < 3; ++k) { b[k] = mn[k]; b[3 + k] = mx[k]; }
        }
        return;
    }
    for (uint32_t h = h0; h < h1; ++h) {
        const uint32_t b = A.level_begin[h], e = A.level_begin[h + 1];
        for (uint32_t t = b + threadIdx.x; t < e; t += kThreads) refit_record(A, A.level_ids[t], h + 1 == h1);
        __syncthreads();
    }
}

}  // namespace

hipError_t launch(const DevArgs& a, const uint32_t* lb, uint32_t heights, hipStream_t s, uint32_t* launches) {
    uint32_t n = 0;
    const uint32_t rec_blocks = (a.nref + kThreads - 1) / kThreads + (a.ntri + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(refit_records_kernel, dim3(rec_blocks), dim3(kThreads), 0, s, a);
    ++n;
    uint32_t h = 0;
    for (; h < heights && lb[h + 1] - lb[h] > kTopMax; ++h) {
        const uint32_t count = lb[h + 1] - lb[h];
        hipLaunchKernelGGL(refit_level_kernel, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a, lb[h], count);
        ++n;
    }
    hipLaunchKernelGGL(refit_top_kernel, dim3(1), dim3(kThreads), 0, s, a, h, heights);
    ++n;
    if (launches) *launches = n;
    return hipGetLastError();
}

}  // namespace rtrefit
