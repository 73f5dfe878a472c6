// rt_sah.hip -- the kernels of rt_scene_sah: the surface-area-heuristic cost of the
// scene as it stands on the GPU, from the inner records and the escape-leaf table alone.
//
//   hA(box) = (dx*dy + dy*dz) + dz*dx, single float operations (-ffp-contract=off)
//   inner   += hA(child box)           for every child slot whose reference is an inner record
//   leaf    += hA(child box) * count   for every child slot that holds a leaf (count from the
//                                      reference, or the escape table when its count field is 31)
// A reference that is neither (the error reference, an id or a table index out of range) adds
// nothing; sums are doubles.
//
//   sah_sum_kernel    one thread per inner record: its four 16-B words, two doubles; the block
//                     adds them up in LDS and stores its partial pair
//   sah_total_kernel  one workgroup: the partial pairs in index order
// No floating-point atomics and nothing handed from workgroup to workgroup inside a kernel (as
// rt_refit.hip, rt_lbvh.hip): the result does not depend on scheduling.
#include "rt_sah.h"
#include "rt_records.h"

namespace rtsah {

namespace {

using rtrec::kCntEscape;
using rtrec::kLeafBit;
constexpr uint32_t kThreads = 256;

__device__ __forceinline__ float half_area(float dx, float dy, float dz) { return (dx * dy + dy * dz) + dz * dx; }

__global__ void __launch_bounds__(kThreads) sah_sum_kernel(const float4* wnodes, uint32_t n_inner, const int2* leaf_table,
                                                           uint32_t n_leaf, uint32_t root, double* part, Result* out) {
    __shared__ double s_inner[kThreads], s_leaf[kThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t id = blockIdx.x * kThreads + tid;
    double inner = 0.0, leaf = 0.0;
    if (id < n_inner) {
        const float4* rec = wnodes + (size_t)id * 4;
        const float4 x = rec[0], y = rec[1], z = rec[2], w = rec[3];   // axis-major: {L.min, R.min, L.max, R.max}
        const uint32_t ref[2] = {__float_as_uint(w.x), __float_as_uint(w.y)};
        const float area[2] = {half_area(x.z - x.x, y.z - y.x, z.z - z.x), half_area(x.w - x.y, y.w - y.y, z.w - z.y)};
        for (int c = 0; c < 2; ++c) {
            if (!(ref[c] & kLeafBit)) {
                if (ref[c] < n_inner) inner += (double)area[c];
                continue;
            }
            int32_t cnt = (int32_t)((ref[c] >> rtrec::kCntShift) & 31u);   // rtrec::ref_count, as written before it
            if ((uint32_t)cnt == kCntEscape) {
                const uint32_t e = rtrec::ref_offset(ref[c]);
                cnt = e < n_leaf ? leaf_table[e].y : 0;
            }
            if (cnt > 0) leaf += (double)area[c] * (double)cnt;
        }
        if (id == root) {
            out->root_box[0] = fminf(x.x, x.y); out->root_box[1] = fminf(y.x, y.y); out->root_box[2] = fminf(z.x, z.y);
            out->root_box[3] = fmaxf(x.z, x.w); out->root_box[4] = fmaxf(y.z, y.w); out->root_box[5] = fmaxf(z.z, z.w);
        }
    }
    s_inner[tid] = inner;
    s_leaf[tid] = leaf;
    __syncthreads();
    for (uint32_t k = kThreads / 2; k > 0; k >>= 1) {
        if (tid < k) {
            s_inner[tid] += s_inner[tid + k];
            s_leaf[tid] += s_leaf[tid + k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[2 * (size_t)blockIdx.x] = s_inner[0];
        part[2 * (size_t)blockIdx.x + 1] = s_leaf[0];
    }
}

// thread t adds the pairs [t * chunk, (t + 1) * chunk) in index order, thread 0 the threads' sums
__global__ void __launch_bounds__(kThreads) sah_total_kernel(const double* part, uint32_t nblocks, Result* out) {
    __shared__ double s_inner[kThreads], s_leaf[kThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (nblocks + kThreads - 1) / kThreads;
    const uint32_t b0 = min(nblocks, tid * chunk), b1 = min(nblocks, b0 + chunk);
    double inner = 0.0, leaf = 0.0;
    for (uint32_t b = b0; b < b1; ++b) {
        inner += part[2 * (size_t)b];
        leaf += part[2 * (size_t)b + 1];
    }
    s_inner[tid] = inner;
    s_leaf[tid] = leaf;
    __syncthreads();
    if (tid != 0) return;
    for (uint32_t t = 1; t < kThreads; ++t) {
        inner += s_inner[t];
        leaf += s_leaf[t];
    }
    out->inner_area = inner;
    out->leaf_area_tris = leaf;
}

}  // namespace

uint32_t blocks_for(uint32_t n_inner) { return (n_inner + kThreads - 1) / kThreads; }

hipError_t launch(const float4* wnodes, uint32_t n_inner, const int2* leaf_table, uint32_t n_leaf, uint32_t root,
                  double* part, Result* out, hipStream_t s) {
    const uint32_t nblocks = blocks_for(n_inner);
    hipLaunchKernelGGL(sah_sum_kernel, dim3(nblocks), dim3(kThreads), 0, s, wnodes, n_inner, leaf_table, n_leaf, root, part,
                       out);
    hipLaunchKernelGGL(sah_total_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)part, nblocks, out);
    return hipGetLastError();
}

}  // namespace rtsah
