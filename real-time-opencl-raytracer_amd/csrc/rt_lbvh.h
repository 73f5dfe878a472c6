// rt_lbvh.h -- device side of rt_build_bvh: the LBVH build of DESIGN.md 15 on the GPU
// (rt_lbvh.hip; the definition and its host twin are csrc/host/lbvh_builder.cpp's).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

namespace rtlbvh {

// The build's buffers; they belong to the context, grow on demand and are freed by release().
struct Scratch {
    struct Buf { void* p = nullptr; size_t bytes = 0; };
    Buf c2, part, keys[2], sort_tmp, radix, parent, flags, ranks, scan_tmp, depth, level_ids, ctl;
    Buf verts, idx, nodes, refs;                      // staging of the host form's arrays
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // around the build's kernels; the caller's stream
    bool timed = false;
    uint32_t launches = 0;
    // host copy of the last build's depth lists: the kept nodes of depth d are
    // level_ids[depth_begin[d] .. depth_begin[d + 1]); deepest = -1 when the root is a leaf
    uint32_t depth_begin[66] = {};
    int deepest = -1;
};

hipError_t reserve(Scratch::Buf& b, size_t bytes);
void release(Scratch& s);

// Builds on `s` from device arrays (n = triangles, validated by the caller: 1 .. 2^25, max_leaf
// 1 .. 8, room for 2n - 1 nodes and n references); extent_keys: the key plan of DESIGN.md 17 in
// place of the per-axis one.  Waits for `s` twice on the way (the index flag with cmin / cmax, the
// depth counts) and returns with the last kernels enqueued: d_nodes / d_refs are
// complete once `s` has drained.  RT_OK, RT_ERR_BAD_SCENE (an index outside [0, nv): nothing after the first stage
// ran), RT_ERR_OUT_OF_MEMORY or RT_ERR_DEVICE, with `err` set.
int build(Scratch& S, hipStream_t s, const float4* d_verts, int32_t nv, const int32_t* d_idx, int32_t n,
          int32_t max_leaf, bool extent_keys, float4* d_nodes, int32_t node_cap, int32_t* d_refs, int32_t* num_nodes, std::string& err);

}  // namespace rtlbvh
