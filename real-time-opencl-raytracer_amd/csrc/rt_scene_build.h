// rt_scene_build.h -- device side of rt_build_scene: the device records of rt_upload_scene built
// on the GPU from the arrays rtlbvh::build leaves behind (rt_scene_build.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#include "rt_lbvh.h"

namespace rtscene {

// The call's own buffers; they belong to the context, grow on demand and are freed by release().
struct Scratch {
    using Buf = rtlbvh::Scratch::Buf;
    Buf ctl, pre, seen, seen_scan, scan_tmp, inner_id, height;
    Buf mats, tri_to_mat;                             // staging of the host arrays
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // around the call's kernels; the caller's stream
    bool timed = false;
    uint32_t launches = 0;
};

void release(Scratch& w);

// index flags of check(): which array holds an index outside its bound
enum { kBadVerts = 1u, kBadNormals = 2u, kBadMats = 4u };

// The first kernel: every vertex, normal and material index against its bound.  Waits for `s` and
// returns the flags in *bad (0: all in range).
int check(Scratch& W, hipStream_t s, const int32_t* d_idx, int32_t nv, const int32_t* d_normal_idx, int32_t nnorm,
          const int32_t* d_tri_to_mat, int32_t nmat, int32_t n, uint32_t* bad, std::string& err);

struct Args {
    // in: the mesh on the device, and rtlbvh::build's output (with what it left in its scratch)
    const float4* verts;
    const float4* normals;
    const int32_t* idx;          // [3 n]
    const int32_t* normal_idx;   // [3 n]
    const int32_t* tri_to_mat;   // [n]
    const float4* mats;          // [nmat] rt_material, 11 float4s each
    const float4* nodes;         // [2 K + 1] BVH_Node_
    const int32_t* refs;         // [n]
    int32_t n, max_leaf;
    uint32_t K;                  // kept (inner) nodes; > 0
    // out
    float4* wnodes;              // [K][4]
    float4* tris;                // [n][3] (+ the pad float4)
    float4* shade;               // [n][7]
    uint32_t* level_ids;         // [K] inner record ids grouped by height
    uint32_t* out;               // [8] rtrefit::DevArgs::out: fast-quotient flag, root box
};

// Enqueues everything after the build on `s` (one wait for `s` on the way: the counts per
// height) and returns with the last kernels enqueued.  level_begin: the refit plan's host copy.
int records(Scratch& W, const rtlbvh::Scratch& S, hipStream_t s, const Args& a, std::vector<uint32_t>& level_begin,
            std::string& err);

// A scene whose root is a leaf: the triangle and shading records only.
int leaf_records(Scratch& W, hipStream_t s, const Args& a, std::string& err);

}  // namespace rtscene
