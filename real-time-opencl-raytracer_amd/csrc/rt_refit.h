// rt_refit.h -- device side of rt_update_vertices: rewrites the uploaded scene's derived
// records in place from a vertex buffer (rt_refit.hip; the plan is csrc/host/refit.cpp's).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rtrefit {

struct DevArgs {
    float4* wnodes;              // [n_inner][4] inner records (rewritten: the three axis float4s)
    float4* tris;                // [nref][3] triangle reference records (rewritten whole)
    float4* shade;               // [ntri][7] shading records (p0..p2, and n0..n2 with normals; albedo stays)
    const int2* leaf_table;      // escape leaves {offset, count}
    const float4* verts;         // [nv] the new vertices
    const float4* normals;       // [nnorm] the new normals, or null
    const int32_t* idx;          // [3 * ntri] vertex index per triangle corner
    const int32_t* normal_idx;   // [3 * ntri]
    const int32_t* ref_tri;      // [nref] 3 * triangle of every reference record
    const uint32_t* level_ids;   // inner record ids grouped by height
    const uint32_t* level_begin; // [heights + 1] starts of the heights' lists in level_ids
    uint32_t* out;               // [8]: [0] fast-quotient flag, [2..7] the root box {min.xyz, max.xyz}
    uint32_t nref, ntri, n_inner, root;
};

// Enqueues the whole update on `s`: the record kernel, one box launch per height while the
// heights' lists are long, and one single-workgroup launch for the top heights.
// h_level_begin: the host copy of level_begin.  *launches: kernels enqueued.
hipError_t launch(const DevArgs& a, const uint32_t* h_level_begin, uint32_t heights, hipStream_t s, uint32_t* launches);

}  // namespace rtrefit
