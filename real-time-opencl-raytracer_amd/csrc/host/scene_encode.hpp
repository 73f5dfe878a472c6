// scene_encode.hpp -- rt_upload_scene's host half: the caller's scene arrays checked and encoded
// into the device layouts (rt_render.hip's DevScene; the child references of rt_records.h).
// Plain C++ over the ABI structs; no HIP, and nothing else of csrc/host.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "rt_abi.h"

namespace rtamd {

struct EncodedScene {
    std::vector<rt_float4> wnodes;   // [max(n_inner, 1)][4] inner records
    std::vector<rt_float4> tris;     // [max(nref, 1)][3] + 1 triangle reference records {v0|id, e1, e2}
    std::vector<rt_float4> shade;    // [ntri][7] shading records
    std::vector<std::pair<int32_t, int32_t>> leaf_table;   // escape leaves {offset, count}; never empty
    std::vector<int32_t> inner_id;   // node -> the id of its inner record, -1: none (rtrefit::plan_build)
    uint32_t root = 0;               // the root's reference
    uint32_t n_inner = 0;
    int fast_div = 0;                // every box coordinate is 0 or in [2^-66, 2^60], every child box min <= max
    int clean = 0;                   // no reachable malformed inner node (kRefError)
};

// The arrays are rt_upload_scene's, all present and of positive counts (nref >= 0, nidx a multiple
// of 3).  RT_OK, or RT_ERR_BAD_SCENE with `err` saying why: an index out of range, a cycle, a leaf
// range past the references.  A reachable inner node with a child offset outside [0, nn) encodes
// as kRefError and clears `clean`, as the reference returns -1 when it pops one.
int encode_scene(const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx, const rt_bvh_node* nodes, int32_t nn,
                 const int32_t* refs, int32_t nref, const rt_float4* normals, int32_t nnorm, const int32_t* normal_idx,
                 const rt_material* mats, int32_t nmat, const int32_t* tri_to_mat, EncodedScene& out, std::string& err);

// The walk references (rt_records.h) of n_rec inner records and of the root: the host twin of the kernel
// that derives them from the records of every scene installed on the device (rt_render.hip
// derive_walk_kernel), integer operation for integer operation.  walk gets two words per record, in
// record order.  tri_unit: the first triangle record's offset in 16-B units (the inner records'
// float4 count); n_refs: triangle reference records in front of the pad record.  False when a child
// or the root has no walk reference (kWalkNone in its place): such a scene renders without the array.
bool derive_walk(const rt_float4* wnodes, size_t n_rec, const std::pair<int32_t, int32_t>* leaf_table, size_t n_leaf,
                 uint32_t tri_unit, uint32_t n_refs, uint32_t root, std::vector<uint32_t>& walk, uint32_t& walk_root);

}  // namespace rtamd
