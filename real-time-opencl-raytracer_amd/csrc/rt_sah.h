// rt_sah.h -- device side of rt_scene_sah: the SAH cost of the uploaded scene's inner records as
// they stand on the GPU (rt_sah.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rtsah {

// what the kernels leave in `out`: the two sums, then the root record's own box (the union of
// its two slots) as {min.xyz, max.xyz}
struct Result {
    double inner_area, leaf_area_tris;
    float root_box[6];
    uint32_t pad[2];
};

// blocks of the first kernel (= partial pairs) for n_inner records
uint32_t blocks_for(uint32_t n_inner);

// Enqueues both kernels on `s`.  wnodes: [n_inner][4] inner records; leaf_table: [n_leaf] escape
// leaves {offset, count}; root: the root's inner record id; part: room for 2 * blocks_for(n_inner)
// doubles; out: one Result.  Read-only on the scene.  n_inner > 0.
hipError_t launch(const float4* wnodes, uint32_t n_inner, const int2* leaf_table, uint32_t n_leaf, uint32_t root,
                  double* part, Result* out, hipStream_t s);

}  // namespace rtsah
