// rt_closest.h -- device side of rt_closest_points: the nearest triangle, its distance and the
// closest point on it for caller-supplied points (rt_closest.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rtclosest {

constexpr uint32_t kThreads = 256;        // a block: 4 waves, a wave takes 64 consecutive points at a time
constexpr int kLdsStack = 16;             // stack entries in a lane's LDS column
constexpr int kGlobalStack = 64 - kLdsStack;   // rows of the global columns: entries kLdsStack .. 63
// the work cursors, as the ray queries' (rt_render.hip grab_group): 8 cursors, 128 B apart
constexpr uint32_t kCursors = 8, kCursorStride = 32;

struct Scene {
    const float4* wnodes;      // [n_inner][4] inner records
    const float4* tris;        // [n_refs][3] triangle reference records
    const int2* leaf_table;    // escape leaves {offset, count}
    uint32_t root;
};

struct Launch {
    const float4* pts;         // rt_point[n], 16-byte aligned
    float4* out;               // rt_closest[n] as two float4 each
    uint32_t n;                // <= 2^30
    uint32_t* fetch;           // kCursors * kCursorStride words, zeroed before the launch
    uint32_t* gstack;          // [kGlobalStack][grid * kThreads] words
    unsigned long long* overflow;
};

// k == 0: rt_closest_points' kernel, one record per point.  k in 1 .. 8: rt_nearest_k's kernel of that k
// (DESIGN.md 23), the k nearest triangles per point; L.out then holds k planes of L.n records, plane j
// at out + j * n.

// the kernel, for the occupancy query that sizes the persistent grid
const void* kernel(int k);

// Enqueues the kernel on `s` with `grid` blocks; start / stop as hipExtLaunchKernel takes them.
// Read-only on the scene.  n > 0, grid > 0.
hipError_t launch(const Scene& S, const Launch& L, int k, uint32_t grid, hipStream_t s, hipEvent_t start, hipEvent_t stop);

}  // namespace rtclosest
