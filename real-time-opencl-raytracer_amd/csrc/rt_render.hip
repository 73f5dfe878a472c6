// rt_render.hip -- MI355X (gfx950) render path: device layouts, kernels, C ABI.
//
// Replaces the reference's per-pixel OpenCL kernel raytracer_bvh
// (x64/Release/volumeRender.cl:1043-1547) and its host glue (RayTracer.cpp).
// Results follow the reference kernel's arithmetic exactly (S_ref,
// the reference as its host builds it, by default; S_strict and S_hw by flag);
// what changes is how the data sits in HBM and how the traversal is scheduled:
//
//  * inner BVH nodes are re-laid out as 64-B records that carry BOTH child
//    boxes plus the two child references (one 64-B fetch per inner visit
//    instead of the reference's 16 B node word + 2 x 32 B child boxes in two
//    dependent rounds, volumeRender.cl:836-867);
//  * a child reference encodes leaf-ness and the leaf's triangle range, so a
//    leaf never costs a node fetch;
//  * triangle references are expanded into 48-B {v0, e1, e2, id} records in
//    leaf order (the reference's 4-level ref -> index -> vertex gather,
//    volumeRender.cl:965-974, becomes one contiguous 48-B read);
//  * per-triangle shading data (3 vertices, 3 normals, albedo) is one 112-B
//    record (volumeRender.cl:1306-1374 gathers from five arrays);
//  * the 65-entry traversal stack (volumeRender.cl:636) lives in LDS for its
//    first RTK_LDS_STACK entries, laid out [entry][lane] (bank-conflict free),
//    the rest spills to a per-pixel global region; the top of stack stays in a
//    register.  Stack semantics (including the overflow -> miss rule at 65)
//    are the reference's, entry for entry;
//  * one wave = one 8x8 pixel tile (the reference's work-group, lanes in Morton
//    order), 4 waves per block; each lane takes one step of its own reference
//    sequence per iteration (traverse_ifif), so a wave's length is its slowest
//    ray, not the sum of its lanes' leaf rounds;
//  * blocks run longest-first, ordered by the previous frame's per-block times;
//    the frame's last-finishing block builds that order in-kernel (no extra launch);
//  * frame scratch is per stream, so frames enqueued on different streams run
//    concurrently (frames in flight; multi-GPU band gather overlaps rendering).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "rt_abi.h"
#include "rt_records.h"
#include "rt_refit.h"
#include "refit.hpp"
#include "scene_encode.hpp"
#include "rt_lbvh.h"
#include "rt_scene_build.h"
#include "rt_sah.h"
#include "rt_closest.h"
#include "lbvh_core.hpp"
#define MULTIHIT_HD __device__ __forceinline__
#include "multihit_core.hpp"

#ifndef RTK_WF_WAVES
#define RTK_WF_WAVES 7      // waves per SIMD the wavefront kernels are bounded to
#endif
#ifndef RTK_FBN_REF_WAVES
#define RTK_FBN_REF_WAVES 8 // waves per SIMD the S_ref depth > 1 first-bounce kernel is bounded to
#endif
#ifndef RTK_WFB_REF_WAVES
#define RTK_WFB_REF_WAVES 8 // waves per SIMD the S_ref bounce kernel is bounded to
#endif
#ifndef RTK_WF_GRID_PCT
#define RTK_WF_GRID_PCT 50  // persistent bounce grid, percent of the blocks the chip holds at once (C5 with
                            // 8 frames per launch: 38 / 44 / 50 / 56 / 62 / 68 / 75 % -> 0.758 / 0.752 / 0.750 / 0.753 /
                            // 0.755 / 0.760 / 0.757 ms, one frame per launch 0.827 vs 0.836 at 75 %, one frame alone
                            // 1.28 vs 1.25: profiles/r06/ab/c5_grid_pct_ab*.txt; round 4 at one frame per launch: 75 %)
#endif
#ifndef RTK_QUERY_REF_WAVES
#define RTK_QUERY_REF_WAVES 8   // waves per SIMD the S_ref query kernels are bounded to (no scratch at 8: DESIGN.md 18)
#endif
#ifndef RTK_QUERY_WAVES
#define RTK_QUERY_WAVES 7       // the same for S_strict / S_hw, as their other kernels
#endif
#ifndef RTK_QATTR_REF_WAVES
#define RTK_QATTR_REF_WAVES 8   // waves per SIMD the S_ref attribute query kernels are bounded to (no scratch: DESIGN.md 19)
#endif
#ifndef RTK_QATTR_WAVES
#define RTK_QATTR_WAVES 7       // the same for S_strict / S_hw
#endif
#ifndef RTK_FAN_REF_WAVES
#define RTK_FAN_REF_WAVES 8     // waves per SIMD the S_ref fan kernels are bounded to (no scratch: DESIGN.md 21)
#endif
#ifndef RTK_FAN_WAVES
#define RTK_FAN_WAVES 6         // the same for S_strict / S_hw: at 7 their fast kernels spill 12 / 24 B
#endif
#ifndef RTK_MULTIHIT_REF_WAVES
// waves per SIMD S_ref's multihit_kernel<k> is bounded to: the most at which it has no scratch
#define RTK_MULTIHIT_REF_WAVES(k) ((k) <= 2 ? 8 : (k) == 3 ? 7 : (k) == 4 ? 6 : (k) <= 7 ? 5 : 4)
#endif
#ifndef RTK_MULTIHIT_WAVES
#define RTK_MULTIHIT_WAVES(k) ((k) == 1 ? 8 : (k) == 2 ? 7 : (k) == 3 ? 6 : (k) <= 5 ? 5 : 4)   // the same for S_strict / S_hw
#endif
#ifndef RTK_QUERY_GRID_PCT
#define RTK_QUERY_GRID_PCT 75   // persistent query grid, percent of the blocks the chip holds at once (C3's 2.07 M primary
                                // rays, closest hit / incoherent rays: 50 % 0.248 / 0.955 ms, 75 % 0.232 / 0.998, 100 % 0.242 /
                                // 1.040: DESIGN.md 18)
#endif
#ifndef RTK_FB_WAVES
#define RTK_FB_WAVES 8      // waves per SIMD the S_ref depth-1 kernel is bounded to
#endif
#ifndef RTK_EXT_EVENTS
#define RTK_EXT_EVENTS 1    // one-launch frames: timing events from hipExtLaunchKernel, no marker packets
                            // around the launch (C2 0.0747 vs 0.0764 ms, rt_render into pageable memory 0.527
                            // vs 0.548 ms; C3, C5 equal: profiles/r05/ab/ext_events_ab.log)
#endif
#ifndef RTK_LDS_STACK
#define RTK_LDS_STACK 16    // LDS part of the traversal stack (C3 peaks at 9; deeper rays restart)
#endif
#ifndef RTK_XFRAME
#define RTK_XFRAME 1        // a batch launch's bounce queues tile-major, frame-minor (first_bounce_batch_kernel; 0: frame-major)
#endif

namespace rtk {

constexpr int kStackSize = 65;                       // volumeRender.cl:636
constexpr float kTmin = 0.001f;                      // volumeRender.cl:640
using rtrec::kCntEscape;
using rtrec::kLeafBit;
using rtrec::kRefError;
constexpr int kLdsStack = RTK_LDS_STACK;
constexpr int kGlobalStack = 64 - kLdsStack;         // slots kLdsStack..63
// Rows of a lane's LDS column below entry 0.  The fast traversal (traverse_ifif) writes slot
// sc - 2 and reads slot sc - 3 on every trip, whatever they hold; at stack counts 1 and 2 those
// are rows -1 and -2, which exist so that neither address needs a clamp.  No row is needed above:
// a trip starts with sc <= kLdsStack + 1 (a deeper stack has left the loop), so the highest row it
// writes is entry kLdsStack - 1.  18 KiB per block: 8 blocks fit a CU's 160 KiB.
constexpr int kLdsGuard = 2;
constexpr int kLdsRows = kLdsGuard + kLdsStack;
constexpr uint32_t kBlockPx = 16;                    // a block = 2 x 2 tiles of 8 x 8 pixels
constexpr uint32_t kBlockThreads = 256;              // every frame kernel's block: 4 waves, one tile each

struct DevScene {
    const float4* __restrict__ wnodes;   // [n_inner][4]
    const float4* __restrict__ tris;     // [n_refs][3] triangle reference records (tri_rec)
    const float4* __restrict__ shade;    // [n_tris][7]
    const int2* __restrict__ leaf_table; // escape leaves {offset, count}
    uint32_t tri_off;                    // byte offset of tris from wnodes (one allocation)
    uint32_t rec_bytes;                  // bytes of that allocation
    uint32_t root;
    uint32_t n_inner;                    // inner records; the first ones are the BVH's top levels (BFS order)
    int fast_div;                        // every box coordinate is 0 or in [2^-66, 2^60], every child box min <= max
    int clean;                           // no reachable malformed inner node (kRefError)
};

// Triangle reference record k (leaf order): {v0.xyz, id}, {e1}, {e2}, 48 B.  (A 40-B
// record -- two 16-B loads + one 8-B load -- measured 5.6 % slower on C3: DESIGN.md 6.2.)
__device__ __forceinline__ const float4* tri_rec(const DevScene& S, int k) { return S.tris + (size_t)k * 3; }

struct Frame {
    float3 a, b, c, campos, light_pos, smin, smax;
    uint32_t w, h;
    int32_t depth;
    uint32_t flags;
    int32_t rank, nranks, band_rows;
    uint32_t local_rows;
    uint32_t tiles_x, tiles_y, num_blocks;   // blocks of kBlockPx x kBlockPx pixels
    const uint32_t* tile_order;   // [num_blocks] block -> tile (static column strips, or longest-first)
    uint32_t* tile_cost;          // [num_blocks] per-tile time of this frame (adaptive order), or null
    uint32_t* lpt_next;           // [num_blocks] longest-first order for the next frame on this slot
    uint32_t* done;               // blocks finished so far (the last one builds lpt_next)
    uint32_t* zero_next;          // the other parity's frame counters, zeroed by this frame
    uint32_t nzero;
};

// A ray in flight between bounces: {pix, o.xyz}, {d.xyz, shadow_sum}, {colour.xyz, 3 * triangle it leaves from}.
struct QRay {
    float4 a, b, c;
};
// Ray queues are SEGMENTED: segment s holds slots [64 s, 64 s + 64) and the rays one wave
// appended, packed from its first slot; seg_cnt[s] says how many.  The producer's wave of
// segment s is a screen tile's 8x8 pixels (bounce 0) or the 64-ray group s of the previous
// bounce's order, so the segments are in screen order and no append contends for a counter.
// The producer also adds each count to its chunk's (kChunkSegs segments) and super-chunk's (1024
// segments) sum, from which wf_compact_sort_kernel's blocks find where their chunk starts
// in the bounce's dense order `perm` (compacted, optionally sorted), with no scan launch.
#ifndef RTK_SORT_SCALE
#define RTK_SORT_SCALE 4    // bounce sort: 2 x this many direction buckets over [-1, 1], one frame per launch
#endif
#ifndef RTK_SORT_SCALE_BATCH
#define RTK_SORT_SCALE_BATCH 8   // the same for launches of >= 4 frames (a chunk holds one tile of every frame, RTK_XFRAME:
                                 // C5 0.744 vs 0.753 ms with 8 buckets; one frame per launch loses with 16: profiles/r06/ab/)
#endif
#ifndef RTK_CHUNK_SEGS
#define RTK_CHUNK_SEGS 32   // segments per sort chunk (C5: 16 -> 0.900 ms, 32 -> 0.881, 64 -> 0.900; profiles/r04/ab/sort_chunk_ab.log)
#endif
constexpr uint32_t kChunkSegs = RTK_CHUNK_SEGS, kSuperSegs = 1024;
struct WQ {
    const QRay* in;           // this bounce's rays (segmented)
    const uint32_t* in_count; // rays in it
    const uint32_t* perm;     // dense order of `in`: i -> slot
    QRay* out;                // next bounce's rays (null: none)
    uint32_t* seg_cnt;        // rays per segment of `out`
    uint32_t* chunk_sum;      // rays per kChunkSegs segments of `out` (zeroed per frame)
    uint32_t* super_sum;      // rays per kSuperSegs segments of `out` (zeroed per frame)
    uint32_t seg;             // the segment this wave appends to (set per wave)
    uint32_t* seg_fill;       // the wave's LDS word: rays appended to `seg` so far
    uint32_t* fetch;          // the launch's work cursors (grab_group)
    int bounce;
};
constexpr uint32_t kSegRays = 64;

// Work distribution of the persistent wavefront kernels: a wave takes the next 64-ray group of
// a queue from one of eight cursors, 128 B apart (its block's group of XCD-sharing blocks,
// blockIdx % 8; MI355X_MICROARCH.md: blocks b and b + 8 share an XCD); cursor c hands out the
// groups c, c + 8, c + 16, ..., so all XCDs work through the queue's screen order together, and a
// wave whose cursor is used up takes from the next one.  One cursor for the whole chip
// serialises every grab on one address: ~8 ns each, 30 k grabs per C5 bounce launch
// (C5: 0.904 vs 0.924 ms per frame, profiles/r04/ab/split_cursor_ab.log; a persistent pass that
// only shaded C5's bounce-1 queue took 0.25 ms on one cursor, 0.16 ms on eight).
constexpr uint32_t kCursors = 8, kCursorStride = 32;
constexpr size_t kCursorSet = (size_t)kCursors * kCursorStride;
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t grab_group(uint32_t* cursors, uint32_t ngroups, uint32_t& home) {
    uint32_t g = kNoGroup, h = home;
    if ((threadIdx.x & 63u) == 0) {
        for (uint32_t k = 0; k < kCursors; ++k) {
            const uint32_t c = (h + k) & (kCursors - 1u);
            const uint32_t gg = c + kCursors * atomicAdd(cursors + c * kCursorStride, 1u);
            if (gg < ngroups) {
                g = gg;
                h = c;
                break;
            }
        }
    }
    home = __builtin_amdgcn_readfirstlane(h);
    return __builtin_amdgcn_readfirstlane(g);
}

// A ray query's launch (rt_trace_rays, query_kernel): rays are rt_ray as two float4 {o.xyz, tmax},
// {d.xyz, reserved}, hits rt_hit as one uint2 {id, t}; n <= 2^30, so ray and group indices fit 32 bits.
struct Query {
    const float4* rays;
    uint2* hits;
    uint32_t n;
    uint32_t* fetch;    // the launch's work cursors (grab_group), zeroed before it
};

// An occlusion fan's launch (rt_trace_fan, fan_kernel): origins are rt_fan_origin as two float4 {o.xyz,
// tmax}, {n.xyz, reserved}, dirs float4 {d.xyz, -}, masks one word per origin and 32-direction chunk,
// chunk-major (word (c, i) at c * n + i).  n <= 2^26 and k <= 4096, so the work items -- (64-origin
// group, chunk) pairs, ceil(n / 64) * chunks <= 2^27 -- fit grab_group's 32 bits.
struct Fan {
    const float4* origins;
    const float4* dirs;
    uint32_t* masks;
    uint32_t n, k, chunks;   // chunks = ceil(k / 32)
    uint32_t* fetch;         // the launch's work cursors (grab_group), zeroed before it
};

struct Outputs {
    uint32_t* out;
    int32_t* hits;
    float* t;
    float* rgb;
    uint32_t* gstack;            // [kGlobalStack][local_pixels]
    unsigned long long* overflow;
    uint32_t* restarts;          // traversals that outgrew the LDS stack and restarted (general code)
    uint64_t local_pixels;
    // measurement instantiation only (rt_fetch_counts, rt_loop_variant_counts): the frame's 8
    // record-fetch counters, then its kVariantCounts loop-variant counters
    unsigned long long* fcount;
    // depth-1 kernel only: out is the whole w x h frame (rt_render_tiled: every context writes
    // its bands' pixels straight into their rows of one frame); 0: out holds this rank's bands
    // (rt_tiling order), as for every other kernel
    uint32_t frame_rows;
    // diagnostic instantiation only (rt_wave_timeline): per wave {start, end, iterations, hw id}
    uint32_t* wtime;
};

// rt_render_device_batch: the cameras of a launch's frames, a kernel argument (read with uniform
// loads by first_bounce_batch_kernel), and the pixels between two frames' outputs.
constexpr int kMaxBatch = RT_MAX_BATCH;
struct BatchCam {
    float4 a, b, c, campos, light_pos;   // .w unused
};
struct BatchCams {
    BatchCam cam[kMaxBatch];
    uint64_t stride;      // pixels from one frame's output to the next
    uint32_t frame_px;    // pixels of one frame (this rank's): frame f's first pixel in the launch's pixel space
};

__device__ __forceinline__ void leaf_range(const DevScene& S, uint32_t ref, int& off, int& cnt) {
    uint32_t c = rtrec::ref_count(ref);
    if (c == kCntEscape) {
        int2 e = S.leaf_table[rtrec::ref_offset(ref)];
        off = e.x;
        cnt = e.y;
    } else {
        off = (int)rtrec::ref_offset(ref);
        cnt = (int)c;
    }
}

// The same range as byte offsets of the records in the fast traversal's allocation
// (triangle records after the inner records, 48 B each): [tk, tend).
// SHIFT (the depth-1 kernels): 48 x = (3 x) << 4 in two full-rate shift-adds, for any 32-bit x (an
// offset has 26 bits, an escape leaf's count is bounded only by the allocation: no 24-bit multiply);
// written out because the compiler turns the C++ of it into two v_mad_u64_u32 with a 64-bit addend
// (DESIGN.md 7.2), which the other kernels keep: the four shift-adds cost them scratch.
// tri_off: S.tri_off as the caller holds it (a VGPR copy where the scene's SGPRs do not survive the loop).
template <bool SHIFT>
__device__ __forceinline__ void leaf_bytes(const DevScene& S, uint32_t tri_off, uint32_t ref, uint32_t& tk, uint32_t& tend) {
    int off, cnt;
    leaf_range(S, ref, off, cnt);
    if (!SHIFT) {
        tk = tri_off + (uint32_t)off * 48u;
        tend = tk + (uint32_t)cnt * 48u;
        return;
    }
    uint32_t o3, c3;
    asm("v_lshl_add_u32 %0, %1, 1, %1" : "=v"(o3) : "v"(off));
    asm("v_lshl_add_u32 %0, %1, 1, %1" : "=v"(c3) : "v"(cnt));
    asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(tk) : "v"(o3), "v"(tri_off));
    asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(tend) : "v"(c3), "v"(tk));
}

// The walk references of the installed scene (rt_records.h), a trailing argument of the
// first-bounce kernels: the root's walk reference and the array's byte offset in the record
// allocation.  Only the depth-1 kernels read it (the host launches them only when off != 0); it is no
// part of DevScene so that every other kernel's arguments, and so its code, stay as they are.
struct Walk {
    uint32_t root, off;
};

struct Stack {
    uint32_t* lds;      // this lane's column: lds[i * 64], i >= -kLdsGuard
    uint32_t* glb;      // this pixel's column: glb[(i - kLdsStack) * gstride]
    uint64_t gstride;
    uint32_t* fc = nullptr;       // measurement instantiation: this lane's 8 fetch counters (LDS, stride 256)
    Walk walk{};                  // the depth-1 kernels' walk references (traverse_ifif with SEL); unused elsewhere
    unsigned long long* vc = nullptr;   // measurement instantiation: the frame's 18 loop-variant counters (traverse_fast)
    __device__ __forceinline__ uint32_t get(int i) const {
        return i < kLdsStack ? lds[i * 64] : glb[(uint64_t)(i - kLdsStack) * gstride];
    }
    __device__ __forceinline__ void put(int i, uint32_t v) const {
        if (i < kLdsStack) lds[i * 64] = v;
        else glb[(uint64_t)(i - kLdsStack) * gstride] = v;
    }
};

// Measurement instantiation only (rt_fetch_counts): one traversal iteration's
// record fetch of every active lane, counted per lane, per quad of lanes and per wave, by
// record kind; plus the wave's iterations and those that mix inner and triangle fetches.
// The vector-memory path merges the requests of the lanes of a QUAD (lanes 4k..4k+3) that
// read the same record (scripts/gather_peak_sweep.py: ~1.2 ns per CU per distinct record per
// quad, a wave-uniform record ~0.16 ns per lane), so its unit of work is a quad request.
// fc: this lane's counters [0/1] lane fetches inner/tri, [2/3] quad-distinct, [4/5]
// wave-distinct, [6] wave iterations, [7] mixed iterations; stride 256 (one block's lanes).
// vmem = false: a record the wave read once through the scalar cache (the traversal's
// wave-uniform prologue): a lane fetch and a wave-distinct record, but no quad request.
// After the 8 fetch counters O.fcount holds the frame's loop-variant counters (rt_loop_variant_counts,
// rt_kernel_body.inc traverse_fast): wave traversals through the generic loop and the 8 octant loops,
// closest-hit then any-hit.
constexpr int kFetchCounts = 8, kVariantCounts = 18;
__device__ __forceinline__ void fetch_count(uint32_t* fc, bool leaf, uint32_t id, bool vmem = true) {
    const uint64_t act = __builtin_amdgcn_read_exec();
    const int lane = (int)(threadIdx.x & 63u);
    bool quad_first = true, wave_first = true;
    for (int j = 0; j < 64; ++j) {   // a lower active lane reading the same record makes this a repeat
        const uint32_t b = (uint32_t)__shfl((int)id, j);
        if (j < lane && ((act >> j) & 1ull) && b == id) {
            wave_first = false;
            if ((j >> 2) == (lane >> 2)) quad_first = false;
        }
    }
    const uint64_t lm = __builtin_amdgcn_ballot_w64(leaf);
    const int t = leaf ? 1 : 0;
    fc[t * 256] += 1u;
    fc[(2 + t) * 256] += (vmem && quad_first) ? 1u : 0u;
    fc[(4 + t) * 256] += wave_first ? 1u : 0u;
    if (lane == (int)__builtin_ctzll(act)) {
        fc[6 * 256] += 1u;
        fc[7 * 256] += (lm != 0 && (act & ~lm) != 0) ? 1u : 0u;
    }
}

// a block's counters (every thread's 8, stride 256) to the frame's 8 (one thread each)
__device__ __forceinline__ void fetch_count_flush(const uint32_t* fc_block, unsigned long long* out) {
    __syncthreads();
    if (threadIdx.x < 8) {
        unsigned long long sum = 0;
        for (int i = 0; i < 256; ++i) sum += fc_block[threadIdx.x * 256 + i];
        atomicAdd(out + threadIdx.x, sum);
    }
}

// local row -> frame row under rt_tiling (bands of band_rows rows, band b -> rank b % nranks)
__device__ __forceinline__ uint32_t frame_row(const Frame& F, uint32_t lr) {
    if (F.nranks <= 1) return lr;
    const uint32_t band = lr / (uint32_t)F.band_rows, rib = lr % (uint32_t)F.band_rows;
    return (band * (uint32_t)F.nranks + (uint32_t)F.rank) * (uint32_t)F.band_rows + rib;
}

// Diagnostic instantiation only (rt_wave_timeline, TR = 2).  Each wave keeps kTlWords LDS words:
// [0] / [1] closest-hit main-loop / wave-uniform-prologue trips, [2] / [3] the same for the shadow
// (any-hit) traversal, [4] s_memrealtime when the closest-hit traversal returned, [5] when the
// shading was done (the shadow traversal starts), [6] when the closest-hit traversal started,
// [7] when its wave-uniform prologue ended; with RTK_TL_SPLIT (a diagnostic build) [8] / [9] the
// closest-hit / shadow main loop's ticks between issuing a trip's record loads and their arrival
// (the trip's memory wait), [10] / [11] those trips' count whose wait was >= kTlLongWait ticks;
// trips counted and times taken by the wave's first active lane.  (In a persistent bounce wave:
// trips over all its groups, times of its last.)
#ifndef RTK_TL_SPLIT
#define RTK_TL_SPLIT 0
#endif
constexpr uint32_t kTlWords = 12, kTlRecord = 20, kTlLongWait = 25;
__device__ __forceinline__ void timeline_step(uint32_t* c, int which) {
    if ((uint32_t)(threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec())) c[which] += 1u;
}
__device__ __forceinline__ void timeline_wait(uint32_t* c, int which, uint32_t ticks) {
    if ((uint32_t)(threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec())) {
        c[8 + which] += ticks;
        c[10 + which] += ticks >= kTlLongWait ? 1u : 0u;
    }
}
__device__ __forceinline__ void timeline_mark(uint32_t* c, int which) {
    if ((uint32_t)(threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec()))
        c[which] = (uint32_t)__builtin_amdgcn_s_memrealtime();
}
// ... and its record (kTlRecord words, wave w of the launch): [0] s_memrealtime (100 MHz, low 32
// bits) at its start, [1] closest hit done, [2] shading done, [3] end of its rays, [4] its end (after
// the block epilogue); [5..8] the four trip counts; [9] HW_REG_XCC_ID; [10] HW_REG_HW_ID (CU, SIMD,
// wave slot); [11] a tag (the tile, or the bounce kernel's 64-ray groups); [12] closest-hit traversal
// start, [13] end of its prologue; [16..19] the RTK_TL_SPLIT words [8..11].  Stamps go to their own
// buffer only; nothing the frame computes reads them.
__device__ __forceinline__ void timeline_store(const Outputs& O, uint32_t w, uint32_t t0, uint32_t t1,
                                               const uint32_t* c, uint32_t tag) {
    const uint32_t t2 = (uint32_t)__builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63u) == 0) {
        uint4* r = reinterpret_cast<uint4*>(O.wtime + (size_t)w * kTlRecord);
        r[0] = make_uint4(t0, c[4], c[5], t1);
        r[1] = make_uint4(t2, c[0], c[1], c[2]);
        r[2] = make_uint4(c[3], (uint32_t)__builtin_amdgcn_s_getreg(20 | (15 << 11)),
                          (uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)), tag);
        r[3] = make_uint4(c[6], c[7], 0u, 0u);
        r[4] = make_uint4(c[8], c[9], c[10], c[11]);
    }
}

// The block's tile.  (Read through the scalar cache instead, with the block size a constant, the
// wave set-up took 6.4 vs 7.3 us, but no config gained: DESIGN.md 7.5.)
__device__ __forceinline__ uint32_t block_tile(const Frame& F) { return F.tile_order[blockIdx.x]; }

// Lane -> pixel inside a block's 16x16 pixels: wave w holds 8x8 tile (w % 2, w / 2), lanes
// in Morton order.  The vector-memory path merges the requests of the four lanes of a quad
// that read the same record (measured 3.7x cheaper per lane than four distinct records,
// scripts/micro/share_fetch.hip), so every quad is a 2x2 pixel square, the pixels most
// likely to walk the same nodes.  Which lane holds which pixel never changes results.
__device__ __forceinline__ void tile_pixel(const Frame& F, uint32_t tb, int wave, int l, uint32_t& x, uint32_t& lr) {
    const uint32_t tx = tb % F.tiles_x, ty = tb / F.tiles_x;
    const uint32_t lx = (uint32_t)((l & 1) | ((l >> 1) & 2) | ((l >> 2) & 4));
    const uint32_t ly = (uint32_t)(((l >> 1) & 1) | ((l >> 2) & 2) | ((l >> 3) & 4));
    x = tx * kBlockPx + (uint32_t)(wave & 1) * 8u + lx;
    lr = ty * kBlockPx + (uint32_t)(wave >> 1) * 8u + ly;
}

// The frame's counters come in two parity sets; frame f uses set f & 1 and clears the
// other one for frame f + 1 on the same stream (the kernels of f never touch it), so no
// launch is spent on zeroing.
__device__ __forceinline__ void zero_next_counters(const Frame& F) {
    const uint32_t bd = blockDim.x;
    const uint32_t n = gridDim.x * bd;
    for (uint32_t i = blockIdx.x * bd + threadIdx.x; i < F.nzero; i += n) F.zero_next[i] = 0u;
}

// Append to the wave's own segment: the active lanes get the next slots of segment `seg`,
// in lane order.  The fill count is an LDS word of the wave, taken by the group's first
// lane, so lanes that arrive in separate groups (if the wave has not reconverged) still
// get distinct slots.
__device__ __forceinline__ QRay* seg_slot(QRay* q, uint32_t seg, uint32_t* fill) {
    const uint64_t m = __builtin_amdgcn_ballot_w64(true);
    const int lane = threadIdx.x & 63;
    const int leader = __builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(fill, (uint32_t)__builtin_popcountll(m));
    base = (uint32_t)__shfl((int)base, leader);
    return q + (size_t)seg * kSegRays + base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
}
// (all 64 lanes, after the wave's appends) the segment's count, also added to its chunk's
// and super-chunk's sums; the fill word is reset for the wave's next segment
__device__ __forceinline__ void seg_close(const WQ& W, uint32_t seg) {
    if ((threadIdx.x & 63u) == 0) {
        const uint32_t c = *W.seg_fill;
        W.seg_cnt[seg] = c;
        if (c) {
            atomicAdd(W.chunk_sum + seg / kChunkSegs, c);
            atomicAdd(W.super_sum + seg / kSuperSegs, c);
        }
        *W.seg_fill = 0u;
    }
}

// Longest-first block order (LPT list scheduling): the hardware hands blocks to free CU
// slots in blockIdx order, so dispatching the blocks that took longest last frame first
// leaves only short blocks for the tail.  Key: log2 of the cost with 3 mantissa bits
// (256 buckets, largest first).
__device__ __forceinline__ uint32_t lpt_key(uint32_t c) {
    if (c == 0) return 0;
    const uint32_t e = 31u - __builtin_clz(c);
    const uint32_t m = e >= 3 ? (c >> (e - 3)) & 7u : (c << (3 - e)) & 7u;
    return min(255u, e * 8u + m);
}

// End of every block of a frame's tile kernel (all 256 threads).  The block's wall time
// (max over its waves) goes to tile_cost[tb]; the block that finishes last sorts all of
// them into the next frame's order (a 256-bucket counting sort), so the order costs no
// launch of its own.  Inter-workgroup hand-off (MI355X_MICROARCH.md, visibility table
// row 1): one lane per block stores its cost write-through (sc1), waits for the store,
// then adds to one agent-scope counter; the block whose add returns num_blocks - 1 is
// last, acquires, and reads every cost with sc1 loads.  `scratch` is >= kEpilogueWords
// words of LDS that no wave uses any more (the traversal stacks); the rest of it holds the
// costs' bucket keys, one byte per block, between the two passes (grids of up to kKeyBytes
// blocks: every BASELINE config at 1080p; larger grids read the costs twice).
// The last block's sort sits at the very end of the frame, on its critical path: its costs
// are read 16 per thread per round trip (four 16-B sc1 loads issued together), not one load
// and one LDS atomic per round trip (RTK_LPT_VEC 0: 2 x 32 dependent L2 round trips for a
// 1080p frame's 8,160 blocks).
#ifndef RTK_LPT_VEC
#define RTK_LPT_VEC 1
#endif
constexpr int kEpilogueWords = 8 + 256 + 2 * 256;   // wave times + flag, histogram, two scan rows
static_assert(4 * kLdsStack * 64 >= kEpilogueWords, "tile_epilogue's scratch must fit the blocks' traversal stacks");
constexpr uint32_t kKeyBytes = (4u * kLdsStack * 64u - (uint32_t)kEpilogueWords) * 4u;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// costs [4 q, 4 q + 4) .. for q = q0 + u * 256 + tid, u < 4, with four sc1 loads in flight
// (inline asm: the compiler neither merges nor splits the 16-B agent-scope loads)
__device__ __forceinline__ void load_costs16(const uint32_t* cost, uint32_t q0, uint32_t nq, u32x4 (&v)[4]) {
    const u32x4* c4 = reinterpret_cast<const u32x4*>(cost);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const u32x4* p = c4 + min(q0 + (uint32_t)u * 256u + threadIdx.x, nq - 1u);   // in range (a repeat if past)
        asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v[u]) : "v"(p) : "memory");
    }
    // the wait "writes" the four results, so no use of them is scheduled above it
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : : "memory");
}
__device__ void tile_epilogue(const Frame& F, uint32_t tb, uint32_t t_start, uint32_t* scratch) {
    if (!F.tile_cost) return;   // launch-uniform
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t t_end = (uint32_t)__builtin_amdgcn_s_memrealtime();
    __syncthreads();   // every wave is done with the stacks
    if (lane == 0) scratch[wave] = t_end - t_start + 1u;
    __syncthreads();
    if (tid == 0) {
        const uint32_t c = max(max(scratch[0], scratch[1]), max(scratch[2], scratch[3]));
        __hip_atomic_store(F.tile_cost + tb, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the cost has landed before the block counts itself done: the last block reads every cost
        // (letting the store and the add fly together measured equal: DESIGN.md 7.5)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t prev = __hip_atomic_fetch_add(F.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        scratch[4] = prev + 1u == gridDim.x ? 1u : 0u;
    }
    __syncthreads();
    if (!scratch[4]) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    uint32_t* hist = scratch + 8;      // [256]
    uint32_t* scan = hist + 256;       // [2][256]
    const uint32_t nb = gridDim.x;   // the order's entries: every block of the launch (all frames of a batch)
    hist[tid] = 0;
    __syncthreads();
#if RTK_LPT_VEC
    uint8_t* kb = reinterpret_cast<uint8_t*>(scratch + kEpilogueWords);
    const bool keep = nb <= kKeyBytes;
    const uint32_t nq = nb >> 2;   // whole 16-B groups of costs
    for (uint32_t q0 = 0; q0 < nq; q0 += 4u * 256u) {
        u32x4 v[4];
        load_costs16(F.tile_cost, q0, nq, v);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t q = q0 + (uint32_t)u * 256u + tid;
            if (q < nq) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t k = lpt_key(v[u][j]);
                    atomicAdd(&hist[k], 1u);
                    if (keep) kb[4u * q + (uint32_t)j] = (uint8_t)k;
                }
            }
        }
    }
    for (uint32_t i = 4u * nq + tid; i < nb; i += 256u) {
        const uint32_t k = lpt_key(__hip_atomic_load(F.tile_cost + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        atomicAdd(&hist[k], 1u);
        if (keep) kb[i] = (uint8_t)k;
    }
#else
    for (uint32_t i = tid; i < nb; i += 256)
        atomicAdd(&hist[lpt_key(__hip_atomic_load(F.tile_cost + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))], 1u);
#endif
    __syncthreads();
    // exclusive prefix over the buckets, largest key first (Hillis-Steele on 256 lanes)
    scan[tid] = hist[255 - tid];
    __syncthreads();
    int src = 0;
    for (uint32_t off = 1; off < 256; off <<= 1) {
        scan[(src ^ 1) * 256 + tid] = scan[src * 256 + tid] + (tid >= off ? scan[src * 256 + tid - off] : 0u);
        __syncthreads();
        src ^= 1;
    }
    hist[255 - tid] = scan[src * 256 + tid] - hist[255 - tid];   // inclusive -> exclusive
    __syncthreads();
#if RTK_LPT_VEC
    if (keep) {
        for (uint32_t i = tid; i < nb; i += 256u) F.lpt_next[atomicAdd(&hist[kb[i]], 1u)] = i;
    } else {
        for (uint32_t q0 = 0; q0 < nq; q0 += 4u * 256u) {
            u32x4 v[4];
            load_costs16(F.tile_cost, q0, nq, v);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t q = q0 + (uint32_t)u * 256u + tid;
                if (q < nq) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) F.lpt_next[atomicAdd(&hist[lpt_key(v[u][j])], 1u)] = 4u * q + (uint32_t)j;
                }
            }
        }
        for (uint32_t i = 4u * nq + tid; i < nb; i += 256u) {
            const uint32_t c = __hip_atomic_load(F.tile_cost + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            F.lpt_next[atomicAdd(&hist[lpt_key(c)], 1u)] = i;
        }
    }
#else
    for (uint32_t i = tid; i < nb; i += 256) {
        const uint32_t c = __hip_atomic_load(F.tile_cost + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        F.lpt_next[atomicAdd(&hist[lpt_key(c)], 1u)] = i;
    }
#endif
    if (tid == 0) __hip_atomic_store(F.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- math-independent kernels ----

// Dense order of a segmented queue (wf_compact_sort_kernel): block b takes the kChunkSegs (32)
// segments [32 b, 32 b + 32), i.e. 2048 slots of one screen-local region (8 tiles of 16x16 pixels at
// bounce 1), finds where its rays start in the dense order from the super-chunk and chunk
// sums before it (d0), and writes perm[d0 ..] with their slots, in slot order -- or with
// `sort` (RT_FLAG_WF_SORT), stably by the
// component of the ray's direction along the scene box's thinnest axis (8 buckets of width
// 1/4).  Rays that leave the scene's slab steeply take few steps, rays running along it
// many: grouping them by that component puts rays of similar length (and similar direction)
// into the same waves of 64, where a wave runs as long as its longest ray.  Simulated on
// C5's bounce queues (the oracle's per-ray step counts): wave iterations -26 % at bounce 1,
// -24 % at bounce 2 against the queue order with 32 buckets; measured, finer buckets cost
// more in lost fetch sharing between neighbouring rays than they save (C5 ms per frame,
// round 3 before the segmented queues: unsorted 1.000-1.002; 2 buckets 1.023, 4 0.970-0.972,
// 6 0.965, 8 0.968-0.970, 12 0.978, 16 0.983, 32 1.004-1.005; profiles/r03/c5_sort/).
// Stable: inside a bucket the rays keep their slot order, so neighbouring pixels (a quad's
// four rays, appended side by side) stay side by side and keep sharing their record fetches.
// Slot j = c0 + 256 p + t is ranked among the entries of its bucket by (pass p, wave, lane):
// peers in a wave by a ballot match on the key's bits, earlier waves and passes by LDS counts.
// The block of the queue's last segment stores the queue's size in *total.  nseg is
// `nseg_fixed` (bounce 1: the first bounce's waves), or when 0 the previous bounce's 64-ray
// groups, ceil(*prev_total / 64).
constexpr uint32_t kLocalSortChunk = kChunkSegs * kSegRays;
__global__ void __launch_bounds__(256) wf_compact_sort_kernel(const QRay* __restrict__ q,
                                                              const uint32_t* __restrict__ seg_cnt,
                                                              const uint32_t* __restrict__ chunk_sum,
                                                              const uint32_t* __restrict__ super_sum, uint32_t nseg_fixed,
                                                              const uint32_t* __restrict__ prev_total,
                                                              uint32_t* __restrict__ total_out, uint32_t* __restrict__ perm,
                                                              uint32_t axis, uint32_t sort) {   // sort: 0, or the key's scale
    constexpr uint32_t kPasses = kLocalSortChunk / 256;
    constexpr uint32_t kBuckets = 2 * (RTK_SORT_SCALE > RTK_SORT_SCALE_BATCH ? RTK_SORT_SCALE : RTK_SORT_SCALE_BATCH);
    constexpr int kKeyBits = kBuckets <= 2 ? 1 : kBuckets <= 4 ? 2 : kBuckets <= 8 ? 3 : kBuckets <= 16 ? 4 : 5;
    static_assert((kBuckets & (kBuckets - 1)) == 0 && kBuckets <= 32, "the key's buckets: a power of two, <= 32");
    __shared__ uint32_t cnt[kBuckets][kPasses * 4];   // [bucket][pass * 4 + wave]: entries, then their offsets
    __shared__ uint32_t total[kBuckets];
    __shared__ uint32_t segc[kChunkSegs];
    __shared__ uint32_t part[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t nseg = nseg_fixed ? nseg_fixed : (*prev_total + kSegRays - 1) / kSegRays;
    const uint32_t b = blockIdx.x, s0 = b * kChunkSegs;
    if (s0 >= nseg) return;   // the grid covers the queue's capacity
    const uint32_t c0 = s0 * kSegRays;
    // d0 = rays in the super-chunks, then the chunks of this super-chunk, before this chunk
    constexpr uint32_t kChunksPerSuper = kSuperSegs / kChunkSegs;
    const uint32_t nsup = b / kChunksPerSuper, nch = b % kChunksPerSuper;
    uint32_t x = 0;
    for (uint32_t i = t; i < nsup; i += 256) x += super_sum[i];
    if (t < nch) x += chunk_sum[nsup * kChunksPerSuper + t];
    for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_down((int)x, o);
    if (lane == 0) part[wave] = x;
    if (t < kChunkSegs) segc[t] = s0 + t < nseg ? seg_cnt[s0 + t] : 0u;
    for (uint32_t i = t; i < kBuckets * kPasses * 4; i += 256) (&cnt[0][0])[i] = 0u;
    __syncthreads();
    const uint32_t d0 = part[0] + part[1] + part[2] + part[3];
    uint32_t key[kPasses], rank[kPasses];
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t p = 0; p < kPasses; ++p) {
        const uint32_t j = c0 + 256u * p + t;   // one segment per wave and pass
        const bool valid = (j % kSegRays) < segc[(j - c0) / kSegRays];
        uint32_t k = 0;
        if (valid && sort) {
            const float4 b = q[j].b;   // {d.xyz, shadow sum}
            const float d = axis == 0 ? b.x : axis == 1 ? b.y : b.z;
            k = d == d ? (uint32_t)min(max((int)((d + 1.0f) * (float)sort), 0), 2 * (int)sort - 1) : 0u;
        }
        uint64_t peers = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
        for (int bit = 0; bit < kKeyBits; ++bit) {
            const uint64_t m = __builtin_amdgcn_ballot_w64((k >> bit) & 1u);
            peers &= ((k >> bit) & 1u) ? m : ~m;
        }
        key[p] = valid ? k : kBuckets;
        rank[p] = (uint32_t)__builtin_popcountll(peers & lt);
        if (valid && (peers & lt) == 0) cnt[k][p * 4 + wave] = (uint32_t)__builtin_popcountll(peers);
    }
    __syncthreads();
    if (t < kBuckets) {   // per bucket: exclusive prefix over (pass, wave)
        uint32_t acc = 0;
        for (uint32_t s = 0; s < kPasses * 4; ++s) {
            const uint32_t c = cnt[t][s];
            cnt[t][s] = acc;
            acc += c;
        }
        total[t] = acc;
    }
    __syncthreads();
    if (t == 0) {   // bucket starts (exclusive prefix over buckets), kept in total[]
        uint32_t acc = 0;
        for (uint32_t k = 0; k < kBuckets; ++k) {
            const uint32_t c = total[k];
            total[k] = acc;
            acc += c;
        }
        if (s0 + kChunkSegs >= nseg) *total_out = d0 + acc;   // the queue's last chunk
    }
    __syncthreads();
#pragma unroll
    for (uint32_t p = 0; p < kPasses; ++p)
        if (key[p] < kBuckets) perm[d0 + total[key[p]] + cnt[key[p]][p * 4 + wave] + rank[p]] = c0 + 256u * p + t;
}

// Random-record gather ceiling (rt_gather_peak): every lane of every wave
// reads a different pseudo-random record of the traversal's inner-record shape (three 16-B
// loads + one 8-B load, 56 of 64 B) from a table of `nrec` 64-B records, `iters` times, four
// records in flight per lane; every CU busy.  A table that fits the XCD's L2 gives the
// ceiling of distinct-record fetches the vector-memory path can serve.
__global__ void __launch_bounds__(256) gather_peak_kernel(const float4* __restrict__ table, uint32_t nrec,
                                                          uint32_t iters, uint32_t* __restrict__ sink) {
    uint32_t x = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 0x9E3779B9u;
    uint32_t acc = 0;
    for (uint32_t i = 0; i < iters; i += 4) {
        float4 q[4][3];
        float2 r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x ^= x << 13; x ^= x >> 17; x ^= x << 5;
            const float4* p = table + (size_t)(x % nrec) * 4;
            q[k][0] = p[0]; q[k][1] = p[1]; q[k][2] = p[2];
            r[k] = *reinterpret_cast<const float2*>(p + 3);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            acc ^= __float_as_uint(q[k][0].x) ^ __float_as_uint(q[k][1].y) ^ __float_as_uint(q[k][2].z) ^
                   __float_as_uint(r[k].y);
    }
    if (acc == 0x9E3779B9u) sink[blockIdx.x] = acc;   // keeps the loads; practically never taken
}

// Dependent-fetch latency (rt_chase_peak, the latency roof of DESIGN.md 6.3): every wave of
// 8 per SIMD on every CU walks `iters` steps of a chain through a table of inner-record-
// shaped 64-B records, like one traversal iteration each: three 16-B loads + one 8-B load
// of the current record, a slab-like dependent chain of packed ops on the boxes, and the
// next record chosen by the result between the record's two child references.  The lanes
// of a quad (group = 4) -- or `group` lanes -- follow one chain, as the lanes of a quad of
// coherent rays do.  Time per launch / iters = the time of one dependent iteration of a
// wave when every wave slot of the chip runs such a chain.
__global__ void __launch_bounds__(256) chase_peak_kernel(const float4* __restrict__ table, uint32_t nrec, uint32_t iters,
                                                         uint32_t group, uint32_t* __restrict__ sink) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    uint32_t idx = ((gid / group) * 2654435761u) % nrec;
    float acc = 0.0f;
    for (uint32_t i = 0; i < iters; ++i) {
        const float4* p = table + (size_t)idx * 4;
        const float4 q0 = p[0], q1 = p[1], q2 = p[2];
        const float2 r = *reinterpret_cast<const float2*>(p + 3);
        // both children's slab intervals from the loaded planes (dependent on the data)
        const float n0 = fmaxf(fmaxf(q0.x * 0.5f - acc, q1.x * 0.5f), q2.x * 0.5f);
        const float f0 = fminf(fminf(q0.z * 0.5f, q1.z * 0.5f - acc), q2.z * 0.5f);
        const float n1 = fmaxf(fmaxf(q0.y * 0.5f, q1.y * 0.5f - acc), q2.y * 0.5f);
        const float f1 = fminf(fminf(q0.w * 0.5f - acc, q1.w * 0.5f), q2.w * 0.5f);
        const bool left = (f0 - n0) >= (f1 - n1);
        idx = __float_as_uint(left ? r.x : r.y);
        acc = (n0 + f1) * 1e-30f;
    }
    if (idx == 0xFFFFFFFFu) sink[blockIdx.x] = __float_as_uint(acc);   // keeps the chain; never taken
}

// Band re-interleave on rank 0 (rt_assemble_bands[_batch]): one block per frame row and
// frame (grid h x nframes), 16-B copies when rows and slots are 16-B aligned.  Pure HBM
// copy: 8 B/pixel.  Rank r's slot starts at r * slot_pixels and holds the frames' band
// buffers frame_pixels apart.
__global__ void __launch_bounds__(256) assemble_bands_kernel(uint32_t* __restrict__ frame,
                                                             const uint32_t* __restrict__ slots, uint64_t slot_pixels,
                                                             uint64_t frame_pixels, uint32_t w, uint32_t h,
                                                             uint32_t nranks, uint32_t band_rows) {
    const uint32_t y = blockIdx.x;
    if (y >= h) return;
    const uint32_t band = y / band_rows;
    const uint32_t rank = band % nranks;
    const uint64_t local_row = (uint64_t)(band / nranks) * band_rows + (y % band_rows);
    const uint32_t* src = slots + (uint64_t)rank * slot_pixels + blockIdx.y * frame_pixels + local_row * w;
    uint32_t* dst = frame + (uint64_t)blockIdx.y * w * h + (uint64_t)y * w;
    if ((w & 3u) == 0 && (slot_pixels & 3u) == 0 && (frame_pixels & 3u) == 0) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (uint32_t i = threadIdx.x; i < w / 4; i += blockDim.x) d4[i] = s4[i];
    } else {
        for (uint32_t i = threadIdx.x; i < w; i += blockDim.x) dst[i] = src[i];
    }
}

// Band put (rt_bands_put): one block per local row of this rank's band buffer, written to
// its row of the frame -- a local frame, or rank 0's frame mapped over xGMI (HIP IPC), where
// whole 16-B-aligned rows make long write bursts.  Pure copy: 8 B/pixel.
__global__ void __launch_bounds__(256) bands_put_kernel(uint32_t* __restrict__ frame,
                                                        const uint32_t* __restrict__ bands, uint32_t w,
                                                        uint32_t local_rows, uint32_t rank, uint32_t nranks,
                                                        uint32_t band_rows) {
    const uint32_t lr = blockIdx.x;
    if (lr >= local_rows) return;
    const uint64_t y = (uint64_t)(lr / band_rows * nranks + rank) * band_rows + lr % band_rows;
    const uint32_t* src = bands + (uint64_t)lr * w;
    uint32_t* dst = frame + y * w;
    if ((w & 3u) == 0) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (uint32_t i = threadIdx.x; i < w / 4; i += blockDim.x) d4[i] = s4[i];
    } else {
        for (uint32_t i = threadIdx.x; i < w; i += blockDim.x) dst[i] = src[i];
    }
}

// ---- per-frame completion of the band puts (rt_bands_put_sync / rt_frame_present) ----
// The sync block lives in rank 0's memory, mapped into every rank with the frames:
//   [0] status (0 ok, 1 a put timed out waiting for its set, 2 a present timed out waiting
//   for the puts), [1] frames presented, [2 .. 2+nsets) release[set] (uses of the set rank 0
//   has presented), then arrive[set][rank] (uses of the set whose rows the rank has put).
// Every wait is bounded (s_memrealtime, 100 MHz): a lost peer ends in a status, never a hang;
// after the first failed wait every later one returns at once (the status is sticky).
constexpr uint32_t kSyncHead = 2;
__device__ __forceinline__ uint64_t now_ticks() { return __builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ uint32_t sys_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The first failure's code is kept: a later wait that returns early because the status is
// already set does not overwrite it (compare-and-swap from 0).
__device__ __forceinline__ void set_status(uint32_t* sync, uint32_t code) {
    uint32_t expect = 0u;
    __hip_atomic_compare_exchange_strong(sync, &expect, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_SYSTEM);
}

// rt_bands_put_sync: at most kPutBlocks blocks, each copying every gridDim.x-th local row.
// Before writing set `set` for its use `use` the put waits until rank 0 has presented the set's
// previous use (back-pressure: a peer never overwrites a frame rank 0 has not yet observed
// complete).  Round 5 found that wait starving a GPU shared by three ranks: every block of every
// waiting put spun, holding its CU slot, while the renders the wait depended on queued behind
// them.  Now (prewaited, the default, RTAMD_PUT_WAIT=wave) the wait is ONE wave of its own
// (put_wait_kernel, bounded by timeout_ticks, status 1 on expiry) enqueued before the put, and the
// put's blocks only check the status word.  RTAMD_PUT_WAIT=stream enqueues hipStreamWaitValue32
// instead -- on device memory that is not HSA signal memory ROCm runs that as its own polling blit
// kernel (__amd_rocclr_streamOpsWait, one per wait in a kernel trace, profiles/r06/qwait_trace/),
// i.e. the same single polling wave but without a bound; RTAMD_PUT_WAIT=kernel: every put block
// waits (round 5).  A present that times out poisons every release word (kReleasePoison) after
// setting the status, so waits in flight end and their puts, seeing the status, write nothing.
// After its rows, every block releases its stores at system scope (each XCD's L2 written back) and counts itself on this
// rank's own counter for the set; the block that completes the count publishes
// arrive[set][rank] = use + 1 with a system-scope release store.
constexpr uint32_t kPutBlocks = 64;
constexpr uint32_t kReleasePoison = 0x7FFFFFFFu;   // >= every use, signed or unsigned compare
__global__ void __launch_bounds__(256) bands_put_sync_kernel(uint32_t* __restrict__ frame,
                                                             const uint32_t* __restrict__ bands, uint32_t w,
                                                             uint32_t local_rows, uint32_t rank, uint32_t nranks,
                                                             uint32_t band_rows, uint32_t* sync, uint32_t* local,
                                                             uint32_t nsets, uint32_t set, uint32_t use,
                                                             uint64_t timeout_ticks, uint32_t prewaited) {
    __shared__ uint32_t s_abort;
    if (threadIdx.x == 0) {
        uint32_t ab = 0;
        if (prewaited) {
            ab = sys_load(sync) != 0u ? 1u : 0u;   // waited for before this launch; a failed exchange writes nothing
        } else if (use > 0) {
            const uint64_t t0 = now_ticks();
            while (sys_load(sync + kSyncHead + set) < use) {
                // once any wait has failed (status != 0) the exchange is over: no further wait
                if (sys_load(sync) != 0u || now_ticks() - t0 > timeout_ticks) {
                    set_status(sync, 1u);
                    ab = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
        }
        s_abort = ab;
    }
    __syncthreads();
    if (s_abort) return;   // the set's arrival is never published: rank 0's present times out too
    for (uint32_t lr = blockIdx.x; lr < local_rows; lr += gridDim.x) {
        const uint64_t y = (uint64_t)(lr / band_rows * nranks + rank) * band_rows + lr % band_rows;
        const uint32_t* src = bands + (uint64_t)lr * w;
        uint32_t* dst = frame + y * w;
        if ((w & 3u) == 0) {
            const uint4* s4 = reinterpret_cast<const uint4*>(src);
            uint4* d4 = reinterpret_cast<uint4*>(dst);
            for (uint32_t i = threadIdx.x; i < w / 4; i += blockDim.x) d4[i] = s4[i];
        } else {
            for (uint32_t i = threadIdx.x; i < w; i += blockDim.x) dst[i] = src[i];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: this block's rows are out of every cache
        const uint32_t prev = __hip_atomic_fetch_add(local + set, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev + 1u == (use + 1u) * gridDim.x) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __hip_atomic_store(sync + kSyncHead + nsets + set * nranks + rank, use + 1u, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// rt_bands_put_sync's wait for set `set`'s release (the default mode): one wave, its first lane
// polling, bounded; on expiry status 1 (the put that follows then writes nothing)
__global__ void __launch_bounds__(64) put_wait_kernel(uint32_t* sync, uint32_t set, uint32_t use, uint64_t timeout_ticks) {
    if (threadIdx.x != 0) return;
    const uint64_t t0 = now_ticks();
    while (sys_load(sync + kSyncHead + set) < use) {
        if (sys_load(sync) != 0u) return;   // the exchange has already failed
        if (now_ticks() - t0 > timeout_ticks) {
            set_status(sync, 1u);
            return;
        }
        __builtin_amdgcn_s_sleep(8);
    }
}

// rt_frame_present (rank 0, one wave): waits until every rank has published its rows of
// use `use` of set `set`, acquires them (system scope) and counts the frame as presented;
// with `release`, also releases the set for its next use (else rt_frame_release does, after
// the caller's consumers of the frame).
__global__ void __launch_bounds__(64) frame_present_kernel(uint32_t* sync, uint32_t nsets, uint32_t set, uint32_t use,
                                                           uint32_t nranks, uint64_t timeout_ticks, uint32_t release) {
    const uint32_t lane = threadIdx.x;
    const uint64_t t0 = now_ticks();
    bool ok = true;
    for (uint32_t r = lane; r < nranks; r += 64) {
        while (sys_load(sync + kSyncHead + nsets + set * nranks + r) < use + 1u) {
            if (sys_load(sync) != 0u || now_ticks() - t0 > timeout_ticks) { ok = false; break; }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    const bool all_ok = __builtin_amdgcn_ballot_w64(!ok) == 0;
    if (!all_ok) {
        if (lane == 0) set_status(sync, 2u);
        // every put waiting in a queue for a set's release goes on (and, seeing the status, writes nothing)
        for (uint32_t s2 = lane; s2 < nsets; s2 += 64)
            __hip_atomic_store(sync + kSyncHead + s2, kReleasePoison, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (lane == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        __hip_atomic_fetch_add(sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (release) __hip_atomic_store(sync + kSyncHead + set, use + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// rt_frame_release: rank 0 is done with use `use` of set `set`; the ranks may refill it.
__global__ void __launch_bounds__(64) frame_release_kernel(uint32_t* sync, uint32_t set, uint32_t use) {
    if (threadIdx.x == 0 && sys_load(sync) == 0u) {   // after a failure the sets stay poisoned (released for good)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // the frame's readers are done (stream order)
        __hip_atomic_store(sync + kSyncHead + set, use + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// rt_frame_checksum: a position-dependent 64-bit sum of a frame (a pixel in the wrong row,
// or a row from another frame, changes it), added into sums[index].
__global__ void __launch_bounds__(256) frame_checksum_kernel(const uint32_t* __restrict__ frame, uint64_t pixels,
                                                             unsigned long long* __restrict__ sums) {
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < pixels; i += (uint64_t)gridDim.x * 256u)
        acc += (((unsigned long long)frame[i] << 32) | (i & 0xFFFFFFFFull)) * 0x9E3779B97F4A7C15ull;
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if ((threadIdx.x & 63u) == 0) atomicAdd(sums, acc);
}

}  // namespace rtk

// Three instantiations of the math + kernels:
//   rtk_ref    (default)            S_ref: the reference as its host builds it
//   rtk_strict (RT_FLAG_STRICT_MATH) S_strict: CPU-reproducible, the oracle's arithmetic
//   rtk_hw     (RT_FLAG_HW_MATH)     S_hw: the reference built with correctly rounded / and sqrt
#define RTK_NS rtk_strict
#define RTK_MATH 0
#include "rt_device_math.h"
#include "rt_kernel_body.inc"
#undef RTK_NS
#undef RTK_MATH
#define RTK_NS rtk_hw
#define RTK_MATH 1
#include "rt_device_math.h"
#include "rt_kernel_body.inc"
#undef RTK_NS
#undef RTK_MATH
#define RTK_NS rtk_ref
#define RTK_MATH 2
#include "rt_device_math.h"
#include "rt_kernel_body.inc"
#undef RTK_NS
#undef RTK_MATH

// The walk references of a scene's inner records (rt_records.h), derived from the records just placed
// on the device: one thread per inner record, its two child references; thread 0 also the root's.
// status[0] != 0 afterwards: some reference has no walk form, the scene renders without the array;
// status[1]: the root's walk reference.  The host twin is rtamd::derive_walk (csrc/host/scene_encode.cpp).
namespace rtk {
__global__ void __launch_bounds__(256) derive_walk_kernel(const float4* __restrict__ wnodes, uint32_t n_rec,
                                                          const int2* __restrict__ leaf_table, uint32_t n_leaf, uint32_t tri_unit,
                                                          uint32_t n_refs, uint32_t root, uint2* __restrict__ walk,
                                                          uint32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int32_t* table = reinterpret_cast<const int32_t*>(leaf_table);
    bool bad = false;
    if (i < n_rec) {
        const float4 q3 = wnodes[(size_t)i * 4 + 3];
        const uint32_t w0 = rtrec::walk_ref(__float_as_uint(q3.x), table, n_leaf, n_rec, tri_unit, n_refs);
        const uint32_t w1 = rtrec::walk_ref(__float_as_uint(q3.y), table, n_leaf, n_rec, tri_unit, n_refs);
        walk[i] = make_uint2(w0, w1);
        bad = w0 == rtrec::kWalkNone || w1 == rtrec::kWalkNone;
    }
    if (i == 0) {
        const uint32_t wr = rtrec::walk_ref(root, table, n_leaf, n_rec, tri_unit, n_refs);
        status[1] = wr;
        bad = bad || wr == rtrec::kWalkNone;
    }
    if (bad) atomicOr(status, 1u);
}
}  // namespace rtk

// ============================================================================
// Host side: context, upload/repack, launch.
// ============================================================================

// A scene on the device and everything it owns.  `own` is the only place that holds
// an owning pointer of a scene array: the accessors return views, and nothing stores one.
struct Scene {
    enum { kRec, kTris, kShade, kLeaf, kIdx, kNormalIdx, kRefTri, kLevelIds, kLevelBegin, kOut, kVerts, kNormals, kCount };
    struct Owned {   // one allocation per kind, capacities in bytes; a move leaves the source empty, and there are no copies
        std::array<void*, kCount> p{};
        std::array<size_t, kCount> cap{};
        Owned() = default;
        Owned(Owned&& o) noexcept { *this = std::move(o); }
        Owned& operator=(Owned&& o) noexcept { p = std::exchange(o.p, {}); cap = std::exchange(o.cap, {}); return *this; }
    } own;
    bool pooled = false;          // rt_build_scene's allocations: released into the spare pool, not freed
    // records: kRec holds the inner records and, unless `split`, the triangle records right after them
    size_t n_wnodes4 = 0, n_tris4 = 0, n_shade4 = 0, n_leaf = 0;   // element counts of the scene arrays
    uint32_t root = 0, n_inner = 0;
    int fast_div = 0, clean = 0;
    bool split = false;           // records >= 2 GiB: two allocations (kRec, kTris), general traversal only
    // Walk references (rt_records.h), derived by install_scene from the records and no part of the scene
    // image: after the triangle records in kRec come two zero units (with the pad float4 that ends the
    // triangle records, one all-zero 48-B record), the array (8 B per inner record) and one status unit.
    // walk_off: the array's byte offset in kRec, 0: none (split records, or a reference without a walk form)
    uint32_t walk_root = 0, walk_off = 0;
    static size_t walk_units(size_t n_wnodes4) { return 2 + (n_wnodes4 / 4 + 1) / 2 + 1; }
    size_t walk_unit0() const { return n_wnodes4 + n_tris4 + 2; }   // the array's first 16-B unit
    size_t rec_units() const { return n_wnodes4 + n_tris4 + (split ? 0 : walk_units(n_wnodes4)); }
    bool have_bounds = false;     // rt_scene_bounds: the uploaded / built / refit root box
    rt_float4 bounds_min{}, bounds_max{};
    // Animated geometry (rt_update_vertices): a refittable scene keeps per-triangle vertex / normal
    // indices, the triangle of every reference record, the refit plan's level lists and
    // rtrefit::DevArgs::out (kIdx .. kOut), and the staging of the host form's arrays (kVerts,
    // kNormals: allocated on first use unless rt_build_scene brought them)
    bool refittable = false;
    std::string why = "no scene uploaded";   // why the scene has no refit data
    int32_t nv = 0, nnorm = 0;
    uint32_t nref = 0, ntri = 0;
    std::vector<uint32_t> level_begin;       // host copy: heights + 1 entries

    float4* wnodes() const { return (float4*)own.p[kRec]; }
    float4* tris() const { return split ? (float4*)own.p[kTris] : wnodes() + n_wnodes4; }
    float4* shade() const { return (float4*)own.p[kShade]; }
    int2* leaf() const { return (int2*)own.p[kLeaf]; }
    int32_t* idx() const { return (int32_t*)own.p[kIdx]; }
    int32_t* normal_idx() const { return (int32_t*)own.p[kNormalIdx]; }
    int32_t* ref_tri() const { return (int32_t*)own.p[kRefTri]; }
    uint32_t* level_ids() const { return (uint32_t*)own.p[kLevelIds]; }
    uint32_t* d_level_begin() const { return (uint32_t*)own.p[kLevelBegin]; }
    uint32_t* out() const { return (uint32_t*)own.p[kOut]; }
    float4* verts() const { return (float4*)own.p[kVerts]; }
    float4* normals() const { return (float4*)own.p[kNormals]; }
    // what a frame reads, in the scene image's order: {array, bytes}
    std::array<std::pair<void*, size_t>, 4> sections() const {
        return {{{wnodes(), n_wnodes4 * 16}, {tris(), n_tris4 * 16}, {shade(), n_shade4 * 16}, {leaf(), n_leaf * 8}}};
    }
};

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // per-frame timing events, a ring over the last kRing frames: e[0]/e[1] around all
    // kernels of the frame; e[2] after the main render kernel when more kernels follow it
    // (has_k; the main kernel is the frame's first, so it spans e[0]..e[2]).  Two records per
    // depth-1 frame: each costs host time on the per-frame path.
    struct FrameEv { hipEvent_t e[3] = {nullptr, nullptr, nullptr}; bool has_k = false; };
    static constexpr int kRing = 64;
    FrameEv ring[kRing];
    uint64_t frames = 0;
    Scene scene;                  // replaced by install_scene alone
    bool have_scene = false;
    // rt_build_scene's allocations of the scene a later call replaced, at most one per kind, for the
    // build after it: a mesh rebuilt again and again allocates and frees nothing
    Scene::Owned spare;
    bool have_params = false;
    rt_params params{};
    uint32_t* d_out = nullptr; size_t out_cap = 0;
    int32_t* d_hits = nullptr; size_t hits_cap = 0;
    float* d_t = nullptr; size_t t_cap = 0;
    float* d_rgb = nullptr; size_t rgb_cap = 0;
    unsigned long long* d_overflow = nullptr;
    // Per-stream frame scratch.  Frames enqueued on different streams may run
    // concurrently (frames in flight); each stream gets its own global stack,
    // frame counters, wavefront queues and adaptive-order state.  Frames on one
    // stream are ordered by it and share one slot.
    struct FrameSlot {
        void* stream = nullptr;
        uint64_t tkey = 0;                                                  // the tiling it renders (0: whole frame)
        uint64_t last_use = 0;
        hipEvent_t idle = nullptr;                                          // recorded after each frame
        uint64_t nframe = 0;                                                // frames rendered on this slot
        uint32_t* d_gstack = nullptr; size_t gstack_cap = 0;                // in pixels
        float4* d_wq[2] = {nullptr, nullptr}; size_t wq_cap[2] = {0, 0};   // wavefront ray queues (ping-pong)
        uint32_t* d_wcnt = nullptr; size_t wcnt_cap = 0;                    // frame counters, 2 parity sets
        size_t wcnt_set = 0;                                                //   of this many words each
        uint32_t* d_perm = nullptr; size_t perm_cap = 0;                    // wavefront: dense queue order
        uint32_t* d_seg = nullptr; size_t seg_cap = 0;                      // wavefront: rays per queue segment
        uint32_t* d_cost = nullptr; size_t cost_cap = 0;   // adaptive order: per-tile times,
        uint32_t* d_lpt = nullptr; size_t lpt_cap = 0;     //   the longest-first order built from them,
        uint32_t* d_done = nullptr;                        //   and the finished-block counter
        uint64_t cost_key = 0; bool cost_ready = false;
        // a query slot (kQueryKey): the launch's work cursors and restart count, and the events around its kernel
        uint32_t* d_qcnt = nullptr;
        hipEvent_t qev[2] = {nullptr, nullptr};
    };
    static constexpr int kMaxSlots = 16;
    std::vector<FrameSlot> slots;
    FrameSlot* last_slot = nullptr;
    uint64_t slot_clock = 0;
    // static block orders (column strips), one per block grid: the row groups of rt_render and
    // the contexts of rt_render_tiled may differ in grid, and a grid's table is never rewritten
    // while a frame may read it (no stream sync to switch grids)
    struct OrderTab { uint32_t tx, ty, k; uint32_t* d; };   // k: frames per launch (rt_render_device_batch)
    static constexpr size_t kMaxOrders = 16;
    std::vector<OrderTab> orders;
    uint32_t scene_gen = 0;                                   // bumped by every upload
    int wf_grid[3] = {0, 0, 0};   // persistent wavefront grid per math mode
    // The query families launch through query_launch, which fills these on first use:
    // the persistent grid of each kernel (0: not computed yet) and the test cap of the families that
    // have one (grid_cap; -1: not read yet)
    int query_grid[2][3] = {{0, 0, 0}, {0, 0, 0}};   // ray queries: [record kind][math]
    int fan_grid[3] = {0, 0, 0};                     // fans: [math]
    int fan_grid_cap = -1;                           //   RTAMD_FAN_GRID_BLOCKS
    int closest_grid = 0;                            // rt_closest_points
    int nearest_grid[RT_NEAREST_MAX_K] = {};         // rt_nearest_k: [k - 1]
    int closest_grid_cap = -1;                       //   RTAMD_CLOSEST_GRID_BLOCKS, both point families
    int multihit_grid[3][RT_TRACE_MAX_K] = {};       // rt_trace_rays_k: [math][k - 1]
    int multihit_grid_cap = -1;                      //   RTAMD_MULTIHIT_GRID_BLOCKS
    // The host forms' staging (stage_in, stage_dst, stage_out), shared by every family, grow-only,
    // capacities in bytes: d_qrays takes the rays, fan origins or points, d_fdirs a fan's direction
    // table, d_qhits gives the hits, masks or records back
    char* d_qrays = nullptr; size_t qrays_cap = 0;
    char* d_qhits = nullptr; size_t qhits_cap = 0;
    char* d_fdirs = nullptr; size_t fdirs_cap = 0;
    // the slot of the last query while no frame has come after it (rt_last_deferred, rt_last_query_timing)
    FrameSlot* query_slot = nullptr;
    bool query_last = false;
    struct { bool on = false; unsigned long long* d_counts = nullptr; } trace;   // rt_fetch_counts
    struct {                                                                    // rt_wave_timeline
        bool on = false;
        uint32_t* d_words = nullptr; size_t cap = 0;   // device buffer, words
        size_t limit = 0, used = 0;                    // words the caller takes, words written
        std::vector<uint32_t> waves;                   // waves per launch
        std::vector<uint32_t> frame, bounce;           // per launch: its frame (of those in flight), its bounce
        uint32_t cur_frame = 0;
    } tline;
    bool frame_rows = false;   // rt_render_tiled: d_out is the whole frame (rtk::Outputs::frame_rows)
    uint32_t* h_stage = nullptr; size_t stage_cap = 0;   // rt_render_tiled: pinned frame for pageable callers
    struct TiledWorker* worker = nullptr;   // rt_render_tiled: this context's host thread (ctxs[1..])
    uint64_t enq_ns[2] = {0, 0};            // host steady clock at the start / end of the last frame's enqueue
    double wait_ms = 0.0;                   // the last synchronous wait (wait_stream's spin cap)
    // rt_render's row groups: one stream (so one frame slot) per group, and the event they start after
    hipStream_t gstream[8] = {};
    hipEvent_t gstart = nullptr;
    std::vector<FrameSlot*> last_group;   // the slots of the last grouped rt_render
    bool timing_valid = false;
    // rt_update_vertices' own state (the scene's refit data is the Scene's)
    struct Refit {
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // around the update's kernels; the caller's stream
        bool timed = false;
        uint32_t launches = 0;
    } refit;
    rtlbvh::Scratch lbvh;                      // rt_build_bvh's buffers; no part of the scene
    rtscene::Scratch sbuild;                   // rt_build_scene's buffers; no part of the scene
    rtlbvh::Scratch::Buf sah_part, sah_out;    // rt_scene_sah's buffers; no part of the scene
    std::string err;
};

static std::string g_err;

// How the synchronous entry points (rt_render, rt_render_tiled: the reference's blocking
// raytrace_gpgpu) wait for a frame.  hipStreamSynchronize may sleep until an interrupt; a frame
// is a fraction of a millisecond, so they poll instead (hipStreamQuery, RTAMD_SYNC=query, the
// default) for up to kSpinWaitMs and only then block.  RTAMD_SYNC=block: hipStreamSynchronize
// at once (A/B).
constexpr double kSpinWaitMs = 50.0;    // cap of the spin
constexpr double kSpinMinMs = 1.0;      // the spin lasts 4x the context's last wait, within [1, 50] ms
static int sync_mode() {
    static const int m = [] {
        const char* v = std::getenv("RTAMD_SYNC");
        return v && std::strcmp(v, "block") == 0 ? 1 : 0;
    }();
    return m;
}
static inline void cpu_relax() { __builtin_ia32_pause(); }
static uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}
// spin_ms: how long to poll before blocking (about the expected frame time: the caller passes a
// multiple of its last wait); a pause between queries leaves the core's sibling and the memory
// system alone
static hipError_t wait_stream(hipStream_t s, double spin_ms = kSpinWaitMs, double* waited_ms = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    auto done = [&](hipError_t e) {
        if (waited_ms) *waited_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return e;
    };
    if (sync_mode() == 1) return done(hipStreamSynchronize(s));
    spin_ms = std::min(kSpinWaitMs, std::max(kSpinMinMs, spin_ms));
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return done(e);
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > spin_ms)
            return done(hipStreamSynchronize(s));
        for (int i = 0; i < 16; ++i) cpu_relax();
    }
}
// a context's synchronous wait: spins about 4x its previous wait, then blocks
static hipError_t wait_ctx(rt_ctx* c, hipStream_t s) {
    double ms = 0.0;
    const hipError_t e = wait_stream(s, 4.0 * c->wait_ms, &ms);
    c->wait_ms = ms;
    return e;
}

// frame counters (one parity set): 8 per bounce ([0] queue size, [2] the bounce launch's
// work cursor), then the restart count (then, sized per frame, the queues' chunk sums)
// per bounce k: [0] its queue size, then (128-B aligned) the work cursors of its persistent
// bounce kernel (rtk::grab_group)
constexpr size_t kBounceWords = 32 + rtk::kCursorSet;
constexpr size_t kRestartSlot = kBounceWords * (RT_MAX_DEPTH + 1);
constexpr size_t kCounters = kRestartSlot + 1;

static int set_err(rt_ctx* c, const std::string& m, int code) {
    if (c) c->err = m; else { g_err = m; rtrefit::clear_error(); }
    return code;
}

#define HIPC(ctx, expr)                                                                          \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return set_err(ctx, std::string(#expr) + ": " + hipGetErrorString(e__), RT_ERR_DEVICE); \
    } while (0)

template <class T>
static int ensure(rt_ctx* c, T*& p, size_t& cap, size_t n) {
    if (n <= cap && p) return RT_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) { p = nullptr; return set_err(c, std::string("hipMalloc: ") + hipGetErrorString(e), RT_ERR_OUT_OF_MEMORY); }
    cap = n;
    return RT_OK;
}

static void free_slot(rt_ctx::FrameSlot& f) {
    for (void* p : {(void*)f.d_gstack, (void*)f.d_wq[0], (void*)f.d_wq[1], (void*)f.d_wcnt,
                    (void*)f.d_perm, (void*)f.d_seg, (void*)f.d_cost, (void*)f.d_lpt, (void*)f.d_done, (void*)f.d_qcnt})
        if (p) (void)hipFree(p);
    if (f.idle) (void)hipEventDestroy(f.idle);
    for (hipEvent_t e : f.qev)
        if (e) (void)hipEventDestroy(e);
    f = rt_ctx::FrameSlot{};
}

// The frame scratch of `stream` (created on first use; beyond kMaxSlots streams the
// least recently used slot is recycled once its last frame has finished -- waited on
// through the slot's own event, the stream itself may be gone by then).
static int slot_for(rt_ctx* c, void* stream, uint64_t tkey, rt_ctx::FrameSlot** out) {
    ++c->slot_clock;
    for (auto& f : c->slots)
        if (f.stream == stream && f.tkey == tkey) { f.last_use = c->slot_clock; *out = &f; return RT_OK; }
    if ((int)c->slots.size() < rt_ctx::kMaxSlots) {
        c->slots.reserve(rt_ctx::kMaxSlots);   // slot pointers stay valid
        c->slots.emplace_back();
        rt_ctx::FrameSlot& f = c->slots.back();
        f.stream = stream;
        f.tkey = tkey;
        f.last_use = c->slot_clock;
        HIPC(c, hipEventCreateWithFlags(&f.idle, hipEventDisableTiming));
        *out = &f;
        return RT_OK;
    }
    rt_ctx::FrameSlot* lru = &c->slots[0];
    for (auto& f : c->slots)
        if (f.last_use < lru->last_use) lru = &f;
    HIPC(c, hipEventSynchronize(lru->idle));
    lru->stream = stream;
    lru->tkey = tkey;
    lru->cost_key = 0;
    lru->cost_ready = false;
    lru->last_use = c->slot_clock;
    *out = lru;
    return RT_OK;
}

// Inner and triangle records in ONE allocation (triangles right after the inner records),
// so the fast traversal addresses both with 32-bit offsets from one buffer descriptor.
// Buffer-load offsets are 31-bit: records of 2 GiB or more (roughly 25 M triangle
// references) get two allocations instead, and such a scene renders with the general
// traversal (pointer loads, any size).  RTAMD_RECORD_LIMIT (bytes) lowers that limit for
// tests.
static uint64_t record_limit() {
    const char* v = std::getenv("RTAMD_RECORD_LIMIT");
    const uint64_t lim = v ? std::strtoull(v, nullptr, 10) : 0;
    return lim && lim < 0x80000000ull ? lim : 0x80000000ull;
}

static bool records_split(size_t n_wnodes4, size_t n_tris4) {
    return (n_wnodes4 + n_tris4 + Scene::walk_units(n_wnodes4)) * 16 >= record_limit();
}

// One array of a scene: from the pool where its allocation of that kind is large enough, else fresh.
static hipError_t scene_alloc(Scene& s, int k, size_t bytes, Scene::Owned* pool) {
    bytes = std::max<size_t>(bytes, 16);
    if (pool && pool->p[k] && pool->cap[k] >= bytes) {
        s.own.p[k] = pool->p[k]; s.own.cap[k] = pool->cap[k];
        pool->p[k] = nullptr; pool->cap[k] = 0;
        return hipSuccess;
    }
    const hipError_t e = hipMalloc(&s.own.p[k], bytes);
    if (e != hipSuccess) s.own.p[k] = nullptr; else s.own.cap[k] = bytes;
    return e;
}

// What a frame reads, with its counts: the inner and triangle records in one allocation or two
// (records_split), the shading records and the escape leaves.
static hipError_t scene_alloc_records(Scene& s, size_t n_wnodes4, size_t n_tris4, size_t n_shade4, size_t n_leaf,
                                      Scene::Owned* pool) {
    s.n_wnodes4 = n_wnodes4; s.n_tris4 = n_tris4; s.n_shade4 = n_shade4; s.n_leaf = n_leaf;
    s.split = records_split(n_wnodes4, n_tris4);
    hipError_t e = scene_alloc(s, Scene::kRec, (s.split ? n_wnodes4 : s.rec_units()) * sizeof(float4), pool);
    if (e == hipSuccess && s.split) e = scene_alloc(s, Scene::kTris, n_tris4 * sizeof(float4), pool);
    if (e == hipSuccess) e = scene_alloc(s, Scene::kShade, n_shade4 * sizeof(float4), pool);
    return e == hipSuccess ? scene_alloc(s, Scene::kLeaf, n_leaf * sizeof(int2), pool) : e;
}

// Every owned array from kind `first` on goes to the pool (which keeps the larger allocation of
// a kind) or, without one, is freed; with first = 0 the scene is then empty.  Idempotent.
static void scene_release(Scene& s, Scene::Owned* pool, int first = 0) {
    for (int k = first; k < Scene::kCount; ++k) {
        if (!s.own.p[k]) continue;
        if (pool && pool->cap[k] < s.own.cap[k]) {
            std::swap(pool->p[k], s.own.p[k]);
            std::swap(pool->cap[k], s.own.cap[k]);
        }
        if (s.own.p[k]) (void)hipFree(s.own.p[k]);
        s.own.p[k] = nullptr; s.own.cap[k] = 0;
    }
    if (first == 0) s = Scene{};
}

// A producer's scene until install_scene takes it: released on every other way out.
struct PendingScene {
    Scene s;
    Scene::Owned* pool;   // where its arrays come from and go back to (rt_build_scene), or NULL
    explicit PendingScene(Scene::Owned* from) : pool(from) { s.pooled = from != nullptr; }
    ~PendingScene() { scene_release(s, pool); }
};

// The context without a scene, after waiting for the frames in flight, which still read it.  The
// arrays rt_build_scene made go to the spare pool, any others are freed.
static int drop_scene(rt_ctx* c) {
    for (auto& f : c->slots)
        if (f.idle) HIPC(c, hipEventSynchronize(f.idle));
    scene_release(c->scene, c->scene.pooled ? &c->spare : nullptr);
    c->have_scene = false;
    c->refit.timed = false;
    return RT_OK;
}

// The walk references of a scene whose records are in place (every producer has waited for its copies
// and kernels): zero the units after the triangle records, derive the array, read the status back.
static int derive_walk(rt_ctx* c, Scene& s) {
    s.walk_root = s.walk_off = 0;
    if (s.split || !s.wnodes() || s.n_tris4 == 0) return RT_OK;
    // RTAMD_NO_WALK=1 (tests): the scene is installed without walk references, as one with a leaf of
    // more than 16 references is, so that the two loop forms can be compared on one scene
    if (const char* v = std::getenv("RTAMD_NO_WALK"); v && v[0] == '1') return RT_OK;
    HIPC(c, hipSetDevice(c->device));
    const uint32_t n_rec = (uint32_t)(s.n_wnodes4 / 4);
    float4* w0 = s.wnodes() + s.n_wnodes4 + s.n_tris4;
    HIPC(c, hipMemsetAsync(w0, 0, Scene::walk_units(s.n_wnodes4) * sizeof(float4), c->stream));
    uint2* walk = (uint2*)(s.wnodes() + s.walk_unit0());
    uint32_t* status = (uint32_t*)(w0 + Scene::walk_units(s.n_wnodes4) - 1);
    hipLaunchKernelGGL(rtk::derive_walk_kernel, dim3((std::max(n_rec, 1u) + 255u) / 256u), dim3(256), 0, c->stream,
                       (const float4*)s.wnodes(), n_rec, (const int2*)s.leaf(), (uint32_t)s.n_leaf, (uint32_t)s.n_wnodes4,
                       (uint32_t)((s.n_tris4 - 1) / 3), s.root, walk, status);
    HIPC(c, hipGetLastError());
    uint32_t st[2] = {1u, 0u};
    HIPC(c, hipMemcpyAsync(st, status, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (st[0] == 0) {
        s.walk_root = st[1];
        s.walk_off = (uint32_t)(s.walk_unit0() * 16);
    }
    return RT_OK;
}

// The single place that replaces the context's scene.
static int install_scene(rt_ctx* c, Scene&& s) {
    if (const int rc = derive_walk(c, s)) return rc;
    if (const int rc = drop_scene(c)) return rc;
    c->scene = std::move(s);
    c->have_scene = true;
    ++c->scene_gen;
    return RT_OK;
}

// Static block -> tile order (the first frame of a geometry, and RT_FLAG_STATIC_ORDER).
// Blocks b, b+8, b+16, ... run on one XCD (round-robin dispatch; a speed assumption
// only, never correctness): XCD k gets the k-th eighth of the tile columns and walks it
// row by row, so all XCDs sweep the frame bottom-up together (balanced) while each L2
// sees one compact screen region.
static std::vector<uint32_t> tile_order_table(uint32_t tx, uint32_t ty) {
    const uint32_t nb = tx * ty;
    std::vector<uint32_t> order(nb);
    std::vector<std::vector<uint32_t>> want(8);
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t c0 = k * tx / 8, c1 = (k + 1) * tx / 8;
        for (uint32_t y = 0; y < ty; ++y)
            for (uint32_t x = c0; x < c1; ++x) want[k].push_back(y * tx + x);
    }
    // blocks of XCD k: b = k, k+8, ...; quota_k = number of such b below nb
    std::vector<uint32_t> quota(8), cursor(8, 0);
    for (uint32_t k = 0; k < 8; ++k) quota[k] = nb > k ? (nb - k + 7) / 8 : 0;
    // surplus tiles of over-full strips go to XCDs with room, keeping row order (by tile index)
    std::vector<uint32_t> spill;
    for (uint32_t k = 0; k < 8; ++k)
        while (want[k].size() > quota[k]) { spill.push_back(want[k].back()); want[k].pop_back(); }
    std::sort(spill.begin(), spill.end());
    size_t si = 0;
    for (uint32_t k = 0; k < 8; ++k)
        while (want[k].size() < quota[k] && si < spill.size()) want[k].push_back(spill[si++]);
    for (uint32_t k = 0; k < 8; ++k) std::sort(want[k].begin(), want[k].end(), [tx](uint32_t a, uint32_t b) {
        return a / tx != b / tx ? a / tx < b / tx : a < b;
    });
    for (uint32_t b = 0; b < nb; ++b) order[b] = want[b & 7][cursor[b & 7]++];
    return order;
}

// Kernels of one math mode (namespace NS), picked at launch by the frame's flags.
template <int M> struct Kernels;
#define RTK_KERNELS(M, NS)                                                                                 \
    template <> struct Kernels<M> {                                                                        \
        static void* first(bool fast, bool next) {                                                        \
            return fast ? (next ? (void*)NS::first_bounce_kernel<true, true> : (void*)NS::first_bounce_kernel<true, false>) \
                        : (next ? (void*)NS::first_bounce_kernel<false, true> : (void*)NS::first_bounce_kernel<false, false>); \
        }                                                                                                  \
        static void* fused(bool fast) { return fast ? (void*)NS::render_kernel<true> : (void*)NS::render_kernel<false>; } \
        static void* bounce(bool fast) {                                                                   \
            return fast ? (void*)NS::wf_bounce_kernel<true> : (void*)NS::wf_bounce_kernel<false>;          \
        }                                                                                                  \
        static void* traced(bool next, bool walk) {                                                        \
            return next ? (void*)NS::first_bounce_kernel<true, true, 1>                                    \
                        : walk ? (void*)NS::first_bounce_kernel<true, false, 1, true>                      \
                               : (void*)NS::first_bounce_kernel<true, false, 1, false>;                    \
        }                                                                                                  \
        static void* traced_bounce() { return (void*)NS::wf_bounce_kernel<true, 1>; }                     \
        static void* query(bool any, bool fast) {                                                          \
            return any ? (fast ? (void*)NS::query_kernel<true, true> : (void*)NS::query_kernel<true, false>) \
                       : (fast ? (void*)NS::query_kernel<false, true> : (void*)NS::query_kernel<false, false>); \
        }                                                                                                  \
        static void* query_attr(bool any, bool fast) {                                                     \
            return any ? (fast ? (void*)NS::query_attr_kernel<true, true> : (void*)NS::query_attr_kernel<true, false>) \
                       : (fast ? (void*)NS::query_attr_kernel<false, true> : (void*)NS::query_attr_kernel<false, false>); \
        }                                                                                                  \
        static void* fan(bool fast) { return fast ? (void*)NS::fan_kernel<true> : (void*)NS::fan_kernel<false>; } \
        static void* multihit(int k) {                                                                     \
            void* const t[RT_TRACE_MAX_K] = {(void*)NS::multihit_kernel<1>, (void*)NS::multihit_kernel<2>, \
                                             (void*)NS::multihit_kernel<3>, (void*)NS::multihit_kernel<4>, \
                                             (void*)NS::multihit_kernel<5>, (void*)NS::multihit_kernel<6>, \
                                             (void*)NS::multihit_kernel<7>, (void*)NS::multihit_kernel<8>}; \
            return t[k - 1];                                                                               \
        }                                                                                                  \
        static void* batch(bool fast, bool next) {                                                         \
            return fast ? (next ? (void*)NS::first_bounce_batch_kernel<true, true> : (void*)NS::first_bounce_batch_kernel<true, false>) \
                        : (next ? (void*)NS::first_bounce_batch_kernel<false, true> : (void*)NS::first_bounce_batch_kernel<false, false>); \
        }                                                                                                  \
    };
RTK_KERNELS(0, rtk_strict)
RTK_KERNELS(1, rtk_hw)
RTK_KERNELS(2, rtk_ref)
#undef RTK_KERNELS

static void* kernel_first(int m, bool fast, bool next) {
    return m == 0 ? Kernels<0>::first(fast, next) : m == 1 ? Kernels<1>::first(fast, next) : Kernels<2>::first(fast, next);
}
static void* kernel_batch(int m, bool fast, bool next) {
    return m == 0 ? Kernels<0>::batch(fast, next) : m == 1 ? Kernels<1>::batch(fast, next) : Kernels<2>::batch(fast, next);
}
static void* kernel_fused(int m, bool fast) {
    return m == 0 ? Kernels<0>::fused(fast) : m == 1 ? Kernels<1>::fused(fast) : Kernels<2>::fused(fast);
}
static void* kernel_traced(int m, bool next, bool walk) {
    return m == 0 ? Kernels<0>::traced(next, walk) : m == 1 ? Kernels<1>::traced(next, walk) : Kernels<2>::traced(next, walk);
}
static void* kernel_traced_bounce(int m) {
    return m == 0 ? Kernels<0>::traced_bounce() : m == 1 ? Kernels<1>::traced_bounce() : Kernels<2>::traced_bounce();
}
static void* kernel_bounce(int m, bool fast) {
    return m == 0 ? Kernels<0>::bounce(fast) : m == 1 ? Kernels<1>::bounce(fast) : Kernels<2>::bounce(fast);
}
static void* kernel_query(int m, bool any, bool fast) {
    return m == 0 ? Kernels<0>::query(any, fast) : m == 1 ? Kernels<1>::query(any, fast) : Kernels<2>::query(any, fast);
}
static void* kernel_query_attr(int m, bool any, bool fast) {
    return m == 0 ? Kernels<0>::query_attr(any, fast) : m == 1 ? Kernels<1>::query_attr(any, fast) : Kernels<2>::query_attr(any, fast);
}
static void* kernel_fan(int m, bool fast) {
    return m == 0 ? Kernels<0>::fan(fast) : m == 1 ? Kernels<1>::fan(fast) : Kernels<2>::fan(fast);
}
static void* kernel_multihit(int m, int k) {
    return m == 0 ? Kernels<0>::multihit(k) : m == 1 ? Kernels<1>::multihit(k) : Kernels<2>::multihit(k);
}
// the timeline instantiation (rt_wave_timeline): S_ref, the fast kernels
static void* kernel_timeline_first(bool next, bool walk) {
    return next ? (void*)rtk_ref::first_bounce_kernel<true, true, 2>
                : walk ? (void*)rtk_ref::first_bounce_kernel<true, false, 2, true> : (void*)rtk_ref::first_bounce_kernel<true, false, 2, false>;
}
static void* kernel_timeline_bounce() { return (void*)rtk_ref::wf_bounce_kernel<true, 2>; }

extern "C" {

int rt_abi_version(void) { return 3; }

int rt_assemble_bands_batch(uint32_t* d_frame, const uint32_t* d_slots, uint64_t slot_pixels, uint64_t frame_pixels,
                            int32_t nframes, uint32_t w, uint32_t h, int32_t nranks, int32_t band_rows, void* stream) {
    if (!d_frame || !d_slots || w == 0 || h == 0 || nranks < 1 || band_rows < 1 || nframes < 1 || nframes > 65535)
        return set_err(nullptr, "rt_assemble_bands: invalid argument", RT_ERR_INVALID_ARG);
    // every rank's bands must fit a frame's buffer (rt_tiling_pixels of the fullest rank),
    // and a rank's frames its slot
    rt_tiling t0{0, nranks, band_rows, 0};
    const uint64_t need = (uint64_t)rt_tiling_pixels(w, h, &t0);
    if (need > frame_pixels || (uint64_t)nframes * frame_pixels > slot_pixels)
        return set_err(nullptr, "rt_assemble_bands: slot_pixels smaller than rank 0's bands", RT_ERR_INVALID_ARG);
    if (((uintptr_t)d_frame | (uintptr_t)d_slots) & 15u)
        return set_err(nullptr, "rt_assemble_bands: buffers must be 16-byte aligned", RT_ERR_INVALID_ARG);
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(rtk::assemble_bands_kernel, dim3(h, nframes), dim3(256), 0, (hipStream_t)stream, d_frame, d_slots,
                       slot_pixels, frame_pixels, w, h, (uint32_t)nranks, (uint32_t)band_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(nullptr, std::string("rt_assemble_bands: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    return RT_OK;
}

int rt_assemble_bands(uint32_t* d_frame, const uint32_t* d_slots, uint64_t slot_pixels, uint32_t w, uint32_t h,
                      int32_t nranks, int32_t band_rows, void* stream) {
    return rt_assemble_bands_batch(d_frame, d_slots, slot_pixels, slot_pixels, 1, w, h, nranks, band_rows, stream);
}

int rt_bands_put(const uint32_t* d_bands, uint32_t* d_frame, uint32_t w, uint32_t h, const rt_tiling* tiling,
                 void* stream) {
    if (!d_bands || !d_frame || w == 0 || h == 0) return set_err(nullptr, "rt_bands_put: invalid argument", RT_ERR_INVALID_ARG);
    rt_tiling whole{0, 1, 16, 0};
    const rt_tiling* T = tiling && tiling->nranks > 1 ? tiling : &whole;
    if (T->rank < 0 || T->rank >= T->nranks || T->band_rows < 1)
        return set_err(nullptr, "rt_bands_put: bad tiling", RT_ERR_INVALID_ARG);
    const int64_t npix = rt_tiling_pixels(w, h, T);
    if (npix <= 0) return npix < 0 ? set_err(nullptr, "rt_bands_put: bad tiling", RT_ERR_INVALID_ARG) : RT_OK;
    if ((w & 3u) == 0 && (((uintptr_t)d_frame | (uintptr_t)d_bands) & 15u))
        return set_err(nullptr, "rt_bands_put: buffers must be 16-byte aligned", RT_ERR_INVALID_ARG);
    const uint32_t local_rows = (uint32_t)(npix / w);
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(rtk::bands_put_kernel, dim3(local_rows), dim3(256), 0, (hipStream_t)stream, d_frame, d_bands, w,
                       local_rows, (uint32_t)T->rank, (uint32_t)T->nranks, (uint32_t)T->band_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(nullptr, std::string("rt_bands_put: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    return RT_OK;
}

int64_t rt_frame_sync_words(int32_t nsets, int32_t nranks) {
    if (nsets < 1 || nranks < 1) return -1;
    return (int64_t)rtk::kSyncHead + nsets + (int64_t)nsets * nranks;
}

// rt_bands_put_sync's wait for a set's release (RTAMD_PUT_WAIT): 0 = one bounded wait wave before the
// put (default, "wave"), 1 = hipStreamWaitValue32 ("stream", where the device supports stream wait
// values), 2 = every put block waits ("kernel", round 5)
// Launches per rebuild of the adaptive longest-first block order (RTAMD_LPT_EVERY=K, K >= 1;
// default 8).  A rebuild launch times its blocks (each block's epilogue: a barrier, its cost
// store and a counter round trip) and its last block sorts them; every other launch runs the
// order as it is and has no epilogue at all, so a wave that is done leaves at once.  Against a
// rebuild every launch (K = 1): C2 0.0605 vs 0.0693 ms per frame, one frame alone 0.172 vs 0.239
// ms; C3 0.2988 vs 0.3028, one frame 0.364 vs 0.372; C4 1.0765 vs 1.089; the orbiting camera
// 0.280 vs 0.283 (K = 16 lets its order go stale: one frame's mean 0.376 vs 0.373 at K = 8);
// profiles/r06/ab_lpt_every/table.txt.  The order is a schedule, never a pixel: same frames.
static uint64_t lpt_every() {
    static const uint64_t k = [] {
        const char* v = std::getenv("RTAMD_LPT_EVERY");
        const long n = v ? std::atol(v) : 8L;
        return (uint64_t)(n >= 1 ? n : 1);
    }();
    return k;
}

static int put_wait_mode() {
    const char* v = std::getenv("RTAMD_PUT_WAIT");
    if (v && std::strcmp(v, "kernel") == 0) return 2;
    if (v && std::strcmp(v, "stream") == 0) {
        int dev = 0, ok = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&ok, hipDeviceAttributeCanUseStreamWaitValue, dev) == hipSuccess && ok)
            return 1;
        (void)hipGetLastError();
        return 2;
    }
    return 0;
}
static uint64_t timeout_ticks(uint32_t ms) { return (uint64_t)(ms ? ms : 10000u) * 100000ull; }   // s_memrealtime: 100 MHz

int rt_bands_put_sync(const uint32_t* d_bands, uint32_t* d_frame, uint32_t w, uint32_t h, const rt_tiling* tiling,
                      uint32_t* d_sync, uint32_t* d_local, int32_t nsets, int32_t set, uint32_t use, uint32_t timeout_ms,
                      void* stream) {
    if (!d_bands || !d_frame || !d_sync || !d_local || w == 0 || h == 0 || nsets < 1 || set < 0 || set >= nsets)
        return set_err(nullptr, "rt_bands_put_sync: invalid argument", RT_ERR_INVALID_ARG);
    rt_tiling whole{0, 1, 16, 0};
    const rt_tiling* T = tiling && tiling->nranks > 1 ? tiling : &whole;
    if (T->rank < 0 || T->rank >= T->nranks || T->band_rows < 1)
        return set_err(nullptr, "rt_bands_put_sync: bad tiling", RT_ERR_INVALID_ARG);
    const int64_t npix = rt_tiling_pixels(w, h, T);
    if (npix <= 0) return set_err(nullptr, "rt_bands_put_sync: this rank owns no rows", RT_ERR_INVALID_ARG);
    if ((w & 3u) == 0 && (((uintptr_t)d_frame | (uintptr_t)d_bands) & 15u))
        return set_err(nullptr, "rt_bands_put_sync: buffers must be 16-byte aligned", RT_ERR_INVALID_ARG);
    const uint32_t local_rows = (uint32_t)(npix / w);
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    const int mode = put_wait_mode();
    if (mode == 0 && use > 0) {   // one wave waits for the set's release; the put's blocks do not
        hipLaunchKernelGGL(rtk::put_wait_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_sync, (uint32_t)set, use,
                           timeout_ticks(timeout_ms));
    } else if (mode == 1 && use > 0) {
        const hipError_t we = hipStreamWaitValue32((hipStream_t)stream, d_sync + rtk::kSyncHead + set, use,
                                                   hipStreamWaitValueGte, 0xFFFFFFFFu);
        if (we != hipSuccess) return set_err(nullptr, std::string("rt_bands_put_sync: hipStreamWaitValue32: ") +
                                                          hipGetErrorString(we), RT_ERR_DEVICE);
    }
    const bool qwait = mode != 2;
    hipLaunchKernelGGL(rtk::bands_put_sync_kernel, dim3(std::min<uint32_t>(local_rows, rtk::kPutBlocks)), dim3(256), 0,
                       (hipStream_t)stream, d_frame, d_bands,
                       w, local_rows, (uint32_t)T->rank, (uint32_t)T->nranks, (uint32_t)T->band_rows, d_sync, d_local,
                       (uint32_t)nsets, (uint32_t)set, use, timeout_ticks(timeout_ms), qwait ? 1u : 0u);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(nullptr, std::string("rt_bands_put_sync: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    return RT_OK;
}

int rt_frame_present(uint32_t* d_sync, int32_t nsets, int32_t set, uint32_t use, int32_t nranks, uint32_t timeout_ms,
                     int32_t release, void* stream) {
    if (!d_sync || nsets < 1 || set < 0 || set >= nsets || nranks < 1)
        return set_err(nullptr, "rt_frame_present: invalid argument", RT_ERR_INVALID_ARG);
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(rtk::frame_present_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_sync, (uint32_t)nsets,
                       (uint32_t)set, use, (uint32_t)nranks, timeout_ticks(timeout_ms), release ? 1u : 0u);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(nullptr, std::string("rt_frame_present: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    return RT_OK;
}

int rt_frame_release(uint32_t* d_sync, int32_t nsets, int32_t set, uint32_t use, void* stream) {
    if (!d_sync || nsets < 1 || set < 0 || set >= nsets)
        return set_err(nullptr, "rt_frame_release: invalid argument", RT_ERR_INVALID_ARG);
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(rtk::frame_release_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d_sync, (uint32_t)set, use);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(nullptr, std::string("rt_frame_release: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    return RT_OK;
}

int rt_frame_sync_status(const uint32_t* d_sync, uint32_t* status, uint32_t* presented) {
    if (!d_sync || !status || !presented) return set_err(nullptr, "rt_frame_sync_status: invalid argument", RT_ERR_INVALID_ARG);
    uint32_t v[2] = {0, 0};
    hipError_t e = hipMemcpy(v, d_sync, sizeof v, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_err(nullptr, std::string("rt_frame_sync_status: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    *status = v[0];
    *presented = v[1];
    return RT_OK;
}

int rt_frame_checksum(const uint32_t* d_frame, uint64_t pixels, uint64_t* d_sum, void* stream) {
    if (!d_frame || !d_sum || pixels == 0) return set_err(nullptr, "rt_frame_checksum: invalid argument", RT_ERR_INVALID_ARG);
    const uint64_t blocks = std::min<uint64_t>(1024, (pixels + 255) / 256);
    (void)hipGetLastError();   // an earlier call's error is not this launch's
    hipLaunchKernelGGL(rtk::frame_checksum_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, d_frame,
                       pixels, (unsigned long long*)d_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(nullptr, std::string("rt_frame_checksum: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    return RT_OK;
}

// (without a context: the latest of the global message and rt_refit_nodes' own, csrc/host/refit.cpp)
const char* rt_last_error(rt_ctx* ctx) {
    if (ctx) return ctx->err.c_str();
    return rtrefit::last_error().empty() ? g_err.c_str() : rtrefit::last_error().c_str();
}

int rt_create(int device, rt_ctx** out) {
    if (!out) return set_err(nullptr, "rt_create: out is NULL", RT_ERR_INVALID_ARG);
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return set_err(nullptr, "rt_create: no HIP device", RT_ERR_DEVICE);
    if (device < 0 || device >= n) return set_err(nullptr, "rt_create: bad device index", RT_ERR_INVALID_ARG);
    rt_ctx* c = new rt_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&c->d_overflow, sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(c->d_overflow, 0, sizeof(unsigned long long)) != hipSuccess) {
        delete c;
        return set_err(nullptr, "rt_create: HIP init failed", RT_ERR_DEVICE);
    }
    *out = c;
    return RT_OK;
}

static void tiled_worker_stop(rt_ctx* c);
int rt_destroy(rt_ctx* c) {
    if (!c) return RT_ERR_INVALID_ARG;
    tiled_worker_stop(c);   // rt_render_tiled's host thread for this context, if it has one
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& f : c->slots)
        if (f.idle) (void)hipEventSynchronize(f.idle);   // frames may still run on caller streams
    scene_release(c->scene, nullptr);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->d_hits) (void)hipFree(c->d_hits);
    if (c->d_t) (void)hipFree(c->d_t);
    if (c->d_rgb) (void)hipFree(c->d_rgb);
    if (c->d_overflow) (void)hipFree(c->d_overflow);
    if (c->d_qrays) (void)hipFree(c->d_qrays);
    if (c->d_qhits) (void)hipFree(c->d_qhits);
    if (c->d_fdirs) (void)hipFree(c->d_fdirs);
    for (auto& f : c->slots) free_slot(f);
    for (auto& o : c->orders) (void)hipFree(o.d);
    if (c->tline.d_words) (void)hipFree(c->tline.d_words);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (auto& f : c->ring)
        for (hipEvent_t& e : f.e)
            if (e) (void)hipEventDestroy(e);
    for (int g = 0; g < 8; ++g) {
        if (c->gstream[g]) (void)hipStreamSynchronize(c->gstream[g]);
        if (c->gstream[g]) (void)hipStreamDestroy(c->gstream[g]);
    }
    if (c->gstart) (void)hipEventDestroy(c->gstart);
    for (hipEvent_t& e : c->refit.ev)
        if (e) (void)hipEventDestroy(e);
    rtlbvh::release(c->lbvh);
    rtscene::release(c->sbuild);
    for (rtlbvh::Scratch::Buf* b : {&c->sah_part, &c->sah_out})
        if (b->p) (void)hipFree(b->p);
    for (void* p : c->spare.p)
        if (p) (void)hipFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return RT_OK;
}

int rt_upload_scene(rt_ctx* c, const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx,
                    const rt_bvh_node* nodes, int32_t nn, const int32_t* refs, int32_t nref,
                    const rt_float4* normals, int32_t nnorm, const int32_t* normal_idx, const rt_material* mats,
                    int32_t nmat, const int32_t* tri_to_mat) {
    if (!c) return RT_ERR_INVALID_ARG;
    if (!verts || nv <= 0 || !idx || nidx <= 0 || nidx % 3 || !nodes || nn <= 0 || !refs || nref < 0 || !normals ||
        nnorm <= 0 || !normal_idx || !mats || nmat <= 0 || !tri_to_mat)
        return set_err(c, "rt_upload_scene: missing or empty array", RT_ERR_INVALID_ARG);
    rtamd::EncodedScene enc;
    static_assert(sizeof(rt_float4) == sizeof(float4) && sizeof(enc.leaf_table[0]) == sizeof(int2), "the encoded layouts");
    std::string why;
    if (const int rc = rtamd::encode_scene(verts, nv, idx, nidx, nodes, nn, refs, nref, normals, nnorm, normal_idx, mats, nmat,
                                           tri_to_mat, enc, why))
        return set_err(c, why, rc);

    HIPC(c, hipSetDevice(c->device));
    if (const int rc = drop_scene(c)) return rc;   // before the new one is allocated: peak memory is one scene's
    PendingScene ps(nullptr);
    Scene& S = ps.s;
    HIPC(c, scene_alloc_records(S, enc.wnodes.size(), enc.tris.size(), enc.shade.size(), enc.leaf_table.size(), nullptr));
    HIPC(c, hipMemcpy(S.wnodes(), enc.wnodes.data(), S.n_wnodes4 * sizeof(float4), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(S.tris(), enc.tris.data(), S.n_tris4 * sizeof(float4), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(S.shade(), enc.shade.data(), S.n_shade4 * sizeof(float4), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(S.leaf(), enc.leaf_table.data(), S.n_leaf * sizeof(int2), hipMemcpyHostToDevice));
    S.root = enc.root; S.n_inner = enc.n_inner; S.fast_div = enc.fast_div; S.clean = enc.clean;
    S.bounds_min = nodes[0].min; S.bounds_max = nodes[0].max; S.have_bounds = true;
    // refit data (rt_update_vertices): only a refittable scene gets it; any other renders as ever
    rtrefit::Plan plan;
    if (rtrefit::plan_build(nodes, nn, nref, enc.inner_id.data(), plan, S.why) != RT_OK) return install_scene(c, std::move(S));
    if (plan.ids.size() != (size_t)S.n_inner) {   // (a refittable scene is clean: every inner node has a record)
        S.why = "refit: the plan does not cover the inner records";
        return install_scene(c, std::move(S));
    }
    uint32_t out0[8] = {(uint32_t)S.fast_div, 0u, 0u, 0u, 0u, 0u, 0u, 0u};   // rtrefit::DevArgs::out: the flag, then the root box
    std::memcpy(out0 + 2, &nodes[0].min, 12);
    std::memcpy(out0 + 5, &nodes[0].max, 12);
    auto put = [&](int k, const void* src, size_t bytes) {
        hipError_t e = scene_alloc(S, k, bytes, nullptr);
        if (e == hipSuccess && bytes) e = hipMemcpy(S.own.p[k], src, bytes, hipMemcpyHostToDevice);
        return e == hipSuccess;
    };
    if (!put(Scene::kIdx, idx, (size_t)nidx * 4) || !put(Scene::kNormalIdx, normal_idx, (size_t)nidx * 4) ||
        !put(Scene::kRefTri, refs, (size_t)nref * 4) || !put(Scene::kLevelIds, plan.ids.data(), plan.ids.size() * 4) ||
        !put(Scene::kLevelBegin, plan.level_begin.data(), plan.level_begin.size() * 4) || !put(Scene::kOut, out0, sizeof out0)) {
        (void)hipGetLastError();
        scene_release(S, nullptr, Scene::kIdx);   // the records stay: the scene renders, without refit data
        S.why = "refit: out of device memory for the refit data";
        return install_scene(c, std::move(S));
    }
    S.level_begin = plan.level_begin;
    S.nv = nv; S.nnorm = nnorm; S.nref = (uint32_t)nref; S.ntri = (uint32_t)(nidx / 3);
    S.why.clear();
    S.refittable = true;
    return install_scene(c, std::move(S));
}

// ---- animated geometry: vertex updates with an on-GPU refit ----
// Both forms are synchronous, like rt_upload_scene: they wait for the frames in flight, run the
// update on the context's stream, wait for it and read back the fast-quotient flag and the
// root box.  scene_gen stays: the adaptive block order of a slightly moved scene is still a
// good order, and pixels do not depend on it.
static int update_vertices(rt_ctx* c, const char* who, const rt_float4* verts, int32_t nv, const rt_float4* normals,
                           int32_t nnorm, bool on_device, void* stream) {
    if (!c) return set_err(nullptr, std::string(who) + ": ctx is NULL", RT_ERR_INVALID_ARG);
    if (!c->have_scene) return set_err(c, std::string(who) + ": no scene uploaded", RT_ERR_NO_SCENE);
    rt_ctx::Refit& r = c->refit;
    Scene& S = c->scene;
    if (!S.refittable) return set_err(c, std::string(who) + ": the scene has no refit data (" + S.why + ")", RT_ERR_BAD_SCENE);
    if (!verts || nv != S.nv || (normals && nnorm != S.nnorm))
        return set_err(c, std::string(who) + ": vertices / normals must be the upload's counts (" + std::to_string(S.nv) +
                              ", " + std::to_string(S.nnorm) + ")", RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    for (hipEvent_t& e : r.ev)
        if (!e) HIPC(c, hipEventCreate(&e));
    for (auto& f : c->slots)
        if (f.idle) HIPC(c, hipEventSynchronize(f.idle));   // frames in flight still read the old records
    const float4* d_verts = (const float4*)verts;
    const float4* d_normals = (const float4*)normals;
    if (on_device) {   // the caller's stream may still be producing d_verts
        HIPC(c, hipEventRecord(r.ev[2], (hipStream_t)stream));
        HIPC(c, hipStreamWaitEvent(c->stream, r.ev[2], 0));
    } else {
        Scene::Owned* pool = S.pooled ? &c->spare : nullptr;   // the staging is the scene's, like its other arrays
        if (!S.verts()) HIPC(c, scene_alloc(S, Scene::kVerts, (size_t)S.nv * sizeof(float4), pool));
        HIPC(c, hipMemcpyAsync(S.verts(), verts, (size_t)S.nv * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        d_verts = S.verts();
        if (normals) {
            if (!S.normals()) HIPC(c, scene_alloc(S, Scene::kNormals, (size_t)S.nnorm * sizeof(float4), pool));
            HIPC(c, hipMemcpyAsync(S.normals(), normals, (size_t)S.nnorm * sizeof(float4), hipMemcpyHostToDevice, c->stream));
            d_normals = S.normals();
        }
    }
    rtrefit::DevArgs a{};
    a.wnodes = S.wnodes(); a.tris = S.tris(); a.shade = S.shade(); a.leaf_table = S.leaf();
    a.verts = d_verts; a.normals = d_normals;
    a.idx = S.idx(); a.normal_idx = S.normal_idx(); a.ref_tri = S.ref_tri();
    a.level_ids = S.level_ids(); a.level_begin = S.d_level_begin(); a.out = S.out();
    a.nref = S.nref; a.ntri = S.ntri; a.n_inner = S.n_inner; a.root = S.root;
    HIPC(c, hipEventRecord(r.ev[0], c->stream));
    HIPC(c, rtrefit::launch(a, S.level_begin.data(), (uint32_t)S.level_begin.size() - 1u, c->stream, &r.launches));
    HIPC(c, hipEventRecord(r.ev[1], c->stream));
    uint32_t out[8] = {};
    HIPC(c, hipMemcpyAsync(out, S.out(), sizeof out, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, wait_stream(c->stream));
    r.timed = true;
    S.fast_div = out[0] ? 1 : 0;
    float box[6];
    std::memcpy(box, out + 2, sizeof box);
    S.bounds_min.x = box[0]; S.bounds_min.y = box[1]; S.bounds_min.z = box[2];
    S.bounds_max.x = box[3]; S.bounds_max.y = box[4]; S.bounds_max.z = box[5];
    return RT_OK;
}

int rt_update_vertices(rt_ctx* c, const rt_float4* verts, int32_t nv, const rt_float4* normals, int32_t nnorm) {
    return update_vertices(c, "rt_update_vertices", verts, nv, normals, nnorm, false, nullptr);
}

int rt_update_vertices_device(rt_ctx* c, const rt_float4* d_verts, int32_t nv, const rt_float4* d_normals, int32_t nnorm,
                              void* stream) {
    return update_vertices(c, "rt_update_vertices_device", d_verts, nv, d_normals, nnorm, true, stream);
}

int rt_scene_bounds(rt_ctx* c, rt_float4* mn, rt_float4* mx) {
    if (!c || !mn || !mx) return set_err(c, "rt_scene_bounds: invalid argument", RT_ERR_INVALID_ARG);
    if (!c->have_scene) return set_err(c, "rt_scene_bounds: no scene uploaded", RT_ERR_NO_SCENE);
    if (!c->scene.have_bounds)
        return set_err(c, "rt_scene_bounds: the scene came from a scene image, which carries no root box", RT_ERR_BAD_SCENE);
    *mn = c->scene.bounds_min;
    *mx = c->scene.bounds_max;
    return RT_OK;
}

int rt_last_update_timing(rt_ctx* c, float* total_ms) {
    if (!c || !total_ms) return set_err(c, "rt_last_update_timing: invalid argument", RT_ERR_INVALID_ARG);
    if (!c->refit.timed) return set_err(c, "rt_last_update_timing: no update since the upload", RT_ERR_INVALID_ARG);
    HIPC(c, hipEventElapsedTime(total_ms, c->refit.ev[0], c->refit.ev[1]));
    return RT_OK;
}

// ---- on-GPU LBVH build ----
// Both forms are synchronous.  They run on the context's stream with the context's own scratch
// and touch nothing of the uploaded scene: frames in flight on other streams are not waited for.
static int build_bvh(rt_ctx* c, const char* who, const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx,
                     int32_t max_leaf_arg, rt_bvh_node* nodes, int32_t node_cap, int32_t* refs, int32_t ref_cap,
                     int32_t* num_nodes, bool on_device, void* stream) {
    if (!c) return set_err(nullptr, std::string(who) + ": ctx is NULL", RT_ERR_INVALID_ARG);
    if (!verts || nv <= 0 || !idx || !nodes || !refs || !num_nodes)
        return set_err(c, std::string(who) + ": missing array", RT_ERR_INVALID_ARG);
    int32_t max_leaf = 0;
    bool extent_keys = false;
    if (!lbvh::split_max_leaf(max_leaf_arg, max_leaf, extent_keys))
        return set_err(c, std::string(who) + ": max_leaf must be 1 .. 8 (| RT_BUILD_EXTENT_KEYS)", RT_ERR_INVALID_ARG);
    if (nidx <= 0 || nidx % 3 != 0 || nidx / 3 > lbvh::kMaxTris)
        return set_err(c, std::string(who) + ": needs 1 .. 2^25 triangles, 3 indices each", RT_ERR_INVALID_ARG);
    const int32_t n = nidx / 3;
    if ((int64_t)node_cap < 2 * (int64_t)n - 1 || ref_cap < n)
        return set_err(c, std::string(who) + ": needs room for 2n - 1 nodes and n references", RT_ERR_INVALID_ARG);
    rtlbvh::Scratch& S = c->lbvh;
    if (on_device) {
        if (((uintptr_t)verts | (uintptr_t)nodes) & 15u)
            return set_err(c, std::string(who) + ": d_verts and d_nodes must be 16-byte aligned", RT_ERR_INVALID_ARG);
    } else {
        for (int32_t i = 0; i < nidx; ++i)
            if (idx[i] < 0 || idx[i] >= nv) return set_err(c, "mesh_indices out of range", RT_ERR_BAD_SCENE);
    }
    HIPC(c, hipSetDevice(c->device));
    for (hipEvent_t& e : S.ev)
        if (!e) HIPC(c, hipEventCreate(&e));
    S.timed = false;
    const float4* d_verts = (const float4*)verts;
    const int32_t* d_idx = idx;
    float4* d_nodes = (float4*)nodes;
    int32_t* d_refs = refs;
    if (on_device) {   // the caller's stream may still be producing the inputs
        HIPC(c, hipEventRecord(S.ev[2], (hipStream_t)stream));
        HIPC(c, hipStreamWaitEvent(c->stream, S.ev[2], 0));
    } else {
        if (rtlbvh::reserve(S.verts, (size_t)nv * sizeof(float4)) != hipSuccess ||
            rtlbvh::reserve(S.idx, (size_t)nidx * 4) != hipSuccess ||
            rtlbvh::reserve(S.nodes, (size_t)(2 * (int64_t)n - 1) * sizeof(rt_bvh_node)) != hipSuccess ||
            rtlbvh::reserve(S.refs, (size_t)n * 4) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(c, std::string(who) + ": out of device memory", RT_ERR_OUT_OF_MEMORY);
        }
        HIPC(c, hipMemcpyAsync(S.verts.p, verts, (size_t)nv * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(S.idx.p, idx, (size_t)nidx * 4, hipMemcpyHostToDevice, c->stream));
        d_verts = (const float4*)S.verts.p;
        d_idx = (const int32_t*)S.idx.p;
        d_nodes = (float4*)S.nodes.p;
        d_refs = (int32_t*)S.refs.p;
    }
    HIPC(c, hipEventRecord(S.ev[0], c->stream));
    std::string err;
    int32_t nn = 0;
    const int rc = rtlbvh::build(S, c->stream, d_verts, nv, d_idx, n, max_leaf, extent_keys, d_nodes, 2 * n - 1, d_refs, &nn,
                                 err);
    if (rc != RT_OK) {
        (void)hipStreamSynchronize(c->stream);
        return set_err(c, rc == RT_ERR_BAD_SCENE ? err : std::string(who) + ": " + err, rc);
    }
    HIPC(c, hipEventRecord(S.ev[1], c->stream));
    if (!on_device) {
        HIPC(c, hipMemcpyAsync(nodes, d_nodes, (size_t)nn * sizeof(rt_bvh_node), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(refs, d_refs, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    S.timed = true;
    *num_nodes = nn;
    return RT_OK;
}

int rt_build_bvh(rt_ctx* c, const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx, int32_t max_leaf,
                 rt_bvh_node* nodes, int32_t node_cap, int32_t* refs, int32_t ref_cap, int32_t* num_nodes) {
    return build_bvh(c, "rt_build_bvh", verts, nv, idx, nidx, max_leaf, nodes, node_cap, refs, ref_cap, num_nodes, false,
                     nullptr);
}

int rt_build_bvh_device(rt_ctx* c, const rt_float4* d_verts, int32_t nv, const int32_t* d_idx, int32_t nidx,
                        int32_t max_leaf, rt_bvh_node* d_nodes, int32_t node_cap, int32_t* d_refs, int32_t ref_cap,
                        int32_t* num_nodes, void* stream) {
    return build_bvh(c, "rt_build_bvh_device", d_verts, nv, d_idx, nidx, max_leaf, d_nodes, node_cap, d_refs, ref_cap,
                     num_nodes, true, stream);
}

int rt_last_build_timing(rt_ctx* c, float* total_ms) {
    if (!c || !total_ms) return set_err(c, "rt_last_build_timing: invalid argument", RT_ERR_INVALID_ARG);
    if (!c->lbvh.timed) return set_err(c, "rt_last_build_timing: no successful build on this context", RT_ERR_INVALID_ARG);
    HIPC(c, hipEventElapsedTime(total_ms, c->lbvh.ev[0], c->lbvh.ev[1]));
    return RT_OK;
}

// ---- a renderable scene built on the GPU ----
// rt_build_bvh's tree and rt_upload_scene's records without a host round trip: the index check,
// rtlbvh::build into context-owned scratch, then rtscene's kernels write the records into arrays
// of their own, taken from the spare pool where they fit.  install_scene hands them to the context
// only when everything has succeeded; until then the previous scene is untouched, and it stays on
// any failure, when the new arrays go (back) to the pool.
static int build_scene(rt_ctx* c, const char* who, const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx,
                       int32_t max_leaf_arg, const rt_float4* normals, int32_t nnorm, const int32_t* normal_idx,
                       const rt_material* mats, int32_t nmat, const int32_t* tri_to_mat, bool on_device, void* stream) {
    if (!c) return set_err(nullptr, std::string(who) + ": ctx is NULL", RT_ERR_INVALID_ARG);
    if (!verts || !idx || !normals || !normal_idx || !mats || !tri_to_mat)
        return set_err(c, std::string(who) + ": missing array", RT_ERR_INVALID_ARG);
    if (nv <= 0 || nnorm <= 0 || nmat <= 0) return set_err(c, std::string(who) + ": empty array", RT_ERR_INVALID_ARG);
    int32_t max_leaf = 0;
    bool extent_keys = false;
    if (!lbvh::split_max_leaf(max_leaf_arg, max_leaf, extent_keys))
        return set_err(c, std::string(who) + ": max_leaf must be 1 .. 8 (| RT_BUILD_EXTENT_KEYS)", RT_ERR_INVALID_ARG);
    if (nidx <= 0 || nidx % 3 != 0 || nidx / 3 > lbvh::kMaxTris)
        return set_err(c, std::string(who) + ": needs 1 .. 2^25 triangles, 3 indices each", RT_ERR_INVALID_ARG);
    const int32_t n = nidx / 3;
    if (on_device) {
        if (((uintptr_t)verts | (uintptr_t)normals) & 15u)
            return set_err(c, std::string(who) + ": d_verts and d_normals must be 16-byte aligned", RT_ERR_INVALID_ARG);
    } else {
        for (int32_t i = 0; i < nidx; ++i) {
            if (idx[i] < 0 || idx[i] >= nv) return set_err(c, "mesh_indices out of range", RT_ERR_BAD_SCENE);
            if (normal_idx[i] < 0 || normal_idx[i] >= nnorm) return set_err(c, "mesh_normals_indices out of range", RT_ERR_BAD_SCENE);
        }
        for (int32_t t = 0; t < n; ++t)
            if (tri_to_mat[t] < 0 || tri_to_mat[t] >= nmat) return set_err(c, "tri_to_material out of range", RT_ERR_BAD_SCENE);
    }
    HIPC(c, hipSetDevice(c->device));
    rtlbvh::Scratch& S = c->lbvh;
    rtscene::Scratch& W = c->sbuild;
    for (hipEvent_t& e : W.ev)
        if (!e) HIPC(c, hipEventCreate(&e));
    W.timed = false;
    auto fail = [&](int rc, const std::string& m) {
        (void)hipStreamSynchronize(c->stream);   // nothing of this call is still running when its arrays go
        (void)hipGetLastError();
        return set_err(c, m, rc);
    };
    auto oom = [&] { return fail(RT_ERR_OUT_OF_MEMORY, std::string(who) + ": out of device memory"); };

    PendingScene ps(&c->spare);
    Scene& N = ps.s;
    auto take = [&](int k, size_t bytes) { return scene_alloc(N, k, bytes, ps.pool); };
    if (take(Scene::kIdx, (size_t)nidx * 4) != hipSuccess || take(Scene::kNormalIdx, (size_t)nidx * 4) != hipSuccess ||
        take(Scene::kRefTri, (size_t)n * 4) != hipSuccess || take(Scene::kOut, 32) != hipSuccess ||
        rtlbvh::reserve(W.mats, (size_t)nmat * sizeof(rt_material)) != hipSuccess ||
        rtlbvh::reserve(S.nodes, (size_t)(2 * (int64_t)n - 1) * sizeof(rt_bvh_node)) != hipSuccess)
        return oom();
    const float4* d_verts = (const float4*)verts;
    const float4* d_normals = (const float4*)normals;
    const int32_t* d_tri_to_mat = tri_to_mat;
    hipMemcpyKind kind = hipMemcpyDeviceToDevice;
    if (on_device) {   // the caller's stream may still be producing the inputs
        HIPC(c, hipEventRecord(W.ev[2], (hipStream_t)stream));
        HIPC(c, hipStreamWaitEvent(c->stream, W.ev[2], 0));
    } else {
        kind = hipMemcpyHostToDevice;
        if (take(Scene::kVerts, (size_t)nv * sizeof(float4)) != hipSuccess ||
            take(Scene::kNormals, (size_t)nnorm * sizeof(float4)) != hipSuccess ||
            rtlbvh::reserve(W.tri_to_mat, (size_t)n * 4) != hipSuccess)
            return oom();
        HIPC(c, hipMemcpyAsync(N.verts(), verts, (size_t)nv * sizeof(float4), kind, c->stream));
        HIPC(c, hipMemcpyAsync(N.normals(), normals, (size_t)nnorm * sizeof(float4), kind, c->stream));
        HIPC(c, hipMemcpyAsync(W.tri_to_mat.p, tri_to_mat, (size_t)n * 4, kind, c->stream));
        d_verts = N.verts();
        d_normals = N.normals();
        d_tri_to_mat = (const int32_t*)W.tri_to_mat.p;
    }
    // the scene's own copies of the index arrays (rt_update_vertices reads them)
    HIPC(c, hipMemcpyAsync(N.idx(), idx, (size_t)nidx * 4, kind, c->stream));
    HIPC(c, hipMemcpyAsync(N.normal_idx(), normal_idx, (size_t)nidx * 4, kind, c->stream));
    HIPC(c, hipMemcpyAsync(W.mats.p, mats, (size_t)nmat * sizeof(rt_material), hipMemcpyHostToDevice, c->stream));

    HIPC(c, hipEventRecord(W.ev[0], c->stream));
    std::string err;
    uint32_t bad = 0;
    int rc = rtscene::check(W, c->stream, N.idx(), nv, N.normal_idx(), nnorm, d_tri_to_mat, nmat, n, &bad, err);
    if (rc != RT_OK) return fail(rc, std::string(who) + ": " + err);
    if (bad)
        return fail(RT_ERR_BAD_SCENE, bad & rtscene::kBadVerts     ? "mesh_indices out of range"
                                      : bad & rtscene::kBadNormals ? "mesh_normals_indices out of range"
                                                                   : "tri_to_material out of range");
    int32_t nn = 0;
    rc = rtlbvh::build(S, c->stream, d_verts, nv, N.idx(), n, max_leaf, extent_keys, (float4*)S.nodes.p, 2 * n - 1,
                       N.ref_tri(), &nn, err);
    if (rc != RT_OK) return fail(rc, rc == RT_ERR_BAD_SCENE ? err : std::string(who) + ": " + err);
    const uint32_t K = (uint32_t)(nn - 1) / 2u;
    if (scene_alloc_records(N, (size_t)std::max<uint32_t>(K, 1u) * 4, (size_t)n * 3 + 1, (size_t)n * 7, 1, ps.pool) != hipSuccess ||
        take(Scene::kLevelIds, (size_t)K * 4) != hipSuccess)
        return oom();
    HIPC(c, hipMemsetAsync(N.tris() + (size_t)n * 3, 0, sizeof(float4), c->stream));   // the trailing pad
    HIPC(c, hipMemsetAsync(N.leaf(), 0, sizeof(int2), c->stream));                      // no escape leaves: {0, 0}
    rtscene::Args a{};
    a.verts = d_verts; a.normals = d_normals; a.idx = N.idx(); a.normal_idx = N.normal_idx(); a.tri_to_mat = d_tri_to_mat;
    a.mats = (const float4*)W.mats.p; a.nodes = (const float4*)S.nodes.p; a.refs = N.ref_tri();
    a.n = n; a.max_leaf = max_leaf; a.K = K;
    a.wnodes = N.wnodes(); a.tris = N.tris(); a.shade = N.shade();
    a.level_ids = N.level_ids(); a.out = N.out();
    std::vector<uint32_t>& level_begin = N.level_begin;
    uint32_t out[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (K == 0) {   // the root is a leaf: no inner record, four zero float4s in its place
        HIPC(c, hipMemsetAsync(N.wnodes(), 0, 4 * sizeof(float4), c->stream));
        rc = rtscene::leaf_records(W, c->stream, a, err);
        level_begin.assign(1, 0u);
    } else {
        rc = rtscene::records(W, S, c->stream, a, level_begin, err);
    }
    if (rc != RT_OK) return fail(rc, std::string(who) + ": " + err);
    HIPC(c, hipEventRecord(W.ev[1], c->stream));
    rt_bvh_node root_leaf{};
    if (K == 0) HIPC(c, hipMemcpyAsync(&root_leaf, S.nodes.p, sizeof root_leaf, hipMemcpyDeviceToHost, c->stream));
    else HIPC(c, hipMemcpyAsync(out, N.out(), sizeof out, hipMemcpyDeviceToHost, c->stream));
    if (wait_stream(c->stream) != hipSuccess) return fail(RT_ERR_DEVICE, std::string(who) + ": the build's kernels failed");
    if (K == 0) {
        const float box[6] = {root_leaf.min.x, root_leaf.min.y, root_leaf.min.z, root_leaf.max.x, root_leaf.max.y, root_leaf.max.z};
        std::memcpy(out + 2, box, sizeof box);
        HIPC(c, hipMemcpy(N.out(), out, sizeof out, hipMemcpyHostToDevice));
    }
    if (take(Scene::kLevelBegin, 67 * 4) != hipSuccess) return oom();   // (every plan fits: at most 66 heights)
    HIPC(c, hipMemcpy(N.d_level_begin(), level_begin.data(), level_begin.size() * 4, hipMemcpyHostToDevice));

    N.root = K ? 0u : rtrec::leaf_ref((uint32_t)n, 0u);   // the root's record is the breadth-first order's first
    N.n_inner = K;
    N.fast_div = out[0] ? 1 : 0;
    N.clean = 1;
    float box[6];
    std::memcpy(box, out + 2, sizeof box);
    N.bounds_min = rt_float4{box[0], box[1], box[2], 1.0f};
    N.bounds_max = rt_float4{box[3], box[4], box[5], 1.0f};
    N.have_bounds = true;
    N.nv = nv; N.nnorm = nnorm; N.nref = (uint32_t)n; N.ntri = (uint32_t)n;
    N.why.clear();
    N.refittable = true;
    if (const int rc2 = install_scene(c, std::move(N))) return rc2;   // the context takes the new scene
    W.timed = true;
    return RT_OK;
}

int rt_build_scene(rt_ctx* c, const rt_float4* verts, int32_t nv, const int32_t* idx, int32_t nidx, int32_t max_leaf,
                   const rt_float4* normals, int32_t nnorm, const int32_t* normal_idx, const rt_material* mats, int32_t nmat,
                   const int32_t* tri_to_mat) {
    return build_scene(c, "rt_build_scene", verts, nv, idx, nidx, max_leaf, normals, nnorm, normal_idx, mats, nmat, tri_to_mat,
                       false, nullptr);
}

int rt_build_scene_device(rt_ctx* c, const rt_float4* d_verts, int32_t nv, const int32_t* d_idx, int32_t nidx, int32_t max_leaf,
                          const rt_float4* d_normals, int32_t nnorm, const int32_t* d_normal_idx, const rt_material* mats,
                          int32_t nmat, const int32_t* d_tri_to_mat, void* stream) {
    return build_scene(c, "rt_build_scene_device", d_verts, nv, d_idx, nidx, max_leaf, d_normals, nnorm, d_normal_idx, mats,
                       nmat, d_tri_to_mat, true, stream);
}

int rt_last_scene_build_timing(rt_ctx* c, float* total_ms) {
    if (!c || !total_ms) return set_err(c, "rt_last_scene_build_timing: invalid argument", RT_ERR_INVALID_ARG);
    if (!c->sbuild.timed)
        return set_err(c, "rt_last_scene_build_timing: no successful rt_build_scene on this context", RT_ERR_INVALID_ARG);
    HIPC(c, hipEventElapsedTime(total_ms, c->sbuild.ev[0], c->sbuild.ev[1]));
    return RT_OK;
}

int rt_scene_walk_refs(rt_ctx* c, int32_t host_twin, uint32_t* words, uint64_t cap, uint64_t* n_words, uint32_t* root) {
    if (!c || !n_words || !root || (!words && cap)) return set_err(c, "rt_scene_walk_refs: invalid argument", RT_ERR_INVALID_ARG);
    if (!c->have_scene) return set_err(c, "rt_scene_walk_refs: no scene", RT_ERR_NO_SCENE);
    HIPC(c, hipSetDevice(c->device));
    const Scene& S = c->scene;
    *n_words = 0;
    *root = rtrec::kWalkNone;
    const size_t n_rec = S.n_wnodes4 / 4;
    std::vector<uint32_t> walk;
    if (host_twin) {   // the records as they stand on the device, through rtamd::derive_walk
        if (S.split || S.n_tris4 == 0) return RT_OK;
        std::vector<rt_float4> wn(S.n_wnodes4);
        std::vector<std::pair<int32_t, int32_t>> table(S.n_leaf);
        HIPC(c, hipMemcpy(wn.data(), S.wnodes(), S.n_wnodes4 * sizeof(float4), hipMemcpyDeviceToHost));
        if (S.n_leaf) HIPC(c, hipMemcpy(table.data(), S.leaf(), S.n_leaf * sizeof(int2), hipMemcpyDeviceToHost));
        uint32_t wr = rtrec::kWalkNone;
        if (!rtamd::derive_walk(wn.data(), n_rec, table.data(), table.size(), (uint32_t)S.n_wnodes4,
                                (uint32_t)((S.n_tris4 - 1) / 3), S.root, walk, wr))
            return RT_OK;
        *root = wr;
    } else {
        if (!S.walk_off) return RT_OK;
        walk.resize(2 * n_rec);
        HIPC(c, hipMemcpy(walk.data(), (const char*)S.wnodes() + S.walk_off, walk.size() * 4, hipMemcpyDeviceToHost));
        *root = S.walk_root;
    }
    *n_words = walk.size();
    if (walk.size() && words) std::memcpy(words, walk.data(), std::min<uint64_t>(cap, walk.size()) * 4);
    return RT_OK;
}

int rt_refit_level_counts(rt_ctx* c, uint32_t* counts, int32_t cap, int32_t* heights) {
    if (!c || !heights || cap < 0 || (cap > 0 && !counts))
        return set_err(c, "rt_refit_level_counts: invalid argument", RT_ERR_INVALID_ARG);
    if (!c->have_scene) return set_err(c, "rt_refit_level_counts: no scene uploaded", RT_ERR_NO_SCENE);
    const Scene& r = c->scene;
    if (!r.refittable || r.level_begin.empty())
        return set_err(c, "rt_refit_level_counts: the scene has no refit data (" + r.why + ")", RT_ERR_BAD_SCENE);
    const int32_t h = (int32_t)r.level_begin.size() - 1;
    for (int32_t i = 0; i < h && i < cap; ++i) counts[i] = r.level_begin[i + 1] - r.level_begin[i];
    *heights = h;
    return RT_OK;
}

// ---- the SAH cost of the scene as it stands on the GPU ----
// Read-only and synchronous on the context's stream; frames in flight read the same records and
// are not waited for.
int rt_scene_sah(rt_ctx* c, double* inner_area, double* leaf_area_tris, double* root_area) {
    if (!c || !inner_area || !leaf_area_tris || !root_area)
        return set_err(c, "rt_scene_sah: invalid argument", RT_ERR_INVALID_ARG);
    if (!c->have_scene) return set_err(c, "rt_scene_sah: no scene uploaded", RT_ERR_NO_SCENE);
    auto half_area = [](const float mn[3], const float mx[3]) {
        const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
        return (double)((dx * dy + dy * dz) + dz * dx);
    };
    const Scene& S = c->scene;
    const float bmn[3] = {S.bounds_min.x, S.bounds_min.y, S.bounds_min.z};
    const float bmx[3] = {S.bounds_max.x, S.bounds_max.y, S.bounds_max.z};
    HIPC(c, hipSetDevice(c->device));
    if (S.n_inner == 0) {   // the root is a leaf: its box is the scene's, its count the reference's
        if (!S.have_bounds)
            return set_err(c, "rt_scene_sah: a root-leaf scene from a scene image carries no box", RT_ERR_BAD_SCENE);
        int64_t cnt = rtrec::ref_count(S.root);
        if (!(S.root & rtrec::kLeafBit)) cnt = 0;
        if ((uint32_t)cnt == rtrec::kCntEscape) {
            const uint32_t e = rtrec::ref_offset(S.root);
            int2 entry = make_int2(0, 0);
            if (e < S.n_leaf) HIPC(c, hipMemcpy(&entry, S.leaf() + e, sizeof entry, hipMemcpyDeviceToHost));
            cnt = std::max(entry.y, 0);
        }
        *root_area = half_area(bmn, bmx);
        *inner_area = 0.0;
        *leaf_area_tris = *root_area * (double)cnt;
        return RT_OK;
    }
    const uint32_t n_inner = (uint32_t)std::min<size_t>(S.n_inner, S.n_wnodes4 / 4);   // (an image's header is not trusted)
    const uint32_t nblocks = rtsah::blocks_for(n_inner);
    if (rtlbvh::reserve(c->sah_part, 2 * (size_t)nblocks * sizeof(double)) != hipSuccess ||
        rtlbvh::reserve(c->sah_out, sizeof(rtsah::Result)) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, "rt_scene_sah: out of device memory", RT_ERR_OUT_OF_MEMORY);
    }
    rtsah::Result res{};
    HIPC(c, hipMemsetAsync(c->sah_out.p, 0, sizeof res, c->stream));
    HIPC(c, rtsah::launch(S.wnodes(), n_inner, S.leaf(), (uint32_t)S.n_leaf, S.root, (double*)c->sah_part.p,
                          (rtsah::Result*)c->sah_out.p, c->stream));
    HIPC(c, hipMemcpyAsync(&res, c->sah_out.p, sizeof res, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, wait_stream(c->stream));
    // rt_scene_bounds' box; a scene image carries none: the root record's own box, the union of its two slots
    *root_area = S.have_bounds ? half_area(bmn, bmx) : half_area(res.root_box, res.root_box + 3);
    *inner_area = *root_area + res.inner_area;
    *leaf_area_tris = res.leaf_area_tris;
    return RT_OK;
}

// ---- scene image: the uploaded device layouts as one contiguous device buffer ----
// [header, 256 B][inner records][triangle records][shading records][escape leaves],
// each section 256-B aligned.  Multi-GPU runs build the scene once and broadcast the image
// over RCCL ("ncclBroadcast of scene buffers at load"); every rank loads it.
namespace {
constexpr uint32_t kImageMagic = 0x52544D49u;   // "IMTR"
constexpr uint32_t kImageVersion = 2;            // 2: no triangle-rank section (round 2's hit-node sort keys)
struct ImageHeader {
    uint32_t magic, version;
    uint64_t n_wnodes4, n_tris4, n_shade4, n_leaf;
    uint32_t root, n_inner;
    int32_t fast_div, clean;
};
static_assert(sizeof(ImageHeader) <= 256, "image header fits its section");
inline uint64_t sect(uint64_t bytes) { return (bytes + 255u) & ~uint64_t(255u); }
uint64_t image_bytes(const ImageHeader& h) {
    return 256 + sect(h.n_wnodes4 * 16) + sect(h.n_tris4 * 16) + sect(h.n_shade4 * 16) + sect(h.n_leaf * 8);
}
}  // namespace

int rt_scene_image_size(rt_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return RT_ERR_INVALID_ARG;
    if (!c->have_scene) return set_err(c, "rt_scene_image_size: no scene uploaded", RT_ERR_NO_SCENE);
    const Scene& S = c->scene;
    ImageHeader h{kImageMagic, kImageVersion, S.n_wnodes4, S.n_tris4, S.n_shade4, S.n_leaf, 0, 0, 0, 0};
    *bytes = image_bytes(h);
    return RT_OK;
}

int rt_scene_image_pack(rt_ctx* c, void* d_image, uint64_t bytes, void* stream) {
    if (!c || !d_image) return RT_ERR_INVALID_ARG;
    if (!c->have_scene) return set_err(c, "rt_scene_image_pack: no scene uploaded", RT_ERR_NO_SCENE);
    const Scene& S = c->scene;
    const ImageHeader h{kImageMagic, kImageVersion, S.n_wnodes4, S.n_tris4, S.n_shade4, S.n_leaf,
                        S.root, S.n_inner, S.fast_div, S.clean};
    if (bytes < image_bytes(h)) return set_err(c, "rt_scene_image_pack: buffer too small", RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    uint8_t* p = (uint8_t*)d_image;
    HIPC(c, hipMemcpyAsync(p, &h, sizeof h, hipMemcpyHostToDevice, s));
    p += 256;
    for (const auto& q : S.sections()) {
        HIPC(c, hipMemcpyAsync(p, q.first, q.second, hipMemcpyDeviceToDevice, s));
        p += sect(q.second);
    }
    HIPC(c, hipStreamSynchronize(s));   // the header's host copy is a stack object
    return RT_OK;
}

int rt_scene_image_load(rt_ctx* c, const void* d_image, uint64_t bytes, void* stream) {
    if (!c || !d_image || bytes < 256) return set_err(c, "rt_scene_image_load: invalid argument", RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    ImageHeader h;
    HIPC(c, hipMemcpyAsync(&h, d_image, sizeof h, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (h.magic != kImageMagic || h.version != kImageVersion || image_bytes(h) > bytes || h.n_wnodes4 == 0 || h.n_tris4 == 0 ||
        h.n_leaf == 0)
        return set_err(c, "rt_scene_image_load: not a scene image", RT_ERR_BAD_SCENE);
    if (const int rc = drop_scene(c)) return rc;   // before the new one is allocated: peak memory is one scene's
    PendingScene ps(nullptr);
    Scene& S = ps.s;
    HIPC(c, scene_alloc_records(S, h.n_wnodes4, h.n_tris4, h.n_shade4, h.n_leaf, nullptr));
    const uint8_t* p = (const uint8_t*)d_image + 256;
    for (const auto& q : S.sections()) {
        HIPC(c, hipMemcpyAsync(q.first, p, q.second, hipMemcpyDeviceToDevice, s));
        p += sect(q.second);
    }
    HIPC(c, hipStreamSynchronize(s));
    S.root = h.root; S.n_inner = h.n_inner; S.fast_div = h.fast_div; S.clean = h.clean;
    S.why = "the scene came from rt_scene_image_load; upload it with rt_upload_scene to update it";
    return install_scene(c, std::move(S));   // (an image carries no root box: have_bounds stays false)
}

int rt_set_params(rt_ctx* c, const rt_params* p) {
    if (!c || !p) return RT_ERR_INVALID_ARG;
    c->params = *p;
    c->have_params = true;
    return RT_OK;
}

int64_t rt_tiling_pixels(uint32_t w, uint32_t h, const rt_tiling* t) {
    if (!t || t->nranks <= 1) return (int64_t)w * h;
    if (t->band_rows <= 0 || t->rank < 0 || t->rank >= t->nranks) return -1;
    const int64_t nbands = ((int64_t)h + t->band_rows - 1) / t->band_rows;
    int64_t rows = 0;
    for (int64_t b = t->rank; b < nbands; b += t->nranks) rows += std::min<int64_t>(t->band_rows, (int64_t)h - b * t->band_rows);
    return rows * w;
}

// The scene as every frame and query kernel takes it.  flags: RT_FLAG_EXACT_DIV keeps the slab test's division.
static rtk::DevScene dev_scene(const Scene& sc, uint32_t flags) {
    return rtk::DevScene{sc.wnodes(),
                         sc.tris(),
                         sc.shade(),
                         sc.leaf(),
                         (uint32_t)(sc.n_wnodes4 * 16),
                         (uint32_t)(sc.rec_units() * 16),
                         sc.root,
                         sc.n_inner,
                         (sc.fast_div && !(flags & RT_FLAG_EXACT_DIV)) ? 1 : 0,
                         sc.clean};
}
// the fast kernels (any quotient domain: traverse_fast picks the variant) need a clean scene
// whose records one buffer descriptor covers; frames and queries alike
static bool scene_fast(const Scene& sc) { return sc.clean != 0 && !sc.split; }

// rt_render_device, and (batch != null) rt_render_device_batch: nbatch depth-1 frames with the
// cameras batch[0..nbatch-1] in one launch, frame i at d_out + i * bstride
static int render_frames(rt_ctx* c, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, const rt_tiling* tiling,
                         uint32_t* d_out, const rt_aux* d_aux, void* stream, const rt_params* batch, int32_t nbatch,
                         uint64_t bstride) {
    if (!c || !d_out || w == 0 || h == 0 || depth < 0 || depth > RT_MAX_DEPTH)
        return set_err(c, "rt_render_device: invalid argument", RT_ERR_INVALID_ARG);
    if (batch) {
        if (nbatch < 1 || nbatch > rtk::kMaxBatch)
            return set_err(c, "rt_render_device_batch: nframes must be 1.." + std::to_string(rtk::kMaxBatch), RT_ERR_INVALID_ARG);
        if (depth < 1 || (depth > 1 && !(flags & RT_FLAG_WAVEFRONT)))
            return set_err(c, "rt_render_device_batch: depth 1, or depth > 1 with RT_FLAG_WAVEFRONT", RT_ERR_INVALID_ARG);
        for (int32_t i = 1; i < nbatch; ++i) {
            if (std::memcmp(&batch[i].scene_aabb_min, &batch[0].scene_aabb_min, 2 * sizeof(rt_float4)) != 0)
                return set_err(c, "rt_render_device_batch: the frames' scene boxes differ", RT_ERR_INVALID_ARG);
            // the bounce launches shade every frame's rays with one light (the reference's is a
            // global, RayTracer.cpp:60)
            if (depth > 1 && std::memcmp(&batch[i].light_pos, &batch[0].light_pos, sizeof(rt_float4)) != 0)
                return set_err(c, "rt_render_device_batch: depth > 1 needs one light position for all frames",
                               RT_ERR_INVALID_ARG);
        }
        if (c->trace.on || c->tline.on)
            return set_err(c, "rt_render_device_batch: not with rt_fetch_counts / rt_wave_timeline", RT_ERR_INVALID_ARG);
    }
    const uint32_t K = batch ? (uint32_t)nbatch : 1u;
    if ((flags & RT_FLAG_STRICT_MATH) && (flags & RT_FLAG_HW_MATH))
        return set_err(c, "rt_render_device: RT_FLAG_STRICT_MATH and RT_FLAG_HW_MATH exclude each other", RT_ERR_INVALID_ARG);
    if (!c->have_scene) return set_err(c, "rt_render_device: no scene uploaded", RT_ERR_NO_SCENE);
    if (!batch && !c->have_params) return set_err(c, "rt_render_device: no params set", RT_ERR_NO_SCENE);
    rt_tiling whole{0, 1, 16, 0};
    const rt_tiling* T = tiling ? tiling : &whole;
    const int64_t npix = rt_tiling_pixels(w, h, T);
    if (npix < 0) return set_err(c, "rt_render_device: bad tiling", RT_ERR_INVALID_ARG);
    if (batch && bstride < (uint64_t)npix)
        return set_err(c, "rt_render_device_batch: frame_stride below the frame's pixels", RT_ERR_INVALID_ARG);
    // a batch launch's pixel space: frame f's pixel p is f * fpx + p -- the global traversal stack
    // is indexed in it, and at depth > 1 so are the rays the bounce launches carry, which finish
    // at out[f * fpx + p]: there fpx is the frame stride (frames need not be contiguous: a rank's
    // band buffers padded to the largest rank's, bench.py at N > 1), at depth 1 the frame's pixels
    const uint64_t fpx = batch && depth > 1 ? bstride : (uint64_t)npix;
    if (batch && fpx * K >= (1ull << 32))
        return set_err(c, "rt_render_device_batch: more than 2^32 pixels in one launch", RT_ERR_INVALID_ARG);
    if (batch && d_aux) return set_err(c, "rt_render_device_batch: no aux planes", RT_ERR_INVALID_ARG);
    const bool aux = d_aux && d_aux->hits && d_aux->t && d_aux->rgb;
    if (d_aux && !aux && (d_aux->hits || d_aux->t || d_aux->rgb))
        return set_err(c, "rt_render_device: aux needs hits, t and rgb together", RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    if (npix == 0) return RT_OK;
    int rc = RT_OK;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    rt_ctx::FrameSlot* Lp = nullptr;
    // a slot per (stream, tiling): one stream may render several tilings in turn (rt_render's row
    // groups), each with its own longest-first order
    const uint64_t tkey = T->nranks > 1 ? ((uint64_t)(uint32_t)T->rank << 40) ^ ((uint64_t)(uint32_t)T->nranks << 20) ^
                                              (uint64_t)(uint32_t)T->band_rows ^ (1ull << 63)
                                        : 0;
    if ((rc = slot_for(c, (void*)s, tkey, &Lp))) return rc;
    rt_ctx::FrameSlot& L = *Lp;
    c->last_slot = &L;
    c->last_group.clear();
    c->query_last = false;
    const int math = (flags & RT_FLAG_STRICT_MATH) ? 0 : (flags & RT_FLAG_HW_MATH) ? 1 : 2;

    rtk::Frame F;
    const rt_params& P = batch ? batch[0] : c->params;
    F.a = make_float3(P.a.x, P.a.y, P.a.z);
    F.b = make_float3(P.b.x, P.b.y, P.b.z);
    F.c = make_float3(P.c.x, P.c.y, P.c.z);
    F.campos = make_float3(P.campos.x, P.campos.y, P.campos.z);
    F.light_pos = make_float3(P.light_pos.x, P.light_pos.y, P.light_pos.z);
    F.smin = make_float3(P.scene_aabb_min.x, P.scene_aabb_min.y, P.scene_aabb_min.z);
    F.smax = make_float3(P.scene_aabb_max.x, P.scene_aabb_max.y, P.scene_aabb_max.z);
    F.w = w;
    F.h = h;
    F.depth = depth;
    F.flags = flags;
    F.rank = T->nranks > 1 ? T->rank : 0;
    F.nranks = T->nranks > 1 ? T->nranks : 1;
    F.band_rows = T->nranks > 1 ? T->band_rows : 16;
    F.local_rows = (uint32_t)(npix / w);
    F.tiles_x = (w + rtk::kBlockPx - 1) / rtk::kBlockPx;
    F.tiles_y = (F.local_rows + rtk::kBlockPx - 1) / rtk::kBlockPx;
    F.num_blocks = F.tiles_x * F.tiles_y;

    const Scene& sc = c->scene;
    rtk::DevScene S = dev_scene(sc, flags);
    rtk::Outputs O;
    O.out = d_out;
    O.hits = aux ? d_aux->hits : nullptr;
    O.t = aux ? d_aux->t : nullptr;
    O.rgb = aux ? d_aux->rgb : nullptr;
    O.overflow = c->d_overflow;
    O.local_pixels = fpx * K;   // a batch launch's pixel space: its frames one after the other
    O.fcount = nullptr;
    O.frame_rows = c->frame_rows && !batch ? 1u : 0u;
    O.wtime = nullptr;
    const bool traced = c->trace.on;
    const bool tline = c->tline.on;
    // rt_wave_timeline: launch k's wave records at the next free words of the device buffer
    auto tline_region = [&](uint32_t waves) -> uint32_t* {
        if (c->tline.used + (size_t)waves * rtk::kTlRecord > c->tline.limit) return nullptr;
        uint32_t* p = c->tline.d_words + c->tline.used;
        c->tline.used += (size_t)waves * rtk::kTlRecord;
        c->tline.waves.push_back(waves);
        c->tline.frame.push_back(c->tline.cur_frame);
        c->tline.bounce.push_back((uint32_t)c->tline.waves.size() - 1u);   // fixed up by the caller below
        return p;
    };

    rt_ctx::FrameEv& E = c->ring[c->frames % rt_ctx::kRing];
    for (hipEvent_t& e : E.e)
        if (!e) HIPC(c, hipEventCreate(&e));
    E.has_k = false;
    // depth 1 always takes the wavefront route: it is then one first_bounce_kernel launch,
    // the fused kernel specialised to a single bounce
    const bool wavefront = ((flags & RT_FLAG_WAVEFRONT) && depth > 0) || depth == 1;

    if ((rc = ensure(c, L.d_gstack, L.gstack_cap, (size_t)fpx * rtk::kGlobalStack * K))) return rc;
    O.gstack = L.d_gstack;
    // frame counters, two parity sets: per bounce k (kBounceWords from kBounceWords k) its
    // queue size and its work cursor; [kRestartSlot] restarted traversals; then per queue
    // k = 1 .. its chunk sums and super-chunk sums (segmented queues, rtk::WQ)
    const size_t nseg = (size_t)F.num_blocks * 4 * K;   // bounce 0's waves (every frame's); later queues have fewer groups
    const size_t nchunk = (nseg + rtk::kChunkSegs - 1) / rtk::kChunkSegs;
    const size_t nsuper = (nseg + rtk::kSuperSegs - 1) / rtk::kSuperSegs;
    const size_t set_words = (kCounters + (depth > 1 ? (size_t)(depth - 1) * (nchunk + nsuper) : 0) + 31) & ~(size_t)31;
    if (!L.d_wcnt || L.wcnt_set < set_words) {
        if ((rc = ensure(c, L.d_wcnt, L.wcnt_cap, 2 * set_words))) return rc;
        HIPC(c, hipMemsetAsync(L.d_wcnt, 0, 2 * set_words * sizeof(uint32_t), s));
        L.wcnt_set = set_words;
    }
    const uint64_t par = L.nframe & 1u;
    uint32_t* cnt = L.d_wcnt + par * L.wcnt_set;
    F.zero_next = L.d_wcnt + (par ^ 1u) * L.wcnt_set;
    F.nzero = (uint32_t)L.wcnt_set;   // all of it: the next frame may be deeper than this one
    auto sums = [&](int k) { return cnt + kCounters + (size_t)(k - 1) * (nchunk + nsuper); };   // queue k >= 1
    O.restarts = cnt + kRestartSlot;

    // static block order: a host-built table per block grid, made once (a new table goes into
    // a new allocation, so frames in flight that read another grid's table never wait)
    F.tile_order = nullptr;
    for (const auto& o : c->orders)
        if (o.tx == F.tiles_x && o.ty == F.tiles_y && o.k == K) F.tile_order = o.d;
    if (!F.tile_order) {
        if (c->orders.size() >= rt_ctx::kMaxOrders) {   // many grids: drop them all, once every frame is done
            HIPC(c, hipStreamSynchronize(s));
            for (auto& f : c->slots)
                if (f.idle) HIPC(c, hipEventSynchronize(f.idle));
            for (auto& o : c->orders) (void)hipFree(o.d);
            c->orders.clear();
        }
        std::vector<uint32_t> tab = tile_order_table(F.tiles_x, F.tiles_y);
        if (K > 1) {   // a batch: each tile of the static order for every frame, side by side
            std::vector<uint32_t> tk((size_t)tab.size() * K);
            for (size_t i = 0; i < tk.size(); ++i) tk[i] = tab[i / K] + (uint32_t)(i % K) * F.num_blocks;
            tab.swap(tk);
        }
        uint32_t* d = nullptr;
        size_t cap = 0;
        if ((rc = ensure(c, d, cap, tab.size()))) return rc;
        const hipError_t e = hipMemcpy(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return set_err(c, std::string("rt_render_device: order table: ") + hipGetErrorString(e), RT_ERR_DEVICE);
        }
        c->orders.push_back(rt_ctx::OrderTab{F.tiles_x, F.tiles_y, K, d});
        F.tile_order = d;
    }
    // Adaptive longest-first order from the previous frame of the same geometry on this
    // slot, built by that frame's last block; the first frame runs the static order.
    F.tile_cost = nullptr;
    F.lpt_next = nullptr;
    F.done = nullptr;
    if (!(flags & RT_FLAG_STATIC_ORDER)) {
        const uint32_t units = F.num_blocks * K;   // every frame's blocks (the order's entries)
        const bool fresh = L.cost_cap < units || !L.d_done;
        if ((rc = ensure(c, L.d_cost, L.cost_cap, units))) return rc;
        if ((rc = ensure(c, L.d_lpt, L.lpt_cap, units))) return rc;
        if (!L.d_done) {
            size_t one = 0;
            if ((rc = ensure(c, L.d_done, one, 1))) return rc;
        }
        const uint64_t key = ((uint64_t)F.tiles_x << 48) ^ ((uint64_t)F.tiles_y << 32) ^ F.local_rows ^
                             ((uint64_t)c->scene_gen << 20) ^ ((uint64_t)K << 60);
        if (fresh || key != L.cost_key) {
            HIPC(c, hipMemsetAsync(L.d_done, 0, sizeof(uint32_t), s));
            L.cost_key = key;
            L.cost_ready = false;
        }
        if (L.cost_ready) F.tile_order = L.d_lpt;
        // The order is rebuilt every lpt_every()-th launch on the slot (and whenever it is not
        // ready): only those launches time their blocks, and their last block sorts; the others
        // run the order as it is, with no epilogue at all (a wave that is done leaves at once).
        if (!L.cost_ready || L.nframe % lpt_every() == 0) {
            F.tile_cost = L.d_cost;
            F.lpt_next = L.d_lpt;
            F.done = L.d_done;
        }
    }
    const bool fast = scene_fast(sc);
    // The depth-1 kernels walk by the scene's walk references.  A scene without them (a leaf of more
    // than 16 references: only an uploaded foreign BVH has one) renders its depth-1 frames with the
    // general traversal, as an unclean scene does: same pixels.
    const bool fast0 = fast && (depth > 1 || sc.walk_off != 0);
    rtk::Walk walk{sc.walk_root, sc.walk_off};
    const dim3 grid(F.num_blocks * K), block(rtk::kBlockThreads);
    int ax = aux ? 1 : 0;
    // A frame of one launch (depth 1, or the fused kernel) with RTK_EXT_EVENTS takes its timing
    // events from the launch itself (hipExtLaunchKernel: start and stop stamped by the dispatch),
    // instead of two marker packets around it on the stream.
    const bool one_launch = (!wavefront || depth == 1) && !traced && !tline;
    const bool ext_ev = RTK_EXT_EVENTS && one_launch;
    if (!ext_ev) HIPC(c, hipEventRecord(E.e[0], s));
    (void)hipGetLastError();   // the launches below are checked with hipGetLastError: not an earlier call's error

    // The frame's first kernel zeroes the other parity set for the next frame: from then on
    // the next frame on this slot must use that set, even if a later launch of this frame
    // fails (its set's queue counts and cursors are then stale).
    if (!wavefront) {
        void* args[] = {&S, &F, &O, &ax};
        if (ext_ev) HIPC(c, hipExtLaunchKernel(kernel_fused(math, fast), grid, block, args, 0, s, E.e[0], E.e[1], 0));
        else HIPC(c, hipLaunchKernel(kernel_fused(math, fast), grid, block, args, 0, s));
        ++L.nframe;
    } else {
        // Wavefront: bounce 0 over tiles, then one persistent launch per further bounce
        // over the queue of rays still in flight.
        if (!c->wf_grid[math] && depth > 1) {
            int cus = 0, b1 = 0;
            HIPC(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
            HIPC(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&b1, (const void*)kernel_bounce(math, true), 256, 0));
            c->wf_grid[math] = std::max(8, std::max(b1, 1) * cus * RTK_WF_GRID_PCT / 100);
        }
        // segmented queues: bounce 0's waves (4 per block) each own a segment of 64 slots;
        // later bounces have at most as many 64-ray groups
        const size_t slots = nseg * rtk::kSegRays;
        if (depth > 1) {
            if ((rc = ensure(c, L.d_wq[0], L.wq_cap[0], slots * 3))) return rc;   // 3 float4 per QRay
            if ((rc = ensure(c, L.d_wq[1], L.wq_cap[1], slots * 3))) return rc;
            if ((rc = ensure(c, L.d_perm, L.perm_cap, slots))) return rc;
            if ((rc = ensure(c, L.d_seg, L.seg_cap, nseg))) return rc;
        }
        const bool sort = (flags & RT_FLAG_WF_SORT) && depth > 1;
        // the local sort's key axis: the scene box's thinnest
        const float ext[3] = {F.smax.x - F.smin.x, F.smax.y - F.smin.y, F.smax.z - F.smin.z};
        const uint32_t thin = ext[1] <= ext[0] && ext[1] <= ext[2] ? 1u : ext[2] < ext[0] ? 2u : 0u;
        auto qbuf = [&](int k) { return depth > 1 ? (rtk::QRay*)L.d_wq[k & 1] : (rtk::QRay*)nullptr; };
        {
            rtk::WQ W{};
            W.out = depth > 1 ? qbuf(1) : nullptr;
            W.seg_cnt = L.d_seg;
            W.chunk_sum = sums(1);
            W.super_sum = sums(1) + nchunk;
            W.bounce = 0;
            void* args[] = {&S, &F, &O, &W, &ax, &walk};
            if (traced) {   // rt_fetch_counts: the counting instantiation of the same kernel
                O.fcount = c->trace.d_counts;
                HIPC(c, hipLaunchKernel(kernel_traced(math, depth > 1, sc.walk_off != 0), grid, block, args, 0, s));
            } else if (tline) {   // rt_wave_timeline: the stamping instantiation
                if (!(O.wtime = tline_region(F.num_blocks * 4u)))
                    return set_err(c, "rt_wave_timeline: buffer too small", RT_ERR_INVALID_ARG);
                HIPC(c, hipLaunchKernel(kernel_timeline_first(depth > 1, sc.walk_off != 0), grid, block, args, 0, s));
            } else if (batch) {
                rtk::BatchCams C{};
                for (uint32_t i = 0; i < K; ++i) {
                    const rt_params& Q = batch[i];
                    C.cam[i] = rtk::BatchCam{make_float4(Q.a.x, Q.a.y, Q.a.z, 0.0f), make_float4(Q.b.x, Q.b.y, Q.b.z, 0.0f),
                                             make_float4(Q.c.x, Q.c.y, Q.c.z, 0.0f),
                                             make_float4(Q.campos.x, Q.campos.y, Q.campos.z, 0.0f),
                                             make_float4(Q.light_pos.x, Q.light_pos.y, Q.light_pos.z, 0.0f)};
                }
                C.stride = bstride;
                C.frame_px = (uint32_t)fpx;
                void* bargs[] = {&S, &F, &O, &W, &C, &walk};
                void* kb = kernel_batch(math, fast0, depth > 1);
                if (ext_ev) HIPC(c, hipExtLaunchKernel(kb, grid, block, bargs, 0, s, E.e[0], E.e[1], 0));
                else HIPC(c, hipLaunchKernel(kb, grid, block, bargs, 0, s));
            } else if (ext_ev) {
                HIPC(c, hipExtLaunchKernel(kernel_first(math, fast0, depth > 1), grid, block, args, 0, s, E.e[0], E.e[1], 0));
            } else {
                HIPC(c, hipLaunchKernel(kernel_first(math, fast0, depth > 1), grid, block, args, 0, s));
            }
            ++L.nframe;
        }
        if (depth > 1) {
            HIPC(c, hipEventRecord(E.e[2], s));
            E.has_k = true;
        }
        // the bounce launches take no part in the adaptive order or the counter clearing
        rtk::Frame Fb = F;
        Fb.tile_cost = nullptr;
        Fb.nzero = 0;
        for (int k = 1; k < depth; ++k) {  // bounce k over its queue
            rtk::WQ W{};
            W.in = qbuf(k);
            uint32_t* bc = cnt + kBounceWords * k;
            W.in_count = bc;
            // the queue's dense (compacted, optionally sorted) order and its size
            hipLaunchKernelGGL(rtk::wf_compact_sort_kernel, dim3((uint32_t)nchunk), dim3(256), 0, s,
                               (const rtk::QRay*)qbuf(k), (const uint32_t*)L.d_seg, (const uint32_t*)sums(k),
                               (const uint32_t*)(sums(k) + nchunk), k == 1 ? (uint32_t)nseg : 0u,
                               (const uint32_t*)(bc - kBounceWords), bc, L.d_perm, thin,
                               sort ? (K >= 4 ? (uint32_t)RTK_SORT_SCALE_BATCH : (uint32_t)RTK_SORT_SCALE) : 0u);
            W.perm = L.d_perm;
            W.out = k + 1 < depth ? qbuf(k + 1) : nullptr;
            W.seg_cnt = L.d_seg;
            W.chunk_sum = sums(k + 1);
            W.super_sum = sums(k + 1) + nchunk;
            W.fetch = bc + 32;
            W.bounce = k;
            void* args[] = {&S, &Fb, &O, &W, &ax};
            void* kb = traced ? kernel_traced_bounce(math) : kernel_bounce(math, fast);
            if (tline) {
                if (!(O.wtime = tline_region((uint32_t)c->wf_grid[math] * 4u)))
                    return set_err(c, "rt_wave_timeline: buffer too small", RT_ERR_INVALID_ARG);
                kb = kernel_timeline_bounce();
            }
            HIPC(c, hipLaunchKernel(kb, dim3(c->wf_grid[math]), dim3(256), args, 0, s));
        }
    }
    HIPC(c, hipGetLastError());
    if (!ext_ev) HIPC(c, hipEventRecord(E.e[1], s));
    HIPC(c, hipEventRecord(L.idle, s));
    if (F.tile_cost) L.cost_ready = true;
    c->timing_valid = true;
    ++c->frames;
    return RT_OK;
}

int rt_render_device(rt_ctx* c, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, const rt_tiling* tiling,
                     uint32_t* d_out, const rt_aux* d_aux, void* stream) {
    const uint64_t t0 = now_ns();
    const int rc = render_frames(c, w, h, depth, flags, tiling, d_out, d_aux, stream, nullptr, 1, 0);
    if (c) {
        c->enq_ns[0] = t0;
        c->enq_ns[1] = now_ns();
    }
    return rc;
}

int rt_last_enqueue_time(rt_ctx* c, uint64_t* begin_ns, uint64_t* end_ns) {
    if (!c || !begin_ns || !end_ns) return RT_ERR_INVALID_ARG;
    *begin_ns = c->enq_ns[0];
    *end_ns = c->enq_ns[1];
    return RT_OK;
}

int rt_render_device_batch(rt_ctx* c, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, const rt_tiling* tiling,
                           const rt_params* params, int32_t nframes, uint32_t* d_out, uint64_t frame_stride,
                           void* stream) {
    if (!params) return set_err(c, "rt_render_device_batch: no params", RT_ERR_INVALID_ARG);
    return render_frames(c, w, h, depth, flags, tiling, d_out, nullptr, stream, params, nframes, frame_stride);
}

// rt_render_batch: rt_render's synchronous boundary for nframes frames of one launch (the frames
// of a camera path the host already knows): into pinned, device-mapped memory directly, else
// through the ctx's device frame buffer and one read-back of all frames.
int rt_render_batch(rt_ctx* c, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, const rt_params* params,
                    int32_t nframes, uint32_t* out_bgr) {
    if (!c || !out_bgr || !params || w == 0 || h == 0 || nframes < 1 || nframes > rtk::kMaxBatch)
        return set_err(c, "rt_render_batch: invalid argument", RT_ERR_INVALID_ARG);
    const size_t npix = (size_t)w * h;
    HIPC(c, hipSetDevice(c->device));
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, out_bgr) == hipSuccess && pa.type == hipMemoryTypeHost && pa.devicePointer) {
        const int rc = render_frames(c, w, h, depth, flags, nullptr, (uint32_t*)pa.devicePointer, nullptr, c->stream,
                                     params, nframes, npix);
        if (rc) return rc;
        HIPC(c, wait_ctx(c, c->stream));
        return RT_OK;
    }
    (void)hipGetLastError();   // pageable memory: not an error, the read-back path below
    int rc = ensure(c, c->d_out, c->out_cap, npix * (size_t)nframes);
    if (rc) return rc;
    if ((rc = render_frames(c, w, h, depth, flags, nullptr, c->d_out, nullptr, c->stream, params, nframes, npix)))
        return rc;
    HIPC(c, hipMemcpyAsync(out_bgr, c->d_out, npix * (size_t)nframes * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, wait_ctx(c, c->stream));
    return RT_OK;
}

// rt_render: the reference's synchronous boundary (raytrace_gpgpu renders the whole frame, then
// reads it back: RayTracer.cpp:330-344), with the readback overlapped with the rendering.
//  * Pinned host memory the device can write (hipHostMalloc, or registered as mapped): the
//    frame is rendered straight into it; the kernel's pixel stores cross the host link while
//    the frame renders, with no readback after it (C3: 0.40 ms per frame against 0.55 for
//    render-then-copy, profiles/r04/ab/host_boundary_ab.log).
//  * Otherwise (pageable memory, or aux planes wanted), a frame of at least kGroupMinPixels is
//    cut into kRenderGroups groups of contiguous rows (rt_tiling with one band per "rank", so a
//    group's rows are one contiguous run of the frame and of its aux planes), each rendered
//    straight into its part of the device frame on its own stream (its own frame slot and
//    longest-first order), concurrently; a group's rows are copied to the host as soon as it is
//    done (C3 pageable: 0.49 vs 0.55 ms; 3, 6 or 8 groups, stream priorities, or the groups
//    rendered one after another on one or several streams measured slower, same log).
// The pixels are those of one whole-frame launch (a pixel's arithmetic does not depend on how
// the frame is cut: DESIGN.md 5; tests/test_render_gpu.py test_render_readback_paths_agree).
constexpr uint32_t kRenderGroups = 4;
constexpr uint64_t kGroupMinPixels = 512 * 512;

int rt_render(rt_ctx* c, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, uint32_t* out_bgr,
              const rt_aux* aux) {
    if (!c || !out_bgr) return set_err(c, "rt_render: invalid argument", RT_ERR_INVALID_ARG);
    if (w == 0 || h == 0 || depth < 0 || depth > RT_MAX_DEPTH) return set_err(c, "rt_render: invalid argument", RT_ERR_INVALID_ARG);
    const size_t npix = (size_t)w * h;
    HIPC(c, hipSetDevice(c->device));
    int rc = ensure(c, c->d_out, c->out_cap, npix);
    if (rc) return rc;
    rt_aux dev{nullptr, nullptr, nullptr};
    const bool want = aux && (aux->hits || aux->t || aux->rgb);
    const size_t dd = (size_t)std::max(depth, 1);
    if (want) {
        if ((rc = ensure(c, c->d_hits, c->hits_cap, npix * dd * 2))) return rc;
        if ((rc = ensure(c, c->d_t, c->t_cap, npix * dd))) return rc;
        if ((rc = ensure(c, c->d_rgb, c->rgb_cap, npix * 3))) return rc;
        dev = rt_aux{c->d_hits, c->d_t, c->d_rgb};
    }
    if (!want) {
        // the caller's buffer is pinned host memory the device can write (hipHostMalloc, or
        // registered as mapped): the kernel's pixel stores go straight to it over the host link
        // while the frame renders, with no readback after it
        hipPointerAttribute_t pa;
        if (hipPointerGetAttributes(&pa, out_bgr) == hipSuccess && pa.type == hipMemoryTypeHost && pa.devicePointer) {
            rc = rt_render_device(c, w, h, depth, flags, nullptr, (uint32_t*)pa.devicePointer, nullptr, c->stream);
            if (rc) return rc;
            HIPC(c, wait_ctx(c, c->stream));
            return RT_OK;
        }
        (void)hipGetLastError();   // pageable memory: not an error, the readback path below
    }
    // the group's rows: band_rows a multiple of the 16-row block, at most one band per group
    uint32_t groups = npix >= kGroupMinPixels ? kRenderGroups : 1;
    const uint32_t band_rows = ((h + groups - 1) / groups + 15u) & ~15u;
    groups = (h + band_rows - 1) / band_rows;
    if (groups <= 1) {
        rc = rt_render_device(c, w, h, depth, flags, nullptr, c->d_out, want ? &dev : nullptr, c->stream);
        if (rc) return rc;
        HIPC(c, hipMemcpyAsync(out_bgr, c->d_out, npix * 4, hipMemcpyDeviceToHost, c->stream));
        if (want) {
            if (aux->hits) HIPC(c, hipMemcpyAsync(aux->hits, c->d_hits, npix * depth * 2 * 4, hipMemcpyDeviceToHost, c->stream));
            if (aux->t) HIPC(c, hipMemcpyAsync(aux->t, c->d_t, npix * depth * 4, hipMemcpyDeviceToHost, c->stream));
            if (aux->rgb) HIPC(c, hipMemcpyAsync(aux->rgb, c->d_rgb, npix * 3 * 4, hipMemcpyDeviceToHost, c->stream));
        }
        HIPC(c, wait_ctx(c, c->stream));
        return RT_OK;
    }
    for (uint32_t g = 0; g < groups; ++g)   // group g's kernels and readback on gstream[g]
        if (!c->gstream[g]) HIPC(c, hipStreamCreateWithFlags(&c->gstream[g], hipStreamNonBlocking));
    // after whatever the ctx's own stream still holds (the synchronous entry points leave it idle)
    if (!c->gstart) HIPC(c, hipEventCreateWithFlags(&c->gstart, hipEventDisableTiming));
    // The frame's timing entry (rt_last_timing / rt_timing_average): the span from here, on the
    // ctx stream, to the end of the last group's kernels, joined back to the ctx stream.  The
    // groups' own entries go into the ring after it and are dropped again below, so one
    // grouped frame is one timing entry, like any other frame.
    const uint64_t f0 = c->frames;
    rt_ctx::FrameEv& FE = c->ring[f0 % rt_ctx::kRing];
    for (hipEvent_t& e : FE.e)
        if (!e) HIPC(c, hipEventCreate(&e));
    FE.has_k = false;
    HIPC(c, hipEventRecord(FE.e[0], c->stream));
    HIPC(c, hipEventRecord(c->gstart, c->stream));
    c->frames = f0 + 1;
    std::vector<rt_ctx::FrameSlot*> slots;
    // every group's kernels first, then the readbacks in group order: a copy into pageable
    // memory may block the host until it is done, and the later groups must already be queued
    for (uint32_t g = 0; g < groups; ++g) {
        hipStream_t s = c->gstream[g];
        HIPC(c, hipStreamWaitEvent(s, c->gstart, 0));
        const rt_tiling t{(int32_t)g, (int32_t)groups, (int32_t)band_rows, 0};
        const size_t p0 = (size_t)g * band_rows * w;
        rt_aux ga{nullptr, nullptr, nullptr};
        if (want) ga = rt_aux{c->d_hits + p0 * depth * 2, c->d_t + p0 * depth, c->d_rgb + p0 * 3};
        rc = rt_render_device(c, w, h, depth, flags, &t, c->d_out + p0, want ? &ga : nullptr, s);
        if (rc) return rc;
        slots.push_back(c->last_slot);
    }
    for (uint32_t g = 0; g < groups; ++g)   // the frame ends with the last group's kernels
        HIPC(c, hipStreamWaitEvent(c->stream, c->ring[(f0 + 1 + g) % rt_ctx::kRing].e[1], 0));
    HIPC(c, hipEventRecord(FE.e[1], c->stream));
    c->frames = f0 + 1;
    for (uint32_t g = 0; g < groups; ++g) {
        hipStream_t s = c->gstream[g];
        const size_t p0 = (size_t)g * band_rows * w, np = (size_t)std::min<uint64_t>(band_rows, h - (uint64_t)g * band_rows) * w;
        HIPC(c, hipMemcpyAsync(out_bgr + p0, c->d_out + p0, np * 4, hipMemcpyDeviceToHost, s));
        if (want) {
            if (aux->hits) HIPC(c, hipMemcpyAsync(aux->hits + p0 * depth * 2, c->d_hits + p0 * depth * 2, np * depth * 2 * 4, hipMemcpyDeviceToHost, s));
            if (aux->t) HIPC(c, hipMemcpyAsync(aux->t + p0 * depth, c->d_t + p0 * depth, np * depth * 4, hipMemcpyDeviceToHost, s));
            if (aux->rgb) HIPC(c, hipMemcpyAsync(aux->rgb + p0 * 3, c->d_rgb + p0 * 3, np * 3 * 4, hipMemcpyDeviceToHost, s));
        }
    }
    for (uint32_t g = 0; g < groups; ++g) HIPC(c, wait_ctx(c, c->gstream[g]));
    c->last_group = slots;
    return RT_OK;
}

static int frame_times(rt_ctx* c, uint64_t f, float& total, float& kernel) {
    rt_ctx::FrameEv& E = c->ring[f % rt_ctx::kRing];
    HIPC(c, hipEventSynchronize(E.e[1]));
    HIPC(c, hipEventElapsedTime(&total, E.e[0], E.e[1]));
    kernel = total;
    if (E.has_k) HIPC(c, hipEventElapsedTime(&kernel, E.e[0], E.e[2]));
    return RT_OK;
}

int rt_last_timing(rt_ctx* c, float* total_ms, float* traverse_ms) {
    if (!c || !total_ms) return RT_ERR_INVALID_ARG;
    if (!c->timing_valid || c->frames == 0) return set_err(c, "rt_last_timing: nothing rendered", RT_ERR_NO_SCENE);
    float t = 0, k = 0;
    int rc;
    if ((rc = frame_times(c, c->frames - 1, t, k))) return rc;
    *total_ms = t;
    if (traverse_ms) *traverse_ms = k;
    return RT_OK;
}

int rt_timing_average(rt_ctx* c, int32_t n, float* total_ms, float* traverse_ms) {
    if (!c || !total_ms || n < 1) return RT_ERR_INVALID_ARG;
    if (c->frames == 0) return set_err(c, "rt_timing_average: nothing rendered", RT_ERR_NO_SCENE);
    const uint64_t m = std::min<uint64_t>({(uint64_t)n, c->frames, (uint64_t)rt_ctx::kRing});
    double st = 0, sk = 0;
    for (uint64_t i = 0; i < m; ++i) {
        float t = 0, k = 0;
        int rc;
        if ((rc = frame_times(c, c->frames - 1 - i, t, k))) return rc;
        st += t;
        sk += k;
    }
    *total_ms = (float)(st / (double)m);
    if (traverse_ms) *traverse_ms = (float)(sk / (double)m);
    return RT_OK;
}

}  // extern "C": the families' shared path has templates

// ---- the query families: ray queries, fans, closest points, k nearest ----
// Every family launches through query_launch and is a query to everything that waits for or
// reports on one.  A query takes a frame slot of its own kind per stream (kQueryKey: no tiling has
// that key), so install_scene and update_vertices wait for it through the slot's idle event as they
// do for frames, and queries on different streams may run concurrently.  The slot holds the spill
// stack (one column per lane of the persistent grid, sized once: the grid is the context's), the
// launch's work cursors and restart count (zeroed on the stream before every launch) and the two
// events around the kernel.  A family brings its checks (over check_count and check_flags_scene),
// its kernel arguments and its launch; the host forms stage through stage_in, stage_dst and stage_out.
constexpr uint64_t kQueryKey = 1ull << 62;
constexpr int64_t kMaxQueryRays = 1ll << 30;
constexpr uint32_t kQueryFlags = RT_FLAG_HW_MATH | RT_FLAG_STRICT_MATH | RT_FLAG_EXACT_DIV | RT_FLAG_ANY_HIT;

// The refusals that need no GPU, `who` naming the entry point in the message, are every family's in
// this order: check_count, the family's own (NULL pointers; before them a fan's k), check_flags_scene.
static int check_count(rt_ctx* c, const char* who, int64_t n, int64_t n_max, const char* range) {
    if (!c) return set_err(nullptr, std::string(who) + ": ctx is NULL", RT_ERR_INVALID_ARG);
    if (n < 0 || n > n_max) return set_err(c, std::string(who) + ": n must be " + range, RT_ERR_INVALID_ARG);
    return RT_OK;
}
static int check_flags_scene(rt_ctx* c, const char* who, uint32_t flags, uint32_t mask, const char* not_ours) {
    if (flags & ~mask) return set_err(c, std::string(who) + not_ours, RT_ERR_INVALID_ARG);
    if ((flags & RT_FLAG_STRICT_MATH) && (flags & RT_FLAG_HW_MATH))
        return set_err(c, std::string(who) + ": RT_FLAG_STRICT_MATH and RT_FLAG_HW_MATH exclude each other", RT_ERR_INVALID_ARG);
    if (!c->have_scene) return set_err(c, std::string(who) + ": no scene uploaded", RT_ERR_NO_SCENE);
    return RT_OK;
}

// RTAMD_FAN_GRID_BLOCKS, RTAMD_CLOSEST_GRID_BLOCKS, RTAMD_MULTIHIT_GRID_BLOCKS = <b> (tests): at most b blocks in the family's grids,
// so that a wave takes many items.  Read once per context (memo -1: not read yet); 0: no cap.
static int grid_cap(const char* var, int& memo) {
    if (memo < 0) {
        const char* v = std::getenv(var);
        const long b = v ? std::strtol(v, nullptr, 10) : 0;
        memo = b > 0 && b < (1l << 20) ? (int)b : 0;
    }
    return memo;
}

// One query on `s`, checked arguments.  `grid_memo` is the context's cell for the persistent grid of
// `kernel` (the family's kernel whose occupancy sizes it): computed once, under `cap` blocks if that
// is not 0.  `items` is what the launch's waves take one at a time, four waves to a block.
// launch(slot, grid) enqueues the kernel between the slot's events, on zeroed cursors.
template <class Launch>
static int query_launch(rt_ctx* c, hipStream_t s, int& grid_memo, const void* kernel, int cap, uint32_t items, Launch launch) {
    int rc = RT_OK;
    rt_ctx::FrameSlot* Lp = nullptr;
    if ((rc = slot_for(c, (void*)s, kQueryKey, &Lp))) return rc;
    rt_ctx::FrameSlot& L = *Lp;
    if (!grid_memo) {
        int cus = 0, b1 = 0;
        HIPC(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        HIPC(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&b1, kernel, rtk::kBlockThreads, 0));
        grid_memo = std::max(8, std::max(b1, 1) * cus * RTK_QUERY_GRID_PCT / 100);
        if (cap) grid_memo = std::min(grid_memo, cap);
    }
    // the stack columns are sized for the kernel's whole grid, whatever the launch takes: a later, larger
    // query allocates nothing (ensure keeps a larger allocation, so the families share the slot's columns)
    const size_t full = (size_t)grid_memo;
    const uint32_t grid = (uint32_t)std::min<size_t>(full, (items + 3u) / 4u);
    if ((rc = ensure(c, L.d_gstack, L.gstack_cap, full * rtk::kBlockThreads * rtk::kGlobalStack))) return rc;
    if (!L.d_qcnt) {
        size_t qcnt_cap = 0;
        if ((rc = ensure(c, L.d_qcnt, qcnt_cap, rtk::kCursorSet + 32))) return rc;
    }
    for (hipEvent_t& e : L.qev)
        if (!e) HIPC(c, hipEventCreate(&e));
    HIPC(c, hipMemsetAsync(L.d_qcnt, 0, (rtk::kCursorSet + 32) * sizeof(uint32_t), s));
    (void)hipGetLastError();
    HIPC(c, launch(L, grid));
    HIPC(c, hipGetLastError());
    HIPC(c, hipEventRecord(L.idle, s));
    c->query_slot = &L;
    c->query_last = true;
    return RT_OK;
}

// what the render kernels' body writes besides a query's records: the spill stack, its stride, the counters
static rtk::Outputs query_outputs(rt_ctx* c, const rt_ctx::FrameSlot& L, uint32_t grid) {
    rtk::Outputs O{};
    O.gstack = L.d_gstack;
    O.overflow = c->d_overflow;
    O.restarts = L.d_qcnt + rtk::kCursorSet;
    O.local_pixels = (uint64_t)grid * rtk::kBlockThreads;   // the stack's stride: the lanes launched
    return O;
}

// Pinned host memory that the device can reach (hipHostMalloc, or registered as mapped) at an
// address aligned to `align`: that address, which a host form then uses directly, as rt_render does.
static void* mapped_host(const void* p, size_t align) {
    hipPointerAttribute_t pa;
    if (hipPointerGetAttributes(&pa, p) == hipSuccess && pa.type == hipMemoryTypeHost && pa.devicePointer &&
        !((uintptr_t)pa.devicePointer & (align - 1)))
        return pa.devicePointer;
    (void)hipGetLastError();   // pageable memory: not an error
    return nullptr;
}

// A host form's input of `bytes` bytes -> *dev: the caller's memory where mapped_host gives it, else a
// copy made on c->stream in the staging buffer `buf` (grow-only, `cap` in bytes)
template <class T>
static int stage_in(rt_ctx* c, const T* host, size_t bytes, size_t align, char*& buf, size_t& cap, const T** dev) {
    if ((*dev = (const T*)mapped_host(host, align))) return RT_OK;
    if (const int rc = ensure(c, buf, cap, bytes)) return rc;
    HIPC(c, hipMemcpyAsync(buf, host, bytes, hipMemcpyHostToDevice, c->stream));
    *dev = (const T*)buf;
    return RT_OK;
}
// A host form's output of `bytes` bytes -> *dev: the caller's memory where mapped_host gives it, else
// d_qhits, which stage_out copies back on c->stream after the query (and nothing where nothing was staged)
template <class T>
static int stage_dst(rt_ctx* c, T* host, size_t bytes, size_t align, T** dev) {
    if ((*dev = (T*)mapped_host(host, align))) return RT_OK;
    if (const int rc = ensure(c, c->d_qhits, c->qhits_cap, bytes)) return rc;
    *dev = (T*)c->d_qhits;
    return RT_OK;
}
static int stage_out(rt_ctx* c, void* host, const void* dev, size_t bytes) {
    if (dev == c->d_qhits) HIPC(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    return RT_OK;
}

extern "C" {

// ---- ray queries ----
static int query_check(rt_ctx* c, const char* who, const void* rays, int64_t n, uint32_t flags, const void* hits) {
    if (const int rc = check_count(c, who, n, kMaxQueryRays, "0..2^30")) return rc;
    if (n > 0 && (!rays || !hits)) return set_err(c, std::string(who) + ": rays or hits is NULL", RT_ERR_INVALID_ARG);
    return check_flags_scene(c, who, flags, kQueryFlags, ": a flag that is not a ray query's");
}

// A query's record kind: rt_hit (query_kernel) or rt_hit_attr (query_attr_kernel).  Both
// kinds share the slot, its events and its idle record, so everything that waits for a query waits for either.
enum QueryKind { kQueryHit = 0, kQueryAttr = 1 };
static void* kernel_query_of(QueryKind kind, int m, bool any, bool fast) {
    return kind == kQueryAttr ? kernel_query_attr(m, any, fast) : kernel_query(m, any, fast);
}

// checked arguments, n > 0; d_hits: rt_hit[n] or rt_hit_attr[n], by kind
static int query_enqueue(rt_ctx* c, QueryKind kind, const rt_ray* d_rays, int64_t n, uint32_t flags, void* d_hits, hipStream_t s) {
    const int math = (flags & RT_FLAG_STRICT_MATH) ? 0 : (flags & RT_FLAG_HW_MATH) ? 1 : 2;
    const bool any = (flags & RT_FLAG_ANY_HIT) != 0;
    rtk::DevScene S = dev_scene(c->scene, flags);
    void* kernel = kernel_query_of(kind, math, any, scene_fast(c->scene));
    const uint32_t ngroups = (uint32_t)((n + rtk::kSegRays - 1) / rtk::kSegRays);
    return query_launch(c, s, c->query_grid[kind][math], kernel_query_of(kind, math, false, true), 0, ngroups,
                        [&](rt_ctx::FrameSlot& L, uint32_t grid) {
                            rtk::Outputs O = query_outputs(c, L, grid);
                            rtk::Query Q{(const float4*)d_rays, (uint2*)d_hits, (uint32_t)n, L.d_qcnt};
                            void* args[] = {&S, &O, &Q};
                            return hipExtLaunchKernel(kernel, dim3(grid), dim3(rtk::kBlockThreads), args, 0, s, L.qev[0], L.qev[1], 0);
                        });
}

// the two entry points of either record kind; `who` names the caller's
static int trace_rays_device(rt_ctx* c, QueryKind kind, const char* who, const rt_ray* d_rays, int64_t n, uint32_t flags,
                             void* d_hits, void* stream) {
    if (const int rc = query_check(c, who, d_rays, n, flags, d_hits)) return rc;
    if (n == 0) return RT_OK;
    const uintptr_t hmask = kind == kQueryAttr ? 15u : 7u;
    if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_hits & hmask))
        return set_err(c, std::string(who) + (kind == kQueryAttr ? ": d_rays and d_hits must be 16-byte aligned"
                                                                 : ": d_rays must be 16-byte aligned and d_hits 8-byte aligned"),
                       RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    return query_enqueue(c, kind, d_rays, n, flags, d_hits, stream ? (hipStream_t)stream : c->stream);
}

static int trace_rays_host(rt_ctx* c, QueryKind kind, const char* who, const rt_ray* rays, int64_t n, uint32_t flags, void* hits) {
    if (const int rc = query_check(c, who, rays, n, flags, hits)) return rc;
    if (n == 0) return RT_OK;
    HIPC(c, hipSetDevice(c->device));
    const size_t hit_bytes = (size_t)n * (kind == kQueryAttr ? sizeof(rt_hit_attr) : sizeof(rt_hit));
    const rt_ray* d_rays = nullptr;
    void* d_hits = nullptr;
    int rc = RT_OK;
    if ((rc = stage_in(c, rays, (size_t)n * sizeof(rt_ray), 16, c->d_qrays, c->qrays_cap, &d_rays))) return rc;
    if ((rc = stage_dst(c, hits, hit_bytes, kind == kQueryAttr ? 16 : 8, &d_hits))) return rc;
    if ((rc = query_enqueue(c, kind, d_rays, n, flags, d_hits, c->stream))) return rc;
    if ((rc = stage_out(c, hits, d_hits, hit_bytes))) return rc;
    HIPC(c, wait_ctx(c, c->stream));
    return RT_OK;
}

int rt_trace_rays_device(rt_ctx* c, const rt_ray* d_rays, int64_t n, uint32_t flags, rt_hit* d_hits, void* stream) {
    return trace_rays_device(c, kQueryHit, "rt_trace_rays_device", d_rays, n, flags, d_hits, stream);
}

int rt_trace_rays(rt_ctx* c, const rt_ray* rays, int64_t n, uint32_t flags, rt_hit* hits) {
    return trace_rays_host(c, kQueryHit, "rt_trace_rays", rays, n, flags, hits);
}

int rt_trace_rays_attr_device(rt_ctx* c, const rt_ray* d_rays, int64_t n, uint32_t flags, rt_hit_attr* d_hits, void* stream) {
    return trace_rays_device(c, kQueryAttr, "rt_trace_rays_attr_device", d_rays, n, flags, d_hits, stream);
}

int rt_trace_rays_attr(rt_ctx* c, const rt_ray* rays, int64_t n, uint32_t flags, rt_hit_attr* hits) {
    return trace_rays_host(c, kQueryAttr, "rt_trace_rays_attr", rays, n, flags, hits);
}

// ---- first k hits ----
// rt_trace_rays with k records per ray, in k planes of n: the same slot, staging and events; the kernel is
// multihit_kernel<k> of the arithmetic the flags name, and its grid is that kernel's own.
constexpr uint32_t kMultihitFlags = RT_FLAG_HW_MATH | RT_FLAG_STRICT_MATH | RT_FLAG_EXACT_DIV;

static int multihit_check(rt_ctx* c, const char* who, const void* rays, int64_t n, int32_t k, uint32_t flags, const void* out) {
    if (const int rc = check_count(c, who, n, kMaxQueryRays, "0..2^30")) return rc;
    if (n > 0 && (!rays || !out)) return set_err(c, std::string(who) + ": rays or out is NULL", RT_ERR_INVALID_ARG);
    if (const int rc = check_flags_scene(c, who, flags, kMultihitFlags, ": a flag that is not a first-k-hits query's")) return rc;
    if (k < 1 || k > RT_TRACE_MAX_K) return set_err(c, std::string(who) + ": k must be 1..8", RT_ERR_INVALID_ARG);
    if (n * k > kMaxQueryRays) return set_err(c, std::string(who) + ": n * k must be at most 2^30", RT_ERR_INVALID_ARG);
    return RT_OK;
}

// checked arguments, n > 0
static int multihit_enqueue(rt_ctx* c, const rt_ray* d_rays, int64_t n, int32_t k, uint32_t flags, rt_hit_uv* d_out, hipStream_t s) {
    const int math = (flags & RT_FLAG_STRICT_MATH) ? 0 : (flags & RT_FLAG_HW_MATH) ? 1 : 2;
    rtk::DevScene S = dev_scene(c->scene, flags);
    void* kernel = kernel_multihit(math, k);
    const uint32_t ngroups = (uint32_t)((n + rtk::kSegRays - 1) / rtk::kSegRays);
    return query_launch(c, s, c->multihit_grid[math][k - 1], kernel, grid_cap("RTAMD_MULTIHIT_GRID_BLOCKS", c->multihit_grid_cap),
                        ngroups, [&](rt_ctx::FrameSlot& L, uint32_t grid) {
                            rtk::Outputs O = query_outputs(c, L, grid);
                            rtk::Query Q{(const float4*)d_rays, (uint2*)d_out, (uint32_t)n, L.d_qcnt};
                            void* args[] = {&S, &O, &Q};
                            return hipExtLaunchKernel(kernel, dim3(grid), dim3(rtk::kBlockThreads), args, 0, s, L.qev[0], L.qev[1], 0);
                        });
}

int rt_trace_rays_k_device(rt_ctx* c, const rt_ray* d_rays, int64_t n, int32_t k, uint32_t flags, rt_hit_uv* d_out, void* stream) {
    if (const int rc = multihit_check(c, "rt_trace_rays_k_device", d_rays, n, k, flags, d_out)) return rc;
    if (n == 0) return RT_OK;
    if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_out & 15u))
        return set_err(c, "rt_trace_rays_k_device: d_rays and d_out must be 16-byte aligned", RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    return multihit_enqueue(c, d_rays, n, k, flags, d_out, stream ? (hipStream_t)stream : c->stream);
}

int rt_trace_rays_k(rt_ctx* c, const rt_ray* rays, int64_t n, int32_t k, uint32_t flags, rt_hit_uv* out) {
    if (const int rc = multihit_check(c, "rt_trace_rays_k", rays, n, k, flags, out)) return rc;
    if (n == 0) return RT_OK;
    HIPC(c, hipSetDevice(c->device));
    const size_t out_bytes = (size_t)n * (size_t)k * sizeof(rt_hit_uv);
    const rt_ray* d_rays = nullptr;
    rt_hit_uv* d_out = nullptr;
    int rc = RT_OK;
    if ((rc = stage_in(c, rays, (size_t)n * sizeof(rt_ray), 16, c->d_qrays, c->qrays_cap, &d_rays))) return rc;
    if ((rc = stage_dst(c, out, out_bytes, 16, &d_out))) return rc;
    if ((rc = multihit_enqueue(c, d_rays, n, k, flags, d_out, c->stream))) return rc;
    if ((rc = stage_out(c, out, d_out, out_bytes))) return rc;
    HIPC(c, wait_ctx(c, c->stream));
    return RT_OK;
}

// ---- occlusion fans ----
constexpr int64_t kMaxFanOrigins = 1ll << 26;
constexpr uint32_t kFanFlags = RT_FLAG_HW_MATH | RT_FLAG_STRICT_MATH | RT_FLAG_EXACT_DIV;

static int fan_check(rt_ctx* c, const char* who, const void* origins, int64_t n, const void* dirs, int32_t k, uint32_t flags,
                     const void* masks) {
    if (const int rc = check_count(c, who, n, kMaxFanOrigins, "0..2^26")) return rc;
    if (n > 0 && (k < 1 || k > RT_FAN_MAX_DIRS))
        return set_err(c, std::string(who) + ": k must be 1..RT_FAN_MAX_DIRS", RT_ERR_INVALID_ARG);
    if (n > 0 && (!origins || !dirs || !masks)) return set_err(c, std::string(who) + ": origins, dirs or masks is NULL", RT_ERR_INVALID_ARG);
    return check_flags_scene(c, who, flags, kFanFlags, ": a flag that is not a fan's");
}

// checked arguments, n > 0
static int fan_enqueue(rt_ctx* c, const rt_fan_origin* d_origins, int64_t n, const rt_float4* d_dirs, int32_t k, uint32_t flags,
                       uint32_t* d_masks, hipStream_t s) {
    const int math = (flags & RT_FLAG_STRICT_MATH) ? 0 : (flags & RT_FLAG_HW_MATH) ? 1 : 2;
    rtk::DevScene S = dev_scene(c->scene, flags);
    void* kernel = kernel_fan(math, scene_fast(c->scene));
    const uint32_t chunks = ((uint32_t)k + 31u) / 32u;
    const uint32_t items = (uint32_t)((n + rtk::kSegRays - 1) / rtk::kSegRays) * chunks;   // <= 2^27
    return query_launch(c, s, c->fan_grid[math], kernel_fan(math, true), grid_cap("RTAMD_FAN_GRID_BLOCKS", c->fan_grid_cap), items,
                        [&](rt_ctx::FrameSlot& L, uint32_t grid) {
                            rtk::Outputs O = query_outputs(c, L, grid);
                            rtk::Fan Fn{(const float4*)d_origins, (const float4*)d_dirs, d_masks, (uint32_t)n, (uint32_t)k, chunks, L.d_qcnt};
                            void* args[] = {&S, &O, &Fn};
                            return hipExtLaunchKernel(kernel, dim3(grid), dim3(rtk::kBlockThreads), args, 0, s, L.qev[0], L.qev[1], 0);
                        });
}

int rt_trace_fan_device(rt_ctx* c, const rt_fan_origin* d_origins, int64_t n, const rt_float4* d_dirs, int32_t k, uint32_t flags,
                        uint32_t* d_masks, void* stream) {
    if (const int rc = fan_check(c, "rt_trace_fan_device", d_origins, n, d_dirs, k, flags, d_masks)) return rc;
    if (n == 0) return RT_OK;
    if (((uintptr_t)d_origins & 15u) || ((uintptr_t)d_dirs & 15u) || ((uintptr_t)d_masks & 3u))
        return set_err(c, "rt_trace_fan_device: d_origins and d_dirs must be 16-byte aligned and d_masks 4-byte aligned",
                       RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    return fan_enqueue(c, d_origins, n, d_dirs, k, flags, d_masks, stream ? (hipStream_t)stream : c->stream);
}

int rt_trace_fan(rt_ctx* c, const rt_fan_origin* origins, int64_t n, const rt_float4* dirs, int32_t k, uint32_t flags,
                 uint32_t* masks) {
    if (const int rc = fan_check(c, "rt_trace_fan", origins, n, dirs, k, flags, masks)) return rc;
    if (n == 0) return RT_OK;
    HIPC(c, hipSetDevice(c->device));
    const size_t mask_bytes = (size_t)(((uint32_t)k + 31u) / 32u) * (size_t)n * sizeof(uint32_t);
    const rt_fan_origin* d_origins = nullptr;
    const rt_float4* d_dirs = nullptr;
    uint32_t* d_masks = nullptr;
    int rc = RT_OK;
    if ((rc = stage_in(c, origins, (size_t)n * sizeof(rt_fan_origin), 16, c->d_qrays, c->qrays_cap, &d_origins))) return rc;
    if ((rc = stage_in(c, dirs, (size_t)k * sizeof(rt_float4), 16, c->d_fdirs, c->fdirs_cap, &d_dirs))) return rc;
    if ((rc = stage_dst(c, masks, mask_bytes, 4, &d_masks))) return rc;
    if ((rc = fan_enqueue(c, d_origins, n, d_dirs, k, flags, d_masks, c->stream))) return rc;
    if ((rc = stage_out(c, masks, d_masks, mask_bytes))) return rc;
    HIPC(c, wait_ctx(c, c->stream));
    return RT_OK;
}

// ---- closest-point queries ----
// The point kernels (rt_closest.hip) restart nothing: the slot's restart count stays 0.
static_assert(rtclosest::kThreads == rtk::kBlockThreads && rtclosest::kGlobalStack == rtk::kGlobalStack &&
                  rtclosest::kCursors == rtk::kCursors && rtclosest::kCursorStride == rtk::kCursorStride,
              "rt_closest.hip shares the query slot's spill columns and cursors");

static int closest_check(rt_ctx* c, const char* who, const void* pts, int64_t n, uint32_t flags, const void* out) {
    if (const int rc = check_count(c, who, n, kMaxQueryRays, "0..2^30")) return rc;
    if (n > 0 && (!pts || !out)) return set_err(c, std::string(who) + ": pts or out is NULL", RT_ERR_INVALID_ARG);
    return check_flags_scene(c, who, flags, 0, ": flags must be 0");
}

// checked arguments, n > 0.  k == 0: rt_closest_points' kernel and one record per point; k in 1 ..
// RT_NEAREST_MAX_K: rt_nearest_k's kernel of that k and k planes of n records.
static int points_enqueue(rt_ctx* c, const rt_point* d_pts, int64_t n, int k, rt_closest* d_out, hipStream_t s) {
    const Scene& sc = c->scene;
    const rtclosest::Scene S{sc.wnodes(), sc.tris(), sc.leaf(), sc.root};
    const uint32_t ngroups = (uint32_t)((n + rtk::kSegRays - 1) / rtk::kSegRays);
    return query_launch(c, s, k ? c->nearest_grid[k - 1] : c->closest_grid, rtclosest::kernel(k),
                        grid_cap("RTAMD_CLOSEST_GRID_BLOCKS", c->closest_grid_cap), ngroups,
                        [&](rt_ctx::FrameSlot& L, uint32_t grid) {
                            const rtclosest::Launch Q{(const float4*)d_pts, (float4*)d_out, (uint32_t)n, L.d_qcnt, L.d_gstack, c->d_overflow};
                            return rtclosest::launch(S, Q, k, grid, s, L.qev[0], L.qev[1]);
                        });
}

// the two entry points of rt_closest_points (k == 0) and rt_nearest_k, after their checks
static int points_device(rt_ctx* c, const char* who, const rt_point* d_pts, int64_t n, int k, rt_closest* d_out, void* stream) {
    if (n == 0) return RT_OK;
    if (((uintptr_t)d_pts & 15u) || ((uintptr_t)d_out & 15u))
        return set_err(c, std::string(who) + ": d_pts and d_out must be 16-byte aligned", RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    return points_enqueue(c, d_pts, n, k, d_out, stream ? (hipStream_t)stream : c->stream);
}

static int points_host(rt_ctx* c, const rt_point* pts, int64_t n, int k, rt_closest* out) {
    if (n == 0) return RT_OK;
    HIPC(c, hipSetDevice(c->device));
    const size_t out_bytes = (size_t)n * (size_t)(k ? k : 1) * sizeof(rt_closest);
    const rt_point* d_pts = nullptr;
    rt_closest* d_out = nullptr;
    int rc = RT_OK;
    if ((rc = stage_in(c, pts, (size_t)n * sizeof(rt_point), 16, c->d_qrays, c->qrays_cap, &d_pts))) return rc;
    if ((rc = stage_dst(c, out, out_bytes, 16, &d_out))) return rc;
    if ((rc = points_enqueue(c, d_pts, n, k, d_out, c->stream))) return rc;
    if ((rc = stage_out(c, out, d_out, out_bytes))) return rc;
    HIPC(c, wait_ctx(c, c->stream));
    return RT_OK;
}

int rt_closest_points_device(rt_ctx* c, const rt_point* d_pts, int64_t n, uint32_t flags, rt_closest* d_out, void* stream) {
    if (const int rc = closest_check(c, "rt_closest_points_device", d_pts, n, flags, d_out)) return rc;
    return points_device(c, "rt_closest_points_device", d_pts, n, 0, d_out, stream);
}

int rt_closest_points(rt_ctx* c, const rt_point* pts, int64_t n, uint32_t flags, rt_closest* out) {
    if (const int rc = closest_check(c, "rt_closest_points", pts, n, flags, out)) return rc;
    return points_host(c, pts, n, 0, out);
}

// ---- k nearest triangles ----
// rt_closest_points with k records per point, in k planes of n; the kernel is rt_closest.hip's nearest_kernel<k>.
static int nearest_check(rt_ctx* c, const char* who, const void* pts, int64_t n, int32_t k, uint32_t flags, const void* out) {
    if (const int rc = closest_check(c, who, pts, n, flags, out)) return rc;
    if (k < 1 || k > RT_NEAREST_MAX_K) return set_err(c, std::string(who) + ": k must be 1..8", RT_ERR_INVALID_ARG);
    if (n * k > kMaxQueryRays) return set_err(c, std::string(who) + ": n * k must be at most 2^30", RT_ERR_INVALID_ARG);
    return RT_OK;
}

int rt_nearest_k_device(rt_ctx* c, const rt_point* d_pts, int64_t n, int32_t k, uint32_t flags, rt_closest* d_out, void* stream) {
    if (const int rc = nearest_check(c, "rt_nearest_k_device", d_pts, n, k, flags, d_out)) return rc;
    return points_device(c, "rt_nearest_k_device", d_pts, n, k, d_out, stream);
}

int rt_nearest_k(rt_ctx* c, const rt_point* pts, int64_t n, int32_t k, uint32_t flags, rt_closest* out) {
    if (const int rc = nearest_check(c, "rt_nearest_k", pts, n, k, flags, out)) return rc;
    return points_host(c, pts, n, k, out);
}

int rt_last_query_timing(rt_ctx* c, float* ms) {
    if (!c || !ms) return set_err(c, "rt_last_query_timing: invalid argument", RT_ERR_INVALID_ARG);
    if (!c->query_slot || !c->query_slot->qev[1]) return set_err(c, "rt_last_query_timing: no ray query yet", RT_ERR_NO_SCENE);
    HIPC(c, hipEventSynchronize(c->query_slot->qev[1]));
    HIPC(c, hipEventElapsedTime(ms, c->query_slot->qev[0], c->query_slot->qev[1]));
    return RT_OK;
}

int rt_last_deferred(rt_ctx* c, uint32_t* count) {
    if (!c || !count) return RT_ERR_INVALID_ARG;
    *count = 0;
    // the last frame: one slot, or every row group of the last grouped rt_render
    if (c->query_last && c->query_slot) {   // a ray query came after the last frame: its restarts
        rt_ctx::FrameSlot* L = c->query_slot;
        HIPC(c, hipEventSynchronize(L->idle));
        HIPC(c, hipMemcpy(count, L->d_qcnt + rtk::kCursorSet, sizeof(uint32_t), hipMemcpyDeviceToHost));
        return RT_OK;
    }
    std::vector<rt_ctx::FrameSlot*> ls = c->last_group;
    if (ls.empty()) ls.push_back(c->last_slot);
    for (rt_ctx::FrameSlot* L : ls) {
        if (!L || !L->d_wcnt || L->nframe == 0) continue;
        HIPC(c, hipEventSynchronize(L->idle));
        const uint64_t par = (L->nframe - 1) & 1u;   // the last frame's parity set
        uint32_t v = 0;
        HIPC(c, hipMemcpy(&v, L->d_wcnt + par * L->wcnt_set + kRestartSlot, sizeof(uint32_t), hipMemcpyDeviceToHost));
        *count += v;
    }
    return RT_OK;
}

// One frame through the counting instantiation (TR == 1) of the fast kernels: its 8 fetch counters
// (out8) and its loop-variant counters (out18), either may be null.
static int counted_frame(rt_ctx* c, const char* who, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, uint64_t* out8,
                         uint64_t* out18) {
    constexpr int kN = rtk::kFetchCounts + rtk::kVariantCounts;
    if (!c || (!out8 && !out18) || w == 0 || h == 0 || depth < 1 || depth > RT_MAX_DEPTH)
        return set_err(c, std::string(who) + ": invalid argument", RT_ERR_INVALID_ARG);
    // the fetch counters are about the fast quotient's loops; the variant counters also say what
    // RT_FLAG_EXACT_DIV does (every traversal through the generic division form)
    if ((depth > 1 && !(flags & RT_FLAG_WAVEFRONT)) || (out8 && (flags & RT_FLAG_EXACT_DIV)) || !c->have_scene || !c->scene.clean || c->scene.split)
        return set_err(c, std::string(who) + ": the fast kernels of a clean scene, depth 1 or the wavefront path",
                       RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    int rc = ensure(c, c->d_out, c->out_cap, (size_t)w * h);
    if (rc) return rc;
    unsigned long long* d = nullptr;
    HIPC(c, hipMalloc((void**)&d, kN * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, kN * sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) {
        c->trace.on = true;
        c->trace.d_counts = d;
        rc = rt_render_device(c, w, h, depth, flags | RT_FLAG_STATIC_ORDER, nullptr, c->d_out, nullptr, c->stream);
        c->trace.on = false;
        c->trace.d_counts = nullptr;
    }
    unsigned long long hc[kN] = {};
    if (e == hipSuccess && rc == RT_OK) e = hipMemcpyAsync(hc, d, sizeof hc, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return set_err(c, std::string(who) + ": " + hipGetErrorString(e), RT_ERR_DEVICE);
    if (out8)
        for (int k = 0; k < rtk::kFetchCounts; ++k) out8[k] = hc[k];
    if (out18)
        for (int k = 0; k < rtk::kVariantCounts; ++k) out18[k] = hc[rtk::kFetchCounts + k];
    return RT_OK;
}

int rt_fetch_counts(rt_ctx* c, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, uint64_t* out8) {
    return counted_frame(c, "rt_fetch_counts", w, h, depth, flags, out8, nullptr);
}

int rt_loop_variant_counts(rt_ctx* c, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, uint64_t* out18) {
    return counted_frame(c, "rt_loop_variant_counts", w, h, depth, flags, nullptr, out18);
}

int rt_gather_peak(rt_ctx* c, uint32_t table_records, uint32_t iters, float* ms, uint64_t* records) {
    if (!c || !ms || !records || table_records == 0 || iters == 0 || iters % 4)
        return set_err(c, "rt_gather_peak: invalid argument", RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    int cus = 0;
    HIPC(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const uint32_t blocks = (uint32_t)cus * 8u;   // 8 blocks of 4 waves per CU: 8 waves per SIMD
    float4* table = nullptr;
    uint32_t* sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPC(c, hipMalloc((void**)&table, (size_t)table_records * 64));
    hipError_t e = hipMalloc((void**)&sink, blocks * 4);
    if (e == hipSuccess) e = hipMemsetAsync(table, 0x3C, (size_t)table_records * 64, c->stream);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rtk::gather_peak_kernel, dim3(blocks), dim3(256), 0, c->stream, table, table_records, iters, sink);
        e = hipEventRecord(e0, c->stream);
    }
    if (e == hipSuccess) {
        for (int k = 0; k < 4; ++k)
            hipLaunchKernelGGL(rtk::gather_peak_kernel, dim3(blocks), dim3(256), 0, c->stream, table, table_records, iters,
                               sink);
        e = hipEventRecord(e1, c->stream);
    }
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    if (e == hipSuccess) e = hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(table);
    if (sink) (void)hipFree(sink);
    if (e != hipSuccess) return set_err(c, std::string("rt_gather_peak: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    *ms = t / 4.0f;
    *records = (uint64_t)blocks * 256u * iters;
    return RT_OK;
}

int rt_chase_peak(rt_ctx* c, uint32_t table_records, uint32_t iters, uint32_t group, float* ms, uint64_t* waves) {
    if (!c) return RT_ERR_INVALID_ARG;
    int cus = 0;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    return rt_chase_latency(c, table_records, iters, group, (uint32_t)cus * 8u, ms, waves);   // 8 waves per SIMD
}

int rt_chase_latency(rt_ctx* c, uint32_t table_records, uint32_t iters, uint32_t group, uint32_t blocks, float* ms,
                     uint64_t* waves) {
    if (!c || !ms || !waves || table_records < 2 || iters == 0 || group == 0 || group > 64 || (64 % group) ||
        blocks == 0 || blocks > (1u << 20))
        return set_err(c, "rt_chase_peak: invalid argument", RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    // the table: random child references (two per record, both valid), boxes from a fixed pattern
    std::vector<float4> tab((size_t)table_records * 4);
    uint32_t x = 0x9E3779B9u;
    for (uint32_t i = 0; i < table_records; ++i) {
        uint32_t rr[2];
        for (uint32_t& v : rr) {
            x ^= x << 13; x ^= x >> 17; x ^= x << 5;
            v = x % table_records;
        }
        const float a = (float)(i % 97), b = (float)(i % 89);
        tab[(size_t)i * 4 + 0] = make_float4(a, b, a + 3.0f, b + 5.0f);
        tab[(size_t)i * 4 + 1] = make_float4(b, a, b + 7.0f, a + 2.0f);
        tab[(size_t)i * 4 + 2] = make_float4(a + 1.0f, b + 1.0f, a + 9.0f, b + 4.0f);
        float r0, r1;
        std::memcpy(&r0, &rr[0], 4);
        std::memcpy(&r1, &rr[1], 4);
        tab[(size_t)i * 4 + 3] = make_float4(r0, r1, 0.0f, 0.0f);
    }
    float4* table = nullptr;
    uint32_t* sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPC(c, hipMalloc((void**)&table, tab.size() * sizeof(float4)));
    hipError_t e = hipMalloc((void**)&sink, blocks * 4);
    if (e == hipSuccess) e = hipMemcpy(table, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rtk::chase_peak_kernel, dim3(blocks), dim3(256), 0, c->stream, table, table_records, iters, group, sink);
        e = hipEventRecord(e0, c->stream);
    }
    if (e == hipSuccess) {
        for (int k = 0; k < 4; ++k)
            hipLaunchKernelGGL(rtk::chase_peak_kernel, dim3(blocks), dim3(256), 0, c->stream, table, table_records, iters,
                               group, sink);
        e = hipEventRecord(e1, c->stream);
    }
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    if (e == hipSuccess) e = hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(table);
    if (sink) (void)hipFree(sink);
    if (e != hipSuccess) return set_err(c, std::string("rt_chase_peak: ") + hipGetErrorString(e), RT_ERR_DEVICE);
    *ms = t / 4.0f;
    *waves = (uint64_t)blocks * 4u;
    return RT_OK;
}

// ---- one frame on several GPUs, one process (rt_render_tiled) ----

int rt_scene_copy(rt_ctx* dst, rt_ctx* src) {
    if (!dst || !src) return set_err(dst, "rt_scene_copy: invalid argument", RT_ERR_INVALID_ARG);
    if (dst == src) return RT_OK;
    if (!src->have_scene) return set_err(dst, "rt_scene_copy: the source context has no scene", RT_ERR_NO_SCENE);
    HIPC(dst, hipSetDevice(dst->device));
    if (const int rc = drop_scene(dst)) return rc;   // before the new one is allocated: peak memory is one scene's
    const Scene& F = src->scene;
    PendingScene ps(nullptr);
    Scene& S = ps.s;
    HIPC(dst, scene_alloc_records(S, F.n_wnodes4, F.n_tris4, F.n_shade4, F.n_leaf, nullptr));
    // device to device on one GPU, else peer to peer (xGMI), both on dst's stream
    const auto to = S.sections(), from = F.sections();
    for (size_t i = 0; i < to.size(); ++i) {
        if (!to[i].second) continue;
        if (dst->device == src->device)
            HIPC(dst, hipMemcpyAsync(to[i].first, from[i].first, to[i].second, hipMemcpyDeviceToDevice, dst->stream));
        else
            HIPC(dst, hipMemcpyPeerAsync(to[i].first, dst->device, from[i].first, src->device, to[i].second, dst->stream));
    }
    HIPC(dst, hipStreamSynchronize(dst->stream));
    S.root = F.root; S.n_inner = F.n_inner; S.fast_div = F.fast_div; S.clean = F.clean;
    S.why = "the scene came from rt_scene_copy; upload it with rt_upload_scene to update it";
    S.have_bounds = F.have_bounds; S.bounds_min = F.bounds_min; S.bounds_max = F.bounds_max;
    return install_scene(dst, std::move(S));
}

// rt_render_tiled: the frame is cut into 8-row bands dealt round-robin over the contexts
// (rt_tiling).  Every context renders its bands on its own stream with the
// frame-row output of the kernels (rtk::Outputs::frame_rows): each pixel store goes straight to
// its place in ONE host frame, so every GPU sends its own rows over its own host link while it
// renders, and there is no gather, copy or re-interleave step.  That frame is the caller's
// buffer when it is pinned memory the devices can write, else ctx 0's pinned staging frame,
// copied to the caller's memory after the join.  Then every stream is synchronised: returns
// with the frame complete in out_bgr, like raytrace_gpgpu (RayTracer.cpp:330-344).
constexpr int32_t kTiledBandRows = 8;
constexpr int32_t kMaxTiled = 64;

// One context's part of a tiled frame: its bands straight into the frame's rows (depth 1), or
// into its band buffer and then one row-copy kernel; then the wait for its stream (also after a
// failed enqueue: nothing may still write into the frame when rt_render_tiled returns).
struct TiledJob {
    uint32_t w, h;
    int32_t depth;
    uint32_t flags;
    rt_tiling t;
    uint32_t* frame;   // the frame as THIS context's device addresses it
};
static int tiled_enqueue(rt_ctx* c, const TiledJob& j) {
    int rc = RT_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_err(c, "hipSetDevice failed", RT_ERR_DEVICE);
    if (j.depth == 1) {   // the depth-1 kernel writes its pixels into the frame's rows itself
        c->frame_rows = true;
        rc = rt_render_device(c, j.w, j.h, j.depth, j.flags, &j.t, j.frame, nullptr, c->stream);
        c->frame_rows = false;
    } else {              // other kernels: the context's bands, then one row-copy kernel into the frame
        const int64_t lp = rt_tiling_pixels(j.w, j.h, &j.t);
        if (lp > 0 && (rc = ensure(c, c->d_out, c->out_cap, (size_t)lp)) == RT_OK &&
            (rc = rt_render_device(c, j.w, j.h, j.depth, j.flags, &j.t, c->d_out, nullptr, c->stream)) == RT_OK &&
            rt_bands_put(c->d_out, j.frame, j.w, j.h, &j.t, c->stream) != RT_OK)
            rc = set_err(c, g_err, RT_ERR_DEVICE);
    }
    return rc;
}
static int tiled_wait(rt_ctx* c, int rc) {
    const hipError_t e = hipSetDevice(c->device) == hipSuccess ? wait_ctx(c, c->stream) : hipErrorInvalidDevice;
    if (e != hipSuccess && rc == RT_OK) rc = set_err(c, hipGetErrorString(e), RT_ERR_DEVICE);
    return rc;
}
static int tiled_part(rt_ctx* c, const TiledJob& j) { return tiled_wait(c, tiled_enqueue(c, j)); }

// rt_render_tiled's host thread per context (ctxs[1..n-1]; ctxs[0]'s part runs on the caller's
// thread).  The hand-off is a sequence number the worker spins on, so all contexts enqueue at
// once instead of one after another (~3-4 us of host time each): a condition
// variable costs about as much as the enqueue it would save, so a worker spins for
// kWorkerSpinMs after its last frame (a frame loop keeps it spinning) and only then sleeps.
// RTAMD_TILED_WORKERS=0: every part on the caller's thread, one after another (A/B).
constexpr double kWorkerSpinMs = 20.0;
struct TiledWorker {
    std::thread th;
    std::atomic<uint64_t> posted{0}, finished{0};
    std::atomic<bool> stop{false}, asleep{false};
    std::mutex m;
    std::condition_variable cv;
    TiledJob job{};
    int rc = RT_OK;
};
static void tiled_worker_loop(rt_ctx* c, TiledWorker* W) {
    (void)hipSetDevice(c->device);
    uint64_t seen = 0;
    for (;;) {
        auto t0 = std::chrono::steady_clock::now();
        uint32_t spins = 0;
        while (W->posted.load(std::memory_order_acquire) == seen && !W->stop.load(std::memory_order_relaxed)) {
            cpu_relax();
            if ((++spins & 4095u) == 0 &&
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > kWorkerSpinMs) {
                std::unique_lock<std::mutex> lk(W->m);
                W->asleep.store(true);   // seq_cst with the poster's store of `posted` then load of `asleep`
                W->cv.wait(lk, [&] { return W->posted.load() != seen || W->stop.load(); });
                W->asleep.store(false);
                t0 = std::chrono::steady_clock::now();
            }
        }
        if (W->stop.load()) return;
        seen = W->posted.load(std::memory_order_acquire);
        W->rc = tiled_part(c, W->job);
        W->finished.store(seen, std::memory_order_release);
    }
}
static void tiled_post(rt_ctx* c, const TiledJob& j) {
    if (!c->worker) {
        c->worker = new TiledWorker();
        c->worker->th = std::thread(tiled_worker_loop, c, c->worker);
    }
    TiledWorker* W = c->worker;
    W->job = j;
    W->posted.fetch_add(1);   // seq_cst (the worker's asleep store / posted load pair)
    if (W->asleep.load()) {
        std::lock_guard<std::mutex> lk(W->m);
        W->cv.notify_one();
    }
}
static int tiled_join(rt_ctx* c) {
    TiledWorker* W = c->worker;
    const uint64_t want = W->posted.load();
    while (W->finished.load(std::memory_order_acquire) != want) cpu_relax();
    return W->rc;
}
static void tiled_worker_stop(rt_ctx* c) {
    if (!c->worker) return;
    {
        std::lock_guard<std::mutex> lk(c->worker->m);
        c->worker->stop.store(true);
        c->worker->cv.notify_one();
    }
    if (c->worker->th.joinable()) c->worker->th.join();
    delete c->worker;
    c->worker = nullptr;
}
static bool tiled_workers_on() {
    const char* v = std::getenv("RTAMD_TILED_WORKERS");
    return !(v && std::strcmp(v, "0") == 0);
}

int32_t rt_tiled_direct_ok(int32_t n, const uint64_t* dev_addrs) {
    if (n < 1 || !dev_addrs) return 0;
    for (int32_t k = 0; k < n; ++k)
        if (!dev_addrs[k] || (dev_addrs[k] & 15u)) return 0;   // unmapped on that device, or not 16-B aligned
    return 1;
}

// rt_render_tiled: the frame is cut into 8-row bands dealt round-robin over the contexts
// (rt_tiling).  Every context renders its bands on its own stream with the
// frame-row output of the kernels (rtk::Outputs::frame_rows): each pixel store goes straight to
// its place in ONE host frame, so every GPU sends its own rows over its own host link while it
// renders, and there is no gather, copy or re-interleave step.  That frame is the caller's
// buffer when every context's device can address it (hipHostGetDevicePointer on each device:
// portable pinned memory, or memory registered and mapped for all of them), else ctxs[0]'s
// portable pinned staging frame, copied to the caller's memory after the join.  Each context
// addresses the frame through its own device's mapping.  ctxs[1..] enqueue and wait on their own
// host threads (TiledWorker), ctxs[0] on the caller's; returns with the frame complete in out_bgr,
// like raytrace_gpgpu (RayTracer.cpp:330-344).
int rt_render_tiled(rt_ctx** ctxs, int32_t n, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, uint32_t* out_bgr) {
    if (!ctxs || n < 1 || n > kMaxTiled || !out_bgr || w == 0 || h == 0 || depth < 0 || depth > RT_MAX_DEPTH)
        return set_err(nullptr, "rt_render_tiled: invalid argument", RT_ERR_INVALID_ARG);
    for (int32_t k = 0; k < n; ++k) {
        if (!ctxs[k]) return set_err(nullptr, "rt_render_tiled: ctxs[k] is NULL", RT_ERR_INVALID_ARG);
        for (int32_t j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return set_err(nullptr, "rt_render_tiled: a context appears twice", RT_ERR_INVALID_ARG);
    }
    rt_ctx* c0 = ctxs[0];
    if ((flags & RT_FLAG_STRICT_MATH) && (flags & RT_FLAG_HW_MATH))
        return set_err(c0, "rt_render_tiled: RT_FLAG_STRICT_MATH and RT_FLAG_HW_MATH exclude each other", RT_ERR_INVALID_ARG);
    if (!c0->have_params) return set_err(c0, "rt_render_tiled: no params set on ctxs[0]", RT_ERR_NO_SCENE);
    for (int32_t k = 0; k < n; ++k)
        if (!ctxs[k]->have_scene)
            return set_err(c0, "rt_render_tiled: ctxs[" + std::to_string(k) + "] has no scene (rt_scene_copy)", RT_ERR_NO_SCENE);
    if (n == 1) return rt_render(c0, w, h, depth, flags, out_bgr, nullptr);
    const size_t npix = (size_t)w * h;
    // the frame as every context's device addresses it: the caller's buffer if all of them map it
    uint64_t addr[kMaxTiled] = {};
    for (int32_t k = 0; k < n; ++k) {
        void* dp = nullptr;
        if (hipSetDevice(ctxs[k]->device) == hipSuccess && hipHostGetDevicePointer(&dp, out_bgr, 0) == hipSuccess)
            addr[k] = (uint64_t)(uintptr_t)dp;
    }
    (void)hipGetLastError();   // pageable memory: not an error
    const bool staged = !rt_tiled_direct_ok(n, addr);
    if (staged) {
        HIPC(c0, hipSetDevice(c0->device));
        if (c0->stage_cap < npix) {
            if (c0->h_stage) (void)hipHostFree(c0->h_stage);
            c0->h_stage = nullptr;
            c0->stage_cap = 0;
            HIPC(c0, hipHostMalloc((void**)&c0->h_stage, npix * 4, hipHostMallocPortable | hipHostMallocMapped));
            c0->stage_cap = npix;
        }
        for (int32_t k = 0; k < n; ++k) {
            void* dp = nullptr;
            HIPC(c0, hipSetDevice(ctxs[k]->device));
            HIPC(c0, hipHostGetDevicePointer(&dp, c0->h_stage, 0));
            addr[k] = (uint64_t)(uintptr_t)dp;
        }
    }
    const bool workers = tiled_workers_on();
    int32_t posted = 0;
    for (int32_t k = 1; k < n; ++k) {
        rt_ctx* c = ctxs[k];
        c->params = c0->params;   // ctxs[0]'s camera drives the frame (updateCamera, RayTracer.cpp:671)
        c->have_params = true;
    }
    if (workers)
        for (; posted < n - 1; ++posted)
            tiled_post(ctxs[posted + 1], TiledJob{w, h, depth, flags, rt_tiling{posted + 1, n, kTiledBandRows, 0},
                                                  (uint32_t*)(uintptr_t)addr[posted + 1]});
    int rc = RT_OK;
    if (workers) {
        rc = tiled_part(c0, TiledJob{w, h, depth, flags, rt_tiling{0, n, kTiledBandRows, 0}, (uint32_t*)(uintptr_t)addr[0]});
    } else {   // every part enqueued on this thread, one after another, then every stream waited for
        int rk[kMaxTiled];
        for (int32_t k = 0; k < n; ++k)
            rk[k] = tiled_enqueue(ctxs[k], TiledJob{w, h, depth, flags, rt_tiling{k, n, kTiledBandRows, 0},
                                                    (uint32_t*)(uintptr_t)addr[k]});
        for (int32_t k = 0; k < n; ++k) {
            const int r = tiled_wait(ctxs[k], rk[k]);
            if (r && rc == RT_OK) {
                rc = r;
                if (k) c0->err = "rt_render_tiled: ctxs[" + std::to_string(k) + "]: " + ctxs[k]->err;
            }
        }
    }
    // join every posted part, also after a failure (nothing may still write into the frame)
    for (int32_t k = 1; k <= posted; ++k) {
        const int r = tiled_join(ctxs[k]);
        if (r && rc == RT_OK) {
            rc = r;
            c0->err = "rt_render_tiled: ctxs[" + std::to_string(k) + "]: " + ctxs[k]->err;
        }
    }
    (void)hipSetDevice(c0->device);
    if (rc) return rc;
    if (staged) std::memcpy(out_bgr, c0->h_stage, npix * 4);
    return RT_OK;
}

// ---- diagnostics: where a frame's time goes ----

int rt_wave_timeline(rt_ctx* c, uint32_t w, uint32_t h, int32_t depth, uint32_t flags, int32_t frames, uint32_t* words,
                     uint64_t cap_words, uint64_t* used_words) {
    constexpr uint32_t kHead = 128, kMaxLaunches = 32;
    if (!c || !words || !used_words || cap_words < kHead || w == 0 || h == 0 || depth < 1 || depth > RT_MAX_DEPTH ||
        frames < 1 || frames > 8 || (uint64_t)frames * (uint64_t)depth > kMaxLaunches)
        return set_err(c, "rt_wave_timeline: invalid argument", RT_ERR_INVALID_ARG);
    if ((flags & (RT_FLAG_STRICT_MATH | RT_FLAG_HW_MATH | RT_FLAG_EXACT_DIV)) || (depth > 1 && !(flags & RT_FLAG_WAVEFRONT)) ||
        !c->have_scene || !c->scene.clean || c->scene.split)
        return set_err(c, "rt_wave_timeline: the default arithmetic's fast kernels of a clean scene, depth 1 or the wavefront path",
                       RT_ERR_INVALID_ARG);
    HIPC(c, hipSetDevice(c->device));
    const size_t npix = (size_t)w * h;
    int rc = ensure(c, c->d_out, c->out_cap, npix * (size_t)frames);
    if (rc) return rc;
    if ((rc = ensure(c, c->tline.d_words, c->tline.cap, (size_t)cap_words))) return rc;
    // frame f in flight renders on stream f: the ctx stream, then the row-group streams (their own
    // frame slots and longest-first orders); a few untimed rounds first, so every stream's order is
    // built from its own previous frame, as for the frames the product keeps in flight
    hipStream_t st[8];
    st[0] = c->stream;
    for (int32_t f = 1; f < frames; ++f) {
        if (!c->gstream[f - 1]) HIPC(c, hipStreamCreateWithFlags(&c->gstream[f - 1], hipStreamNonBlocking));
        st[f] = c->gstream[f - 1];
    }
    if (frames > 1) {
        for (int r = 0; r < 3; ++r)
            for (int32_t f = 0; f < frames; ++f)
                if ((rc = rt_render_device(c, w, h, depth, flags, nullptr, c->d_out + (size_t)f * npix, nullptr, st[f])))
                    return rc;
        for (int32_t f = 0; f < frames; ++f) HIPC(c, hipStreamSynchronize(st[f]));
    }
    HIPC(c, hipMemsetAsync(c->tline.d_words, 0, (size_t)cap_words * 4, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    c->tline.on = true;
    c->tline.limit = (size_t)cap_words - kHead;
    c->tline.used = 0;
    c->tline.waves.clear();
    c->tline.frame.clear();
    c->tline.bounce.clear();
    const uint64_t f0 = c->frames;
    for (int32_t f = 0; f < frames && rc == RT_OK; ++f) {
        c->tline.cur_frame = (uint32_t)f;
        const size_t first = c->tline.waves.size();
        rc = rt_render_device(c, w, h, depth, flags, nullptr, c->d_out + (size_t)f * npix, nullptr, st[f]);
        for (size_t i = first; i < c->tline.bounce.size(); ++i) c->tline.bounce[i] = (uint32_t)(i - first);
    }
    c->tline.on = false;
    for (int32_t f = 0; f < frames; ++f) HIPC(c, hipStreamSynchronize(st[f]));
    if (rc) return rc;
    float t = 0.0f, k = 0.0f;
    if ((rc = frame_times(c, f0, t, k))) return rc;   // the first frame's kernels
    const size_t L = c->tline.waves.size();
    if (L > kMaxLaunches) return set_err(c, "rt_wave_timeline: too many launches", RT_ERR_INVALID_ARG);
    std::memset(words, 0, kHead * 4);
    words[0] = (uint32_t)L;
    words[1] = (uint32_t)frames;
    words[2] = (uint32_t)std::lround((double)t * 1e6);   // the first frame's kernels, HIP events, ns
    words[3] = (uint32_t)std::lround((double)k * 1e6);   // its first launch
    words[4] = rtk::kTlRecord;                            // words per wave record
    words[5] = RTK_TL_SPLIT;                              // memory-wait words stamped
    for (size_t i = 0; i < L; ++i) {
        words[8 + i] = c->tline.waves[i];
        words[40 + i] = c->tline.frame[i];
        words[72 + i] = c->tline.bounce[i];
    }
    HIPC(c, hipMemcpy(words + kHead, c->tline.d_words, c->tline.used * 4, hipMemcpyDeviceToHost));
    *used_words = kHead + c->tline.used;
    return RT_OK;
}

int rt_overflow_count(rt_ctx* c, uint64_t* count) {
    if (!c || !count) return RT_ERR_INVALID_ARG;
    unsigned long long v = 0;
    HIPC(c, hipMemcpy(&v, c->d_overflow, sizeof v, hipMemcpyDeviceToHost));
    *count = v;
    return RT_OK;
}

}  // extern "C"
