// multihit_core.hpp -- the list and the traversal of a first-k-hits ray query (rt_trace_rays_k,
// DESIGN.md 24) that the host twin (multihit.cpp) and the HIP kernels (multihit_kernel<K> of
// rt_kernel_body.inc) share.  Plain inline templates, no HIP types and no float arithmetic: the
// arithmetic lives in the Scene adaptor, which is the ray as well as the scene,
//   S.slab(cur, n0, f0, n1, f1, r0, r1)   the slab test of inner record cur's two child boxes (near and far
//                                         parameter of each) and its two child references
//   S.leaf(ref, off, cnt)                 a leaf reference's range of triangle reference records
//   S.tri_t(k, t, id)                     ray_tri of triangle reference record k, and its triangle id
// so one text of the control flow serves the three device arithmetics and the host's S_strict.
// The includer defines MULTIHIT_HD: `inline` for a host unit, `__device__ __forceinline__` for a kernel.
#pragma once
#include <cstdint>

#include "rt_records.h"

#ifndef MULTIHIT_HD
#define MULTIHIT_HD inline
#endif

namespace multihit {

constexpr int kMaxK = 8;
constexpr int kStackSize = 65;      // the general traversal's (volumeRender.cl:636)
constexpr float kTmin = 0.001f;     // volumeRender.cl:640; a constant, not a per-ray value

// The general traversal's state (rt_kernel_body.inc Trav) with a list in place of the one hit:
// L[0 .. K-1], sorted by (t, id), every entry starting as the sentinel {id = -1, t = tmax}.  K is a
// template parameter so that the list is indexed statically only (registers on the device).  An entry
// keeps (t, id, at), `at` the triangle reference record it was found in: u and v are ray_tri_uv of that
// record at the end.  The reference stack is [0 .. sc-1] with entry sc-1 the node being visited (cur);
// entry sc-2 is kept in nxt, entries 0 .. sc-3 live in the Stack.  sc == 0: finished.
template <int K>
struct StateK {
    uint32_t cur, nxt;
    int sc;
    int tk, tend;     // the leaf the lane is inside: its next and its end reference record; tk >= tend: in none
    float t[K];
    int32_t id[K];
    int32_t at[K];
    bool overflow;
    uint64_t inner_visits, tri_tests;   // STATS only
};

template <int K>
MULTIHIT_HD void start(StateK<K>& T, uint32_t root, float tmax) {
    T.cur = root;
    T.nxt = 0;
    T.sc = 1;
    T.tk = T.tend = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        T.t[j] = tmax;
        T.id[j] = -1;
        T.at[j] = 0;
    }
    T.overflow = false;
    T.inner_visits = T.tri_tests = 0;
}

// all K records a miss (an overflow, or the error reference)
template <int K>
MULTIHIT_HD void end_as_miss(StateK<K>& T) {
#pragma unroll
    for (int j = 0; j < K; ++j) T.id[j] = -1;
    T.sc = 0;
}

template <int K, class Stack>
MULTIHIT_HD void pop(StateK<K>& T, const Stack& st) {
    --T.sc;
    T.cur = T.nxt;
    if (T.sc >= 2) T.nxt = st.get(T.sc - 2);
}

// The candidate (t, id) of a triangle test.  Range: dropped unless t > kTmin (a NaN is dropped).
// Presence: an id the list holds is dropped (the SBVH references a triangle from several leaves).
// Acceptance: against the last entry; tmax is exclusive, and the id rule applies to a found entry only.
// Insertion: before the first entry the candidate precedes in (t, id); the entries from there move down
// one and the last falls off.  A sentinel needs no case of its own: an accepted t is strictly below
// tmax.  An entry that has fallen off and is met again through another reference is refused by
// acceptance: K entries of the list precede it in the order, and the list only ever moves towards
// the front of the order.
template <int K>
MULTIHIT_HD void offer(StateK<K>& T, float t, int32_t id, int32_t at) {
    if (!(t > kTmin)) return;
    bool present = false;
#pragma unroll
    for (int j = 0; j < K; ++j) present = present || T.id[j] == id;
    if (present) return;
    if (!(t < T.t[K - 1] || (t == T.t[K - 1] && T.id[K - 1] >= 0 && id < T.id[K - 1]))) return;
    // before[j]: the candidate precedes entry j; false .. false true .. true along the sorted list
    bool before[K];
#pragma unroll
    for (int j = 0; j < K; ++j) before[j] = t < T.t[j] || (t == T.t[j] && id < T.id[j]);
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        if (j > 0 && before[j - 1]) {
            T.t[j] = T.t[j - 1];
            T.id[j] = T.id[j - 1];
            T.at[j] = T.at[j - 1];
        } else if (before[j]) {
            T.t[j] = t;
            T.id[j] = id;
            T.at[j] = at;
        }
    }
}

// One step of a ray's own sequence: one triangle test of the leaf it sits on (arriving there first,
// if it has just come), or one inner visit.  trav_step<true>'s decisions with T.tHit read as the last
// entry's t: a leaf's references are all tested, in order; a child is wanted iff
// (n <= f) && (f >= kTmin) && (n <= bound); both wanted push the farther one (n0 > n1 swaps, a tie
// goes left) unless the stack is full, which ends the ray as an overflow.
template <bool STATS, int K, class Scene, class Stack>
MULTIHIT_HD void step(StateK<K>& T, const Scene& S, const Stack& st) {
    if (T.tk >= T.tend && (T.cur & rtrec::kLeafBit)) {
        int off, cnt;
        S.leaf(T.cur, off, cnt);
        if (cnt <= 0) {
            pop(T, st);
            return;
        }
        T.tk = off;
        T.tend = off + cnt;
    }
    if (T.tk < T.tend) {
        float t;
        int32_t id;
        S.tri_t(T.tk, t, id);
        if (STATS) ++T.tri_tests;
        offer(T, t, id, (int32_t)T.tk);
        if (++T.tk == T.tend) {
            T.tk = T.tend = 0;
            pop(T, st);
        }
        return;
    }
    if (T.cur == rtrec::kRefError) {
        end_as_miss(T);
        return;
    }
    float n0, f0, n1, f1;
    uint32_t r0, r1;
    S.slab(T.cur, n0, f0, n1, f1, r0, r1);
    if (STATS) ++T.inner_visits;
    const float bound = T.t[K - 1];
    const bool w0 = (n0 <= f0) && (f0 >= kTmin) && (n0 <= bound);
    const bool w1 = (n1 <= f1) && (f1 >= kTmin) && (n1 <= bound);
    if (w0 && w1) {
        if (T.sc >= kStackSize) {
            T.overflow = true;
            end_as_miss(T);
            return;
        }
        const bool swap = n0 > n1;   // near child first, a tie goes left
        if (T.sc >= 2) st.put(T.sc - 2, T.nxt);
        T.nxt = swap ? r0 : r1;
        T.cur = swap ? r1 : r0;
        ++T.sc;
    } else if (w0 || w1) {
        T.cur = w0 ? r0 : r1;
    } else {
        pop(T, st);
    }
}

}  // namespace multihit
