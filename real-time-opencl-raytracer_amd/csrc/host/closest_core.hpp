// closest_core.hpp -- the arithmetic and the traversal of a closest-point query and of
// its k-answer form (at the end) that
// the host twin (closest_points.cpp) and the HIP kernel (rt_closest.hip) share.  Plain inline
// functions and templates, no HIP types; the kernel compiles them for the device through CLOSEST_HD.
// Every float operation here is a single IEEE binary32 operation, fmaf only where it is written
// (both sides are built with -ffp-contract=off, the device with correctly rounded division), so
// both sides compute the same words.
#pragma once
#include <cmath>
#include <cstdint>

#include "rt_records.h"

#ifndef CLOSEST_HD
#if defined(__HIPCC__)
#define CLOSEST_HD __host__ __device__ inline
#else
#define CLOSEST_HD inline
#endif
#endif

namespace closest {

constexpr int kStackSize = 65;   // a push at this stack count is the reference's overflow (volumeRender.cl:914)
constexpr float kInf = __builtin_inff();

struct V3 {
    float x, y, z;
};

// rt_device_math.h's dot
CLOSEST_HD float dot3(const V3& a, const V3& b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
CLOSEST_HD V3 sub3(const V3& a, const V3& b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// x, y, z finite and r > 0 (+inf is legal; NaN, 0, -0 and negatives are not)
CLOSEST_HD bool point_ok(float x, float y, float z, float r) {
    return fabsf(x) < kInf && fabsf(y) < kInf && fabsf(z) < kInf && r > 0.0f;
}

struct TriPoint {
    float u, v, d2;
    V3 p;
};

// The closest point of triangle {p0, p0 + e1, p0 + e2} to q: Ericson's region walk on the words of
// the triangle reference record.  The tests run in this order and the first that holds decides; the
// quotient of the region found is one correctly rounded division.  A degenerate triangle may give
// NaN, which acceptance refuses.
CLOSEST_HD TriPoint tri_point(const V3& q, const V3& p0, const V3& e1, const V3& e2) {
    const V3 ap = sub3(q, p0);
    const float d1 = dot3(e1, ap), d2 = dot3(e2, ap);
    const V3 bp = sub3(ap, e1);
    const float d3 = dot3(e1, bp), d4 = dot3(e2, bp);
    const V3 cp = sub3(ap, e2);
    const float d5 = dot3(e1, cp), d6 = dot3(e2, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float a = d4 - d3, b = d5 - d6;
    float u, v;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        u = 0.0f; v = 0.0f;
    } else if (d3 >= 0.0f && d4 <= d3) {
        u = 1.0f; v = 0.0f;
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        u = d1 / (d1 - d3); v = 0.0f;
    } else if (d6 >= 0.0f && d5 <= d6) {
        u = 0.0f; v = 1.0f;
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        u = 0.0f; v = d2 / (d2 - d6);
    } else if (va <= 0.0f && a >= 0.0f && b >= 0.0f) {
        const float w = a / (a + b);
        u = 1.0f - w; v = w;
    } else {
        const float den = 1.0f / ((va + vb) + vc);
        u = vb * den; v = vc * den;
    }
    TriPoint r;
    r.u = u;
    r.v = v;
    r.p = V3{fmaf(v, e2.x, fmaf(u, e1.x, p0.x)), fmaf(v, e2.y, fmaf(u, e1.y, p0.y)), fmaf(v, e2.z, fmaf(u, e1.z, p0.z))};
    const V3 df = sub3(q, r.p);
    r.d2 = dot3(df, df);
    return r;
}

// Squared distance from q to the box [lo, hi]: per axis e = maxNum(maxNum(lo - q, q - hi), 0) (IEEE
// maxNum: fmaxf, v_max3_f32), then dot(e, e).  The sign of a zero box word cannot show: e * e = +0.
CLOSEST_HD float box_d2(const V3& q, const V3& lo, const V3& hi) {
    const V3 e{fmaxf(fmaxf(lo.x - q.x, q.x - hi.x), 0.0f), fmaxf(fmaxf(lo.y - q.y, q.y - hi.y), 0.0f),
               fmaxf(fmaxf(lo.z - q.z, q.z - hi.z), 0.0f)};
    return dot3(e, e);
}
// a box with a NaN word is never visited (maxNum alone would drop the NaN)
CLOSEST_HD bool box_ordered(const V3& lo, const V3& hi) {
    return !(__builtin_isunordered(lo.x, hi.x) || __builtin_isunordered(lo.y, hi.y) || __builtin_isunordered(lo.z, hi.z));
}

// One query in flight.  cur / nxt / sc are the general ray traversal's (rt_kernel_body.inc
// trav_step): cur is the reference stood on, nxt the top of the stack, entries 0 .. sc - 3 live in
// the Stack; sc = 0: finished.  [tk, tend): the triangle records left of the leaf stood on.
struct State {
    uint32_t cur, nxt;
    int sc;
    int tk, tend;
    float best;      // r * r, then the accepted d2
    int32_t bid;     // -1, then the accepted id
    float u, v;
    V3 p;
    bool overflow;
    uint64_t inner_visits, tri_tests;   // STATS only
};

CLOSEST_HD void start(State& T, uint32_t root, float r) {
    T.cur = root;
    T.nxt = 0;
    T.sc = 1;
    T.tk = T.tend = 0;
    T.best = r * r;
    T.bid = -1;
    T.u = T.v = 0.0f;
    T.p = V3{0.0f, 0.0f, 0.0f};
    T.overflow = false;
    T.inner_visits = T.tri_tests = 0;
}

// the query ends as a miss (an overflow, or the error reference)
CLOSEST_HD void end_as_miss(State& T) {
    T.bid = -1;
    T.best = kInf;
    T.sc = 0;
}

template <class Stack>
CLOSEST_HD void pop(State& T, const Stack& st) {
    --T.sc;
    T.cur = T.nxt;
    if (T.sc >= 2) T.nxt = st.get(T.sc - 2);
}

// One step of one query: one triangle test of the leaf stood on, or one inner visit.  A popped
// reference is visited unconditionally: no distance is kept on the stack.
//   Scene:  inner(id, lo0, hi0, lo1, hi1, r0, r1)  the record's two child boxes and references
//           leaf(ref, off, cnt)                    rtk::leaf_range
//           tri(k, p0, e1, e2, id)                 triangle reference record k
//   Stack:  get(i), put(i, word)                   entries 0 .. 62
template <bool STATS, class Scene, class Stack>
CLOSEST_HD void step(State& T, const V3& q, const Scene& S, const Stack& st) {
    if (T.tk >= T.tend && (T.cur & rtrec::kLeafBit)) {
        int off, cnt;
        S.leaf(T.cur, off, cnt);
        if (cnt <= 0) {   // an empty leaf does nothing
            pop(T, st);
            return;
        }
        T.tk = off;
        T.tend = off + cnt;
    }
    if (T.tk < T.tend) {
        V3 p0, e1, e2;
        int32_t id;
        S.tri(T.tk, p0, e1, e2, id);
        const TriPoint r = tri_point(q, p0, e1, e2);
        if (STATS) ++T.tri_tests;
        if (r.d2 < T.best || (r.d2 == T.best && T.bid >= 0 && id < T.bid)) {
            T.best = r.d2;
            T.bid = id;
            T.u = r.u;
            T.v = r.v;
            T.p = r.p;
        }
        if (++T.tk == T.tend) {
            T.tk = T.tend = 0;
            pop(T, st);
        }
        return;
    }
    if (T.cur == rtrec::kRefError) {   // a malformed inner node: an error miss, as for rays
        end_as_miss(T);
        return;
    }
    V3 lo0, hi0, lo1, hi1;
    uint32_t r0, r1;
    S.inner(T.cur, lo0, hi0, lo1, hi1, r0, r1);
    if (STATS) ++T.inner_visits;
    const float b0 = box_d2(q, lo0, hi0), b1 = box_d2(q, lo1, hi1);
    const bool w0 = box_ordered(lo0, hi0) && b0 <= T.best;   // <=: an equally near lower id is still found
    const bool w1 = box_ordered(lo1, hi1) && b1 <= T.best;
    if (w0 && w1) {
        if (T.sc >= kStackSize) {
            T.overflow = true;
            end_as_miss(T);
            return;
        }
        const bool swap = b0 > b1;   // near child first, a tie goes left
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

// The 8 words of the record: {id, d2, u, v, p, 0}; a miss is {-1, +inf, 0, 0, 0, 0, 0, 0}.
CLOSEST_HD void result_words(const State& T, uint32_t w[8]) {
    const bool found = T.bid >= 0;
    union { float f; uint32_t u; } c;
    w[0] = (uint32_t)T.bid;
    c.f = found ? T.best : kInf; w[1] = c.u;
    c.f = found ? T.u : 0.0f;    w[2] = c.u;
    c.f = found ? T.v : 0.0f;    w[3] = c.u;
    c.f = found ? T.p.x : 0.0f;  w[4] = c.u;
    c.f = found ? T.p.y : 0.0f;  w[5] = c.u;
    c.f = found ? T.p.z : 0.0f;  w[6] = c.u;
    w[7] = 0u;
}

// ---- the k nearest triangles ----
// The traversal above with a list in place of the one answer: L[0 .. K-1], sorted by (d2, id), every
// entry starting as the sentinel {id = -1, d2 = r * r}.  K is a template parameter so that the list is
// indexed statically only (registers on the device).  An entry keeps (d2, id, at), `at` the triangle
// reference record it was found in; u, v and p are tri_point's of that record again at the end.
constexpr int kMaxK = 8;

template <int K>
struct StateK {
    uint32_t cur, nxt;
    int sc;
    int tk, tend;
    float d2[K];
    int32_t id[K];
    int32_t at[K];
    bool overflow;
    uint64_t inner_visits, tri_tests;   // STATS only
};

template <int K>
CLOSEST_HD void start(StateK<K>& T, uint32_t root, float r) {
    T.cur = root;
    T.nxt = 0;
    T.sc = 1;
    T.tk = T.tend = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        T.d2[j] = r * r;
        T.id[j] = -1;
        T.at[j] = 0;
    }
    T.overflow = false;
    T.inner_visits = T.tri_tests = 0;
}

// all K records a miss (an overflow, or the error reference)
template <int K>
CLOSEST_HD void end_as_miss(StateK<K>& T) {
#pragma unroll
    for (int j = 0; j < K; ++j) T.id[j] = -1;
    T.sc = 0;
}

template <int K, class Stack>
CLOSEST_HD void pop(StateK<K>& T, const Stack& st) {
    --T.sc;
    T.cur = T.nxt;
    if (T.sc >= 2) T.nxt = st.get(T.sc - 2);
}

// The candidate (d2, id) of a triangle test.  Presence: an id the list holds is dropped (the SBVH
// references a triangle from several leaves).  Acceptance: the single answer's rule against the last
// entry; a NaN is never accepted and r is exclusive.  Insertion: before the first entry the candidate
// precedes in (d2, id); the entries from there move down one and the last falls off.  A sentinel needs
// no case of its own: an accepted d2 is strictly below r * r.  An entry that has fallen off and is met
// again through another reference is refused by acceptance: K entries of the list precede it in the
// order, and the list only ever moves towards the front of the order.
template <int K>
CLOSEST_HD void offer(StateK<K>& T, float d2, int32_t id, int32_t at) {
    bool present = false;
#pragma unroll
    for (int j = 0; j < K; ++j) present = present || T.id[j] == id;
    if (present) return;
    if (!(d2 < T.d2[K - 1] || (d2 == T.d2[K - 1] && T.id[K - 1] >= 0 && id < T.id[K - 1]))) return;
    // before[j]: the candidate precedes entry j; false .. false true .. true along the sorted list
    bool before[K];
#pragma unroll
    for (int j = 0; j < K; ++j) before[j] = d2 < T.d2[j] || (d2 == T.d2[j] && id < T.id[j]);
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        if (j > 0 && before[j - 1]) {
            T.d2[j] = T.d2[j - 1];
            T.id[j] = T.id[j - 1];
            T.at[j] = T.at[j - 1];
        } else if (before[j]) {
            T.d2[j] = d2;
            T.id[j] = id;
            T.at[j] = at;
        }
    }
}

// step with the list: the bound is the last entry's d2
template <bool STATS, int K, class Scene, class Stack>
CLOSEST_HD void step(StateK<K>& T, const V3& q, const Scene& S, const Stack& st) {
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
        V3 p0, e1, e2;
        int32_t id;
        S.tri(T.tk, p0, e1, e2, id);
        const TriPoint r = tri_point(q, p0, e1, e2);
        if (STATS) ++T.tri_tests;
        offer(T, r.d2, id, (int32_t)T.tk);
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
    V3 lo0, hi0, lo1, hi1;
    uint32_t r0, r1;
    S.inner(T.cur, lo0, hi0, lo1, hi1, r0, r1);
    if (STATS) ++T.inner_visits;
    const float b0 = box_d2(q, lo0, hi0), b1 = box_d2(q, lo1, hi1);
    const bool w0 = box_ordered(lo0, hi0) && b0 <= T.d2[K - 1];   // <=: an equally near lower id is still found
    const bool w1 = box_ordered(lo1, hi1) && b1 <= T.d2[K - 1];
    if (w0 && w1) {
        if (T.sc >= kStackSize) {
            T.overflow = true;
            end_as_miss(T);
            return;
        }
        const bool swap = b0 > b1;   // near child first, a tie goes left
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

// The 8 words of entry (id, at): tri_point of its triangle reference record again, the words the
// single answer carries; a miss (id < 0) is {-1, +inf, 0, 0, 0, 0, 0, 0}.
template <class Scene>
CLOSEST_HD void entry_words(int32_t eid, int32_t at, const V3& q, const Scene& S, uint32_t w[8]) {
    union { float f; uint32_t u; } c;
    w[0] = 0xFFFFFFFFu;
    c.f = kInf; w[1] = c.u;
    w[2] = w[3] = w[4] = w[5] = w[6] = w[7] = 0u;
    if (eid < 0) return;
    V3 p0, e1, e2;
    int32_t id;
    S.tri(at, p0, e1, e2, id);
    const TriPoint r = tri_point(q, p0, e1, e2);
    w[0] = (uint32_t)id;
    c.f = r.d2;  w[1] = c.u;
    c.f = r.u;   w[2] = c.u;
    c.f = r.v;   w[3] = c.u;
    c.f = r.p.x; w[4] = c.u;
    c.f = r.p.y; w[5] = c.u;
    c.f = r.p.z; w[6] = c.u;
}

}  // namespace closest
