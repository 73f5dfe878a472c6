// rt_kernel_body.inc -- traversal + per-pixel pipeline, compiled once per math
// mode by rt_render.hip (namespace RTK_NS, RTK_MATH; see rt_device_math.h).
// Uses the layouts, stack helpers and block epilogue of namespace rtk.
namespace RTK_NS {
using rtk::DevScene;
using rtk::Frame;
using rtk::Outputs;
using rtk::Stack;
using rtk::leaf_range;
using rtk::leaf_bytes;
using rtk::kLeafBit;
using rtk::kRefError;
using rtk::kStackSize;
using rtk::kTmin;
using rtk::kLdsStack;
using rtk::QRay;
using rtk::WQ;
using rtk::tile_epilogue;

// ---------------------------------------------------------------------------
// Slab test of both children of one inner record (ray_box, volumeRender.cl:612-624,
// applied as :863-867): quotients (box - o) / d.
//
// S_strict / S_hw: the IEEE quotient.  Fast form (Markstein; verified on 1e9 samples
// by scripts/verify_fastdiv.c): with y = RN(1/d), q = RN(a*y), r = fma(-q,d,a) is exact
// and fma(r,y,q) == RN(a/d) whenever 2^-64 <= |d| <= 2 and a == +-0 or
// 2^-90 <= |a| <= 2^61 (an exact zero may lose its sign: the slab test only compares).
//
// S_ref: the 2.5-ulp quotient ldexp(mant(a) * rcp(mant(d)), exp(a) - exp(d)).  With
// Y = ldexp(rcp(mant(d)), -exp(d)) (the ray's "1.0f/d" in that mode) this is exactly
// a * Y whenever Y is normal or infinite (d == +-0 or |d| >= 2^-126) and a * Y is not
// subnormal: both are RN(mant(a) * rcp(mant(d))) scaled by a power of two, and scaling
// commutes with rounding in the normal range; for d == +-0 both give +-inf, or NaN
// when a == +-0.  One multiply per plane.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float xdiv(float a, float d, float y) {
    const float q = a * y;
    const float r = __builtin_fmaf(-q, d, a);
    return __builtin_fmaf(r, y, q);
}
// Numerators are (box - o): when |o| and every box coordinate are 0 or in
// [2^-66, 2^60] (the box side is checked at upload -> S.fast_div, which also says that
// every child box has min <= max on every axis: the octant loops' precondition), both are
// multiples of 2^-89, so a non-zero difference is >= 2^-89 and <= 2^61.
__device__ __forceinline__ bool axis_ok(float o, float d) {
    const float ad = fabsf(d), ao = fabsf(o);
    const bool o_ok = ao == 0.0f || (ao >= 0x1p-66f && ao <= 0x1p60f);
    if (kMath == 2) return o_ok && (ad == 0.0f || ad >= 0x1p-126f);
    return ad == 0.0f || (ad >= 0x1p-64f && ad <= 2.0f && o_ok);
}
__device__ __forceinline__ bool fast_div_ok(const Ray& r) {
    return axis_ok(r.ori.x, r.dir.x) && axis_ok(r.ori.y, r.dir.y) && axis_ok(r.ori.z, r.dir.z);
}
// The per-ray reciprocal the slab test multiplies by: RN(1/d) (= the reference's
// inv_dir, volumeRender.cl:210) for the Markstein form, the 2.5-ulp rcp in S_ref.
__device__ __forceinline__ F3 slab_recip(const Ray& r) {
    if (kMath == 2) return F3{rcp_(r.dir.x), rcp_(r.dir.y), rcp_(r.dir.z)};
    return r.inv_dir;
}

// Record layout is axis-major (rt_render.hip): q0 = {L.min.x, R.min.x, L.max.x, R.max.x},
// q1 / q2 the same for y / z, so the fast path runs both children of an axis through one
// packed f32 op (v_pk_add/mul/fma_f32: two lanes' worth per issue, same IEEE rounding).
// o, d and y come as one half of a register pair, broadcast by op_sel (LLVM materialises
// such broadcasts as register copies, and 9 extra VGPRs spill); hence inline asm, one
// step per statement so the six (axis, plane) chains of a node issue stage by stage.
typedef float v2f __attribute__((ext_vector_type(2)));
// SB != 0: the box pair is wave-uniform and sits in SGPRs (the wave-uniform prologue's record, which
// the scalar cache delivered) and is read from there, with no copy of the record into VGPRs.
// SB 1: as the packed op's src0, an SGPR pair: one constant-bus operand, both halves read as a pair
// (scripts/micro/pk_sgpr.hip checks that on the GPU).  SB 2 (the depth-1 kernels): each value as src0
// of a plain v_sub_f32, the same IEEE result as the packed op's half, and pk_mulb's plain twin
// multiplies: 24 instructions for 12, and yet the faster form there (C3 0.2315 vs 0.2374 ms per frame,
// DESIGN.md 7.5); the other kernels gain scratch from it and keep the packed one.
template <int S, int SB = 0> __device__ __forceinline__ v2f pk_sub(v2f b, v2f O) {   // a = b - o
    v2f a;
    if (SB == 2) {
        const float o = S ? O.y : O.x;
        asm("v_sub_f32 %0, %1, %2" : "=v"(a.x) : "s"(b.x), "v"(o));
        asm("v_sub_f32 %0, %1, %2" : "=v"(a.y) : "s"(b.y), "v"(o));
        return a;
    }
    if (SB == 1) {
        if (S) asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(a) : "s"(b), "v"(O));
        else   asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(a) : "s"(b), "v"(O));
        return a;
    }
    if (S) asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(a) : "v"(b), "v"(O));
    else   asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(a) : "v"(b), "v"(O));
    return a;
}
template <int S, int SB = 0> __device__ __forceinline__ v2f pk_mulb(v2f a, v2f Y) {  // q = a * y
    v2f q;
    if (SB == 2) {
        const float y = S ? Y.y : Y.x;
        asm("v_mul_f32 %0, %1, %2" : "=v"(q.x) : "v"(a.x), "v"(y));
        asm("v_mul_f32 %0, %1, %2" : "=v"(q.y) : "v"(a.y), "v"(y));
        return q;
    }
    if (S) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(q) : "v"(a), "v"(Y));
    else   asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(q) : "v"(a), "v"(Y));
    return q;
}
template <int S> __device__ __forceinline__ v2f pk_res(v2f q, v2f D, v2f a) {  // r = fma(-q, d, a)
    v2f r;
    if (S) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(r) : "v"(q), "v"(D), "v"(a));
    else   asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(r) : "v"(q), "v"(D), "v"(a));
    return r;
}
template <int S> __device__ __forceinline__ v2f pk_cor(v2f r, v2f Y, v2f q) {  // fma(r, y, q)
    v2f o;
    if (S) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(o) : "v"(r), "v"(Y), "v"(q));
    else   asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(o) : "v"(r), "v"(Y), "v"(q));
    return o;
}
// Markstein with d == +-0: y = 1/d = +-inf and a * y is already the IEEE quotient a / d
// (+-inf, or NaN for a == +-0); the correction step would turn it into NaN (inf * 0).
__device__ __forceinline__ v2f pk_pick(bool dzero, v2f res, v2f q) {
    res.x = dzero ? q.x : res.x;
    res.y = dzero ? q.y : res.y;
    return res;
}
__device__ __forceinline__ float min_(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float max_(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float min3_(float a, float b, float c) {
    float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
}
__device__ __forceinline__ float max3_(float a, float b, float c) {
    float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
}
// The ray's o / d / y in 5 register pairs (10 VGPRs), each value used by op_sel.
struct RayPk {
    v2f oxy, ozdz, yxy, dxy, yz;
    bool zx, zy, zz;   // direction component == +-0
};
__device__ __forceinline__ RayPk ray_pk(const F3& o, const F3& d, const F3& y) {
    // Route the nine values through registers: built straight from the F3
    // members, LLVM turns the pairs into 8-byte loads of a stack copy of the ray.
    float ox = o.x, oy = o.y, oz = o.z, dx = d.x, dy = d.y, dz = d.z, yx = y.x, yy = y.y, yz = y.z;
    asm("" : "+v"(ox), "+v"(oy), "+v"(oz), "+v"(dx), "+v"(dy), "+v"(dz), "+v"(yx), "+v"(yy), "+v"(yz));
    return RayPk{v2f{ox, oy}, v2f{oz, dz}, v2f{yx, yy}, v2f{dx, dy}, v2f{yz, yz}, d.x == 0.0f, d.y == 0.0f,
                 d.z == 0.0f};
}
// OCT -1: near and far picked per lane by the min/max network.  OCT 0..7 (bit k set: direction
// component k is negative in every lane of the wave, and none is +-0; traverse_fast): near and far
// are known by name.  On an axis with box.min <= box.max (checked at upload -> S.fast_div) the
// subtraction of a common o and the multiplication by a common y -- or the correctly rounded
// quotient by a common d -- are monotone and give no NaN inside the fast quotient's domain, so
// d > 0 orders the two slab values as the box's planes and d < 0 the other way round: min(a, b) is
// a or b itself, and n and f are one v_max3 / v_min3 each, 4 VALU per visit instead of 16.  Which
// of two equal values comes out (+-0 included) may differ; everything downstream only compares.
template <bool ZERO = true, int OCT = -1, int SB = 0>
__device__ __forceinline__ void slab2_pk(const float4& q0, const float4& q1, const float4& q2, const RayPk& R,
                                         float& n0, float& f0, float& n1, float& f1) {
    // x: o, d, y = lo halves of R.oxy / R.dxy / R.yxy; y: the hi halves; z: lo / hi of R.ozdz, lo of R.yz
    const v2f a0 = pk_sub<0, SB>(v2f{q0.x, q0.y}, R.oxy), a1 = pk_sub<0, SB>(v2f{q0.z, q0.w}, R.oxy);
    const v2f a2 = pk_sub<1, SB>(v2f{q1.x, q1.y}, R.oxy), a3 = pk_sub<1, SB>(v2f{q1.z, q1.w}, R.oxy);
    const v2f a4 = pk_sub<0, SB>(v2f{q2.x, q2.y}, R.ozdz), a5 = pk_sub<0, SB>(v2f{q2.z, q2.w}, R.ozdz);
    const v2f m0 = pk_mulb<0, SB>(a0, R.yxy), m1 = pk_mulb<0, SB>(a1, R.yxy);
    const v2f m2 = pk_mulb<1, SB>(a2, R.yxy), m3 = pk_mulb<1, SB>(a3, R.yxy);
    const v2f m4 = pk_mulb<0, SB>(a4, R.yz), m5 = pk_mulb<0, SB>(a5, R.yz);
    v2f ax, bx, ay, by, az, bz;
    if (kMath == 2) {   // S_ref: a * Y is the quotient (see above)
        ax = m0; bx = m1; ay = m2; by = m3; az = m4; bz = m5;
    } else {
        const v2f r0 = pk_res<0>(m0, R.dxy, a0), r1 = pk_res<0>(m1, R.dxy, a1);
        const v2f r2 = pk_res<1>(m2, R.dxy, a2), r3 = pk_res<1>(m3, R.dxy, a3);
        const v2f r4 = pk_res<1>(m4, R.ozdz, a4), r5 = pk_res<1>(m5, R.ozdz, a5);
        ax = pk_cor<0>(r0, R.yxy, m0); bx = pk_cor<0>(r1, R.yxy, m1);
        ay = pk_cor<1>(r2, R.yxy, m2); by = pk_cor<1>(r3, R.yxy, m3);
        az = pk_cor<0>(r4, R.yz, m4); bz = pk_cor<0>(r5, R.yz, m5);
        if (ZERO) {
            ax = pk_pick(R.zx, ax, m0); bx = pk_pick(R.zx, bx, m1);
            ay = pk_pick(R.zy, ay, m2); by = pk_pick(R.zy, by, m3);
            az = pk_pick(R.zz, az, m4); bz = pk_pick(R.zz, bz, m5);
        }
    }
    if (OCT >= 0) {
        static_assert(OCT < 0 || !ZERO, "an octant loop has no zero direction component");
        const v2f nx = (OCT & 1) ? bx : ax, fx = (OCT & 1) ? ax : bx;
        const v2f ny = (OCT & 2) ? by : ay, fy = (OCT & 2) ? ay : by;
        const v2f nz = (OCT & 4) ? bz : az, fz = (OCT & 4) ? az : bz;
        n0 = max3_(nx.x, ny.x, nz.x);
        f0 = min3_(fx.x, fy.x, fz.x);
        n1 = max3_(nx.y, ny.y, nz.y);
        f1 = min3_(fx.y, fy.y, fz.y);
        return;
    }
    // v_min/v_max return the other operand for a NaN input, as fmin/fmax (a NaN only
    // arises for a zero direction component); the nesting is the reference's.  asm
    // keeps LLVM from canonicalising the asm results (12 extra v_max).
    n0 = max3_(min_(ax.x, bx.x), min_(ay.x, by.x), min_(az.x, bz.x));
    f0 = min3_(max_(ax.x, bx.x), max_(ay.x, by.x), max_(az.x, bz.x));
    n1 = max3_(min_(ax.y, bx.y), min_(ay.y, by.y), min_(az.y, bz.y));
    f1 = min3_(max_(ax.y, bx.y), max_(ay.y, by.y), max_(az.y, bz.y));
}
// Division form (any ray, any scene): the mode's `/` on every plane.
__device__ __forceinline__ void slab2_div(const float4& q0, const float4& q1, const float4& q2, const F3& o,
                                          const F3& d, float& n0, float& f0, float& n1, float& f1) {
    const v2f ax = v2f{div_(q0.x - o.x, d.x), div_(q0.y - o.x, d.x)}, bx = v2f{div_(q0.z - o.x, d.x), div_(q0.w - o.x, d.x)};
    const v2f ay = v2f{div_(q1.x - o.y, d.y), div_(q1.y - o.y, d.y)}, by = v2f{div_(q1.z - o.y, d.y), div_(q1.w - o.y, d.y)};
    const v2f az = v2f{div_(q2.x - o.z, d.z), div_(q2.y - o.z, d.z)}, bz = v2f{div_(q2.z - o.z, d.z), div_(q2.w - o.z, d.z)};
    n0 = fmaxf(fmaxf(fminf(ax.x, bx.x), fminf(ay.x, by.x)), fminf(az.x, bz.x));
    f0 = fminf(fminf(fmaxf(ax.x, bx.x), fmaxf(ay.x, by.x)), fmaxf(az.x, bz.x));
    n1 = fmaxf(fmaxf(fminf(ax.y, bx.y), fminf(ay.y, by.y)), fminf(az.y, bz.y));
    f1 = fminf(fminf(fmaxf(ax.y, bx.y), fmaxf(ay.y, by.y)), fmaxf(az.y, bz.y));
}

// ---------------------------------------------------------------------------
// General traversal: traverse_bvh (volumeRender.cl:658-1010), reference visit order,
// entry for entry, the full 65-entry stack (LDS, then global), malformed nodes, any
// quotient domain.  The reference stack is [0 .. sc-1] with entry sc-1 the node being
// visited (`cur`); entry sc-2 is kept in a register too (`nxt`), entries 0..sc-3 live
// in `st`.  Error, overflow and the any-hit early return end it by setting sc = 0.
// ---------------------------------------------------------------------------
struct Trav {
    uint32_t cur, nxt;
    int sc;        // reference stack_count; 0 = finished
    int result;    // tri_index (volumeRender.cl:780), 3 * triangle or -1
    float tHit;
};

template <bool CLOSEST>
__device__ __forceinline__ void trav_step(const DevScene& S, const Ray& ray, const F3& y, bool fast, Trav& T,
                                          const Stack& st, bool& overflow) {
    const F3 o = ray.ori, d = ray.dir;
    // descend through inner nodes until this lane sits on a leaf (while-while)
    while (T.sc > 0 && !(T.cur & kLeafBit)) {
        if (T.cur == kRefError) {  // volumeRender.cl:841,855-856
            T.result = -1;
            T.sc = 0;
            break;
        }
        const float4* np = S.wnodes + (size_t)T.cur * 4;
        const float4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
        float n0, f0, n1, f1;
        if (fast) slab2_pk<true>(q0, q1, q2, ray_pk(o, d, y), n0, f0, n1, f1);
        else slab2_div(q0, q1, q2, o, d, n0, f0, n1, f1);
        const bool i0 = (n0 <= f0) && (f0 >= kTmin) && (n0 <= T.tHit);
        const bool i1 = (n1 <= f1) && (f1 >= kTmin) && (n1 <= T.tHit);
        const uint32_t r0 = __float_as_uint(q3.x), r1 = __float_as_uint(q3.y);
        if (i0 && i1) {
            if (T.sc >= kStackSize) {  // volumeRender.cl:914
                overflow = true;
                T.result = -1;
                T.sc = 0;
                break;
            }
            const bool swap = n0 > n1;  // near child first, tie -> left (:901-906)
            if (T.sc >= 2) st.put(T.sc - 2, T.nxt);
            T.nxt = swap ? r0 : r1;
            T.cur = swap ? r1 : r0;
            ++T.sc;
        } else if (i0 || i1) {
            T.cur = i0 ? r0 : r1;
        } else {
            --T.sc;
            T.cur = T.nxt;
            if (T.sc >= 2) T.nxt = st.get(T.sc - 2);
        }
    }
    if (T.sc > 0) {
        // leaf: Moller-Trumbore over the leaf's references, in order (:965-997)
        int off, cnt;
        leaf_range(S, T.cur, off, cnt);
        bool stop = false;
        for (int i = 0; i < cnt; ++i) {
            const float4* tp = tri_rec(S, off + i);
            const float4 a0 = tp[0], a1 = tp[1], a2 = tp[2];
            const F3 e2 = F3{a2.x, a2.y, a2.z};
            const float t = ray_tri(ray, F3{a0.x, a0.y, a0.z}, F3{a1.x, a1.y, a1.z}, e2);
            if (t < T.tHit && t > kTmin) {
                T.tHit = t;
                T.result = __float_as_int(a0.w);
                if (!CLOSEST) { stop = true; break; }  // any-hit: first hit returns (:986)
            }
        }
        if (stop) {
            T.sc = 0;
        } else {
            --T.sc;
            T.cur = T.nxt;
            if (T.sc >= 2) T.nxt = st.get(T.sc - 2);
        }
    }
}

template <bool CLOSEST>
__device__ int traverse(const DevScene& S, const Ray& ray, float& tHit, const Stack& st, bool& overflow) {
    Trav T;
    T.cur = S.root;
    T.nxt = 0;
    T.sc = 1;
    T.result = -1;
    T.tHit = tHit;
    const bool fast = S.fast_div && fast_div_ok(ray);
    const F3 y = slab_recip(ray);
    do {
        trav_step<CLOSEST>(S, ray, y, fast, T, st, overflow);
    } while (T.sc > 0);
    tHit = T.tHit;
    return T.result;
}

// ---------------------------------------------------------------------------
// Fast traversal (clean scenes, stack within the LDS part).
//
// Lane-independent ("if-if") steps: every iteration each lane takes ONE step of its
// own reference sequence -- an inner visit, or one triangle of the leaf it sits on --
// instead of while-while rounds in which the whole wave descends until every lane
// has reached a leaf.  Each lane's sequence of visits, tests and stack operations is
// exactly the reference's (only the interleaving of lanes in time changes), so results
// are bit-identical; the wave runs max over lanes of (visits + tests) iterations
// (DESIGN.md 6.2).  One fetch per lane per iteration into shared registers: the inner
// record of `cur` (48 B of child boxes + 8 B of child refs), or triangle record `tk`.
//
// Stack entries 0..sc-3 live in this lane's LDS column, so slot sc-2 is always free:
// every inner visit writes `nxt` there unconditionally (a push keeps it) and reads slot
// sc-3 (what a pop needs) before it knows whether it pops; push / advance / pop are
// selects.  The stack count travels as `sb` = kStackBase + (sc - 1) * 256: slot sc - 3 is
// that many bytes (less kStackBase) above the column's lowest guard row (rtk::kLdsGuard), the
// read is at that address, the write 256 B above it, a push or pop moves sb by 256, and no
// address is clamped.  A lane is in the loop while (int)sb >= kStackBase.  kStackBase is
// chosen so that the push to sc = kLdsStack + 2, the first stack deeper than the LDS part,
// carries sb into the sign bit: the lane leaves the loop by the loop's own compare, before
// any row past its column is touched, and sb < 0 afterwards says that the caller must restart
// the ray with the general traversal (same result).  A pop from sc = 1 and kStackDone (an
// any-hit's first hit) leave it with 0 <= sb < kStackBase.
// MODE 0: packed fast quotient; 1: + Markstein's zero-direction select (S_strict / S_hw
// only); 2: the division form (a ray outside the fast quotient's domain).
// ---------------------------------------------------------------------------
constexpr bool kOctLoops = kMath == 2;
constexpr uint32_t kStackBase = 0x80000000u - (uint32_t)(kLdsStack + 1) * 256u, kStackDone = 0u;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ uint32_t lds_get(int a) { return *(lds_u32*)(uintptr_t)(uint32_t)a; }
__device__ __forceinline__ void lds_put(int a, uint32_t v) { *(lds_u32*)(uintptr_t)(uint32_t)a = v; }
// The LDS addresses of slot sc - 3 (read) and slot sc - 2 (written) of the column whose entry 0 is at
// col0.  GUARD: the column has its guard rows.  A kernel whose LDS has no room for them (the fused
// kernel: 7 blocks per CU with its parked rays) clamps both to entry 0, as every kernel once did.
template <bool GUARD> __device__ __forceinline__ int slot_get(int col0, uint32_t sb) {
    return GUARD ? (int)((uint32_t)col0 - (kStackBase + rtk::kLdsGuard * 256u) + sb)
                 : col0 + max((int)(sb - kStackBase) - 512, 0);
}
template <bool GUARD> __device__ __forceinline__ int slot_put(int get_at, int col0, uint32_t sb) {
    return GUARD ? get_at + 256 : col0 + max((int)(sb - kStackBase) - 256, 0);
}

// put_at: the LDS address of slot sc - 2.  SB: the record is wave-uniform, in SGPRs (pk_sub).
template <int MODE, int OCT = -1, int SB = 0>
__device__ __forceinline__ void inner_step(const float4& q0, const float4& q1, const float4& q2, float2 refs,
                                           const RayPk& rp, float th, uint32_t popped, int put_at,
                                           uint32_t& cur, uint32_t& nxt, uint32_t& sb) {
    float n0, f0, n1, f1;
    if (MODE == 2) {
        slab2_div(q0, q1, q2, F3{rp.oxy.x, rp.oxy.y, rp.ozdz.x}, F3{rp.dxy.x, rp.dxy.y, rp.ozdz.y}, n0, f0, n1, f1);
    } else {
        slab2_pk<MODE == 1, MODE == 0 ? OCT : -1, SB>(q0, q1, q2, rp, n0, f0, n1, f1);
    }
    // (n <= f) && (n <= th) == n <= min(f, th) for every input: th is a finite hit distance, and n
    // and f are NaN together or not at all (per axis the NaN-ignoring min and max of the two slab
    // values are NaN only when both are; n and f compose those with NaN-ignoring max and min), and
    // a NaN n fails both forms.  (Three compares and two mask ANDs instead: C3 0.2978 vs 0.2914 ms,
    // DESIGN.md 7.5.)
    const bool i0 = (n0 <= min_(f0, th)) && (f0 >= kTmin);
    const bool i1 = (n1 <= min_(f1, th)) && (f1 >= kTmin);
    const uint32_t r0 = __float_as_uint(refs.x), r1 = __float_as_uint(refs.y);
    lds_put(put_at, nxt);
    const bool both = i0 && i1, none = !i0 && !i1;
    const bool swap = n0 > n1;  // near child first, tie -> left (:901-906)
    const uint32_t nearr = swap ? r1 : r0, farr = swap ? r0 : r1, one = i0 ? r0 : r1;
    const uint32_t ncur = both ? nearr : (none ? nxt : one);
    nxt = both ? farr : (none ? popped : nxt);
    cur = ncur;
    sb += (both ? 256u : 0u) - (none ? 256u : 0u);
}

// The ray travels in RayPk's registers only: its origin and direction are rebuilt from
// them for the triangle tests and on return (same values), so the caller's copy is dead
// during the loop (-9 VGPRs).
__device__ __forceinline__ Ray ray_of(const RayPk& rp, const F3& inv) {
    Ray r;
    r.ori = F3{rp.oxy.x, rp.oxy.y, rp.ozdz.x};
    r.dir = F3{rp.dxy.x, rp.dxy.y, rp.ozdz.y};
    r.inv_dir = inv;
    return r;
}

// record loads of the fast traversal: raw buffer loads at a byte offset from one descriptor
// (0x00020000: the gfx9 dword 3 of a raw buffer; out-of-range offsets read 0, never fault)
__device__ __forceinline__ float4 rec_load4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}
__device__ __forceinline__ float2 rec_load2(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
    return make_float2(__uint_as_float(v[0]), __uint_as_float(v[1]));
}

// CUR (the depth-1 kernels on a scene with walk references, DESIGN.md 7.2): `cur` is a walk reference
// (rt_records.h) and itself the leaf cursor.  Its unit offset << 4 is the byte offset of the record the trip reads,
// an inner record or the leaf's next triangle record, so the three record loads have no select, no
// decode and no exec region in front of them, and tk, tend and tri_off are gone; an inner lane's two
// child references come from the walk array, 8 B at walk_off + (cur << 1).  A leaf lane steps to its
// next record by one add (kWalkNext: three units on, one reference fewer) and pops after the record
// whose count field is 0.  An empty leaf is one trip on the all-zero pad record, which cannot hit by
// arithmetic alone in any mode: e1 = e2 = 0 give det = 0, its reciprocal inf, u = 0 * inf = NaN and
// so t = NaN, and t < th is false (tests/test_walk_cursor_gpu.py).  Every lane's visits, tests,
// stack operations and fetches are those of the other form, but for the record an empty leaf's one
// trip reads: the pad record here, the record its reference names (triangle record 0) there.
template <bool CLOSEST, int MODE, int TR, bool SEL = false, bool GUARD = true, int OCT = -1, bool CUR = false>
__device__ __forceinline__ bool traverse_ifif(const DevScene& S, Ray& ray_io, float& tHit, const Stack& st,
                                              int& result) {
    static_assert(!CUR || SEL, "the cursor loop is the depth-1 kernels'");
    // The trimmed trip (DESIGN.md 7.2) is the depth-1 kernels' (SEL): the uniform prologue loop and the
    // lean main-loop head (kLean: offset select next to the leaf compare, child refs loaded inside the
    // inner step's region), the slab test on scalar operands (kScalarBox 2) and the shift-add decode
    // (kShiftDecode).  The wavefront and query kernels keep the earlier forms of
    // all of them: they run slower with the lean head (C5 0.738 vs 0.703 ms per frame) and gain scratch
    // from every partial combination.  The fused kernel (GUARD false: 7 waves' registers, already in
    // scratch) takes the scalar box operands in their packed form and the decode, with which it loses
    // 4 B of scratch; the uniform loop or the lean head cost it 4 B.
    constexpr bool kLean = SEL, kShiftDecode = SEL || !GUARD;
    constexpr int kScalarBox = MODE == 2 ? 0 : SEL ? 2 : GUARD ? 0 : 1;   // pk_sub's SB
    const int col0 = (int)(uint32_t)(uintptr_t)(lds_u32*)st.lds;   // the column's entry 0, as an LDS byte address
    const RayPk rp = ray_pk(ray_io.ori, ray_io.dir, slab_recip(ray_io));
    // the packed reciprocal goes back as inv_dir: RN(1/d) itself in S_strict / S_hw, the
    // 2.5-ulp one in S_ref (after a traversal callers use only ori and dir, and the
    // general traversal recomputes slab_recip)
    const F3 inv_keep = F3{rp.yxy.x, rp.yxy.y, rp.yz.x};
    uint32_t cur = CUR ? st.walk.root : S.root, nxt = 0;
    uint32_t sb = kStackBase;   // sc = 1
    int res = -1;
    float th = tHit;
    // leaf state as byte offsets into the record allocation: the next triangle record and
    // the end of the leaf's range (no per-iteration multiply; < 2^31 by record_limit).
    // tk >= tend whenever the lane is not inside a leaf: a leaf `cur` with tk >= tend is one
    // the lane has just arrived at, and the main loop decodes it at the top of its next trip,
    // the one place that does (the root, a child, or what a pop brought back).
    uint32_t tk = 0, tend = 0;
    // The decode's one scene field.  The depth-1 kernels (SEL) hold it in a VGPR through the loops: as
    // one of the scene's SGPRs it is spilled around them and comes back by v_readlane_b32, its whole
    // four-register tuple, on every arrival.
    // CUR: the walk array's byte offset takes its place, the inner step's one scene field.
    uint32_t tri_off = CUR ? st.walk.off : S.tri_off;
    if (SEL && kOctLoops) asm("" : "+v"(tri_off));
    // inner and triangle records share one allocation: buffer loads at a 32-bit byte offset
    // from one descriptor (no 64-bit address arithmetic per iteration)
    const __amdgpu_buffer_rsrc_t recs =
        __builtin_amdgcn_make_buffer_rsrc((void*)S.wnodes, (short)0, (int)S.rec_bytes, 0x00020000);
    // Wave-uniform prologue: while every lane still in the loop sits on the same inner node
    // (the top of the tree, for a tile's coherent rays), that record is read once for the
    // wave through the scalar cache (uniform address, constant address space) instead of
    // by every quad through the vector-memory path.  Each lane's step is the same
    // inner_step as below; the first iteration whose nodes differ (or reach a leaf) hands
    // the unchanged per-lane state to the main loop.
    typedef unsigned int su4 __attribute__((ext_vector_type(4)));
    typedef unsigned int su2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(4))) su4 csu4;
    typedef const __attribute__((address_space(4))) su2 csu2;
    if (TR == 2 && CLOSEST) rtk::timeline_mark(st.fc, 6);   // the closest-hit traversal starts
    // One prologue step of the lanes in exec, all on inner node c0: the record comes in SGPRs and
    // the slab test reads it from there (pk_sub's SB; the division form is plain C++).
    const auto uniform_step = [&](uint32_t c0) __attribute__((always_inline)) {
        const int at = slot_get<GUARD>(col0, sb);
        const uint32_t popped = lds_get(at);
        if (TR == 1) rtk::fetch_count(st.fc, false, CUR ? cur >> 2 : cur, false);
        if (TR == 2) rtk::timeline_step(st.fc, CLOSEST ? 1 : 3);
        csu4* rec = (csu4*)((const char*)S.wnodes + ((size_t)c0 << (CUR ? 4 : 6)));
        const su4 u0 = rec[0], u1 = rec[1], u2 = rec[2];
        // CUR: the two walk references, one more scalar load (both offsets are below 2^31)
        const su2 u3 = CUR ? *(csu2*)((const char*)S.wnodes + (size_t)(st.walk.off + (c0 << 1))) : *(csu2*)(rec + 3);
        const float4 q0 = make_float4(__uint_as_float(u0.x), __uint_as_float(u0.y), __uint_as_float(u0.z), __uint_as_float(u0.w));
        const float4 q1 = make_float4(__uint_as_float(u1.x), __uint_as_float(u1.y), __uint_as_float(u1.z), __uint_as_float(u1.w));
        const float4 q2 = make_float4(__uint_as_float(u2.x), __uint_as_float(u2.y), __uint_as_float(u2.z), __uint_as_float(u2.w));
        const float2 q3 = make_float2(__uint_as_float(u3.x), __uint_as_float(u3.y));
        inner_step<MODE, OCT, kScalarBox>(q0, q1, q2, q3, rp, th, popped, slot_put<GUARD>(at, col0, sb), cur, nxt, sb);
    };
    if (kLean) {
        // The loop itself is wave-uniform (scalar branches only): a per-lane loop condition makes the
        // compiler fold every exit, the uniform ones too, into exec-mask arithmetic on every trip.
        // Lanes that have finished (they never come back) sit out the step's one exec region; c0 is
        // the node of the first lane still in the loop, and one compare serves both exit tests: with
        // its leaf bit cleared a leaf c0 differs from that lane's own `cur`.
        for (;;) {
            const bool live = (int)sb >= (int)kStackBase;
            const uint64_t lm = __builtin_amdgcn_ballot_w64(live);
            if (lm == 0) break;
            const uint32_t c0 = __builtin_amdgcn_readlane(cur, __builtin_ctzll(lm));
            if ((__builtin_amdgcn_ballot_w64(cur != (c0 & ~kLeafBit)) & lm) != 0) break;
            // (keeps the compiler from merging the uniform exit with the per-lane condition below
            // into one divergent branch, which brings the mask arithmetic back)
            asm volatile("");
            if (live) uniform_step(c0);
        }
    } else {
        while ((int)sb >= (int)kStackBase) {
            const uint32_t c0 = __builtin_amdgcn_readfirstlane(cur);
            if (__builtin_amdgcn_ballot_w64(cur != c0) != 0 || (c0 & kLeafBit)) break;
            uniform_step(c0);
        }
    }
    if (TR == 2 && CLOSEST) rtk::timeline_mark(st.fc, 7);   // its wave-uniform prologue is over
    while (CUR && (int)sb >= (int)kStackBase) {
        const bool leaf = (int)cur < 0;
        // (a bare cur << 4 would keep the count field's lowest bit, bit 27, as bit 31 of the offset)
        const uint32_t off = (cur & rtrec::kWalkUnitMask) << 4;
        const int at = slot_get<GUARD>(col0, sb);
        const uint32_t popped = lds_get(at);
        // (counting key of an empty leaf's trip: the other form reads, and keys, the record its reference
        // names, triangle record 0 in every encoding of this library (scene_encode.cpp writes an empty
        // leaf with offset 0), where this one reads the pad record, 48 B below the walk array)
        if (TR == 1) rtk::fetch_count(st.fc, leaf, leaf ? (0x80000000u | (off == tri_off - 48u ? S.tri_off : off)) : cur >> 2);
        if (TR == 2) rtk::timeline_step(st.fc, CLOSEST ? 0 : 2);
        uint32_t t_issue = 0;
        if (TR == 2 && RTK_TL_SPLIT) t_issue = (uint32_t)__builtin_amdgcn_s_memrealtime();
        const float4 q0 = rec_load4(recs, off), q1 = rec_load4(recs, off + 16u), q2 = rec_load4(recs, off + 32u);
        // the child refs: as below, the first instruction of the inner step's region (the timeline's
        // split diagnostic: right after the boxes)
        constexpr bool kRefsEarly = TR == 2 && RTK_TL_SPLIT;
        float2 q3;
        if (kRefsEarly) {
            q3 = make_float2(0.0f, 0.0f);
            if (!leaf) q3 = rec_load2(recs, tri_off + (cur << 1));
            asm volatile("" ::: "memory");
            asm volatile("" ::"v"(q0.x), "v"(q1.x), "v"(q2.x), "v"(q3.x));
            rtk::timeline_wait(st.fc, CLOSEST ? 0 : 1, (uint32_t)__builtin_amdgcn_s_memrealtime() - t_issue);
        }
        if (!leaf) {
            if (!kRefsEarly) {
                q3 = rec_load2(recs, tri_off + (cur << 1));
                __builtin_amdgcn_sched_barrier(0);
            }
            inner_step<MODE, OCT>(q0, q1, q2, q3, rp, th, popped, slot_put<GUARD>(at, col0, sb), cur, nxt, sb);
        } else {
            const F3 e2 = F3{q2.x, q2.y, q2.z};
            const float t = ray_tri(ray_of(rp, inv_keep), F3{q0.x, q0.y, q0.z}, F3{q1.x, q1.y, q1.z}, e2);
            const bool hit = t < th && t > kTmin;
            th = hit ? t : th;
            res = hit ? __float_as_int(q0.w) : res;
            const bool pop = cur < rtrec::kWalkLastBelow;   // count field 0: this was the leaf's last record
            cur = pop ? nxt : cur + rtrec::kWalkNext;
            nxt = pop ? popped : nxt;
            sb -= pop ? 256u : 0u;
            if (!CLOSEST) sb = hit ? kStackDone : sb;   // any-hit: first hit returns (:986)
        }
    }
    while (!CUR && (int)sb >= (int)kStackBase) {
        const bool leaf = (cur & kLeafBit) != 0;
        // SEL (the depth-1 kernel): a select between the two byte offsets, so the loads issue
        // without an exec-masked branch in front of them (C3 -1.4 %, C4 -1.6 %; the wavefront
        // kernels are faster with the branch, C5 +1.2 %: DESIGN.md 6.2).  tk is already a
        // byte offset: no multiply (a 24-bit one here was wrong from 2^24 records on).
        // The select stands next to the leaf compare, whose mask it then reads as it is (a ballot
        // in a later block is rebuilt from a 0 / 1 VGPR: two VALU more on the way to the loads); a
        // lane that arrives on its leaf takes the offset from the decode instead.
        uint32_t off = 0;
        const auto select_off = [&]() __attribute__((always_inline)) {
            if (SEL) {
                asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(off) : "v"(cur << 6), "v"(tk), "s"(__builtin_amdgcn_ballot_w64(leaf)));
            } else {
                off = leaf ? tk : cur << 6;
            }
        };
        if (kLean) select_off();
        if (leaf && tk >= tend) {
            leaf_bytes<kShiftDecode>(S, tri_off, cur, tk, tend);
            off = tk;
        }
        if (!kLean) select_off();
        const int at = slot_get<GUARD>(col0, sb);
        const uint32_t popped = lds_get(at);
        // TR 1 (measurement instantiation only, rt_fetch_counts): this iteration's fetches counted;
        // TR 2 (rt_wave_timeline): the wave's loop trips counted
        if (TR == 1) rtk::fetch_count(st.fc, leaf, leaf ? (0x80000000u | tk) : cur);
        if (TR == 2) rtk::timeline_step(st.fc, CLOSEST ? 0 : 2);
        uint32_t t_issue = 0;
        if (TR == 2 && RTK_TL_SPLIT) t_issue = (uint32_t)__builtin_amdgcn_s_memrealtime();
        const float4 q0 = rec_load4(recs, off), q1 = rec_load4(recs, off + 16u), q2 = rec_load4(recs, off + 32u);
        // The child refs are loaded by the inner lanes only, as the first instruction of the inner
        // step's exec region, which precedes the triangle step in program order: in a mixed
        // iteration the load is out before any wait of that trip (one round trip per trip; the
        // scheduling barrier keeps it in front of the slab test's first wait).  Leaf lanes never
        // read q3.  The earlier form (every kernel without SEL; the timeline's split diagnostic, which waits
        // for all four loads before either step): a masked load in a region of its own right after the
        // boxes, and a barrier that keeps the compiler from sinking it behind the triangle lanes' wait.
        constexpr bool kRefsEarly = (TR == 2 && RTK_TL_SPLIT) || !kLean;
        float2 q3;
        if (kRefsEarly) {
            q3 = make_float2(0.0f, 0.0f);
            if (!leaf) q3 = rec_load2(recs, off + 48u);
            asm volatile("" ::: "memory");
        }
        if (TR == 2 && RTK_TL_SPLIT) {   // diagnostic: the trip's memory wait (all four loads in)
            asm volatile("" ::"v"(q0.x), "v"(q1.x), "v"(q2.x), "v"(q3.x));
            rtk::timeline_wait(st.fc, CLOSEST ? 0 : 1, (uint32_t)__builtin_amdgcn_s_memrealtime() - t_issue);
        }
        if (!leaf) {
            if (!kRefsEarly) {
                q3 = rec_load2(recs, off + 48u);
                __builtin_amdgcn_sched_barrier(0);
            }
            inner_step<MODE, OCT>(q0, q1, q2, q3, rp, th, popped, slot_put<GUARD>(at, col0, sb), cur, nxt, sb);
        } else {
            // Moller-Trumbore on one reference of the leaf, in order (:965-997).  An empty leaf
            // (tk == tend) tests the record after its range (in the allocation, or zeros) and
            // drops the result.  Hit, advance and pop are selects: one block of bookkeeping.
            const F3 e2 = F3{q2.x, q2.y, q2.z};
            const float t = ray_tri(ray_of(rp, inv_keep), F3{q0.x, q0.y, q0.z}, F3{q1.x, q1.y, q1.z}, e2);
            const bool hit = t < th && t > kTmin && tk < tend;
            th = hit ? t : th;
            res = hit ? __float_as_int(q0.w) : res;
            tk += 48u;
            const bool pop = tk >= tend;   // leaf done
            cur = pop ? nxt : cur;
            nxt = pop ? popped : nxt;
            sb -= pop ? 256u : 0u;
            if (!CLOSEST) sb = hit ? kStackDone : sb;   // any-hit: first hit returns (:986)
        }
    }
    tHit = th;
    result = res;
    ray_io = ray_of(rp, inv_keep);
    return (int)sb >= 0;
}

// Markstein's zero-direction select costs 12 VALU per visit and is needed by ~1e-5 of
// rays, the division form by fewer still: a wave runs those variants only when one of
// its rays needs them (wave-uniform branch, one code copy each).
//
// Octant loops (slab2_pk's OCT): when no active lane has a zero direction component and each
// component's sign is the same in all of them -- an 8x8 tile's primary rays, or its shadow rays
// toward the one light, unless the tile straddles a zero of a component -- the wave runs the copy
// of the MODE 0 loop compiled for that octant, 12 VALU per inner visit shorter.  The choice is
// made here, once per traversal, by ballots over the active lanes; the loops themselves gain
// nothing.  Every other wave runs the generic MODE 0 loop, as before.
// OCTS: the kernel has the octant loops.  Those are S_ref's depth-1 kernels (kOctLoops and SEL:
// first_bounce_kernel and first_bounce_batch_kernel without NEXT), which stay within 64 VGPRs with no
// scratch.  With nine copies of the loop the register allocator gave every other kernel more
// scratch than it has (S_strict / S_hw first-bounce 0 -> 8 B, S_hw render_kernel 104 -> 120 B, S_ref
// render_kernel 28 -> 40 B, wf_bounce_kernel 24 -> 32 B, the depth > 1 batch kernel 0 -> 8 B), so
// they keep the generic loop alone.
// TR 1 (rt_loop_variant_counts): the loop a wave's traversal took, counted in st.vc[0] (generic;
// MODE 1 and 2 too) or st.vc[1 + octant], closest-hit traversals first, any-hit ones 9 further.
template <bool CLOSEST, int TR>
__device__ __forceinline__ void variant_count(const Stack& st, int which) {
    if (TR == 1 && (uint32_t)(threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec()))
        atomicAdd(st.vc + (CLOSEST ? 0 : 9) + which, 1ull);
}
// WALK: the traversal runs the cursor loop (traverse_ifif's CUR): the depth-1 kernels launched for a
// scene with walk references.  The host picks those instantiations, product, counting and timeline
// alike; a scene without walk references gets the ones without WALK.
template <bool CLOSEST, int TR, bool SEL = false, bool GUARD = true, bool OCTS = false, bool WALK = false>
__device__ __forceinline__ bool traverse_fast(const DevScene& S, Ray& ray, float& tHit, const Stack& st,
                                              int& result) {
    if (!S.fast_div || __builtin_amdgcn_ballot_w64(!fast_div_ok(ray))) {
        variant_count<CLOSEST, TR>(st, 0);
        return traverse_ifif<CLOSEST, 2, TR, SEL, GUARD, -1, WALK>(S, ray, tHit, st, result);
    }
    if (kMath != 2) {
        const bool z = ray.dir.x == 0.0f || ray.dir.y == 0.0f || ray.dir.z == 0.0f;
        if (__builtin_amdgcn_ballot_w64(z)) {
            variant_count<CLOSEST, TR>(st, 0);
            return traverse_ifif<CLOSEST, 1, TR, SEL, GUARD, -1, WALK>(S, ray, tHit, st, result);
        }
    }
    if (OCTS) {
        // S_ref's MODE 0 also serves zero components (see slab2_pk), hence the zero test here; no lane
        // has a NaN (fast_div_ok), so d < 0 is the sign bit of a non-zero d
        const bool z = ray.dir.x == 0.0f || ray.dir.y == 0.0f || ray.dir.z == 0.0f;
        const uint64_t act = __builtin_amdgcn_read_exec();
        const uint64_t sx = __builtin_amdgcn_ballot_w64(ray.dir.x < 0.0f), sy = __builtin_amdgcn_ballot_w64(ray.dir.y < 0.0f),
                       sz = __builtin_amdgcn_ballot_w64(ray.dir.z < 0.0f);
        const bool uniform = (sx == 0 || sx == act) && (sy == 0 || sy == act) && (sz == 0 || sz == act);
        const int oct = (sx ? 1 : 0) | (sy ? 2 : 0) | (sz ? 4 : 0);
        if (__builtin_amdgcn_ballot_w64(z) == 0 && uniform) {
            variant_count<CLOSEST, TR>(st, 1 + oct);
            switch (oct) {
                case 0: return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, 0, WALK>(S, ray, tHit, st, result);
                case 1: return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, 1, WALK>(S, ray, tHit, st, result);
                case 2: return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, 2, WALK>(S, ray, tHit, st, result);
                case 3: return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, 3, WALK>(S, ray, tHit, st, result);
                case 4: return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, 4, WALK>(S, ray, tHit, st, result);
                case 5: return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, 5, WALK>(S, ray, tHit, st, result);
                case 6: return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, 6, WALK>(S, ray, tHit, st, result);
                default: return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, 7, WALK>(S, ray, tHit, st, result);
            }
        }
    }
    variant_count<CLOSEST, TR>(st, 0);
    return traverse_ifif<CLOSEST, 0, TR, SEL, GUARD, -1, WALK>(S, ray, tHit, st, result);
}

// Closest-hit / any-hit of one ray: the fast traversal, restarted with the general
// code when its stack outgrows the LDS part (counted in O.restarts).  t_restart: what t was on
// entry, which the restart begins from again (a frame's rays: HitRecordInit's constant; a query's
// ray: its own tmax).
template <bool CLOSEST, bool FASTONLY, int TR = 0, bool SEL = false, bool GUARD = true, bool OCTS = false, bool WALK = false>
__device__ __forceinline__ int trace(const DevScene& S, const Outputs& O, Ray& ray, float& t, const Stack& st,
                                     bool& overflow, float t_restart = 4294967296.0f) {
    int hit;
    if (FASTONLY) {
        if (traverse_fast<CLOSEST, TR, SEL, GUARD, OCTS, WALK>(S, ray, t, st, hit)) return hit;
        atomicAdd(O.restarts, 1u);
        t = t_restart;
    }
    return traverse<CLOSEST>(S, ray, t, st, overflow);
}

// ---- per-pixel pieces shared by the fused and the wavefront kernels ----

// volumeRender.cl:1169-1190: image-plane point, ray from it away from the eye
__device__ __forceinline__ Ray primary_ray(const Frame& F, uint32_t x, uint32_t y) {
    const float xf = (float)(((double)x - 0.5) / (double)(float)F.w);
    const float yf = (float)(((double)y - 0.5) / (double)(float)F.h);
    const F3 a = F3{F.a.x, F.a.y, F.a.z}, b = F3{F.b.x, F.b.y, F.b.z}, c = F3{F.c.x, F.c.y, F.c.z};
    const F3 campos = F3{F.campos.x, F.campos.y, F.campos.z};
    const F3 t1 = mad3(a, xf, c);   // c + (a * xf)
    const F3 t2 = b * yf;
    const F3 image_pos = t1 + t2;
    return ray_init(image_pos, image_pos - campos);
}

__device__ __forceinline__ bool scene_box_hit(const Frame& F, const Ray& r) {
    return ray_box_scene(F3{F.smin.x, F.smin.y, F.smin.z}, F3{F.smax.x, F.smax.y, F.smax.z}, r.ori, r.inv_dir);
}

// volumeRender.cl:1306-1403 (shading at a closest hit) -> colour term, hit point, normal, light dir
__device__ __forceinline__ void shade_hit(const DevScene& S, const Frame& F, const Ray& ray, float tHit, int hit,
                                          F3& rez, F3& hitpoint, F3& normal, F3& L) {
    const F3 light_pos = F3{F.light_pos.x, F.light_pos.y, F.light_pos.z};
    const float4* sp = S.shade + (size_t)(hit / 3) * 7;
    const float4 p0 = sp[0], p1 = sp[1], p2 = sp[2], m0 = sp[3], m1 = sp[4], m2 = sp[5], alb = sp[6];
    const F3 vNew = mad3(ray.dir, tHit - 0.001f, ray.ori);   // r.ori + r.dir * (t - 0.001f)
    normal = normalize(normal_at(vNew, xyz(p0), xyz(p1), xyz(p2), xyz(m0), xyz(m1), xyz(m2)));
    const F3 l1 = normalize(light_pos - vNew);
    const F3 v = normalize(ray.ori - vNew);
    const F3 n = normalize(normal);
    const F3 albedo = xyz(alb);
    const float f0 = 40.0f * (1.0f / 255.0f);
    rez = cook_torrance_ggx(n, l1, v, albedo, f0, 0.5f) * 3.0f;
    rez = rez + F3{0.3f, 0.3f, 0.3f} * albedo;   // ambient_color: its own statement (:1402-1403)
    hitpoint = vNew;
    L = normalize(light_pos - hitpoint);
}

// volumeRender.cl:1519-1546
__device__ __forceinline__ F3 finish_color(F3 color, float shadow_sum, int ray_depth) {
    if (ray_depth >= 1) {
        const float dd = (float)ray_depth;
        color = F3{div_(color.x, dd), div_(color.y, dd), div_(color.z, dd)};
        shadow_sum = div_(shadow_sum, dd);
        return color * shadow_sum;
    }
    return F3{0, 0, 0};
}

// Next bounce's ray (volumeRender.cl:1493-1498), parked in LDS `next` ({o, d}, stride 64).
__device__ __forceinline__ void park_next(const F3& dir, const F3& normal, const F3& hitpoint, float* next) {
    const F3 refl = reflect(dir, normal);
    const F3 no = mad3(refl, 0.001f, hitpoint);   // hitpoint + refl * 0.001f
    next[0] = no.x; next[64] = no.y; next[128] = no.z;
    next[192] = refl.x; next[256] = refl.y; next[320] = refl.z;
}

// Shadow ray from a hit (volumeRender.cl:1437-1460): any-hit, shadowed iff hit && t > 0.025.
template <bool FASTONLY, int TR = 0, bool SEL = false, bool GUARD = true, bool OCTS = false, bool WALK = false>
__device__ __forceinline__ float shadow_coef(const DevScene& S, const Outputs& O, const F3& hitpoint, const F3& L,
                                             const Stack& st, bool& overflow, int& sh) {
    Ray sray = ray_init(mad3(L, 0.001f, hitpoint), L);   // hitpoint + L * 0.001f
    float ts = 4294967296.0f;
    sh = trace<false, FASTONLY, TR, SEL, GUARD, OCTS, WALK>(S, O, sray, ts, st, overflow);
    return (sh >= 0 && ts > 0.025f) ? 0.25f : 1.0f;
}

// ============================================================================
// Fused kernel (depth > 1 without RT_FLAG_WAVEFRONT): one lane = one pixel, the
// whole pipeline (volumeRender.cl:1164-1546) in one pass.
// ============================================================================
template <bool FASTONLY>
__device__ __forceinline__ void render_pixel(const DevScene& S, const Frame& F, const Outputs& O, int want_aux,
                                             uint32_t x, uint32_t y, uint32_t pix, const Stack& st, float* next) {
    bool overflow = false;
    const int depth = F.depth;
    Ray ray = primary_ray(F, x, y);
    if (want_aux) {
        for (int k = 0; k < depth; ++k) {
            O.hits[((size_t)pix * depth + k) * 2 + 0] = -2;
            O.hits[((size_t)pix * depth + k) * 2 + 1] = -2;
            O.t[(size_t)pix * depth + k] = -1.0f;
        }
    }
    float tHit = 4294967296.0f;  // HitRecordInit: t = UINT_MAX
    bool cont = scene_box_hit(F, ray);
    F3 color = F3{0, 0, 0};
    float shadow_sum = 0.0f;
    int ray_depth = 0;
    const bool do_shadow = !(F.flags & RT_FLAG_NO_SHADOW);
    while (cont && ray_depth < depth) {
        const int hit = trace<true, FASTONLY, 0, false, false>(S, O, ray, tHit, st, overflow);
        if (want_aux) {
            O.hits[((size_t)pix * depth + ray_depth) * 2] = hit;
            O.t[(size_t)pix * depth + ray_depth] = tHit;
        }
        if (hit >= 0) {
            const int kk = ray_depth;
            ray_depth++;
            F3 rez, hitpoint, normal, L;
            shade_hit(S, F, ray, tHit, hit, rez, hitpoint, normal, L);
            // color += rez (volumeRender.cl:1483) does not depend on the shadow ray: doing it
            // first is the same float op on the same operands and frees rez for the trace.
            color = color + rez;
            // the reflected ray is built now and parked in LDS, so the shadow traversal
            // below does not keep hitpoint / normal / the old ray live
            cont = ray_depth < depth;
            if (cont) park_next(ray.dir, normal, hitpoint, next);
            float coef = 1.0f;
            if (do_shadow) {
                int sh;
                coef = shadow_coef<FASTONLY, 0, false, false>(S, O, hitpoint, L, st, overflow, sh);
                if (want_aux) O.hits[((size_t)pix * depth + kk) * 2 + 1] = sh;
            }
            shadow_sum += coef;
            if (cont) {
                ray = ray_init(F3{next[0], next[64], next[128]}, F3{next[192], next[256], next[320]});
                tHit = 4294967296.0f;
            }
        } else {
            cont = false;
        }
    }
    color = finish_color(color, shadow_sum, ray_depth);
    if (want_aux) {
        O.rgb[(size_t)pix * 3 + 0] = color.x;
        O.rgb[(size_t)pix * 3 + 1] = color.y;
        O.rgb[(size_t)pix * 3 + 2] = color.z;
    }
    O.out[pix] = rgb_to_int(color.x * 255.0f, color.y * 255.0f, color.z * 255.0f);
    if (overflow) atomicAdd(O.overflow, 1ull);
}

template <bool FASTONLY>
__global__ void __launch_bounds__(256, 7) render_kernel(DevScene S, Frame F, Outputs O, int want_aux) {
    // no guard rows (traverse_ifif's GUARD = false): with them and s_next, 24 KiB per block, only 6
    // blocks fit a CU, and the compiler then no longer holds the kernel to 7 waves' registers
    __shared__ uint32_t s_stack[4][kLdsStack][64];
    __shared__ float s_next[4][6][64];  // next bounce's ray {o, d}, parked during the shadow trace
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    rtk::zero_next_counters(F);
    const uint32_t tb = rtk::block_tile(F);
    const uint32_t t_start = (uint32_t)__builtin_amdgcn_s_memrealtime();
    uint32_t x, lr;
    rtk::tile_pixel(F, tb, wave, lane, x, lr);
    const uint32_t y = lr < F.local_rows ? rtk::frame_row(F, lr) : F.h;
    if (x < F.w && y < F.h) {
        const uint32_t pix = lr * F.w + x;  // < 2^32 local pixels
        Stack st;
        st.lds = &s_stack[wave][0][lane];
        st.glb = O.gstack + pix;
        st.gstride = O.local_pixels;
        render_pixel<FASTONLY>(S, F, O, want_aux, x, y, pix, st, &s_next[wave][0][lane]);
    }
    tile_epilogue(F, tb, t_start, &s_stack[0][0][0]);
}

// ============================================================================
// Wavefront path (RT_FLAG_WAVEFRONT; and every depth-1 frame, whose first launch is
// the whole frame): one launch per bounce over a compacted queue of the rays still in
// flight (SURVEY.md 8f #3).  Bounce k's queue holds exactly the pixels whose first k
// rays all hit; a ray carries its pixel, the ray_init inputs of its next ray
// (volumeRender.cl:1493-1498) and the colour and shadow sum so far, so the per-pixel
// arithmetic is the fused kernel's.  Each wave appends to a segment of its own (rtk::WQ),
// so a queue is in the screen order of the tiles that produced it whatever order the
// blocks ran in (neighbouring origins share waves); rtk::wf_compact_sort_kernel compacts
// each screen-local chunk of kChunkSegs segments and, with RT_FLAG_WF_SORT, orders it by the rays'
// direction, so rays of similar length share waves.
// ============================================================================

enum { kFinishMiss = 0, kFinishHit = 1, kContinue = 2 };

// One bounce (volumeRender.cl:1236-1517) of the ray of pixel `pix` that is its k-th:
// closest hit, shading, shadow ray, next ray.  A ray that continues is appended to
// W.out as soon as its next ray is known, BEFORE its shadow trace (whether it continues
// does not depend on the shadow ray): its record goes out with the colour so far and
// only the shadow sum is stored after the shadow trace, so nothing is parked across that
// trace (no LDS for the next ray).  `color += rez` before the shadow trace is the same
// float op on the same operands as after it (volumeRender.cl:1483).
template <bool FASTONLY, int TR = 0, bool SEL = false, bool OCTS = false, bool WALK = false>
__device__ __forceinline__ int wf_bounce(const DevScene& S, const Frame& F, const Outputs& O, const WQ& W,
                                         int want_aux, uint32_t pix, int k, Ray ray, F3& color, float& ss,
                                         const Stack& st, bool& overflow) {
    const int depth = F.depth;
    float tHit = 4294967296.0f;
    const int hit = trace<true, FASTONLY, TR, SEL, true, OCTS, WALK>(S, O, ray, tHit, st, overflow);
    if (TR == 2) rtk::timeline_mark(st.fc, 4);   // the closest-hit traversal is done
    if (want_aux) {
        O.hits[((size_t)pix * depth + k) * 2] = hit;
        O.t[(size_t)pix * depth + k] = tHit;
    }
    if (hit < 0) return kFinishMiss;
    F3 rez, hitpoint, normal, L;
    shade_hit(S, F, ray, tHit, hit, rez, hitpoint, normal, L);
    if (TR == 2) rtk::timeline_mark(st.fc, 5);   // shaded: the shadow ray starts
    const bool cont = k + 1 < depth;
    color = color + rez;
    QRay* q = nullptr;
    if (cont && W.out) {
        // volumeRender.cl:1493-1498: the next ray's ray_init inputs {hitpoint + refl * 0.001f, refl}
        const F3 refl = reflect(ray.dir, normal);
        const F3 no = mad3(refl, 0.001f, hitpoint);
        q = rtk::seg_slot(W.out, W.seg, W.seg_fill);
        q->a = make_float4(__uint_as_float(pix), no.x, no.y, no.z);
        q->c = make_float4(color.x, color.y, color.z, __int_as_float(hit));  // hit: the triangle the ray leaves
        float* b = reinterpret_cast<float*>(&q->b);
        b[0] = refl.x; b[1] = refl.y; b[2] = refl.z;
    }
    float coef = 1.0f;
    if (!(F.flags & RT_FLAG_NO_SHADOW)) {
        int sh;
        coef = shadow_coef<FASTONLY, TR, SEL, true, OCTS, WALK>(S, O, hitpoint, L, st, overflow, sh);
        if (want_aux) O.hits[((size_t)pix * depth + k) * 2 + 1] = sh;
    }
    ss += coef;
    if (q) reinterpret_cast<float*>(&q->b)[3] = ss;
    return cont ? kContinue : kFinishHit;
}

// oi: the packed pixel's slot in O.out (pix, or its place in the whole frame: O.frame_rows)
__device__ __forceinline__ void wf_finish(const Outputs& O, int want_aux, uint32_t pix, size_t oi, F3 color, float ss,
                                          int ray_depth) {
    color = finish_color(color, ss, ray_depth);
    if (want_aux) {
        O.rgb[(size_t)pix * 3 + 0] = color.x;
        O.rgb[(size_t)pix * 3 + 1] = color.y;
        O.rgb[(size_t)pix * 3 + 2] = color.z;
    }
    O.out[oi] = rgb_to_int(color.x * 255.0f, color.y * 255.0f, color.z * 255.0f);
}

__device__ __forceinline__ void wf_aux_init(const Outputs& O, int depth, uint32_t pix) {
    for (int k = 0; k < depth; ++k) {
        O.hits[((size_t)pix * depth + k) * 2 + 0] = -2;
        O.hits[((size_t)pix * depth + k) * 2 + 1] = -2;
        O.t[(size_t)pix * depth + k] = -1.0f;
    }
}

// One pixel's bounce 0 (wave-uniform call: the appends are wave-aggregated).  ROWS (the
// depth-1 kernel): with O.frame_rows the packed pixel goes to its place in the whole frame.
// qbase: added to the pixel index a continuing ray carries in the queue (the frame's first
// pixel in a batch launch's pixel space, first_bounce_batch_kernel; 0 otherwise).
template <bool FASTONLY, int TR, bool SEL, bool ROWS, bool WALK>
__device__ __forceinline__ void first_bounce_pixel(const DevScene& S, const Frame& F, const Outputs& O, const WQ& W,
                                                   int want_aux, uint32_t x, uint32_t lr, uint32_t* lds, uint32_t* fc,
                                                   rtk::Walk walk, uint32_t qbase = 0u) {
    const uint32_t y = lr < F.local_rows ? rtk::frame_row(F, lr) : F.h;
    const bool valid = x < F.w && y < F.h;
    const uint32_t pix = valid ? lr * F.w + x : 0u;
    const size_t oi = ROWS && O.frame_rows ? (size_t)y * F.w + x : (size_t)pix;
    F3 color = F3{0, 0, 0};
    float ss = 0.0f;
    bool overflow = false;
    if (valid) {
        Ray ray = primary_ray(F, x, y);
        if (want_aux) wf_aux_init(O, F.depth, pix);
        if (F.depth < 1 || !scene_box_hit(F, ray)) {
            wf_finish(O, want_aux, pix, oi, color, ss, 0);
        } else {
            Stack st;
            st.lds = lds;
            st.glb = O.gstack + pix;
            st.gstride = O.local_pixels;
            st.fc = fc;
            if (WALK) st.walk = walk;
            if (TR == 1) st.vc = O.fcount + rtk::kFetchCounts;
            const int r = wf_bounce<FASTONLY, TR, SEL, kOctLoops && SEL, WALK>(S, F, O, W, want_aux, pix + qbase, 0, ray, color, ss, st, overflow);
            if (r != kContinue) wf_finish(O, want_aux, pix, oi, color, ss, r == kFinishHit ? 1 : 0);
        }
    }
    if (overflow) atomicAdd(O.overflow, 1ull);
}

// Bounce 0, one lane per pixel, one wave per 8x8 tile (the reference's work-group),
// four tiles per block; continuing rays go to W.out.  At depth 1 this is the whole
// frame: without the bounce loop it fits 8 waves per SIMD in S_ref (62 VGPRs, no scratch), its
// traversal computes record offsets without a branch (SEL), and in S_ref it has the octant loops (OCTS).
// NEXT (depth > 1): continuing rays are appended to W.out, wave w of tile tb to segment
// 4 tb + w (screen order).
// TR 1: the measurement instantiation (rt_fetch_counts) that counts every fetch; TR 2: the
// diagnostic instantiation (rt_wave_timeline) that stamps every wave's start, end of its
// pixels and end of the block epilogue and counts its loop trips (rtk::timeline_*), at the
// product kernel's wave bound.
template <bool FASTONLY, bool NEXT, int TR = 0, bool WALK = !NEXT>
__global__ void __launch_bounds__(256, TR == 1 ? 4 : kMath != 2 ? RTK_WF_WAVES : NEXT ? RTK_FBN_REF_WAVES : RTK_FB_WAVES) first_bounce_kernel(DevScene S, Frame F, Outputs O, WQ W, int want_aux, rtk::Walk walk) {
    __shared__ uint32_t s_stack[4][rtk::kLdsRows][64];
    __shared__ uint32_t s_fc[TR == 1 ? 8 * 256 : TR == 2 ? 4 * rtk::kTlWords : 1];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t* lds = &s_stack[wave][rtk::kLdsGuard][lane];
    rtk::zero_next_counters(F);
    const uint32_t tb = rtk::block_tile(F);
    const uint32_t t_start = (uint32_t)__builtin_amdgcn_s_memrealtime();
    uint32_t x, lr;
    rtk::tile_pixel(F, tb, wave, lane, x, lr);
    if (TR == 1)
        for (int k = 0; k < 8; ++k) s_fc[k * 256 + threadIdx.x] = 0u;
    if (TR == 2 && lane < (int)rtk::kTlWords) s_fc[wave * rtk::kTlWords + lane] = 0u;
    __shared__ uint32_t s_fill[4];
    if (lane == 0) s_fill[wave] = 0u;
    WQ Wn = W;
    if (!NEXT) Wn.out = nullptr;   // depth 1: nothing continues
    Wn.seg = tb * 4u + (uint32_t)wave;
    Wn.seg_fill = &s_fill[wave];
    static_assert(!WALK || !NEXT, "the cursor loop is the depth-1 kernels'");
    first_bounce_pixel<FASTONLY, TR, !NEXT, !NEXT, WALK>(S, F, O, Wn, want_aux, x, lr, lds,
                                                                  TR == 1 ? &s_fc[threadIdx.x] : TR == 2 ? &s_fc[wave * rtk::kTlWords] : nullptr, walk);
    if (NEXT) rtk::seg_close(Wn, Wn.seg);
    if (TR == 1) rtk::fetch_count_flush(s_fc, O.fcount);
    const uint32_t t_pix = TR == 2 ? (uint32_t)__builtin_amdgcn_s_memrealtime() : 0u;
    tile_epilogue(F, tb, t_start, &s_stack[0][0][0]);
    if (TR == 2) rtk::timeline_store(O, blockIdx.x * 4u + (uint32_t)wave, t_start, t_pix, &s_fc[wave * rtk::kTlWords], tb);
}

// Several frames of one size in ONE launch (rt_render_device_batch, throughput mode): bounce 0
// of every frame.  The grid holds every frame's blocks; entry e of the block order is frame
// e / nb, tile e % nb (nb = F.num_blocks, the blocks of one frame), so the static order runs a
// tile of every frame side by side and the adaptive one sorts all frames' blocks longest-first
// together: the frames' long waves start first and overlap inside one launch, where separate
// frames in flight each put theirs behind the others' on streams the hardware serves a few at a
// time.  Frame f's camera comes from the launch's BatchCams (a kernel argument: uniform loads),
// its pixels go to out + f * stride.  The launch's pixel space is the frames one after the
// other (frame f's pixel p is f * frame_px + p): the global traversal stack is indexed in it
// (O.local_pixels = all frames' pixels), and so are the rays that continue (NEXT, depth > 1):
// wave w of entry e appends to segment 4 e + w, so the bounce queues hold the frames one after
// the other and the bounce launches run over all of them at once, each ray finishing at its own
// pixel of its own frame (at depth > 1 frame_px is the frames' stride, so that pixel is out[f * stride + p]).
// Per pixel this is first_bounce_kernel's code, so every frame equals its own single render.
template <bool FASTONLY, bool NEXT>
__global__ void __launch_bounds__(256, kMath != 2 ? RTK_WF_WAVES : NEXT ? RTK_FBN_REF_WAVES : RTK_FB_WAVES) first_bounce_batch_kernel(DevScene S, Frame F, Outputs O, WQ W, rtk::BatchCams C, rtk::Walk walk) {
    __shared__ uint32_t s_stack[4][rtk::kLdsRows][64];
    __shared__ uint32_t s_fill[4];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    rtk::zero_next_counters(F);
    const uint32_t e = rtk::block_tile(F);
    const uint32_t f = e / F.num_blocks, tb = e - f * F.num_blocks;
    const uint32_t t_start = (uint32_t)__builtin_amdgcn_s_memrealtime();
    uint32_t x, lr;
    rtk::tile_pixel(F, tb, wave, lane, x, lr);
    Frame Ff = F;
    const rtk::BatchCam& cam = C.cam[f];
    Ff.a = make_float3(cam.a.x, cam.a.y, cam.a.z);
    Ff.b = make_float3(cam.b.x, cam.b.y, cam.b.z);
    Ff.c = make_float3(cam.c.x, cam.c.y, cam.c.z);
    Ff.campos = make_float3(cam.campos.x, cam.campos.y, cam.campos.z);
    Ff.light_pos = make_float3(cam.light_pos.x, cam.light_pos.y, cam.light_pos.z);
    Outputs Of = O;
    Of.out = O.out + (size_t)f * C.stride;
    Of.gstack = O.gstack + (size_t)f * C.frame_px;
    if (lane == 0) s_fill[wave] = 0u;
    WQ Wn = W;
    if (!NEXT) Wn.out = nullptr;   // depth 1: nothing continues
    // RTK_XFRAME (A/B): the continuing rays of one screen tile of all the launch's frames side by side
    // in the queue (tile-major, frame-minor), so a sort chunk holds the same screen region of every
    // frame and the bounce waves work through one region of all frames at a time
    const uint32_t qe = RTK_XFRAME ? tb * (gridDim.x / F.num_blocks) + f : e;
    Wn.seg = qe * 4u + (uint32_t)wave;
    Wn.seg_fill = &s_fill[wave];
    first_bounce_pixel<FASTONLY, 0, !NEXT, !NEXT, !NEXT>(S, Ff, Of, Wn, 0, x, lr, &s_stack[wave][rtk::kLdsGuard][lane], nullptr,
                                                       walk, f * C.frame_px);
    if (NEXT) rtk::seg_close(Wn, Wn.seg);
    tile_epilogue(F, e, t_start, &s_stack[0][0][0]);
}

// Bounce W.bounce (>= 1) over its queue: persistent waves take 64 rays at a time, group g
// = rays [64 g, 64 g + 64) of the dense order W.perm, and append the rays that continue to
// segment g of W.out.  The groups go out in queue order, so at any time the whole chip works
// on one screen region: C5's scene (0.7 GB of records) does not fit the Infinity Cache, and
// dealing the XCDs 8 separate regions of the queue (each L2 its own) made the frame 1.76x
// slower (1.71 vs 0.97 ms).
// TR: the measurement instantiation (rt_fetch_counts).
// Bounded to 8 waves per SIMD in S_ref (64 VGPRs + 20 B of scratch outside the traversal
// loop; at 7 waves 71 VGPRs), as is the depth > 1 first-bounce kernel (the same 59 VGPRs either
// way, but scheduled for 8 waves): C5 0.849-0.851 vs 0.876-0.883 ms with both at 7
// (profiles/r04/ab/wf_waves_grid_ab.log, "w8"); this kernel at 8 alone: 0.892 vs 0.880-0.884
// (wfb8_sched_ab.log).  S_strict / S_hw keep 7 (at 8 they spill 40-72 B).
// TR 2 (rt_wave_timeline): per wave its start, end, loop trips and the number of 64-ray groups
// it took (in the record's tile word).
template <bool FASTONLY, int TR = 0>
__global__ void __launch_bounds__(256, TR == 1 ? 4 : (kMath == 2 ? RTK_WFB_REF_WAVES : RTK_WF_WAVES)) wf_bounce_kernel(DevScene S, Frame F, Outputs O, WQ W, int want_aux) {
    __shared__ uint32_t s_stack[4][rtk::kLdsRows][64];
    __shared__ uint32_t s_fc[TR == 1 ? 8 * 256 : TR == 2 ? 4 * rtk::kTlWords : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t t_start = TR == 2 ? (uint32_t)__builtin_amdgcn_s_memrealtime() : 0u;
    uint32_t ngroups = 0;
    if (TR == 1)
        for (int c = 0; c < 8; ++c) s_fc[c * 256 + threadIdx.x] = 0u;
    if (TR == 2 && lane < (int)rtk::kTlWords) s_fc[wave * rtk::kTlWords + lane] = 0u;
    __shared__ uint32_t s_fill[4];
    if (lane == 0) s_fill[wave] = 0u;
    const uint32_t n = *W.in_count;
    const int k = W.bounce;
    uint32_t home = blockIdx.x & (rtk::kCursors - 1u);
    for (;;) {
        const uint32_t g = rtk::grab_group(W.fetch, (n + rtk::kSegRays - 1) / rtk::kSegRays, home);
        if (g == rtk::kNoGroup) break;
        ++ngroups;
        const uint32_t base = g * rtk::kSegRays;
        const uint32_t i = base + (uint32_t)lane;
        const bool valid = i < n;
        QRay q;
        q.a = q.b = q.c = make_float4(0, 0, 0, 0);
        if (valid) q = W.in[W.perm[i]];
        WQ Wg = W;
        Wg.seg = base / rtk::kSegRays;
        Wg.seg_fill = &s_fill[wave];
        const uint32_t pix = __float_as_uint(q.a.x);
        F3 color = F3{q.c.x, q.c.y, q.c.z};
        float ss = q.b.w;
        bool overflow = false;
        if (valid) {
            Ray ray = ray_init(F3{q.a.y, q.a.z, q.a.w}, F3{q.b.x, q.b.y, q.b.z});
            Stack st;
            st.lds = &s_stack[wave][rtk::kLdsGuard][lane];
            st.glb = O.gstack + pix;
            st.gstride = O.local_pixels;
            st.fc = TR == 1 ? &s_fc[threadIdx.x] : TR == 2 ? &s_fc[wave * rtk::kTlWords] : nullptr;
            if (TR == 1) st.vc = O.fcount + rtk::kFetchCounts;
            const int r = wf_bounce<FASTONLY, TR>(S, F, O, Wg, want_aux, pix, k, ray, color, ss, st, overflow);
            if (r != kContinue) wf_finish(O, want_aux, pix, pix, color, ss, r == kFinishHit ? k + 1 : k);
        }
        if (W.out) rtk::seg_close(Wg, Wg.seg);
        if (overflow) atomicAdd(O.overflow, 1ull);
    }
    if (TR == 1) rtk::fetch_count_flush(s_fc, O.fcount);
    if (TR == 2) {
        const uint32_t t_end = (uint32_t)__builtin_amdgcn_s_memrealtime();
        rtk::timeline_store(O, blockIdx.x * 4u + (uint32_t)wave, t_start, t_end, &s_fc[wave * rtk::kTlWords], ngroups);
    }
}

// ============================================================================
// Ray queries (rt_trace_rays, DESIGN.md 18): closest hit (ANY = false) or any hit of rays read
// from memory.  A persistent grid, as the bounce kernel's: a wave takes 64 rays at a time (group g
// = rays [64 g, 64 g + 64), rtk::grab_group), a lane reads its ray as two 16-B loads, traces it
// with the frame kernels' trace<> from its own tmax, and stores its rt_hit as one 8-B store (a
// wave's 512 B are contiguous).  No Frame, no shading, no queues.
// A lane whose ray is invalid (a non-finite origin or direction component, a zero direction, a NaN
// tmax) or can accept nothing (tmax <= kTmin) sits the traversal out, as a bounce kernel's lane
// past the end of its queue does, and reports a miss; a miss's t is the ray's tmax word itself.
// The global part of the stack is one column per lane of the GRID (not per ray), so its size does
// not depend on n.
// In S_ref both instantiations of the fast kernel run the octant loops (OCTS): without shading
// they stay within 8 waves' registers with no scratch (DESIGN.md 18).  Record offsets come from a
// select (SEL), as in the depth-1 frame kernel: incoherent rays 0.950 vs 0.999 ms for C3's 2.07 M,
// the frame's own rays the same within the spread.
// ============================================================================
__device__ __forceinline__ bool query_ray_ok(const float4& a, const float4& b) {
    const bool fin = fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff() &&
                     fabsf(b.x) < __builtin_inff() && fabsf(b.y) < __builtin_inff() && fabsf(b.z) < __builtin_inff();
    const bool zero = b.x == 0.0f && b.y == 0.0f && b.z == 0.0f;
    return fin && !zero && a.w > kTmin;   // (false for a NaN tmax too)
}

template <bool ANY, bool FASTONLY>
__global__ void __launch_bounds__(256, kMath == 2 ? RTK_QUERY_REF_WAVES : RTK_QUERY_WAVES) query_kernel(DevScene S, Outputs O, rtk::Query Q) {
    __shared__ uint32_t s_stack[4][rtk::kLdsRows][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ngroups = (Q.n + rtk::kSegRays - 1) / rtk::kSegRays;
    uint32_t home = blockIdx.x & (rtk::kCursors - 1u);
    Stack st;
    st.lds = &s_stack[wave][rtk::kLdsGuard][lane];
    st.glb = O.gstack + ((size_t)blockIdx.x * rtk::kBlockThreads + threadIdx.x);
    st.gstride = O.local_pixels;   // the lanes launched
    for (;;) {
        const uint32_t g = rtk::grab_group(Q.fetch, ngroups, home);
        if (g == rtk::kNoGroup) break;
        const uint32_t i = g * rtk::kSegRays + (uint32_t)lane;
        const bool inside = i < Q.n;   // (false only in the last group's tail)
        float4 a = make_float4(0, 0, 0, 0), b = a;
        if (inside) {
            const float4* rp = Q.rays + (size_t)i * 2;
            a = rp[0];
            b = rp[1];
        }
        const uint32_t tmax_word = __float_as_uint(a.w);
        int hit = -1;
        float t = a.w;
        bool overflow = false;
        if (inside && query_ray_ok(a, b)) {
            Ray ray = ray_init(F3{a.x, a.y, a.z}, F3{b.x, b.y, b.z});
            hit = trace<!ANY, FASTONLY, 0, true, true, kOctLoops>(S, O, ray, t, st, overflow, a.w);
        }
        if (inside) Q.hits[i] = make_uint2((uint32_t)hit, hit >= 0 ? __float_as_uint(t) : tmax_word);
        if (overflow) atomicAdd(O.overflow, 1ull);
    }
}

// ============================================================================
// Ray queries with hit attributes (rt_trace_rays_attr, DESIGN.md 19): query_kernel's grid, ray
// loads, validity test, trace<> instantiation, restart value and spill columns, and after the
// traversal a lane that hit reads the seven 16-B words of triangle id / 3's shading record and
// computes hit_attr (rt_device_math.h): what shade_hit computes at that hit.  A record is four
// 16-B words {id, t, u, v} {p, ndotd} {ng, 0} {ns, 0}; a miss is {-1, tmax word, 0 ...}.
// The wave stages its 64 records in the 16 stack rows of its LDS columns (exactly 4 KiB; free once
// trace<> has returned, and a traversal expects nothing of what they hold when it starts; the
// guard rows below them are not touched) and stores them as four contiguous 1-KiB wave stores.
// The rows are the wave's own, so it waits for its LDS writes and needs no barrier.  (Each lane
// storing its own four words, 64 B apart from its neighbour's, measured 2 to 5 % slower: C3's
// primary rays in S_ref 0.237 / 0.244 against 0.232 / 0.232 ms, incoherent rays 0.997 / 0.994
// against 0.971 / 0.972, DESIGN.md 19.)
// Q.hits is the rt_hit_attr buffer here (16-byte aligned).
// ============================================================================
template <bool ANY, bool FASTONLY>
__global__ void __launch_bounds__(256, kMath == 2 ? RTK_QATTR_REF_WAVES : RTK_QATTR_WAVES) query_attr_kernel(DevScene S, Outputs O, rtk::Query Q) {
    __shared__ __attribute__((aligned(16))) uint32_t s_stack[4][rtk::kLdsRows][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ngroups = (Q.n + rtk::kSegRays - 1) / rtk::kSegRays;
    uint32_t home = blockIdx.x & (rtk::kCursors - 1u);
    Stack st;
    st.lds = &s_stack[wave][rtk::kLdsGuard][lane];
    st.glb = O.gstack + ((size_t)blockIdx.x * rtk::kBlockThreads + threadIdx.x);
    st.gstride = O.local_pixels;   // the lanes launched
    uint4* const out = (uint4*)Q.hits;
    for (;;) {
        const uint32_t g = rtk::grab_group(Q.fetch, ngroups, home);
        if (g == rtk::kNoGroup) break;
        const uint32_t i = g * rtk::kSegRays + (uint32_t)lane;
        const bool inside = i < Q.n;   // (false only in the last group's tail)
        float4 a = make_float4(0, 0, 0, 0), b = a;
        if (inside) {
            const float4* rp = Q.rays + (size_t)i * 2;
            a = rp[0];
            b = rp[1];
        }
        uint4 r0 = make_uint4(0xFFFFFFFFu, __float_as_uint(a.w), 0u, 0u), r1 = make_uint4(0u, 0u, 0u, 0u), r2 = r1, r3 = r1;
        bool overflow = false;
        if (inside && query_ray_ok(a, b)) {
            Ray ray = ray_init(F3{a.x, a.y, a.z}, F3{b.x, b.y, b.z});
            float t = a.w;
            const int hit = trace<!ANY, FASTONLY, 0, true, true, kOctLoops>(S, O, ray, t, st, overflow, a.w);
            if (hit >= 0) {
                const float4* sp = S.shade + (size_t)(hit / 3) * 7;
                const float4 p0 = sp[0], p1 = sp[1], p2 = sp[2], m0 = sp[3], m1 = sp[4], m2 = sp[5];
                const HitAttr h = hit_attr(ray, t, xyz(p0), xyz(p1), xyz(p2), xyz(m0), xyz(m1), xyz(m2));
                r0 = make_uint4((uint32_t)hit, __float_as_uint(t), __float_as_uint(h.u), __float_as_uint(h.v));
                r1 = make_uint4(__float_as_uint(h.p.x), __float_as_uint(h.p.y), __float_as_uint(h.p.z), __float_as_uint(h.ndotd));
                r2 = make_uint4(__float_as_uint(h.ng.x), __float_as_uint(h.ng.y), __float_as_uint(h.ng.z), 0u);
                r3 = make_uint4(__float_as_uint(h.ns.x), __float_as_uint(h.ns.y), __float_as_uint(h.ns.z), 0u);
            }
        }
        uint4* const stage = (uint4*)&s_stack[wave][rtk::kLdsGuard][0];   // 256 words of 16 B: record l at 4 l
        stage[lane * 4 + 0] = r0;
        stage[lane * 4 + 1] = r1;
        stage[lane * 4 + 2] = r2;
        stage[lane * 4 + 3] = r3;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const uint32_t left = min(Q.n - g * rtk::kSegRays, rtk::kSegRays) * 4u;   // 16-B words of this group that exist
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t j = k * 64u + (uint32_t)lane;
            const uint4 w = stage[j];
            if (j < left) out[(size_t)g * 256u + j] = w;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read out before the next traversal writes the rows
        if (overflow) atomicAdd(O.overflow, 1ull);
    }
}

// ============================================================================
// Occlusion fans (rt_trace_fan, DESIGN.md 21): n origins against the same k directions, one bit per
// ray.  query_kernel's persistent grid, stack columns, trace<> instantiation (any hit) and restart
// value; a work item is (group g of 64 consecutive origins, chunk c of 32 directions), items in
// origin-group-major order so that the waves at work at one time are near each other in the scene.
// Lane = origin: it loads its record once per item as two 16-B loads and walks the chunk's
// directions, whose loads are wave-uniform, so every traversal of the wave has ONE direction (in
// S_ref: one octant loop, unless a component is zero).  Per direction a lane whose ray is not traced
// -- rt_fan_expand's rule: query_ray_ok, a finite normal, and a zero normal or dot(n, d) > 0 on the
// raw words -- sits the traversal out as query_kernel's invalid lanes do, and a direction no lane of
// the wave is traced for is skipped.  The hit bits gather in a register and the lane stores its one
// word after the chunk (a wave's 256 B are contiguous: the layout is chunk-major); every mask word
// has exactly one writer.  Each ray is ray_init(o, d_j) by the frame's own function, per lane: the
// bits are the expanded query's by construction.
// ============================================================================
template <bool FASTONLY>
__global__ void __launch_bounds__(256, kMath == 2 ? RTK_FAN_REF_WAVES : RTK_FAN_WAVES) fan_kernel(DevScene S, Outputs O, rtk::Fan Fn) {
    __shared__ uint32_t s_stack[4][rtk::kLdsRows][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t nitems = ((Fn.n + rtk::kSegRays - 1) / rtk::kSegRays) * Fn.chunks;
    uint32_t home = blockIdx.x & (rtk::kCursors - 1u);
    Stack st;
    st.lds = &s_stack[wave][rtk::kLdsGuard][lane];
    st.glb = O.gstack + ((size_t)blockIdx.x * rtk::kBlockThreads + threadIdx.x);
    st.gstride = O.local_pixels;   // the lanes launched
    for (;;) {
        const uint32_t item = rtk::grab_group(Fn.fetch, nitems, home);
        if (item == rtk::kNoGroup) break;
        const uint32_t g = item / Fn.chunks, c = item - g * Fn.chunks;
        const uint32_t i = g * rtk::kSegRays + (uint32_t)lane;
        const bool inside = i < Fn.n;   // (false only in the last group's tail)
        float4 a = make_float4(0, 0, 0, 0), b = a;
        if (inside) {
            const float4* op = Fn.origins + (size_t)i * 2;
            a = op[0];
            b = op[1];
        }
        const F3 nrm = F3{b.x, b.y, b.z};
        const bool nfin = fabsf(b.x) < __builtin_inff() && fabsf(b.y) < __builtin_inff() && fabsf(b.z) < __builtin_inff();
        const bool nocull = b.x == 0.0f && b.y == 0.0f && b.z == 0.0f;
        const uint32_t j0 = c * 32u, j1 = min(j0 + 32u, Fn.k);
        uint32_t bits = 0u, overflows = 0u;
        for (uint32_t j = j0; j < j1; ++j) {
            const float4 d = Fn.dirs[j];   // wave-uniform
            const bool traced = inside && nfin && query_ray_ok(a, d) && (nocull || dot(nrm, F3{d.x, d.y, d.z}) > 0.0f);
            if (__builtin_amdgcn_ballot_w64(traced) == 0) continue;
            if (traced) {
                Ray ray = ray_init(F3{a.x, a.y, a.z}, F3{d.x, d.y, d.z});
                float t = a.w;
                bool overflow = false;
                const int hit = trace<false, FASTONLY, 0, true, true, kOctLoops>(S, O, ray, t, st, overflow, a.w);
                if (hit >= 0) bits |= 1u << (j & 31u);
                if (overflow) ++overflows;
            }
        }
        if (inside) Fn.masks[(size_t)c * Fn.n + i] = bits;
        if (overflows) atomicAdd(O.overflow, (unsigned long long)overflows);
    }
}

// ============================================================================
// First k hits (rt_trace_rays_k, DESIGN.md 24): for each ray the first K distinct triangles along it,
// ordered by (t, id), with u and v.  The list and the control flow are csrc/host/multihit_core.hpp's, the
// text the host twin runs; this namespace's arithmetic comes in through RayScene, which is the general
// traverse<true>'s: ray_init, its choice between the fast quotient and the division form, its slab
// test, ray_tri.  query_kernel's persistent grid, cursor grab, ray loads and validity test; the stack
// is the general traversal's Stack (16 LDS rows per lane, then the slot's global columns: no guard rows,
// which only traverse_ifif touches).  Lanes step independently, one step per trip (if-if, as
// closest_kernel: the bound is the lane's own).  At the end a lane evaluates ray_tri_uv for the
// entries it found and stores plane j of its ray to out[j * n + i], one 16-B store per plane, a wave's
// 1 KiB contiguous.  One instantiation per K, so the list is indexed statically only.  Nothing restarts:
// O.restarts stays 0.
// A caller who needs one hit should call rt_trace_rays: K = 1 runs this general loop, not the fast one.
// ============================================================================
struct RayScene {
    const DevScene& S;
    const Ray& ray;
    const F3 y;        // slab_recip(ray)
    const bool fast;   // traverse's choice: S.fast_div && fast_div_ok(ray)
    __device__ __forceinline__ void slab(uint32_t cur, float& n0, float& f0, float& n1, float& f1, uint32_t& r0, uint32_t& r1) const {
        const float4* np = S.wnodes + (size_t)cur * 4;
        const float4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
        if (fast) slab2_pk<true>(q0, q1, q2, ray_pk(ray.ori, ray.dir, y), n0, f0, n1, f1);
        else slab2_div(q0, q1, q2, ray.ori, ray.dir, n0, f0, n1, f1);
        r0 = __float_as_uint(q3.x);
        r1 = __float_as_uint(q3.y);
    }
    __device__ __forceinline__ void leaf(uint32_t ref, int& off, int& cnt) const { leaf_range(S, ref, off, cnt); }
    __device__ __forceinline__ void tri_t(int k, float& t, int32_t& id) const {
        const float4* tp = tri_rec(S, k);
        const float4 a0 = tp[0], a1 = tp[1], a2 = tp[2];
        t = ray_tri(ray, F3{a0.x, a0.y, a0.z}, F3{a1.x, a1.y, a1.z}, F3{a2.x, a2.y, a2.z});
        id = __float_as_int(a0.w);
    }
};

// waves per SIMD multihit_kernel<K> is bounded to: what its registers allow without scratch (DESIGN.md 24)
constexpr int multihit_waves(int k) {
    return kMath == 2 ? RTK_MULTIHIT_REF_WAVES(k) : RTK_MULTIHIT_WAVES(k);
}

template <int K>
__global__ void __launch_bounds__(256, multihit_waves(K)) multihit_kernel(DevScene S, Outputs O, rtk::Query Q) {
    __shared__ uint32_t s_stack[4][kLdsStack][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ngroups = (Q.n + rtk::kSegRays - 1) / rtk::kSegRays;
    uint32_t home = blockIdx.x & (rtk::kCursors - 1u);
    Stack st;
    st.lds = &s_stack[wave][0][lane];
    st.glb = O.gstack + ((size_t)blockIdx.x * rtk::kBlockThreads + threadIdx.x);
    st.gstride = O.local_pixels;   // the lanes launched
    uint4* const out = (uint4*)Q.hits;
    for (;;) {
        const uint32_t g = rtk::grab_group(Q.fetch, ngroups, home);
        if (g == rtk::kNoGroup) break;
        const uint32_t i = g * rtk::kSegRays + (uint32_t)lane;
        const bool inside = i < Q.n;   // (false only in the last group's tail)
        float4 a = make_float4(0, 0, 0, 0), b = a;
        if (inside) {
            const float4* rp = Q.rays + (size_t)i * 2;
            a = rp[0];
            b = rp[1];
        }
        const bool traced = inside && query_ray_ok(a, b);
        const Ray ray = ray_init(F3{a.x, a.y, a.z}, F3{b.x, b.y, b.z});   // (an untraced lane's is never used)
        const RayScene RS{S, ray, slab_recip(ray), S.fast_div && fast_div_ok(ray)};
        multihit::StateK<K> T;
        multihit::start(T, S.root, a.w);
        if (!traced) T.sc = 0;
        while (T.sc > 0) multihit::step<false>(T, RS, st);
        if (inside) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                uint4 w = make_uint4(0xFFFFFFFFu, __float_as_uint(a.w), 0u, 0u);   // the miss record: the ray's tmax word
                if (T.id[j] >= 0) {
                    const float4* tp = tri_rec(S, T.at[j]);
                    const float4 a0 = tp[0], a1 = tp[1], a2 = tp[2];
                    float u, v;
                    ray_tri_uv(ray, F3{a0.x, a0.y, a0.z}, F3{a1.x, a1.y, a1.z}, F3{a2.x, a2.y, a2.z}, u, v);
                    w = make_uint4((uint32_t)T.id[j], __float_as_uint(T.t[j]), __float_as_uint(u), __float_as_uint(v));
                }
                out[(size_t)j * Q.n + i] = w;
            }
        }
        if (T.overflow) atomicAdd(O.overflow, 1ull);
    }
}

}  // namespace RTK_NS
