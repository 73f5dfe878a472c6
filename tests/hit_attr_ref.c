/* The yardstick of the attribute ray query (rt_trace_rays_attr): a plain-C restatement
 * of the S_strict definition of rt_hit_attr, compiled at test time (tests/hit_attr_common.py) with
 * -O2 -ffp-contract=off.  dot and cross are spelled with fmaf as the device library's (and
 * oracle/rt_oracle.c's); everything else is single float operations in source order; rsqrt is
 * (float)(1 / sqrt((double)x)).  Vertices and normals are rows of four floats, rays and records are
 * rt_ray (8 words) and rt_hit_attr (16 words). */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct { float x, y, z; } f3;

static f3 v3(float x, float y, float z) { f3 r = {x, y, z}; return r; }
static f3 ld3(const float* p) { return v3(p[0], p[1], p[2]); }
static f3 add3(f3 a, f3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
static f3 sub3(f3 a, f3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
static f3 muls(f3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
static f3 smul(float s, f3 a) { return v3(s * a.x, s * a.y, s * a.z); }
static float dot3(f3 a, f3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static f3 cross3(f3 a, f3 b) {
    return v3(fmaf(a.y, b.z, b.y * -a.z), fmaf(a.z, b.x, b.z * -a.x), fmaf(a.x, b.y, b.x * -a.y));
}
static float rsqrt1(float x) { return (float)(1.0 / sqrt((double)x)); }

static f3 normalize3(f3 p) {
    if (p.x == 0.0f && p.y == 0.0f && p.z == 0.0f) return p;
    float l2 = dot3(p, p);
    if (l2 < FLT_MIN) {
        p = muls(p, 0x1p86f);
        l2 = dot3(p, p);
    } else if (l2 == INFINITY) {
        p = muls(p, 0x1p-66f);
        l2 = dot3(p, p);
        if (l2 == INFINITY) {
            p = v3(copysignf(isinf(p.x) ? 1.0f : 0.0f, p.x), copysignf(isinf(p.y) ? 1.0f : 0.0f, p.y),
                   copysignf(isinf(p.z) ? 1.0f : 0.0f, p.z));
            l2 = dot3(p, p);
        }
    }
    return muls(p, rsqrt1(l2));
}

/* the shading normal's interpolation: Cramer barycentrics on absolute positions */
static f3 normal_at(f3 pn, f3 p0, f3 p1, f3 p2, f3 n0, f3 n1, f3 n2) {
    const float Det = p0.x * (p1.y * p2.z - p2.y * p1.z) - p1.x * (p0.y * p2.z - p2.y * p0.z) +
                      p2.x * (p0.y * p1.z - p1.y * p0.z);
    const float D0 = pn.x * (p1.y * p2.z - p2.y * p1.z) - p1.x * (pn.y * p2.z - p2.y * pn.z) +
                     p2.x * (pn.y * p1.z - p1.y * pn.z);
    const float D1 = p0.x * (pn.y * p2.z - p2.y * pn.z) - pn.x * (p0.y * p2.z - p2.y * p0.z) +
                     p2.x * (p0.y * pn.z - pn.y * p0.z);
    const float D2 = p0.x * (p1.y * pn.z - pn.y * p1.z) - p1.x * (p0.y * pn.z - pn.y * p0.z) +
                     pn.x * (p0.y * p1.z - p1.y * p0.z);
    const float l0 = D0 / Det, l1 = D1 / Det, l2 = D2 / Det;
    return add3(add3(smul(l0, n0), smul(l1, n1)), smul(l2, n2));
}

static void put3(uint32_t* w, f3 a) {
    memcpy(w + 0, &a.x, 4);
    memcpy(w + 1, &a.y, 4);
    memcpy(w + 2, &a.z, 4);
}

/* the 64-byte records of n rays for given ids and t (the traversal's); ids[k] < 0 is a miss: -1, the
 * ray's tmax word, 14 zero words.  t_mt (may be null) receives Moller-Trumbore's own t of the hit
 * triangle, dot(e2, qvec) * det, 0 for a miss. */
void ref_hit_attr(const float* verts, const int32_t* idx, const float* normals, const int32_t* normal_idx,
                  const float* rays, const int32_t* ids, const float* t, int64_t n, uint32_t* out, float* t_mt) {
    for (int64_t k = 0; k < n; ++k) {
        const float* ray = rays + 8 * k;
        uint32_t* w = out + 16 * k;
        memset(w, 0, 64);
        if (t_mt) t_mt[k] = 0.0f;
        if (ids[k] < 0) {
            w[0] = 0xFFFFFFFFu;
            memcpy(w + 1, ray + 3, 4);
            continue;
        }
        const int32_t id = ids[k];
        const f3 ori = ld3(ray), dir = normalize3(ld3(ray + 4));
        const f3 p0 = ld3(verts + 4 * idx[id + 0]), p1 = ld3(verts + 4 * idx[id + 1]), p2 = ld3(verts + 4 * idx[id + 2]);
        const f3 n0 = ld3(normals + 4 * normal_idx[id + 0]), n1 = ld3(normals + 4 * normal_idx[id + 1]),
                 n2 = ld3(normals + 4 * normal_idx[id + 2]);
        const f3 e1 = sub3(p1, p0), e2 = sub3(p2, p0);
        const f3 tvec = sub3(ori, p0);
        const f3 pvec = cross3(dir, e2);
        float det = dot3(e1, pvec);
        det = 1.0f / det;
        const float u = dot3(tvec, pvec) * det;
        const f3 qvec = cross3(tvec, e1);
        const float v = dot3(dir, qvec) * det;
        if (t_mt) t_mt[k] = dot3(e2, qvec) * det;
        const f3 p = add3(ori, muls(dir, t[k] - 0.001f));
        const f3 ng = normalize3(cross3(e1, e2));
        const float ndotd = dot3(ng, dir);
        const f3 ns = normalize3(normal_at(p, p0, p1, p2, n0, n1, n2));
        memcpy(w + 0, &id, 4);
        memcpy(w + 1, t + k, 4);
        memcpy(w + 2, &u, 4);
        memcpy(w + 3, &v, 4);
        put3(w + 4, p);
        memcpy(w + 7, &ndotd, 4);
        put3(w + 8, ng);
        put3(w + 12, ns);
    }
}

/* the rays the frame goes on with from each hit, from the attribute records alone: its reflection
 * ray {p + refl * 0.001f, refl}, refl = dir - (2 ns) dot(ns, dir), and its shadow ray {p + L * 0.001f,
 * L}, L = normalize(light - p), both with tmax = 2^32.  A miss gets two all-zero (invalid) rays. */
void ref_next_rays(const float* rays, const uint32_t* attrs, const float* light_pos, int64_t n, float* refl_rays,
                   float* shadow_rays) {
    const f3 light = ld3(light_pos);
    for (int64_t k = 0; k < n; ++k) {
        float a[16];
        memcpy(a, attrs + 16 * k, 64);
        float* rr = refl_rays + 8 * k;
        float* sr = shadow_rays + 8 * k;
        memset(rr, 0, 32);
        memset(sr, 0, 32);
        if ((int32_t)attrs[16 * k] < 0) continue;
        const f3 dir = normalize3(ld3(rays + 8 * k + 4));
        const f3 p = v3(a[4], a[5], a[6]), ns = v3(a[12], a[13], a[14]);
        const f3 refl = sub3(dir, muls(smul(2.0f, ns), dot3(ns, dir)));
        const f3 ro = add3(p, muls(refl, 0.001f));
        const f3 L = normalize3(sub3(light, p));
        const f3 so = add3(p, muls(L, 0.001f));
        rr[0] = ro.x; rr[1] = ro.y; rr[2] = ro.z; rr[3] = 4294967296.0f;
        rr[4] = refl.x; rr[5] = refl.y; rr[6] = refl.z;
        sr[0] = so.x; sr[1] = so.y; sr[2] = so.z; sr[3] = 4294967296.0f;
        sr[4] = L.x; sr[5] = L.y; sr[6] = L.z;
    }
}

/* normalize as the records' directions and normals go through it */
void ref_normalize(const float* in, float* out) {
    const f3 r = normalize3(ld3(in));
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
