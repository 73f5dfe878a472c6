/* multihit_ref.c -- the yardstick of the first-k-hits ray queries: a plain-C
 * restatement of the definition in S_strict, written from the text and sharing no code with
 * csrc/host/multihit_core.hpp or csrc/host/multihit.cpp.  Compiled at test time with
 * cc -O2 -ffp-contract=off (tests/multihit_common.py).  Rays are rt_ray (8 words), output is k planes
 * of n records {id, t, u, v}: out[j * n + i].
 *
 *   multihit_ref_brute     (a) ray_tri on every triangle of the mesh, then the k smallest (t, id) with
 *                              0.001f < t < tmax
 *   multihit_ref_traverse  (b) the traversal over the caller's BVH_Node_ array with the list, the visit
 *                              counts, the overflow and the deepest stack; presence = 0 leaves the
 *                              presence check out (the restatement that shows the duplicate sets bite)
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAXK 16
#define TMIN 0.001f

typedef struct { float x, y, z, w; } f4;
typedef struct { f4 lo, hi; int32_t left, right, first, count; } node_t;   /* BVH_Node_, 48 B */
typedef struct { float ox, oy, oz, tmax, dx, dy, dz; uint32_t reserved; } ray_t;   /* rt_ray, 32 B */
typedef struct { int32_t id; float t, u, v; } rec_t;                      /* rt_hit_uv, 16 B */

static float dot(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
static void cross(const float a[3], const float b[3], float o[3]) {
    o[0] = fmaf(a[1], b[2], b[1] * -a[2]);
    o[1] = fmaf(a[2], b[0], b[2] * -a[0]);
    o[2] = fmaf(a[0], b[1], b[0] * -a[1]);
}

/* the direction a ray travels along: ray_init's normalize, rsqrt in binary64 */
static void unit(const float d[3], float o[3]) {
    float p[3] = {d[0], d[1], d[2]}, l2, s;
    int k;
    l2 = dot(p, p);
    if (l2 < 1.17549435e-38f) {
        for (k = 0; k < 3; ++k) p[k] = p[k] * 0x1p86f;
        l2 = dot(p, p);
    } else if (l2 == INFINITY) {
        for (k = 0; k < 3; ++k) p[k] = p[k] * 0x1p-66f;
        l2 = dot(p, p);
        if (l2 == INFINITY) {
            for (k = 0; k < 3; ++k) p[k] = copysignf(isinf(p[k]) ? 1.0f : 0.0f, p[k]);
            l2 = dot(p, p);
        }
    }
    s = (float)(1.0 / sqrt((double)l2));
    for (k = 0; k < 3; ++k) o[k] = p[k] * s;
}

/* Moller-Trumbore: t, or -1 outside; u and v by the same lines whatever the outcome */
static float ray_tri(const float o[3], const float d[3], const float v0[3], const float e1[3], const float e2[3], float* uo,
                     float* vo) {
    float tvec[3], pvec[3], qvec[3], det, u, v;
    int k;
    for (k = 0; k < 3; ++k) tvec[k] = o[k] - v0[k];
    cross(d, e2, pvec);
    det = dot(e1, pvec);
    det = 1.0f / det;
    u = dot(tvec, pvec) * det;
    cross(tvec, e1, qvec);
    v = dot(d, qvec) * det;
    *uo = u;
    *vo = v;
    if (u < 0.0f || u > 1.0f) return -1.0f;
    if (v < 0.0f || (u + v) > 1.0f) return -1.0f;
    return dot(e2, qvec) * det;
}

static void tri_of_mesh(const f4* verts, const int32_t* idx, int32_t id, const float o[3], const float d[3], rec_t* c) {
    const f4 *a = &verts[idx[id]], *b = &verts[idx[id + 1]], *cc = &verts[idx[id + 2]];
    const float p0[3] = {a->x, a->y, a->z};
    const float e1[3] = {b->x - a->x, b->y - a->y, b->z - a->z};
    const float e2[3] = {cc->x - a->x, cc->y - a->y, cc->z - a->z};
    c->t = ray_tri(o, d, p0, e1, e2, &c->u, &c->v);
    c->id = id;
}

static int is_finite(float x) { return x - x == 0.0f; }
static int valid_ray(const ray_t* r) {
    return is_finite(r->ox) && is_finite(r->oy) && is_finite(r->oz) && is_finite(r->dx) && is_finite(r->dy) && is_finite(r->dz) &&
           !(r->dx == 0.0f && r->dy == 0.0f && r->dz == 0.0f) && r->tmax > TMIN;
}

/* the miss record: the ray's tmax WORD */
static void miss_record(const ray_t* r, rec_t* o) {
    o->id = -1;
    memcpy(&o->t, &r->tmax, 4);
    o->u = 0.0f;
    o->v = 0.0f;
}

/* (t, id) of a before (t, id) of b */
static int precedes(const rec_t* a, const rec_t* b) { return a->t < b->t || (a->t == b->t && a->id < b->id); }

/* (a): k <= MAXK */
void multihit_ref_brute(const f4* verts, const int32_t* idx, int32_t ntri, const ray_t* rays, int64_t n, int32_t k, rec_t* out) {
    int64_t i;
    for (i = 0; i < n; ++i) {
        rec_t keep[MAXK];
        int have = 0, j;
        if (valid_ray(&rays[i])) {
            const float o[3] = {rays[i].ox, rays[i].oy, rays[i].oz}, d0[3] = {rays[i].dx, rays[i].dy, rays[i].dz};
            float d[3];
            int32_t t;
            unit(d0, d);
            for (t = 0; t < ntri; ++t) {
                rec_t c;
                int at = 0;
                tri_of_mesh(verts, idx, 3 * t, o, d, &c);
                if (!(c.t > TMIN && c.t < rays[i].tmax)) continue;
                for (j = 0; j < have; ++j) at += precedes(&keep[j], &c);   /* its rank among the kept */
                if (at >= k) continue;
                if (have < k) ++have;
                for (j = have - 1; j > at; --j) keep[j] = keep[j - 1];
                keep[at] = c;
            }
        }
        for (j = 0; j < k; ++j) {
            if (j < have) out[(int64_t)j * n + i] = keep[j];
            else miss_record(&rays[i], &out[(int64_t)j * n + i]);
        }
    }
}

/* the slab test of one box: near and far parameter, IEEE quotients, the reference's nesting */
static void slab(const node_t* nd, const float o[3], const float d[3], float* nearp, float* farp) {
    const float lo[3] = {nd->lo.x, nd->lo.y, nd->lo.z}, hi[3] = {nd->hi.x, nd->hi.y, nd->hi.z};
    float mn[3], mx[3];
    int k;
    for (k = 0; k < 3; ++k) {
        const float a = (lo[k] - o[k]) / d[k], b = (hi[k] - o[k]) / d[k];
        mn[k] = fminf(a, b);
        mx[k] = fmaxf(a, b);
    }
    *nearp = fmaxf(fmaxf(mn[0], mn[1]), mn[2]);
    *farp = fminf(fminf(mx[0], mx[1]), mx[2]);
}

/* the candidate of a triangle test against the list L[0 .. k-1]: range, presence, acceptance, insertion */
static void candidate(rec_t* L, int k, const rec_t* c, int presence) {
    int j, at;
    const rec_t* last = &L[k - 1];
    if (!(c->t > TMIN)) return;
    if (presence)
        for (j = 0; j < k; ++j)
            if (L[j].id == c->id) return;
    if (!(c->t < last->t || (c->t == last->t && last->id >= 0 && c->id < last->id))) return;
    for (at = 0; at < k - 1; ++at)
        if (precedes(c, &L[at])) break;
    for (j = k - 1; j > at; --j) L[j] = L[j - 1];
    L[at] = *c;
}

/* (b).  stats3: NULL or {overflows, inner visits, triangle tests}; deepest[i]: the largest stack count
 * of ray i (may be NULL) */
void multihit_ref_traverse(const f4* verts, const int32_t* idx, const node_t* nodes, int32_t nn, const int32_t* refs,
                           const ray_t* rays, int64_t n, int32_t k, rec_t* out, uint64_t* stats3, int32_t* deepest,
                           int32_t presence) {
    uint64_t overflows = 0, inner = 0, tests = 0;
    int64_t i;
    for (i = 0; i < n; ++i) {
        rec_t L[MAXK];
        int32_t stack[65];
        int sc = 1, miss = 0, deep = 0, j;
        const float o[3] = {rays[i].ox, rays[i].oy, rays[i].oz}, d0[3] = {rays[i].dx, rays[i].dy, rays[i].dz};
        float d[3];
        for (j = 0; j < k; ++j) {
            L[j].id = -1;
            L[j].t = rays[i].tmax;
            L[j].u = L[j].v = 0.0f;
        }
        stack[0] = 0;
        if (!valid_ray(&rays[i])) sc = 0;
        unit(d0, d);
        while (sc > 0) {
            const node_t* nd = &nodes[stack[sc - 1]];
            if (sc > deep) deep = sc;
            if (nd->left < 0) {   /* a leaf: its references in order, all of them */
                int32_t t;
                for (t = 0; t < nd->count; ++t) {
                    rec_t c;
                    tri_of_mesh(verts, idx, refs[nd->first + t], o, d, &c);
                    ++tests;
                    candidate(L, k, &c, presence);
                }
                --sc;
                continue;
            }
            if (nd->right < 0 || nd->left >= nn || nd->right >= nn) {   /* a malformed inner node: an error miss */
                miss = 1;
                break;
            }
            ++inner;
            {
                const float bound = L[k - 1].t;
                float n0, f0, n1, f1;
                int w0, w1;
                slab(&nodes[nd->left], o, d, &n0, &f0);
                slab(&nodes[nd->right], o, d, &n1, &f1);
                w0 = (n0 <= f0) && (f0 >= TMIN) && (n0 <= bound);
                w1 = (n1 <= f1) && (f1 >= TMIN) && (n1 <= bound);
                if (w0 && w1) {
                    if (sc >= 65) {
                        miss = 1;
                        ++overflows;
                        break;
                    }
                    {
                        const int far_is_left = n0 > n1;   /* near first, a tie goes left */
                        stack[sc - 1] = far_is_left ? nd->left : nd->right;
                        stack[sc] = far_is_left ? nd->right : nd->left;
                        ++sc;
                    }
                } else if (w0) {
                    stack[sc - 1] = nd->left;
                } else if (w1) {
                    stack[sc - 1] = nd->right;
                } else {
                    --sc;
                }
            }
        }
        for (j = 0; j < k; ++j) {
            if (miss || L[j].id < 0) miss_record(&rays[i], &out[(int64_t)j * n + i]);
            else out[(int64_t)j * n + i] = L[j];
        }
        if (deepest) deepest[i] = deep;
    }
    if (stats3) {
        stats3[0] = overflows;
        stats3[1] = inner;
        stats3[2] = tests;
    }
}
