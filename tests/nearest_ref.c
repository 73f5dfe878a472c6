/* nearest_ref.c -- the yardstick of the k-nearest-triangle queries: a plain-C
 * restatement of the definition, written from the text and sharing no code with
 * csrc/host/closest_core.hpp.  Compiled at test time with cc -O2 -ffp-contract=off
 * (tests/nearest_common.py).  Output is k planes of n records: out[j * n + i].
 *
 *   nearest_ref_brute     (a) f on every triangle of the mesh, then the k smallest (d2, id) with d2 < r * r
 *   nearest_ref_traverse  (b) the traversal over the caller's BVH_Node_ array with the list, the visit
 *                             counts, the overflow and the deepest stack; presence = 0 leaves the
 *                             presence check out (the restatement that shows the duplicate set bites)
 *   nearest_ref_tri       f alone, for one point and one triangle given as three vertices
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAXK 16

typedef struct { float x, y, z, w; } f4;
typedef struct { f4 lo, hi; int32_t left, right, first, count; } node_t;   /* BVH_Node_, 48 B */
typedef struct { int32_t id; float d2, u, v, px, py, pz; uint32_t zero; } rec_t;   /* rt_closest, 32 B */

static float dot(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }

/* f(q, p0, e1, e2): the region walk; o = {id unset, d2, u, v, p} */
static void tri_f(const float q[3], const float p0[3], const float e1[3], const float e2[3], rec_t* o) {
    float ap[3], bp[3], cp[3], u, v, p[3], df[3];
    int k;
    for (k = 0; k < 3; ++k) {
        ap[k] = q[k] - p0[k];
        bp[k] = ap[k] - e1[k];
        cp[k] = ap[k] - e2[k];
    }
    const float d1 = dot(e1, ap), d2 = dot(e2, ap), d3 = dot(e1, bp), d4 = dot(e2, bp), d5 = dot(e1, cp), d6 = dot(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
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
    } else if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) {
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        u = 1.0f - w; v = w;
    } else {
        const float den = 1.0f / ((va + vb) + vc);
        u = vb * den; v = vc * den;
    }
    for (k = 0; k < 3; ++k) {
        p[k] = fmaf(v, e2[k], fmaf(u, e1[k], p0[k]));
        df[k] = q[k] - p[k];
    }
    o->d2 = dot(df, df);
    o->u = u; o->v = v;
    o->px = p[0]; o->py = p[1]; o->pz = p[2];
    o->zero = 0;
}

void nearest_ref_tri(const float* q, const float* v0, const float* v1, const float* v2, float* r6) {
    float e1[3], e2[3];
    rec_t o;
    int k;
    for (k = 0; k < 3; ++k) { e1[k] = v1[k] - v0[k]; e2[k] = v2[k] - v0[k]; }
    tri_f(q, v0, e1, e2, &o);
    r6[0] = o.u; r6[1] = o.v; r6[2] = o.px; r6[3] = o.py; r6[4] = o.pz; r6[5] = o.d2;
}

static void tri_of_mesh(const f4* verts, const int32_t* idx, int32_t id, const float q[3], rec_t* o) {
    const f4 *a = &verts[idx[id]], *b = &verts[idx[id + 1]], *c = &verts[idx[id + 2]];
    const float p0[3] = {a->x, a->y, a->z};
    const float e1[3] = {b->x - a->x, b->y - a->y, b->z - a->z};
    const float e2[3] = {c->x - a->x, c->y - a->y, c->z - a->z};
    tri_f(q, p0, e1, e2, o);
    o->id = id;
}

static int is_finite(float x) { return x - x == 0.0f; }
static int valid_point(const f4* p) { return is_finite(p->x) && is_finite(p->y) && is_finite(p->z) && p->w > 0.0f; }

static void miss_record(rec_t* o) {
    memset(o, 0, sizeof *o);
    o->id = -1;
    o->d2 = INFINITY;
}

/* (d2, id) of a before (d2, id) of b */
static int precedes(const rec_t* a, const rec_t* b) { return a->d2 < b->d2 || (a->d2 == b->d2 && a->id < b->id); }

/* (a): k <= MAXK */
void nearest_ref_brute(const f4* verts, const int32_t* idx, int32_t ntri, const f4* pts, int64_t n, int32_t k, rec_t* out) {
    int64_t i;
    for (i = 0; i < n; ++i) {
        rec_t keep[MAXK];
        int have = 0, j;
        if (valid_point(&pts[i])) {
            const float q[3] = {pts[i].x, pts[i].y, pts[i].z};
            const float r2 = pts[i].w * pts[i].w;
            int32_t t;
            for (t = 0; t < ntri; ++t) {
                rec_t c;
                int at = 0;
                tri_of_mesh(verts, idx, 3 * t, q, &c);
                if (!(c.d2 < r2)) continue;
                for (j = 0; j < have; ++j) at += precedes(&keep[j], &c);   /* its rank among the kept */
                if (at >= k) continue;
                if (have < k) ++have;
                for (j = have - 1; j > at; --j) keep[j] = keep[j - 1];
                keep[at] = c;
            }
        }
        for (j = 0; j < k; ++j) {
            if (j < have) out[(int64_t)j * n + i] = keep[j];
            else miss_record(&out[(int64_t)j * n + i]);
        }
    }
}

/* squared distance to a node's box; -1 (never wanted) where a box word is NaN */
static float box_dist(const node_t* nd, const float q[3]) {
    const float lo[3] = {nd->lo.x, nd->lo.y, nd->lo.z}, hi[3] = {nd->hi.x, nd->hi.y, nd->hi.z};
    float e[3];
    int k;
    for (k = 0; k < 3; ++k) {
        if (lo[k] != lo[k] || hi[k] != hi[k]) return -1.0f;
        e[k] = fmaxf(fmaxf(lo[k] - q[k], q[k] - hi[k]), 0.0f);
    }
    return dot(e, e);
}

/* the candidate of a triangle test against the list L[0 .. k-1]: presence, acceptance, insertion */
static void candidate(rec_t* L, int k, const rec_t* c, int presence) {
    int j, at;
    if (presence)
        for (j = 0; j < k; ++j)
            if (L[j].id == c->id) return;
    const rec_t* last = &L[k - 1];
    if (!(c->d2 < last->d2 || (c->d2 == last->d2 && last->id >= 0 && c->id < last->id))) return;
    for (at = 0; at < k - 1; ++at)
        if (precedes(c, &L[at])) break;
    for (j = k - 1; j > at; --j) L[j] = L[j - 1];
    L[at] = *c;
}

/* (b).  stats3: NULL or {overflows, inner visits, triangle tests}; deepest[i]: the largest stack count
 * of point i (may be NULL) */
void nearest_ref_traverse(const f4* verts, const int32_t* idx, const node_t* nodes, int32_t nn, const int32_t* refs,
                          const f4* pts, int64_t n, int32_t k, rec_t* out, uint64_t* stats3, int32_t* deepest, int32_t presence) {
    uint64_t overflows = 0, inner = 0, tests = 0;
    int64_t i;
    for (i = 0; i < n; ++i) {
        rec_t L[MAXK];
        int32_t stack[65];
        int sc = 1, miss = 0, deep = 0, j;
        for (j = 0; j < k; ++j) {
            memset(&L[j], 0, sizeof L[j]);
            L[j].id = -1;
            L[j].d2 = pts[i].w * pts[i].w;
        }
        stack[0] = 0;
        if (!valid_point(&pts[i])) sc = 0;
        const float q[3] = {pts[i].x, pts[i].y, pts[i].z};
        while (sc > 0) {
            const int32_t n0 = stack[sc - 1];
            const node_t* nd = &nodes[n0];
            if (sc > deep) deep = sc;
            if (nd->left < 0) {   /* a leaf: its references in order */
                int32_t t;
                for (t = 0; t < nd->count; ++t) {
                    rec_t c;
                    tri_of_mesh(verts, idx, refs[nd->first + t], q, &c);
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
            const float bound = L[k - 1].d2;
            const float b0 = box_dist(&nodes[nd->left], q), b1 = box_dist(&nodes[nd->right], q);
            const int w0 = b0 >= 0.0f && b0 <= bound, w1 = b1 >= 0.0f && b1 <= bound;
            if (w0 && w1) {
                if (sc >= 65) {
                    miss = 1;
                    ++overflows;
                    break;
                }
                const int far_is_left = b0 > b1;   /* near first, a tie goes left */
                stack[sc - 1] = far_is_left ? nd->left : nd->right;
                stack[sc] = far_is_left ? nd->right : nd->left;
                ++sc;
            } else if (w0) {
                stack[sc - 1] = nd->left;
            } else if (w1) {
                stack[sc - 1] = nd->right;
            } else {
                --sc;
            }
        }
        for (j = 0; j < k; ++j) {
            if (miss || L[j].id < 0) miss_record(&out[(int64_t)j * n + i]);
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
