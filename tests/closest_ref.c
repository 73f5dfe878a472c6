/* closest_ref.c -- the yardstick of the closest-point queries: a plain-C restatement
 * of the definition, written from the text and sharing no code with csrc/host/closest_core.hpp.
 * Compiled at test time with cc -O2 -ffp-contract=off (tests/closest_common.py).
 *
 *   closest_ref_brute     (a) every triangle of the mesh in id order: the minimum of f, lowest id on ties
 *   closest_ref_traverse  (b) the traversal over the caller's BVH_Node_ array, node by node, with the
 *                             visit counts, the overflow, the deepest stack and a watched node
 *   closest_ref_tri       f alone, for one point and one triangle given as three vertices
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct { float x, y, z, w; } f4;
typedef struct { f4 lo, hi; int32_t left, right, first, count; } node_t;   /* BVH_Node_, 48 B */
typedef struct { int32_t id; float d2, u, v, px, py, pz; uint32_t zero; } rec_t;   /* rt_closest, 32 B */

static float dot(const float a[3], const float b[3]) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }

/* f(q, p0, e1, e2): r = {u, v, px, py, pz, d2} */
static void tri_f(const float q[3], const float p0[3], const float e1[3], const float e2[3], float r[6]) {
    float ap[3], bp[3], cp[3], u, v;
    int k;
    for (k = 0; k < 3; ++k) ap[k] = q[k] - p0[k];
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; goto done; }
    for (k = 0; k < 3; ++k) bp[k] = ap[k] - e1[k];
    const float d3 = dot(e1, bp), d4 = dot(e2, bp);
    if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; goto done; }
    const float m14 = d1 * d4, m32 = d3 * d2;
    const float vc = m14 - m32;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; goto done; }
    for (k = 0; k < 3; ++k) cp[k] = ap[k] - e2[k];
    const float d5 = dot(e1, cp), d6 = dot(e2, cp);
    if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 1.0f; goto done; }
    const float m52 = d5 * d2, m16 = d1 * d6;
    const float vb = m52 - m16;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { u = 0.0f; v = d2 / (d2 - d6); goto done; }
    const float m36 = d3 * d6, m54 = d5 * d4;
    const float va = m36 - m54;
    const float a = d4 - d3, b = d5 - d6;
    if (va <= 0.0f && a >= 0.0f && b >= 0.0f) {
        const float w = a / (a + b);
        u = 1.0f - w;
        v = w;
        goto done;
    }
    {
        const float s = (va + vb) + vc;
        const float den = 1.0f / s;
        u = vb * den;
        v = vc * den;
    }
done:
    r[0] = u;
    r[1] = v;
    float df[3];
    for (k = 0; k < 3; ++k) {
        r[2 + k] = fmaf(v, e2[k], fmaf(u, e1[k], p0[k]));
        df[k] = q[k] - r[2 + k];
    }
    r[5] = dot(df, df);
}

void closest_ref_tri(const float* q, const float* v0, const float* v1, const float* v2, float* r6) {
    float e1[3], e2[3];
    int k;
    for (k = 0; k < 3; ++k) { e1[k] = v1[k] - v0[k]; e2[k] = v2[k] - v0[k]; }
    tri_f(q, v0, e1, e2, r6);
}

static int finite_f(float x) { return x == x && x != INFINITY && x != -INFINITY; }
static int valid_point(const f4* p) { return finite_f(p->x) && finite_f(p->y) && finite_f(p->z) && p->w > 0.0f; }

typedef struct { float best; int32_t bid; float r[6]; } answer_t;

static void test_triangle(const f4* verts, const int32_t* idx, int32_t id, const float q[3], answer_t* A) {
    const f4 *a = &verts[idx[id]], *b = &verts[idx[id + 1]], *c = &verts[idx[id + 2]];
    const float p0[3] = {a->x, a->y, a->z};
    const float e1[3] = {b->x - a->x, b->y - a->y, b->z - a->z};
    const float e2[3] = {c->x - a->x, c->y - a->y, c->z - a->z};
    float r[6];
    tri_f(q, p0, e1, e2, r);
    if (r[5] < A->best || (r[5] == A->best && A->bid >= 0 && id < A->bid)) {
        A->best = r[5];
        A->bid = id;
        memcpy(A->r, r, sizeof r);
    }
}

static void write_record(rec_t* o, const answer_t* A, int miss) {
    memset(o, 0, sizeof *o);
    if (miss || A->bid < 0) {
        o->id = -1;
        o->d2 = INFINITY;
        return;
    }
    o->id = A->bid;
    o->d2 = A->best;
    o->u = A->r[0]; o->v = A->r[1];
    o->px = A->r[2]; o->py = A->r[3]; o->pz = A->r[4];
}

void closest_ref_brute(const f4* verts, const int32_t* idx, int32_t ntri, const f4* pts, int64_t n, rec_t* out) {
    int64_t i;
    for (i = 0; i < n; ++i) {
        answer_t A;
        A.best = pts[i].w * pts[i].w;
        A.bid = -1;
        if (valid_point(&pts[i])) {
            const float q[3] = {pts[i].x, pts[i].y, pts[i].z};
            int32_t t;
            for (t = 0; t < ntri; ++t) test_triangle(verts, idx, 3 * t, q, &A);
        }
        write_record(&out[i], &A, 0);
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

/* stats3: NULL or {overflows, inner visits, triangle tests}; watch: a node index or -1, watched[i] = 1
 * where point i's traversal stood on it; deepest[i]: the largest stack count of point i (either may be NULL) */
void closest_ref_traverse(const f4* verts, const int32_t* idx, const node_t* nodes, int32_t nn, const int32_t* refs,
                          const f4* pts, int64_t n, rec_t* out, uint64_t* stats3, int32_t watch, uint8_t* watched,
                          int32_t* deepest) {
    uint64_t overflows = 0, inner = 0, tests = 0;
    int64_t i;
    for (i = 0; i < n; ++i) {
        answer_t A;
        int32_t stack[65];
        int sc = 1, miss = 0, deep = 0;
        A.best = pts[i].w * pts[i].w;
        A.bid = -1;
        if (watched) watched[i] = 0;
        stack[0] = 0;
        if (!valid_point(&pts[i])) sc = 0;
        const float q[3] = {pts[i].x, pts[i].y, pts[i].z};
        while (sc > 0) {
            const int32_t n0 = stack[sc - 1];
            const node_t* nd = &nodes[n0];
            if (sc > deep) deep = sc;
            if (watched && n0 == watch) watched[i] = 1;
            if (nd->left < 0) {   /* a leaf: its references in order */
                int32_t k;
                for (k = 0; k < nd->count; ++k) {
                    test_triangle(verts, idx, refs[nd->first + k], q, &A);
                    ++tests;
                }
                --sc;
                continue;
            }
            if (nd->right < 0 || nd->left >= nn || nd->right >= nn) {   /* a malformed inner node: an error miss */
                miss = 1;
                break;
            }
            ++inner;
            const float b0 = box_dist(&nodes[nd->left], q), b1 = box_dist(&nodes[nd->right], q);
            const int w0 = b0 >= 0.0f && b0 <= A.best, w1 = b1 >= 0.0f && b1 <= A.best;
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
        write_record(&out[i], &A, miss);
        if (deepest) deepest[i] = deep;
    }
    if (stats3) {
        stats3[0] = overflows;
        stats3[1] = inner;
        stats3[2] = tests;
    }
}
