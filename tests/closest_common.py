"""Shared by test_closest.py (CPU) and test_closest_gpu.py: the inputs and the yardsticks of the
closest-point queries.

Inputs, for a golden scene: 2,048 points, seed 11 -- half uniform in the scene box grown by 0.1 x its
diagonal, half a random triangle's random point plus N(0, 1e-3 x diagonal) noise -- under two radii,
+inf and 0.02 x the diagonal.

Yardsticks: tests/closest_ref.c, a plain-C restatement of the definition compiled here at test time
into a temporary folder (removed at exit) with cc -O2 -ffp-contract=off, as tests/fan_ref.c is: (a)
the brute force over all triangles, (b) the traversal over the BVH_Node_ array; and dist64 below, a
float64 numpy point-triangle distance by another method (the plane's foot point where it lies inside,
else the nearest of the three edge segments) that shares no code with either."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from ray_query_common import scene_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["cornell12", "rand2k", "hf40k", "knot16k", "cubes2_obj", "rand3k_bigleaf", "rand4k_sbvh"]
RADII = ["inf", "r02"]
N_POINTS = 2048
SEED = 11
F32 = np.float32
MISS_WORDS = np.array([0xFFFFFFFF, 0x7F800000, 0, 0, 0, 0, 0, 0], np.uint32)

_lib = None
_POINTS = {}
_YARD = {}
_SCENES = {}


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="rtamd_closest_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "closest_ref.so")
        subprocess.run(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(HERE, "closest_ref.c"), "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.closest_ref_brute.restype = None
        L.closest_ref_brute.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp]
        L.closest_ref_traverse.restype = None
        L.closest_ref_traverse.argtypes = [vp, vp, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, C.c_int32, vp, vp]
        L.closest_ref_tri.restype = None
        L.closest_ref_tri.argtypes = [vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def words(rec):
    """rt_closest (or rt_point) records of any dtype as uint32 (n, words per record), contiguous."""
    a = np.ascontiguousarray(rec)
    return a.view(np.uint8).reshape(-1).view(np.uint32).reshape(a.shape[0], a.itemsize * int(np.prod(a.shape[1:], dtype=np.int64)) // 4)


def _mesh(d):
    return (np.ascontiguousarray(d["vertices"], F32).reshape(-1, 4), np.ascontiguousarray(d["indices"], np.int32).reshape(-1))


def diagonal(d):
    v = d["vertices"][:, :3].astype(np.float64)
    return float(np.sqrt(np.sum((v.max(0) - v.min(0)) ** 2)))


def radius(d, which):
    return F32(np.inf) if which == "inf" else F32(0.02 * diagonal(d))


def make_points(d, n=N_POINTS, seed=SEED):
    """float32 (n, 3): the two halves interleaved (even: uniform, odd: near the surface)."""
    v = d["vertices"][:, :3].astype(np.float64)
    idx = np.asarray(d["indices"]).reshape(-1, 3)
    lo, hi, dg = v.min(0), v.max(0), diagonal(d)
    rng = np.random.default_rng(seed)
    half = n // 2
    uni = rng.uniform(lo - 0.1 * dg, hi + 0.1 * dg, (half, 3))
    t = rng.integers(0, idx.shape[0], n - half)
    b = rng.dirichlet((1.0, 1.0, 1.0), n - half)
    tri = v[idx[t]]                                           # (m, 3 vertices, 3)
    near = np.einsum("mk,mkc->mc", b, tri) + rng.normal(0.0, 1e-3 * dg, (n - half, 3))
    out = np.empty((n, 3), F32)
    out[0::2], out[1::2] = uni.astype(F32), near.astype(F32)
    return out


def points(name):
    """The 2,048 points of a fixture, computed once (shared; do not modify)."""
    if name not in _POINTS:
        _POINTS[name] = make_points(scene_arrays(name))
    return _POINTS[name]


def records(name, which):
    import rtamd
    return rtamd.pack_points(points(name), radius(scene_arrays(name), which))


def brute(d, rec):
    """(a): rt_closest words uint32 (n, 8) of the brute force over all triangles of d's mesh."""
    v, idx = _mesh(d)
    pw = words(rec)
    out = np.zeros((pw.shape[0], 8), np.uint32)
    lib().closest_ref_brute(_p(v), _p(idx), idx.size // 3, _p(pw), pw.shape[0], _p(out))
    return out


def traverse(d, rec, watch=-1):
    """(b): (words uint32 (n, 8), {overflows, inner_visits, tri_tests}, watched bool (n,), deepest int32
    (n,)) of the traversal over d's BVH_Node_ array."""
    v, idx = _mesh(d)
    nodes = np.ascontiguousarray(d["nodes"], F32).reshape(-1, 12)
    refs = np.ascontiguousarray(d["tri_indices"], np.int32).reshape(-1)
    pw = words(rec)
    n = pw.shape[0]
    out = np.zeros((n, 8), np.uint32)
    st = np.zeros(3, np.uint64)
    watched = np.zeros(n, np.uint8)
    deepest = np.zeros(n, np.int32)
    lib().closest_ref_traverse(_p(v), _p(idx), _p(nodes), nodes.shape[0], _p(refs), _p(pw), n, _p(out), _p(st), watch,
                               _p(watched), _p(deepest))
    return out, {"overflows": int(st[0]), "inner_visits": int(st[1]), "tri_tests": int(st[2])}, watched.astype(bool), deepest


def ref_tri(q, v0, v1, v2):
    """f of closest_ref.c for one point and one triangle: float32 [u, v, px, py, pz, d2]."""
    a = [np.ascontiguousarray(x, F32) for x in (q, v0, v1, v2)]
    r = np.zeros(6, F32)
    lib().closest_ref_tri(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(r))
    return r


def yardstick(name, which):
    """((a) words, (b) words, (b) stats, deepest) of a fixture's points under a radius, computed once
    (shared; do not modify)."""
    if (name, which) not in _YARD:
        d = scene_arrays(name)
        rec = records(name, which)
        b, st, _, deep = traverse(d, rec)
        _YARD[(name, which)] = (brute(d, rec), b, st, deep)
    return _YARD[(name, which)]


def _seg_d2(q, a, b):
    """float64 squared distance of points q (n, 1, 3) to segments a-b (1, m, 3)."""
    ab = b - a
    den = np.sum(ab * ab, axis=-1)
    t = np.sum((q - a) * ab, axis=-1) / np.where(den > 0.0, den, 1.0)
    t = np.clip(np.where(den > 0.0, t, 0.0), 0.0, 1.0)
    c = a + t[..., None] * ab
    return np.sum((q - c) ** 2, axis=-1)


def _tri_d2(qq, a, b, c, nrm, nn, ok):
    """float64 squared distances of points qq (n, 1, 3) to triangles a, b, c (1, m, 3)."""
    best = np.minimum(np.minimum(_seg_d2(qq, a, b), _seg_d2(qq, b, c)), _seg_d2(qq, c, a))
    # the foot point on the plane, where it lies inside the triangle (three same-side tests)
    h = np.sum((qq - a) * nrm[None], axis=-1)
    foot = qq - (h / np.where(ok, nn, 1.0))[..., None] * nrm[None]
    inside = ok[None]
    for (x, y) in ((a, b), (b, c), (c, a)):
        inside = inside & (np.sum(np.cross(y - x, foot - x) * nrm[None], axis=-1) >= 0.0)
    face = h * h / np.where(ok, nn, 1.0)
    return np.where(inside, np.minimum(best, face), best)


def dist64(d, q, chunk=64):
    """The float64 minimum distance of each point q (n, 3) to the mesh, the triangles formed as the
    records form them (p0, p0 + fl(p1 - p0), p0 + fl(p2 - p0)).  Per point only the triangles whose
    bounding box is no farther than the nearest first vertex are evaluated: the minimum is among them."""
    v = d["vertices"][:, :3].astype(F32)
    idx = np.asarray(d["indices"]).reshape(-1, 3)
    p0 = v[idx[:, 0]]
    e1, e2 = (v[idx[:, 1]] - p0).astype(F32).astype(np.float64), (v[idx[:, 2]] - p0).astype(F32).astype(np.float64)
    a = p0.astype(np.float64)
    b, c = a + e1, a + e2
    nrm = np.cross(e1, e2)
    nn = np.sum(nrm * nrm, axis=-1)
    ok = nn > 0.0
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    out = np.empty(q.shape[0], np.float64)
    for s in range(0, q.shape[0], chunk):
        qq = q[s:s + chunk].astype(np.float64)
        gap = np.maximum(np.maximum(lo[None] - qq[:, None], qq[:, None] - hi[None]), 0.0)
        lower = np.sum(gap * gap, axis=-1)
        upper = np.min(np.sum((qq[:, None] - a[None]) ** 2, axis=-1), axis=1)
        for i in range(qq.shape[0]):
            k = np.flatnonzero(lower[i] <= upper[i])
            d2 = _tri_d2(qq[i][None, None, :], a[k][None], b[k][None], c[k][None], nrm[k], nn[k], ok[k])
            out[s + i] = np.sqrt(d2.min())
    return out


# ---- hand-made scenes ----

def comb40():
    """overflow_comb cut to 40 levels, as ray_edge_common.deep_comb40 cuts it, with the mesh cut to the
    40 triangles its leaves hold (ids unchanged), so that the brute force ranges over what the tree holds."""
    if "comb40" not in _SCENES:
        from ray_edge_common import deep_comb40
        d = dict(deep_comb40())
        d["indices"] = d["indices"][:120].copy()
        d["normals_indices"] = d["normals_indices"][:120].copy()
        d["tri_to_material"] = d["tri_to_material"][:40].copy()
        _SCENES["comb40"] = d
    return _SCENES["comb40"]


# rand2k's node whose box is shrunk: depth 4.  Chosen by yardstick (b): 4 of the 2,048 points change against the
# brute force, and restatements of (b) that re-test a popped reference against `best`, or visit the farther child
# first, each change 30 more -- which is what makes the tree pin the visit order and the unconditional pop.
WRONG_BOX_NODE = 4


def wrong_box(node=None):
    """rand2k with one mid-tree node's box shrunk to half its size about its centre: the boxes no
    longer contain their triangles, so the answer depends on the visit order."""
    node = WRONG_BOX_NODE if node is None else node
    key = ("wrong_box", node)
    if key not in _SCENES:
        d = dict(scene_arrays("rand2k"))
        nodes = np.array(d["nodes"], F32, copy=True)
        lo, hi = nodes[node, 0:3].astype(np.float64), nodes[node, 4:7].astype(np.float64)
        c, h = 0.5 * (lo + hi), 0.25 * (hi - lo)
        nodes[node, 0:3], nodes[node, 4:7] = (c - h).astype(F32), (c + h).astype(F32)
        d["nodes"] = nodes
        _SCENES[key] = d
    return _SCENES[key]


def escape_tree():
    """The hand-made escape-leaf tree of test_lbvh_keys_gpu.py: the first 42 triangles of rand2k in
    leaves of 40 and 2 (a count of 31 or more goes through the escape table), boxes refitted."""
    if "escape" not in _SCENES:
        from refit_common import np_refit
        d = dict(scene_arrays("rand2k"))
        refs = 3 * np.arange(42, dtype=np.int32)
        nodes = np.zeros((3, 12), F32)
        nodes[:, 3] = nodes[:, 7] = 1.0
        nodes.view(np.int32)[:, 8:12] = [[1, 2, -1, 0], [-1, -1, 0, 40], [-1, -1, 40, 2]]
        nodes, _ = np_refit({"nodes": nodes, "tri_indices": refs, "indices": d["indices"]}, d["vertices"])
        d["indices"] = d["indices"][:126].copy()
        d["normals_indices"] = d["normals_indices"][:126].copy()
        d["tri_to_material"] = d["tri_to_material"][:42].copy()
        d["nodes"], d["tri_indices"] = nodes, refs
        _SCENES["escape"] = d
    return _SCENES["escape"]


def two_tri_scene(tris):
    """A scene of the given triangles ((m, 3, 3) float32) in one root leaf."""
    t = np.asarray(tris, F32).reshape(-1, 3, 3)
    m = t.shape[0]
    v = np.zeros((3 * m, 4), F32)
    v[:, :3] = t.reshape(-1, 3)
    v[:, 3] = 1.0
    nodes = np.zeros((1, 12), F32)
    fin = t.reshape(-1, 3)
    nodes[0, 0:3], nodes[0, 4:7] = fin.min(0), fin.max(0)
    nodes[0, 3] = nodes[0, 7] = 1.0
    nodes.view(np.int32)[0, 8:12] = [-1, -1, 0, m]
    mats = np.zeros((1, 44), F32)
    return dict(vertices=v, indices=np.arange(3 * m, dtype=np.int32), nodes=nodes, tri_indices=3 * np.arange(m, dtype=np.int32),
                normals=np.array([[0, 0, 1, 0]], F32), normals_indices=np.zeros(3 * m, np.int32), materials=mats,
                tri_to_material=np.zeros(m, np.int32), scene_min=fin.min(0), scene_max=fin.max(0))


def morton_order(q):
    """The permutation that sorts float32 (n, 3) points by a 30-bit Morton code of their box."""
    lo, hi = q.min(0).astype(np.float64), q.max(0).astype(np.float64)
    c = np.minimum(((q - lo) / np.where(hi > lo, hi - lo, 1.0) * 1024.0).astype(np.int64), 1023)
    code = np.zeros(q.shape[0], np.int64)
    for bit in range(10):
        for ax in range(3):
            code |= ((c[:, ax] >> bit) & 1) << (3 * bit + ax)
    return np.argsort(code, kind="stable")


def edge_points(d):
    """The edge set on scene d: (records, what each is).  Coordinates non-finite; r NaN, 0, -0, -1, the
    smallest subnormal, 1e-30 (r * r underflows to 0), 1e30 (r * r = inf), +inf."""
    import rtamd
    v = d["vertices"][:, :3]
    c = (0.5 * (v.min(0).astype(np.float64) + v.max(0))).astype(F32)
    q, r, what = [], [], []
    for bad, label in ((np.nan, "nan"), (np.inf, "+inf"), (-np.inf, "-inf")):
        for ax in range(3):
            p = c.copy()
            p[ax] = bad
            q.append(p); r.append(F32(np.inf)); what.append(f"coordinate {ax} {label}")
    for rv, label in ((np.nan, "r nan"), (0.0, "r 0"), (-0.0, "r -0"), (-1.0, "r -1"), (1e-45, "r subnormal"),
                      (1e-30, "r 1e-30"), (1e30, "r 1e30"), (np.inf, "r +inf")):
        q.append(c.copy()); r.append(F32(rv)); what.append(label)
    return rtamd.pack_points(np.array(q, F32), np.array(r, F32)), what
