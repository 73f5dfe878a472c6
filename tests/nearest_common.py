"""Shared by test_nearest_k.py (CPU) and test_nearest_k_gpu.py: the inputs and the yardsticks of the
k-nearest-triangle queries.

Inputs are closest_common's (2,048 points per fixture, seed 11, two radii) and the duplicate set: 16
points on each triangle that the tree references from more than one leaf.

Yardsticks: tests/nearest_ref.c, a plain-C restatement of the definition compiled here at test time
into a temporary folder (removed at exit) with cc -O2 -ffp-contract=off: (a) f on every triangle and
the k smallest (d2, id) below r * r, (b) the traversal over the BVH_Node_ array with the list.  Results
are words uint32 (k, n, 8): plane j, point i."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import closest_common as K
from ray_query_common import scene_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
MAX_K = 8
BRUTE_K = 9   # (a) is computed once with nine planes: the planes of a smaller k are its first k
MISS_WORDS = K.MISS_WORDS

_lib = None
_BRUTE = {}
_TRAV = {}
_DUP = {}


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="rtamd_nearest_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "nearest_ref.so")
        subprocess.run(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(HERE, "nearest_ref.c"), "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        vp, i32 = C.c_void_p, C.c_int32
        L.nearest_ref_brute.restype = None
        L.nearest_ref_brute.argtypes = [vp, vp, i32, vp, C.c_int64, i32, vp]
        L.nearest_ref_traverse.restype = None
        L.nearest_ref_traverse.argtypes = [vp, vp, vp, i32, vp, vp, C.c_int64, i32, vp, vp, vp, i32]
        L.nearest_ref_tri.restype = None
        L.nearest_ref_tri.argtypes = [vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def planes(rec):
    """rt_closest records (k, n) of CLOSEST_DTYPE, or words already, as uint32 (k, n, 8)."""
    a = np.ascontiguousarray(rec)
    if a.dtype == np.uint32:
        return a
    return a.view(np.uint8).reshape(-1).view(np.uint32).reshape(a.shape[0], a.shape[1], 8)


def brute(d, rec, k):
    """(a): words uint32 (k, n, 8), k up to 16."""
    v, idx = K._mesh(d)
    pw = K.words(rec)
    out = np.zeros((k, pw.shape[0], 8), np.uint32)
    lib().nearest_ref_brute(_p(v), _p(idx), idx.size // 3, _p(pw), pw.shape[0], k, _p(out))
    return out


def traverse(d, rec, k, presence=True):
    """(b): (words uint32 (k, n, 8), {overflows, inner_visits, tri_tests}, deepest int32 (n,))."""
    v, idx = K._mesh(d)
    nodes = np.ascontiguousarray(d["nodes"], F32).reshape(-1, 12)
    refs = np.ascontiguousarray(d["tri_indices"], np.int32).reshape(-1)
    pw = K.words(rec)
    n = pw.shape[0]
    out = np.zeros((k, n, 8), np.uint32)
    st = np.zeros(3, np.uint64)
    deepest = np.zeros(n, np.int32)
    lib().nearest_ref_traverse(_p(v), _p(idx), _p(nodes), nodes.shape[0], _p(refs), _p(pw), n, k, _p(out), _p(st),
                               _p(deepest), 1 if presence else 0)
    return out, {"overflows": int(st[0]), "inner_visits": int(st[1]), "tri_tests": int(st[2])}, deepest


def ref_tri(q, v0, v1, v2):
    """f of nearest_ref.c for one point and one triangle: float32 [u, v, px, py, pz, d2]."""
    a = [np.ascontiguousarray(x, F32) for x in (q, v0, v1, v2)]
    r = np.zeros(6, F32)
    lib().nearest_ref_tri(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(r))
    return r


def brute9(name, which):
    """(a) with nine planes for a fixture's points under a radius, computed once (shared; do not modify)."""
    if (name, which) not in _BRUTE:
        _BRUTE[(name, which)] = brute(scene_arrays(name), K.records(name, which), BRUTE_K)
    return _BRUTE[(name, which)]


def traversal(name, which, k):
    """(b) for a fixture's points under a radius, computed once per k (shared; do not modify)."""
    if (name, which, k) not in _TRAV:
        _TRAV[(name, which, k)] = traverse(scene_arrays(name), K.records(name, which), k)
    return _TRAV[(name, which, k)]


def multiply_referenced(d):
    """The ids (3 * index) of the triangles that d's tree references more than once, ascending."""
    ids, count = np.unique(np.asarray(d["tri_indices"]).reshape(-1), return_counts=True)
    return ids[count > 1].astype(np.int64)


def duplicate_set(name, per=16, seed=23, draws=48):
    """(records with r = +inf, (a) words (8, n, 8)): `per` points on each multiply-referenced triangle
    of the fixture plus N(0, 1e-3 x diagonal) noise, computed once (shared; do not modify).

    Which points: a second reference shows only where the traversal also visits the second leaf and
    the triangle is among the point's eight nearest, and on cubes2_dae, whose triangles are small
    against the noise, that holds for about 40 % of uniformly drawn points.  So `draws` points are
    drawn per triangle and, as closest_common chooses its wrong-box node, yardstick (b) chooses among
    them: in draw order, first those whose row repeats an id when (b) runs WITHOUT the presence check."""
    if name not in _DUP:
        import rtamd
        d = scene_arrays(name)
        ids = multiply_referenced(d)
        v = d["vertices"][:, :3].astype(np.float64)
        idx = np.asarray(d["indices"]).reshape(-1)
        rng = np.random.default_rng(seed)
        t = np.repeat(ids, draws)
        tri = v[np.stack([idx[t], idx[t + 1], idx[t + 2]], axis=1)]              # (m, 3 vertices, 3)
        b = rng.dirichlet((1.0, 1.0, 1.0), t.size)
        q = np.einsum("mk,mkc->mc", b, tri) + rng.normal(0.0, 1e-3 * K.diagonal(d), (t.size, 3))
        cand = rtamd.pack_points(q.astype(F32), None)
        bites = repeats(traverse(d, cand, MAX_K, presence=False)[0]).reshape(ids.size, draws)
        keep = np.argsort(~bites, axis=1, kind="stable")[:, :per]                # biting draws first, in draw order
        rec = np.ascontiguousarray(cand.reshape(ids.size, draws)[np.arange(ids.size)[:, None], np.sort(keep, axis=1)].reshape(-1))
        _DUP[name] = (rec, brute(d, rec, MAX_K))
    return _DUP[name]


def repeats(w):
    """bool (n,): the rows of words (k, n, 8) in which a found id appears twice."""
    ids = w[:, :, 0].view(np.int32).T                                            # (n, k)
    out = np.zeros(ids.shape[0], bool)
    for a in range(ids.shape[1]):
        for b in range(a + 1, ids.shape[1]):
            out |= (ids[:, a] >= 0) & (ids[:, a] == ids[:, b])
    return out
