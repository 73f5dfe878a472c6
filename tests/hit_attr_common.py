"""Shared by test_hit_attr.py (CPU) and test_hit_attr_gpu.py: the yardstick of the attribute ray
query.

tests/hit_attr_ref.c restates the S_strict definition of rt_hit_attr in plain C.  It is compiled
here, at test time, into a temporary folder (removed at exit) with cc -O2 -ffp-contract=off, as
oracle.build() compiles the oracle.  It is given the ids and t of a traversal (the oracle's) and
returns the 64-byte records those hits must have; test_hit_attr.py pins it to the oracle by
continuing the oracle's own frame from its records.

Records travel as uint32 (n, 16): every comparison is on words."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TMAX_WORD = np.array([4294967296.0], np.float32).view(np.uint32)[0]
# word offsets of a record's fields
ID, T, U, V, P, NDOTD, NG, R0, NS, R1 = 0, 1, 2, 3, 4, 7, 8, 11, 12, 15
FLOAT_FIELDS = {"t": [T], "u": [U], "v": [V], "p": [4, 5, 6], "ndotd": [NDOTD], "ng": [8, 9, 10], "ns": [12, 13, 14]}

_lib = None


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="rtamd_hit_attr_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "hit_attr_ref.so")
        subprocess.run(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(HERE, "hit_attr_ref.c"), "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.ref_hit_attr.restype = None
        L.ref_hit_attr.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp]
        L.ref_next_rays.restype = None
        L.ref_next_rays.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
        L.ref_normalize.restype = None
        L.ref_normalize.argtypes = [vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ray_words(rays):
    """rt_ray records (any dtype) as float32 (n, 8), contiguous."""
    return np.ascontiguousarray(rays).view(np.uint8).reshape(-1).view(np.float32).reshape(-1, 8)


def words(records):
    """rt_hit_attr records (HIT_ATTR_DTYPE or raw) as uint32 (n, 16)."""
    return np.ascontiguousarray(records).view(np.uint8).reshape(-1).view(np.uint32).reshape(-1, 16)


def ref_hit_attr(d, rays, ids, t, want_t=False):
    """The records of `rays` (rt_ray records) on scene arrays `d` for the traversal's ids and t:
    uint32 (n, 16); with want_t also Moller-Trumbore's own t of each hit triangle (0 for a miss)."""
    r = ray_words(rays)
    n = r.shape[0]
    ids = np.ascontiguousarray(ids, np.int32)
    t = np.ascontiguousarray(t, np.float32)
    assert ids.shape == (n,) and t.shape == (n,)
    verts = np.ascontiguousarray(d["vertices"], np.float32)
    normals = np.ascontiguousarray(d["normals"], np.float32)
    assert verts.shape[1] == 4 and normals.shape[1] == 4
    idx = np.ascontiguousarray(d["indices"], np.int32)
    nidx = np.ascontiguousarray(d["normals_indices"], np.int32)
    out = np.zeros((n, 16), np.uint32)
    t_mt = np.zeros(n, np.float32)
    lib().ref_hit_attr(_p(verts), _p(idx), _p(normals), _p(nidx), _p(r), _p(ids), _p(t), n, _p(out), _p(t_mt))
    return (out, t_mt) if want_t else out


def ref_next_rays(rays, attrs, light_pos):
    """(reflection rays, shadow rays), float32 (n, 8) rt_ray records each, built from the records as
    the frame builds them at a hit; a miss gets all-zero rays (invalid: reported as a miss)."""
    r = ray_words(rays)
    a = words(attrs)
    n = r.shape[0]
    assert a.shape[0] == n
    light = np.ascontiguousarray(light_pos, np.float32).reshape(3)
    refl, shadow = np.zeros((n, 8), np.float32), np.zeros((n, 8), np.float32)
    lib().ref_next_rays(_p(r), _p(a), _p(light), n, _p(refl), _p(shadow))
    return refl, shadow


def ref_normalize(v):
    a, out = np.ascontiguousarray(v, np.float32).reshape(3), np.zeros(3, np.float32)
    lib().ref_normalize(_p(a), _p(out))
    return out


def miss_words(rays):
    """The miss record of every ray: -1, the tmax word, 14 zero words."""
    r = ray_words(rays)
    out = np.zeros((r.shape[0], 16), np.uint32)
    out[:, ID] = 0xFFFFFFFF
    out[:, T] = r[:, 3].view(np.uint32)
    return out


def assert_same_records(got, want, label):
    g, w = words(got), words(want)
    assert g.shape == w.shape, f"{label}: {g.shape} records vs {w.shape}"
    bad = np.flatnonzero(np.any(g != w, axis=1))
    if bad.size:
        k = int(bad[0])
        cols = np.flatnonzero(g[k] != w[k])
        raise AssertionError(f"{label}: {bad.size} of {g.shape[0]} records differ, first {bad[:5]}; record {k} words {cols}: "
                             f"{g[k, cols]} vs {w[k, cols]} (as floats {g[k, cols].view(np.float32)} vs {w[k, cols].view(np.float32)})")


_FRAMES = {}


def oracle_frame(name, w=64, h=64):
    """The quantised w x h frame of a golden scene through the oracle, computed once (shared; do not
    modify): dict(d, params, rays, ref) with ref = oracle.render(depth=2, flags=0)."""
    if (name, w, h) not in _FRAMES:
        import rtamd
        from oracle import oracle
        from ray_query_common import quantised_frame, scene_arrays
        d = scene_arrays(name)
        p, o, dirs = quantised_frame(d, w, h)
        _FRAMES[name, w, h] = dict(d=d, params=p, rays=rtamd.pack_rays(o, dirs), ref=oracle.render(d, p, w, h, depth=2, flags=0))
    return _FRAMES[name, w, h]
