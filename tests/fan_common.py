"""Shared by test_fan.py (CPU) and test_fan_gpu.py: the inputs and the yardstick of the occlusion
fans.

Inputs, for a scene d of ray_query_common.scene_arrays: the origins are the hit points of
incoherent_rays(d, 512) by the oracle, o + dir * (t - 0.001) rounded to float32 (0.001 short of the
surface, as the frame's own hit points); the normals are each hit triangle's cross(e1, e2) turned
against the ray, as float32; the directions are the 64-point Fibonacci sphere in float32; tmax is the
default or 0.25 x the scene box's diagonal.

Yardstick: oracle.trace_rays(any_hit=True) on the expanded rays, packed into the fan's layout, with
the traced flags from tests/fan_ref.c, a plain-C restatement of the rule compiled here at test time
into a temporary folder (removed at exit) with cc -O2 -ffp-contract=off, as tests/hit_attr_ref.c is."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from ray_query_common import TMAX_DEFAULT, incoherent_rays, scene_arrays, scene_box

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ["cornell12", "rand2k", "hf40k", "knot16k", "cubes2_obj"]
N_SOURCE_RAYS = 512
K_DIRS = 64
SETTINGS = ["default", "quarter", "nocull"]   # tmax default; tmax 0.25 x diagonal; default tmax and zero normals

_lib = None
_INPUTS = {}
_YARD = {}


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="rtamd_fan_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "fan_ref.so")
        subprocess.run(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(HERE, "fan_ref.c"), "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        vp = C.c_void_p
        L.fan_ref_expand.restype = None
        L.fan_ref_expand.argtypes = [vp, C.c_int64, vp, C.c_int32, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def fibonacci(k=K_DIRS):
    """The k-point Fibonacci sphere as float32 (k, 3): z = 1 - (2 i + 1) / k, azimuth i * pi (3 - sqrt 5)."""
    i = np.arange(k, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / k
    r = np.sqrt(1.0 - z * z)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def origin_words(rec):
    """rt_fan_origin records (any dtype) as uint32 (n, 8), contiguous."""
    return np.ascontiguousarray(rec).view(np.uint8).reshape(-1).view(np.uint32).reshape(-1, 8)


def dir_words(dirs):
    """float32 (k, 3) or (k, 4) directions as the rt_float4 table's uint32 (k, 4), w = 0."""
    d = np.ascontiguousarray(dirs, np.float32)
    out = np.zeros((d.shape[0], 4), np.float32)
    out[:, :d.shape[1]] = d
    return out.view(np.uint32)


def ref_expand(rec, dirs):
    """fan_ref.c on packed origins and a direction table: (rays uint32 (n * k, 8), traced bool (n * k,))."""
    ow, dw = origin_words(rec), dir_words(dirs)
    n, k = ow.shape[0], dw.shape[0]
    rays = np.zeros((n * k, 8), np.uint32)
    traced = np.zeros(n * k, np.uint8)
    lib().fan_ref_expand(_p(ow), n, _p(dw), k, _p(rays), _p(traced))
    return rays, traced.astype(bool)


def pack_bits(bits):
    """bool (n, k) -> the fan's layout uint32 (ceil(k / 32), n): bit j & 31 of word [j >> 5, i]; plain
    loops over the 32 bit positions, independent of rtamd.fan_pack."""
    n, k = bits.shape
    w = (k + 31) // 32
    out = np.zeros((w, n), np.uint32)
    for j in range(k):
        out[j >> 5, :] |= bits[:, j].astype(np.uint32) << np.uint32(j & 31)
    return out


def quarter_diagonal(d):
    lo, hi = scene_box(d)
    return np.float32(0.25 * np.sqrt(np.sum((hi.astype(np.float64) - lo.astype(np.float64)) ** 2)))


def hit_points(d, o, dirs, keep_misses=False):
    """(origins, normals) float32 (m, 3) of the rays (o, dirs) that hit scene d by the oracle's closest
    hit: the hit point 0.001 short of the surface, o + dir * (t - 0.001) with dir the unit direction,
    evaluated in float64 and rounded; the hit triangle's cross(e1, e2), turned against the ray.
    keep_misses: one origin per ray, in ray order; a ray that misses gives its own origin and a zero
    normal (an unculled origin outside the mesh)."""
    import rtamd
    from oracle import oracle
    ids, t, _ = oracle.trace_rays(d, rtamd.pack_rays(o, dirs))
    hit = np.flatnonzero(ids >= 0)
    o64, d64 = o[hit].astype(np.float64), dirs[hit].astype(np.float64)
    d64 /= np.linalg.norm(d64, axis=1)[:, None]
    origins = (o64 + d64 * (t[hit].astype(np.float64) - 0.001)[:, None]).astype(np.float32)
    idx = np.asarray(d["indices"]).reshape(-1)
    v = np.asarray(d["vertices"])[:, :3].astype(np.float32)
    tri = ids[hit]
    p0, p1, p2 = v[idx[tri]], v[idx[tri + 1]], v[idx[tri + 2]]
    e1, e2 = (p1 - p0).astype(np.float32).astype(np.float64), (p2 - p0).astype(np.float32).astype(np.float64)
    ng = np.cross(e1, e2)
    ng[np.sum(ng * d64, axis=1) > 0.0] *= -1.0
    if keep_misses:
        all_o, all_n = np.array(o, np.float32, copy=True), np.zeros(o.shape, np.float32)
        all_o[hit], all_n[hit] = origins, ng.astype(np.float32)
        return all_o, all_n
    return origins, ng.astype(np.float32)


def inputs(name):
    """dict(d, origins (n, 3), normals (n, 3), dirs (64, 3), quarter) of a scene, computed once (shared;
    do not modify)."""
    if name not in _INPUTS:
        d = scene_arrays(name)
        o, dirs, _ = incoherent_rays(d, N_SOURCE_RAYS)
        origins, normals = hit_points(d, o, dirs)
        _INPUTS[name] = dict(d=d, origins=origins, normals=normals, dirs=fibonacci(), quarter=quarter_diagonal(d))
    return _INPUTS[name]


def records(name, setting):
    """The packed rt_fan_origin records of a scene's inputs under one of SETTINGS."""
    import rtamd
    x = inputs(name)
    return rtamd.pack_fan_origins(x["origins"], None if setting == "nocull" else x["normals"],
                                  x["quarter"] if setting == "quarter" else None)


def yardstick_for(d, rec, dirs, want_stats=False):
    """The masks a fan of these records and directions must give on scene arrays d: the oracle's any hit
    of every traced ray of fan_ref.c's expansion, packed.  With want_stats also (traced (n, k), hit
    (n, k), the oracle's counters)."""
    from oracle import oracle
    rays, traced = ref_expand(rec, dirs)
    n, k = origin_words(rec).shape[0], dir_words(dirs).shape[0]
    hit = np.zeros(n * k, bool)
    stats = {}
    if traced.any():
        ids, _, stats = oracle.trace_rays(d, rays[traced], any_hit=True)
        hit[traced] = ids >= 0
    masks = pack_bits(hit.reshape(n, k))
    if want_stats:
        return masks, traced.reshape(n, k), hit.reshape(n, k), stats
    return masks


def yardstick(name, setting):
    """(masks, traced (n, k), hit (n, k), oracle counters) of a scene's inputs under a setting, computed
    once (shared; do not modify)."""
    if (name, setting) not in _YARD:
        x = inputs(name)
        _YARD[(name, setting)] = yardstick_for(x["d"], records(name, setting), x["dirs"], want_stats=True)
    return _YARD[(name, setting)]


F32 = np.float32


def edge_records():
    """The edge set of the rule: normals zero, -0, NaN, inf, 1e30 (against directions of 1e30 the dot
    overflows), plain; tmax 0.001, the float above it, +inf, NaN, default; one origin per pair, and
    three invalid origins."""
    import rtamd
    normals = [(0, 0, 0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf),
               (1e30, 1e30, 1e30), (1e30, -1e30, 0), (-1e30, -1e30, -1e30), (0, 0, 1), (0, 0, -1), (1, 1, 1),
               (1e-45, 0, 0), (-1e-45, 0, 0), (3, -4, 0.5)]
    tmaxs = [F32(0.001), np.nextafter(F32(0.001), F32(1)), F32(np.inf), F32(np.nan), TMAX_DEFAULT, F32(0.0), F32(-1.0)]
    o, nr, tm = [], [], []
    for nv in normals:
        for t in tmaxs:
            o.append((0.5, -0.25, 2.0)); nr.append(nv); tm.append(t)
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        o.append(bad); nr.append((0, 0, 1)); tm.append(TMAX_DEFAULT)
    return rtamd.pack_fan_origins(np.array(o, F32), np.array(nr, F32), np.array(tm, F32))


def edge_dirs():
    """Directions zero (either sign), NaN, inf, subnormal, axis-aligned, 1e30, plain: float32 (k, 3)."""
    sub = F32(1e-45)
    return np.array([(0, 0, 0), (-0.0, 0, -0.0), (np.nan, 1, 0), (0, 1, np.nan), (np.inf, 0, 0), (0, -np.inf, 1),
                     (sub, 0, 0), (0, 0, -sub), (sub, sub, sub), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1),
                     (0, 0, -1), (1e30, 1e30, 1e30), (-1e30, 1e30, 1e30), (-1e30, -1e30, -1e30), (1, 2, 3), (-3, 4, -0.5),
                     (1e-20, 1e-20, 1e-20), (3e38, 3e38, 3e38)], F32)
