"""Shared by test_ray_query.py (CPU) and test_ray_query_gpu.py: the two yardsticks of the ray
queries.

Yardstick 1, one ray through the oracle.  oracle.render of a 1 x 1 frame, depth 1, no shadow ray,
with a = b = 0, c = o, campos = fl(o - d0) and a scene box of +-3e38 traces exactly the ray
(o, fl(o - campos)): image_pos = c + 0 * xf + 0 * yf = o, and the scene-box test passes.  The GPU
is given that float32 difference as its direction.  hits[0, 0, 0] and t[0, 0] are the S_strict
closest hit.

Yardstick 2, a frame's primary rays.  With a, b, c and campos multiples of 2^-6 and power-of-two
w and h, every product and sum of image_pos = c + a * xf + b * yf is exact in float32 (checked here
against float64), so the rays are the same whether or not the compiler contracts, and numpy
float32 gives the very rays the kernels build: o = image_pos, d = fl(image_pos - campos)."""
import ctypes as C

import numpy as np

from conftest import load_golden

N_RAYS = 2000
TMAX_DEFAULT = np.float32(4294967296.0)
TMIN = np.float32(0.001)
BOX = np.float32(3e38)

_SCENES = {}
_CACHE = {}


def scene_arrays(name):
    """A golden scene's arrays, or "rand2k_built": rand2k's mesh with the host twin's tree of
    build_scene(max_leaf=2, keys="extent") (shared; do not modify)."""
    if name not in _SCENES:
        if name == "rand2k_built":
            import rtamd
            d = load_golden("rand2k")
            b = rtamd.Mesh.from_arrays(d["vertices"], d["indices"]).build_lbvh(2, keys="extent")
            _SCENES[name] = dict(d, nodes=b.nodes, tri_indices=b.tri_indices)
        else:
            _SCENES[name] = load_golden(name)
    return _SCENES[name]


def scene_box(d):
    v = d["vertices"][:, :3]
    return v.min(0).astype(np.float32), v.max(0).astype(np.float32)


def incoherent_rays(d, n=N_RAYS, seed=7):
    """(origins, directions, campos) float32 (n, 3): origins uniform in the scene box grown by 20
    units, each aimed at a uniform point d0 away in the box; campos = fl(o - d0) is what the oracle is
    given, and the direction is yardstick 1's fl(o - campos)."""
    lo, hi = scene_box(d)
    rng = np.random.default_rng(seed + d["vertices"].shape[0])
    o = rng.uniform(lo - 20.0, hi + 20.0, (n, 3)).astype(np.float32)
    target = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d0 = (target - o).astype(np.float32)
    campos = (o - d0).astype(np.float32)
    dirs = (o - campos).astype(np.float32)
    assert np.all(np.any(dirs != 0.0, axis=1))
    return o, dirs, campos


def one_ray_params(o, campos):
    p = np.zeros(32, np.float32)
    p[3::4] = 1.0
    p[8:11] = o             # c; a = b = 0
    p[12:15] = campos
    p[24:27] = -BOX
    p[28:31] = BOX
    return p


def oracle_closest(d, o, campos, stats=None):
    """Yardstick 1 for every ray (o, fl(o - campos)): (ids int32[n], t float32[n]); a miss is
    (-1, TMAX_DEFAULT).  `stats`: a dict that receives the summed stack_overflow."""
    from oracle import oracle
    n = o.shape[0]
    ids, t = np.empty(n, np.int32), np.empty(n, np.float32)
    overflow = 0
    for k in range(n):
        r = oracle.render(d, one_ray_params(o[k], campos[k]), 1, 1, depth=1, flags=1, nthreads=1)
        ids[k], t[k] = r["hits"][0, 0, 0], r["t"][0, 0]
        overflow += r["stats"]["stack_overflow"]
    assert not np.any(ids == -2), "a ray was left untraced"
    if stats is not None:
        stats["stack_overflow"] = overflow
    return ids, t


def reference(name):
    """(origins, directions, oracle ids, oracle t, oracle stack overflows, campos) of a scene's
    incoherent rays, computed once."""
    if name not in _CACHE:
        d = scene_arrays(name)
        o, dirs, campos = incoherent_rays(d)
        st = {}
        ids, t = oracle_closest(d, o, campos, st)
        _CACHE[name] = (o, dirs, ids, t, st["stack_overflow"], campos)
    return _CACHE[name]


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_normalize(v):
    from oracle import oracle
    a, out = np.ascontiguousarray(v, np.float32), np.zeros(3, np.float32)
    oracle.lib().oracle_normalize(_fp(a), _fp(out))
    return out


def triangle(d, tri_id):
    """(v0, e1, e2) of the triangle with id 3 * index, as the traversal forms them."""
    i = d["indices"][tri_id:tri_id + 3]
    v = d["vertices"][i, :3].astype(np.float32)
    return v[0].copy(), (v[1] - v[0]).astype(np.float32), (v[2] - v[0]).astype(np.float32)


def oracle_ray_tri(d, o, dirn, tri_id):
    """The oracle's Moller-Trumbore t of the ray (o, normalised direction dirn) and one triangle."""
    from oracle import oracle
    v0, e1, e2 = triangle(d, tri_id)
    o = np.ascontiguousarray(o, np.float32)
    dirn = np.ascontiguousarray(dirn, np.float32)
    return np.float32(oracle.lib().oracle_ray_tri(_fp(o), _fp(dirn), _fp(v0), _fp(e1), _fp(e2)))


def brute_force_closest(d, o, dirs, tmax=TMAX_DEFAULT):
    """The minimum over ALL triangles of oracle_ray_tri within (TMIN, tmax): (id, t); ties
    keep the first triangle in index order, so compare t always and ids only where t is unique."""
    dirn = oracle_normalize(dirs)
    best, bt = -1, np.float32(tmax)
    for k in range(d["indices"].size // 3):
        t = oracle_ray_tri(d, o, dirn, 3 * k)
        if TMIN < t < bt:
            best, bt = 3 * k, t
    return best, bt


def quantised_frame(d, w, h):
    """Yardstick 2: (params float32[32], origins, directions) of a w x h frame (powers of two) whose
    camera is the golden's, quantised to multiples of 2^-6; the rays in pixel order y * w + x."""
    assert w & (w - 1) == 0 and h & (h - 1) == 0
    p = np.array(d["params"], np.float32, copy=True)
    for k in (0, 4, 8, 12):
        p[k:k + 3] = (np.round(p[k:k + 3].astype(np.float64) * 64.0) / 64.0).astype(np.float32)
    a, b, c, campos = (p[k:k + 3] for k in (0, 4, 8, 12))
    x = np.arange(w, dtype=np.float64)
    y = np.arange(h, dtype=np.float64)
    xf = ((x - 0.5) / float(w)).astype(np.float32)   # volumeRender.cl:1169-1170, exact: w is a power of two
    yf = ((y - 0.5) / float(h)).astype(np.float32)
    assert np.array_equal(xf.astype(np.float64), (x - 0.5) / w) and np.array_equal(yf.astype(np.float64), (y - 0.5) / h)
    XF, YF = np.meshgrid(xf, yf)                     # [h, w]
    ax = (a[None, None, :] * XF[..., None]).astype(np.float32)
    t1 = (c[None, None, :] + ax).astype(np.float32)
    by = (b[None, None, :] * YF[..., None]).astype(np.float32)
    ip = (t1 + by).astype(np.float32)
    # every step exact: the float64 evaluation (exact for these operands) gives the same numbers
    a64, b64, c64 = (v.astype(np.float64) for v in (a, b, c))
    exact = c64[None, None, :] + a64[None, None, :] * XF.astype(np.float64)[..., None] \
        + b64[None, None, :] * YF.astype(np.float64)[..., None]
    assert np.array_equal(ax.astype(np.float64), a64[None, None, :] * XF.astype(np.float64)[..., None])
    assert np.array_equal(ip.astype(np.float64), exact), "image_pos is not exact in float32"
    o = ip.reshape(-1, 3)
    dirs = (o - campos[None, :]).astype(np.float32)
    return p, np.ascontiguousarray(o), np.ascontiguousarray(dirs)
