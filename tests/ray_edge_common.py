"""Shared by test_ray_query.py (CPU) and test_ray_query_edges_gpu.py: ray classes at the edges of
what a caller may hand to rt_trace_rays, and the fast quotient's ray-side domain
restated from DESIGN.md 7.2.

Every builder is seeded, returns float32 (origins (n, 3), directions (n, 3), tmax (n,)) with
n <= 2048, and every ray is a legal input by DESIGN.md 18.  tests/test_ray_query.py asserts each
class's defining property on the host and, with the oracle alone, that the classes both hit and
miss.

near_axis and origin_domain lay their rays out in runs of 64 that share the value under test, so a
64-ray group of the query kernel is wholly inside or wholly outside the quotient's domain: a single
lane outside it moves its whole wave to the division form, and a buffer that mixed the two in every
group would never run the fast quotient at all."""
import numpy as np

from ray_query_common import TMAX_DEFAULT, incoherent_rays, scene_arrays, scene_box

F32 = np.float32
GROUP = 64
CLASSES = ["axis1", "axis2", "snapped", "near_axis", "origin_domain", "scaled"] + [f"octant{k}" for k in range(8)]
EDGE_SCENES = ["cornell12", "rand2k", "rand2k_built", "hf40k", "single_tri_rootleaf"]


def p2(k):
    return F32(np.ldexp(1.0, k))


# magnitudes of near_axis's small components: both sides of 2^-64 (S_strict / S_hw) and of 2^-126 (S_ref)
NEAR_AXIS_MAGNITUDES = [p2(-63), p2(-64), np.nextafter(p2(-64), F32(0)), p2(-100), p2(-126), p2(-127), p2(-149)]
# origin components of origin_domain: both sides of 2^-66 and of 2^60, and zero
ORIGIN_VALUES = [F32(0.0), F32(-0.0), p2(-67), -p2(-67), p2(-66), -p2(-66), F32(1e-25), p2(60),
                 np.nextafter(p2(60), F32(np.inf)), p2(61), F32(1e30)]
SCALE_EXPONENTS = {"normal": 0, "below FLT_MIN": -85, "inf": 100}


def axis_ok(o, dn, arithmetic):
    """Whether one axis of a ray is inside the fast quotient's domain (the slab quotient
    and its preconditions), elementwise.  o: origin component, dn: NORMALISED direction component.
    S_strict / S_hw ("strict", "hw"): d == 0, or 2^-64 <= |d| <= 2 and (o == 0 or 2^-66 <= |o| <= 2^60).
    S_ref ("ref"): (o == 0 or 2^-66 <= |o| <= 2^60) and (d == 0 or |d| >= 2^-126)."""
    ao, ad = np.abs(np.asarray(o, F32)), np.abs(np.asarray(dn, F32))
    o_ok = (ao == 0) | ((ao >= p2(-66)) & (ao <= p2(60)))
    if arithmetic == "ref":
        return o_ok & ((ad == 0) | (ad >= p2(-126)))
    return (ad == 0) | ((ad >= p2(-64)) & (ad <= F32(2.0)) & o_ok)


def normalised(dirs):
    """oracle_normalize of every row."""
    from ray_query_common import oracle_normalize
    return np.stack([oracle_normalize(v) for v in np.asarray(dirs, F32).reshape(-1, 3)])


def in_domain(o, dirs, arithmetic):
    """Per ray: all three axes inside the fast quotient's domain (fast_div_ok)."""
    return np.all(axis_ok(o, normalised(dirs), arithmetic), axis=1)


def _rng(d, salt):
    return np.random.default_rng(1000 * salt + d["vertices"].shape[0])


def _default(n):
    return np.full(n, TMAX_DEFAULT, F32)


def _signed_zero(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, F32(-0.0), F32(0.0)).astype(F32)


def _pushed_out(rng, lo, hi, axis, sign):
    """Uniform points of the box, moved 20 units outside along `axis` on the side a ray with
    direction sign `sign` on that axis starts from."""
    n = axis.shape[0]
    o = rng.uniform(lo, hi, (n, 3)).astype(F32)
    o[np.arange(n), axis] = np.where(sign > 0, lo[axis] - F32(20.0), hi[axis] + F32(20.0))
    return o


def axis1(d, n=384, seed=1):
    """One non-zero direction component (+-1, +-2.5 or +-0.375 by turns), the zeros of either sign."""
    lo, hi = scene_box(d)
    rng = _rng(d, seed)
    k = np.arange(n)
    axis, sign = k % 3, np.where((k // 3) % 2 == 0, 1.0, -1.0).astype(F32)
    o = _pushed_out(rng, lo, hi, axis, sign)
    dirs = np.stack([_signed_zero(rng, n) for _ in range(3)], axis=1)
    dirs[k, axis] = sign * np.array([1.0, 2.5, 0.375], F32)[(k // 6) % 3]
    return o, dirs, _default(n)


def axis2(d, n=384, seed=2):
    """Exactly one zero direction component (either sign): the origin's coordinate on that axis is a
    uniform one of the box, the other two are uniform in the box grown by 20, aimed at a uniform point."""
    lo, hi = scene_box(d)
    rng = _rng(d, seed)
    k = np.arange(n)
    axis = k % 3
    o = rng.uniform(lo - 20.0, hi + 20.0, (n, 3)).astype(F32)
    o[k, axis] = rng.uniform(lo, hi, (n, 3)).astype(F32)[k, axis]
    target = rng.uniform(lo, hi, (n, 3)).astype(F32)
    dirs = (target - o).astype(F32)
    dirs[k, axis] = _signed_zero(rng, n)
    return o, dirs, _default(n)


def snapped(d, n=512, seed=3):
    """axis1 and axis2 rays through mesh vertices.  First half: an axis1 ray whose two other origin
    coordinates are a vertex's, so the ray runs through that vertex (and along every box plane and mesh
    edge that holds it and is parallel to the ray).  Second half: an axis2 ray whose origin coordinate on
    the zero axis is a vertex's -- for every fourth one a vertex on the scene box's own plane, a wall of
    cornell12 -- aimed at that vertex: it lies in the plane of that coordinate.  Returns also the vertex
    indices."""
    lo, hi = scene_box(d)
    rng = _rng(d, seed)
    v = np.asarray(d["vertices"], F32)[np.unique(d["indices"]), :3]
    h = n // 2
    k = np.arange(h)
    pick = rng.integers(0, v.shape[0], n)
    # axis1 through a vertex
    axis, sign = k % 3, np.where((k // 3) % 2 == 0, 1.0, -1.0).astype(F32)
    o1 = v[pick[:h]].copy()
    o1[k, axis] = np.where(sign > 0, lo[axis] - F32(20.0), hi[axis] + F32(20.0))
    d1 = np.zeros((h, 3), F32)
    d1[k, axis] = sign
    # axis2 in a vertex's plane, aimed at the vertex
    axis2_ = k % 3
    on_wall = np.flatnonzero(k % 4 == 3)
    for j in on_wall:   # a vertex on the box plane of this ray's zero axis
        a = axis2_[j]
        wall = np.flatnonzero((v[:, a] == lo[a]) | (v[:, a] == hi[a]))
        pick[h + j] = wall[rng.integers(0, wall.size)]
    vv = v[pick[h:]]
    o2 = rng.uniform(lo - 20.0, hi + 20.0, (h, 3)).astype(F32)
    o2[k, axis2_] = vv[k, axis2_]
    d2 = (vv - o2).astype(F32)
    keep = np.all((d2 != 0) | (np.arange(3)[None, :] == axis2_[:, None]), axis=1)
    assert np.all(keep), "a snapped axis2 ray lost a second component"
    o, dirs = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    return o, dirs, _default(n), pick


def near_axis(d, seed=4):
    """A dominant component of +-1.0 and small ones of NEAR_AXIS_MAGNITUDES: per magnitude one run of 64
    rays with both small components at that magnitude (either sign) and one run with one of them zero."""
    lo, hi = scene_box(d)
    rng = _rng(d, seed)
    o, dirs = [], []
    for m in NEAR_AXIS_MAGNITUDES:
        for with_zero in (False, True):
            k = np.arange(GROUP)
            axis, sign = k % 3, np.where((k // 3) % 2 == 0, 1.0, -1.0).astype(F32)
            oo = _pushed_out(rng, lo, hi, axis, sign)
            dd = (np.where(rng.integers(0, 2, (GROUP, 3)) == 1, -1.0, 1.0) * m).astype(F32)
            if with_zero:
                other = (axis + 1 + rng.integers(0, 2, GROUP)) % 3
                dd[k, other] = _signed_zero(rng, GROUP)
            dd[k, axis] = sign
            o.append(oo)
            dirs.append(dd)
    o, dirs = np.concatenate(o), np.concatenate(dirs)
    return o, dirs, _default(o.shape[0])


def origin_domain(d, seed=5):
    """Per value of ORIGIN_VALUES one run of 64 rays: that value on one axis (x, y, z by turns), the other
    two coordinates 1 to 20 units outside the box (so that from 2^60 away the normalised direction's small
    components, at least 2^-60, stay inside the quotient's domain and the origin alone decides), aimed at
    a uniform point of the box; tmax = +inf."""
    lo, hi = scene_box(d)
    rng = _rng(d, seed)
    o, dirs = [], []
    for val in ORIGIN_VALUES:
        k = np.arange(GROUP)
        away = rng.uniform(1.0, 20.0, (GROUP, 3))
        oo = np.where(rng.integers(0, 2, (GROUP, 3)) == 1, lo - away, hi + away).astype(F32)
        oo[k, k % 3] = val
        target = rng.uniform(lo, hi, (GROUP, 3)).astype(F32)
        o.append(oo)
        dirs.append((target - oo).astype(F32))
    o, dirs = np.concatenate(o), np.concatenate(dirs)
    assert np.all(np.isfinite(dirs)) and np.all(np.any(dirs != 0, axis=1))
    return o, dirs, np.full(o.shape[0], np.inf, F32)


def scaled(d, n=256):
    """The scene's first n incoherent rays three times over, the direction times 2^k for the k of
    SCALE_EXPONENTS (an exact scaling: every component stays normal)."""
    o, dirs, _ = incoherent_rays(d, n=n)
    oo = np.concatenate([o] * 3)
    dd = np.concatenate([(dirs * p2(k)).astype(F32) for k in SCALE_EXPONENTS.values()])
    return oo, dd, _default(3 * n)


def normalize_branch(dirs):
    """Which branch of normalize each direction takes ("normal", "below FLT_MIN", "inf"), from dot(d, d)
    evaluated in float64; every product here is at least a factor 2^8 away from both thresholds
    (asserted), so float32's rounding of the dot product cannot change the answer."""
    x = np.asarray(dirs, np.float64)
    l2 = np.sum(x * x, axis=1)
    tiny, huge = np.ldexp(1.0, -126), np.ldexp(1.0, 128)
    assert np.all((l2 < tiny / 256) | (l2 > huge * 256) | ((l2 > tiny * 256) & (l2 < huge / 256)))
    return np.where(l2 < tiny, "below FLT_MIN", np.where(l2 > huge, "inf", "normal"))


def octant_corner(d, k):
    """(eye, extent): the eye of octant_common.octant_params(d, k), outside the box corner the octant's
    rays come from, and the largest side of the scene box it is placed by."""
    from octant_common import _box, octant_params
    return octant_params(d, k).reshape(8, 4)[3, :3].astype(np.float64), _box(d)[1]


def octant(d, k, groups=4, seed=6):
    """64 * groups rays of direction octant k (bit i set: component i negative): origins within 5 % of
    the box's extent of octant_corner, aimed at uniform points of the box."""
    lo, hi = scene_box(d)
    rng = _rng(d, 10 * seed + k)
    n = GROUP * groups
    eye, ext = octant_corner(d, k)
    o = (eye[None, :] + rng.uniform(-0.05 * ext, 0.05 * ext, (n, 3))).astype(F32)
    target = rng.uniform(lo, hi, (n, 3)).astype(F32)
    return o, (target - o).astype(F32), _default(n)


def malformed_nodes(d):
    """Indices of the inner nodes the traversal leaves through its malformed-node exits: a left child
    >= 0 with a right child < 0, or either child >= the node count."""
    ni = np.asarray(d["nodes"]).view(np.int32).reshape(-1, 12)
    nn = ni.shape[0]
    return np.flatnonzero((ni[:, 8] >= 0) & ((ni[:, 9] < 0) | (ni[:, 8] >= nn) | (ni[:, 9] >= nn)))


def aimed_at_malformed(d, n=1024, seed=8):
    """The scene's incoherent rays, every second one aimed anew at a uniform point of the (first)
    malformed node's box, so that a share of the traversals pops that node."""
    o, dirs, _ = incoherent_rays(d, n=n)
    dirs = dirs.copy()
    node = np.asarray(d["nodes"], F32).reshape(-1, 12)[malformed_nodes(d)[0]]
    rng = _rng(d, seed)
    target = rng.uniform(node[0:3], node[4:7], (n, 3)).astype(F32)
    dirs[1::2] = (target - o)[1::2].astype(F32)
    return o, dirs, _default(n)


_CACHE = {}


def edge_scene(name):
    """Scene arrays by name: ray_query_common's scenes, and "bigleaf" (refit_common's escape-leaf tree)."""
    if name == "bigleaf":
        from refit_common import scene_arrays as refit_scene
        return refit_scene("bigleaf")
    if name == "deep_comb40":
        return deep_comb40()
    return scene_arrays(name)


def deep_comb40():
    """overflow_comb cut to 40 levels: every level pushes, so a stack reaches 41 entries -- deeper than
    the LDS part (a restart), within the reference's 65 (no overflow) -- and its rays can hit."""
    if "deep_comb40" not in _CACHE:
        d = dict(scene_arrays("overflow_comb"))
        nodes = np.array(d["nodes"][:80], F32, copy=True)
        nodes.view(np.int32)[78, 8] = 79   # the last inner node: both children its own leaf, as the fixture's last
        d["nodes"], d["tri_indices"] = nodes, d["tri_indices"][:40].copy()
        _CACHE["deep_comb40"] = d
    return _CACHE["deep_comb40"]


def ray_class(name, cls):
    """(origins, directions, tmax) of class `cls` (one of CLASSES) on scene `name`, built once (shared; do
    not modify)."""
    if (name, cls) not in _CACHE:
        d = edge_scene(name)
        if cls.startswith("octant"):
            r = octant(d, int(cls[6:]))
        elif cls == "incoherent":
            o, dirs, _ = incoherent_rays(d)
            r = (o, dirs, _default(o.shape[0]))
        elif cls == "malformed":
            r = aimed_at_malformed(d)
        else:
            r = {"axis1": axis1, "axis2": axis2, "snapped": snapped, "near_axis": near_axis,
                 "origin_domain": origin_domain, "scaled": scaled}[cls](d)[:3]
        assert r[0].dtype == r[1].dtype == r[2].dtype == F32 and r[0].shape[0] <= 2048
        _CACHE[name, cls] = r
    return _CACHE[name, cls]


def pack(o, dirs, tmax):
    import rtamd
    return rtamd.pack_rays(o, dirs, tmax)


def oracle_hits(name, cls, any_hit=False):
    """oracle.trace_rays of a class on a scene, computed once: (ids, t, stats)."""
    key = (name, cls, "any" if any_hit else "closest")
    if key not in _CACHE:
        from oracle import oracle
        _CACHE[key] = oracle.trace_rays(edge_scene(name), pack(*ray_class(name, cls)), any_hit=any_hit)
    return _CACHE[key]
