"""Shared by test_hit_attr_edges.py (CPU) and test_hit_attr_edges_gpu.py: the attribute ray query
 at the edges of normal, ray and mesh space.

An Input is a scene (arrays with a tree), at most 4,096 rays and what is known about its records.  The
inputs come in three groups and are built once per session (shared; do not modify):

 normal  the nine normals/* and five det/* cases of shading_edge_common with the rays of their own
         64 x 64 quantised frame (ray_query_common.quantised_frame), so that a frame and a query trace
         the very same rays; det/offset_1e4 cannot be quantised and takes the float32 primary rays
         built in numpy (float32_frame);
 ray     the fourteen classes of ray_edge_common on its five scenes, and per scene one class with
         per-ray tmax by turns 0.5 t*, the float below t*, t*, the float above t*, 2 t*, +inf
         ("<scene>/tmax");
 mesh    signed_zeros_grid16, signed_zeros_rand512 and degenerate of mesh_edge_common, rand512 scaled
         by 2^k for k in SCALES, and tiny_tris (below), each with the tree of build_lbvh(2), 1,024
         incoherent rays of the unscaled mesh (origins times 2^k: exact) and tmax = +inf.

A Case is what shares one uploaded scene: a normal input, a ray scene with its fifteen inputs, a mesh.

The yardstick is hit_attr_common.ref_hit_attr fed oracle.trace_rays' ids and t.  Records are compared
by assert_same_records_nan: words, except that where the yardstick's float word is a NaN the other
side's must be a NaN of any payload and sign (x86 and gfx950 generate different default NaNs)."""
import numpy as np

import mesh_edge_common as M
import ray_edge_common as E
import shading_edge_common as S
from conftest import load_golden
from hit_attr_common import ID, NDOTD, T, U, V, ray_words, ref_hit_attr, words
from ray_query_common import incoherent_rays, quantised_frame

F32 = np.float32
W = H = 64
FLOAT_WORDS = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14]     # u v p ndotd ng ns
NS_WORDS = [12, 13, 14]

NORMAL_LABELS = [label for label in S.LABELS if label.split("/")[0] in ("normals", "det")]
UNQUANTISABLE = "det/offset_1e4"
FRAME_LABELS = [label for label in NORMAL_LABELS if label != UNQUANTISABLE]
RAY_SCENES = list(E.EDGE_SCENES)
# the class whose rays take the tmax sweep, per scene (each hits with more than a quarter of its rays)
SWEEP_CLASS = {"cornell12": "axis2", "rand2k": "octant3", "rand2k_built": "scaled", "hf40k": "axis1",
               "single_tri_rootleaf": "snapped"}
SCALES = [-6, 20, 37, 38, 40]
MESH_LABELS = ["signed_zeros_grid16", "signed_zeros_rand512", "degenerate"] + [f"rand512*2^{k}" for k in SCALES] + ["tiny_tris"]
GROUPS = ["normal", "ray", "mesh"]
CASES = NORMAL_LABELS + RAY_SCENES + MESH_LABELS

# What each NaN-making input must show among its closest hits: (kind of ns, at least this many; a
# float is a share of the hits).  Every input not listed here has no NaN word in any record.
NAN_MAKING = {
    "normals/nan_component": ("nan", 0.5), "det/floor_y0": ("nan", 0.5), "signed_zeros_grid16": ("nan", 0.5),
    "normals/zero": ("zero", 0.5), "det/slant_through_origin": ("nan", 64), "rand512*2^38": ("nan", 16),
    "rand512*2^40": ("nan", 1),
}
TINY_EXPONENTS = [20, 35, 50, 62]
TINY_SECOND_LEG = 1.0 + 2.0 ** -7


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def group_of(case):
    return "normal" if case in NORMAL_LABELS else "ray" if case in RAY_SCENES else "mesh"


class Input:
    def __init__(self, label, group, case, d, rays, params=None):
        self.label, self.group, self.case, self.d, self.rays, self.params = label, group, case, d, rays, params
        self.frame = group == "normal" and label != UNQUANTISABLE
        self.nan_making = label in NAN_MAKING and NAN_MAKING[label][0] == "nan"
        self._hits, self._want = {}, {}
        assert self.rays.shape[0] <= 4096 and d["indices"].size // 3 <= 40000

    def hits(self, any_hit=False):
        """oracle.trace_rays of the input's rays: (ids, t), computed once."""
        if any_hit not in self._hits:
            from oracle import oracle
            self._hits[any_hit] = oracle.trace_rays(self.d, self.rays, any_hit=any_hit)[:2]
        return self._hits[any_hit]

    def want(self, any_hit=False):
        """The yardstick's records on the oracle's ids and t, and Moller-Trumbore's own t: computed once."""
        if any_hit not in self._want:
            ids, t = self.hits(any_hit)
            with np.errstate(all="ignore"):
                self._want[any_hit] = ref_hit_attr(self.d, self.rays, ids, t, want_t=True)
        return self._want[any_hit]


# ---- the comparison rule ----

def nan_words(records):
    """(n, 16) bool: the float words of the records that hold a NaN."""
    w = words(records)
    m = np.zeros(w.shape, bool)
    m[:, FLOAT_WORDS] = np.isnan(w[:, FLOAT_WORDS].view(F32))
    return m


def assert_same_records_nan(got, want, label):
    """Sixteen words per record.  id, t and the reserved words are compared as words; so are the twelve
    float words, except that where `want`'s is a NaN `got`'s must be a NaN, payload and sign not
    compared.  A miss record of `want` is never excused.  Returns the number of words that took the
    exception (words that differ and are NaN on both sides)."""
    g, w = words(got), words(want)
    assert g.shape == w.shape, f"{label}: {g.shape} records vs {w.shape}"
    nan = nan_words(w)
    assert not nan[w[:, ID].view(np.int32) < 0].any(), f"{label}: a miss record holds a NaN"
    ok = np.where(nan, nan_words(g), g == w)
    bad = np.flatnonzero(~np.all(ok, axis=1))
    if bad.size:
        k = int(bad[0])
        cols = np.flatnonzero(~ok[k])
        raise AssertionError(f"{label}: {bad.size} of {g.shape[0]} records differ, first {bad[:5]}; record {k} words {cols}: "
                             f"{g[k, cols]} vs {w[k, cols]} (as floats {g[k, cols].view(F32)} vs {w[k, cols].view(F32)})")
    return int(np.sum(nan & (g != w)))


# ---- group 1: normal space ----

def float32_frame(params, w, h):
    """(origins, directions) of a w x h frame's primary rays in float32, each product and sum rounded in
    source order (quantised_frame without its quantisation and without its exactness assertion)."""
    p = np.asarray(params, F32)
    a, b, c, campos = (p[k:k + 3] for k in (0, 4, 8, 12))
    xf = ((np.arange(w, dtype=np.float64) - 0.5) / float(w)).astype(F32)
    yf = ((np.arange(h, dtype=np.float64) - 0.5) / float(h)).astype(F32)
    XF, YF = np.meshgrid(xf, yf)
    t1 = (c[None, None, :] + (a[None, None, :] * XF[..., None]).astype(F32)).astype(F32)
    ip = (t1 + (b[None, None, :] * YF[..., None]).astype(F32)).astype(F32)
    o = np.ascontiguousarray(ip.reshape(-1, 3))
    return o, np.ascontiguousarray((o - campos[None, :]).astype(F32))


def _normal_input(label):
    import rtamd
    c = S.case(label)
    d = dict(c.scene, params=c.params)
    if label == UNQUANTISABLE:
        p = np.array(c.params, F32, copy=True)
        o, dirs = float32_frame(p, W, H)
    else:
        p, o, dirs = quantised_frame(d, W, H)
    return Input(label, "normal", label, d, rtamd.pack_rays(o, dirs), params=p)


_FRAMES = {}


def oracle_frame(label):
    """oracle.render(depth=2) of a quantisable normal-space input's 64 x 64 frame, computed once."""
    if label not in _FRAMES:
        from oracle import oracle
        inp = get(label)
        assert inp.frame
        _FRAMES[label] = oracle.render(inp.d, inp.params, W, H, depth=2, flags=0)
    return _FRAMES[label]


# ---- group 2: ray space ----

def sweep_tmax(ids, t, own):
    """Per ray that hits, by turns 0.5 t*, the float below t*, t*, the float above t*, 2 t*, +inf; a ray
    that misses keeps its own tmax.  Returns (tmax, turn)."""
    turn = np.arange(ids.size) % 6
    inf = F32(np.inf)
    choices = np.stack([(F32(0.5) * t).astype(F32), np.nextafter(t, F32(0)), t, np.nextafter(t, inf),
                        (F32(2) * t).astype(F32), np.full(t.size, inf, F32)])
    return np.where(ids >= 0, choices[turn, np.arange(ids.size)], own).astype(F32), turn


def _ray_inputs(scene):
    d = E.edge_scene(scene)
    out = [Input(f"{scene}/{cls}", "ray", scene, d, E.pack(*E.ray_class(scene, cls))) for cls in E.CLASSES]
    o, dirs, tm = E.ray_class(scene, SWEEP_CLASS[scene])
    ids, t, _ = E.oracle_hits(scene, SWEEP_CLASS[scene])
    tmv, turn = sweep_tmax(ids, t, tm)
    sweep = Input(f"{scene}/tmax", "ray", scene, d, E.pack(o, dirs, tmv))
    sweep.turn, sweep.tstar_ids, sweep.tstar = turn, ids, t
    return out + [sweep]


# ---- group 3: mesh space ----

def _with_tree(mesh_arrays):
    """Scene arrays of a mesh: its own arrays and the tree of Mesh.from_arrays(v, i).build_lbvh(2)."""
    import rtamd
    v = np.ascontiguousarray(mesh_arrays["vertices"], F32)
    b = rtamd.Mesh.from_arrays(v, mesh_arrays["indices"]).build_lbvh(2)
    return dict(mesh_arrays, vertices=v, nodes=b.nodes.copy(), tri_indices=b.tri_indices.copy(),
                scene_min=v[:, :3].min(0), scene_max=v[:, :3].max(0))


def tiny_tris():
    """64 right triangles with legs of 2^-e and 2^-e (1 + 2^-7), sixteen each for e in TINY_EXPONENTS.
    Triangle j lies in the plane `axis = c`, |c| from 4 to 19 on either side, its other two coordinates
    small multiples of 2^-e: it stands off all three coordinate planes, its vertices are exact, and the
    Cramer determinant, 2^-2e (1 + 2^-7) c, is a normal float32.  The second leg is not a power of two so
    that |cross(e1, e2)|^2 = 2^-4e (1 + 2^-6 + 2^-14) does not fit the nine bits a subnormal near 2^-140
    has: at e = 35 normalize without its rescale would return another ng.  The corner normals differ.
    Ray j runs along the axis from 2 units off the plane through (a + leg / 4, b + second leg / 2), an
    exact interior point, so u and v are 1/4 and 1/2 to a rounding, by the winding either way round.
    Returns (mesh arrays, origins, directions, exponent per triangle, the triangle id each ray must
    hit)."""
    rng = np.random.default_rng(62)
    mats = load_golden("cornell12")["materials"]
    verts, normals, o, dirs, exps = [], [], [], [], []
    for e in TINY_EXPONENTS:
        leg = np.ldexp(1.0, -e)
        leg2 = leg * TINY_SECOND_LEG
        for j in range(16):
            axis, flip, side = j % 3, (j // 3) % 2 == 1, 1.0 if (j // 6) % 2 == 0 else -1.0
            a, b, c = (2 * j + 1) * leg, (2 * j + 3) * leg, side * (4.0 + j)
            from_above = 1.0 if j % 2 == 0 else -1.0
            u_ax, v_ax = (axis + 1) % 3, (axis + 2) % 3
            p = np.zeros((3, 3))
            p[:, axis], p[:, u_ax], p[:, v_ax] = c, a, b
            p[1, u_ax] += leg
            p[2, v_ax] += leg2
            if flip:
                p[[1, 2]] = p[[2, 1]]
            verts.append(p)
            n = np.zeros((3, 3))
            n[:, axis] = 1.0
            n += 0.3 * rng.uniform(-1.0, 1.0, (3, 3))
            normals.append(n / np.linalg.norm(n, axis=1)[:, None])
            start = np.zeros(3)
            start[axis], start[u_ax], start[v_ax] = c + 2.0 * from_above, a + leg / 4, b + leg2 / 2
            dd = np.zeros(3)
            dd[axis] = -from_above
            o.append(start)
            dirs.append(dd)
            exps.append(e)
    v64 = np.concatenate(verts)
    v = np.ones((v64.shape[0], 4), F32)
    v[:, :3] = v64.astype(F32)
    assert np.array_equal(v[:, :3].astype(np.float64), v64), "a vertex of tiny_tris is not exact in float32"
    nrm = np.zeros((v.shape[0], 4), F32)
    nrm[:, :3] = np.concatenate(normals).astype(F32)
    idx = np.arange(v.shape[0], dtype=np.int32)
    o64 = np.array(o)
    assert np.array_equal(o64.astype(F32).astype(np.float64), o64), "an origin of tiny_tris is not exact in float32"
    arrays = {"vertices": v, "indices": idx, "normals": nrm, "normals_indices": idx.copy(), "materials": mats,
              "tri_to_material": (np.arange(64) % mats.shape[0]).astype(np.int32)}
    return arrays, o64.astype(F32), np.array(dirs, F32), np.array(exps), 3 * np.arange(64, dtype=np.int32)


def _mesh_input(label):
    import rtamd
    inf = F32(np.inf)
    if label == "tiny_tris":
        arrays, o, dirs, exps, own = tiny_tris()
        inp = Input(label, "mesh", label, _with_tree(arrays), rtamd.pack_rays(o, dirs, np.full(o.shape[0], inf, F32)))
        inp.exponents, inp.own = exps, own
        return inp
    if label.startswith("rand512*2^"):
        k = int(label[len("rand512*2^"):])
        base = M.arrays("rand2k_first512")
        v = np.array(base["vertices"], F32, copy=True)
        v[:, :3] = np.ldexp(v[:, :3], k).astype(F32)
        assert np.array_equal(np.ldexp(v[:, :3].astype(np.float64), -k), base["vertices"][:, :3].astype(np.float64))
        o, dirs, _ = incoherent_rays(base, n=1024)
        o = np.ldexp(o, k).astype(F32)
        inp = Input(label, "mesh", label, _with_tree(dict(base, vertices=v)), rtamd.pack_rays(o, dirs, np.full(1024, inf, F32)))
        inp.scale = k
        return inp
    arrays = M.arrays(label)
    o, dirs, _ = incoherent_rays(arrays, n=1024)
    return Input(label, "mesh", label, _with_tree(arrays), rtamd.pack_rays(o, dirs, np.full(1024, inf, F32)))


# ---- the inputs ----

_CASES, _BY_LABEL = {}, {}


def inputs_of(case):
    """The inputs of a case (one of CASES), built once."""
    if case not in _CASES:
        group = group_of(case)
        with np.errstate(all="ignore"):
            _CASES[case] = [_normal_input(case)] if group == "normal" else _ray_inputs(case) if group == "ray" else [_mesh_input(case)]
        for inp in _CASES[case]:
            _BY_LABEL[inp.label] = inp
    return _CASES[case]


def get(label):
    """An input by its label."""
    if label not in _BY_LABEL:
        inputs_of(label if label in CASES else label.split("/")[0])
    return _BY_LABEL[label]


def cases_of(group):
    return [c for c in CASES if group_of(c) == group]


# ---- float64 ----

def triangles64(d, ids):
    """(p0, p1, p2) float64 (n, 3) of the triangles with these hit ids."""
    v = np.asarray(d["vertices"], np.float64)[:, :3]
    tri = np.asarray(d["indices"])[np.asarray(ids)[:, None] + np.arange(3)[None, :]]
    return v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]


def float64_errors(d, rays, records):
    """A gross-error check of records against float64, over the rows that hit and hold no NaN:
    dict(rows, bary, p, ng, ndotd, unit).  bary: the largest |(1 - u - v) p0 + u p1 + v p2 - (o + t d)|
    relative to max|vertex| + |o| + t; p: the largest |p - (o + (t - 0.001) d)| by the same scale; ng and
    ndotd: the largest difference from the winding's unit normal where |cross(e1, e2)|^2 is a normal
    float32; unit: the largest | |ng| - 1 | over every row."""
    a = words(records)
    r = ray_words(rays).astype(np.float64)
    ids = a[:, ID].view(np.int32)
    rows = np.flatnonzero((ids >= 0) & ~nan_words(a).any(axis=1))
    out = dict(rows=int(rows.size), bary=0.0, p=0.0, ng=0.0, ndotd=0.0, unit=0.0)
    if rows.size == 0:
        return out
    a, r, ids = a[rows], r[rows], ids[rows]
    with np.errstate(all="ignore"):
        p0, p1, p2 = triangles64(d, ids)
        f = lambda cols: a[:, cols].view(F32).astype(np.float64)
        t, u, v = f([T])[:, 0], f([U])[:, 0], f([V])[:, 0]
        o, dn = r[:, 0:3], r[:, 4:7].copy()
        big = np.abs(dn).max(axis=1)                         # normalise without overflow or underflow
        dn /= big[:, None]
        dn /= np.linalg.norm(dn, axis=1)[:, None]
        scale = np.abs(np.asarray(d["vertices"], np.float64)[:, :3]).max() + np.linalg.norm(o, axis=1) + t
        surface = o + dn * t[:, None]
        bary = (1.0 - u - v)[:, None] * p0 + u[:, None] * p1 + v[:, None] * p2
        out["bary"] = float(np.max(np.abs(bary - surface).max(axis=1) / scale))
        out["p"] = float(np.max(np.abs(f([4, 5, 6]) - (o + dn * (t - 0.001)[:, None])).max(axis=1) / scale))
        g = np.cross(p1 - p0, p2 - p0)
        l2 = np.sum(g * g, axis=1)
        ng = f([8, 9, 10])
        out["unit"] = float(np.max(np.abs(np.linalg.norm(ng, axis=1) - 1.0)))
        ok = (l2 >= np.ldexp(1.0, -126)) & (l2 < np.ldexp(1.0, 128))
        if np.any(ok):
            gu = g[ok] / np.sqrt(l2[ok])[:, None]
            out["ng"] = float(np.max(np.abs(ng[ok] - gu)))
            out["ndotd"] = float(np.max(np.abs(f([NDOTD])[ok, 0] - np.sum(gu * dn[ok], axis=1))))
    return out


def ns_well_conditioned(d, rays, records):
    """(n,) bool: the hits whose shading normal is well conditioned, from a float64 evaluation on the
    records' own p.  normal_at divides Cramer determinants on absolute positions, each a sum of products
    of three coordinates, by Det = p0 . (p1 x p2): a rounding error of 2^-24 |p0| |p1| |p2| in a numerator
    is a relative error of 2^-24 |p0| |p1| |p2| / |Det| in a weight, and normalize divides by the length
    of the weighted sum; p itself carries a rounding error of 2^-24 (|o| + t).  Well conditioned: finite
    corner normals, |Det| >= 1e-3 |p0| |p1| |p2|, p no further out than twice the farthest corner and
    |o| + t no more than 16 times it, and the weighted sum at least a tenth as long as the longest corner
    normal -- an amplification of at most 1.6e5 on 6e-8, which the normalised ns shows as 1e-2 at most.
    Everywhere else ns may differ between arithmetics by any amount up to 2."""
    a = words(records)
    ids = a[:, ID].view(np.int32)
    ok = np.zeros(ids.size, bool)
    rows = np.flatnonzero((ids >= 0) & ~nan_words(a).any(axis=1))
    if rows.size == 0:
        return ok
    with np.errstate(all="ignore"):
        p0, p1, p2 = triangles64(d, ids[rows])
        nrm = np.asarray(d["normals"], np.float64)[:, :3]
        ni = np.asarray(d["normals_indices"])[ids[rows][:, None] + np.arange(3)[None, :]]
        n0, n1, n2 = nrm[ni[:, 0]], nrm[ni[:, 1]], nrm[ni[:, 2]]
        p = a[rows][:, [4, 5, 6]].view(F32).astype(np.float64)
        r = ray_words(rays)[rows].astype(np.float64)
        reach = np.linalg.norm(r[:, 0:3], axis=1) + a[rows, T].view(F32).astype(np.float64)
        det3 = lambda x, y, z: np.einsum("ij,ij->i", x, np.cross(y, z))
        det = det3(p0, p1, p2)
        size = np.linalg.norm(p0, axis=1) * np.linalg.norm(p1, axis=1) * np.linalg.norm(p2, axis=1)
        far = np.maximum(np.maximum(np.linalg.norm(p0, axis=1), np.linalg.norm(p1, axis=1)), np.linalg.norm(p2, axis=1))
        near = (np.linalg.norm(p, axis=1) <= 2.0 * far) & (reach <= 16.0 * far)
        mix = (det3(p, p1, p2) / det)[:, None] * n0 + (det3(p0, p, p2) / det)[:, None] * n1 + (det3(p0, p1, p) / det)[:, None] * n2
        longest = np.maximum(np.maximum(np.linalg.norm(n0, axis=1), np.linalg.norm(n1, axis=1)), np.linalg.norm(n2, axis=1))
        good = np.isfinite(n0).all(axis=1) & np.isfinite(n1).all(axis=1) & np.isfinite(n2).all(axis=1) & near \
            & (np.abs(det) >= 1e-3 * size) & (np.linalg.norm(mix, axis=1) >= 0.1 * longest) & (size < np.ldexp(1.0, 120))
    ok[rows] = good
    return ok


def ns_counts(records):
    """(hits, hits whose ns holds a NaN, hits whose ns is (0, 0, 0) of either sign)."""
    a = words(records)
    hit = a[:, ID].view(np.int32) >= 0
    ns = a[hit][:, NS_WORDS].view(F32)
    return int(hit.sum()), int(np.isnan(ns).any(axis=1).sum()), int(np.all(ns == 0, axis=1).sum())


def on_edge(records):
    """Hits whose barycentrics lie on an edge exactly: u == 0, v == 0 or u + v == 1 (float32)."""
    a = words(records)
    hit = a[:, ID].view(np.int32) >= 0
    u, v = a[hit, U].view(F32), a[hit, V].view(F32)
    return int(np.sum((u == 0) | (v == 0) | ((u + v).astype(F32) == 1)))
