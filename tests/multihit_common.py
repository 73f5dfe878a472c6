"""Shared by test_multihit.py (CPU) and test_multihit_gpu.py: the inputs and the yardsticks of the
first-k-hits ray queries.

Inputs are ray_query_common's incoherent rays (2,000 per fixture) under two tmax -- the default, and a
finite one per ray drawn around the distance of the point the ray is aimed at, which lies inside the
scene box, so that it cuts the lists short --, the tie scene (rand2k's mesh with every triangle a second
time), the duplicate sets (rays aimed at the triangles a tree references from more than one leaf) and
the edge rays.

Yardsticks: tests/multihit_ref.c, a plain-C restatement of the definition in S_strict, compiled here at
test time into a temporary folder (removed at exit) with cc -O2 -ffp-contract=off: (a) ray_tri on every
triangle and the k smallest (t, id) in (0.001f, tmax), (b) the traversal over the BVH_Node_ array with
the list.  Results are words uint32 (k, n, 4): plane j, ray i."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from ray_query_common import N_RAYS, TMAX_DEFAULT, incoherent_rays, scene_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
FIXTURES = ["cornell12", "rand2k", "hf40k", "knot16k", "cubes2_obj", "rand3k_bigleaf", "rand4k_sbvh"]
TMAXES = ["default", "cut"]
MAX_K = 8
BRUTE_K = 9   # (a) is computed once with nine planes: the planes of a smaller k are its first k
MISS_ID = 0xFFFFFFFF

_lib = None
_RAYS = {}
_BRUTE = {}
_TRAV = {}
_DUP = {}
_SCENES = {}


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="rtamd_multihit_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "multihit_ref.so")
        subprocess.run(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(HERE, "multihit_ref.c"), "-lm"], check=True, capture_output=True)
        L = C.CDLL(so)
        vp, i32 = C.c_void_p, C.c_int32
        L.multihit_ref_brute.restype = None
        L.multihit_ref_brute.argtypes = [vp, vp, i32, vp, C.c_int64, i32, vp]
        L.multihit_ref_traverse.restype = None
        L.multihit_ref_traverse.argtypes = [vp, vp, vp, i32, vp, vp, C.c_int64, i32, vp, vp, vp, i32]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _mesh(d):
    return (np.ascontiguousarray(d["vertices"], F32).reshape(-1, 4), np.ascontiguousarray(d["indices"], np.int32).reshape(-1))


def ray_words(rays):
    """RAY_DTYPE records as uint32 (n, 8), contiguous."""
    a = np.ascontiguousarray(rays)
    return a.view(np.uint8).reshape(-1).view(np.uint32).reshape(a.shape[0], 8)


def planes(rec):
    """rt_hit_uv records (k, n) of HIT_UV_DTYPE, or words already, as uint32 (k, n, 4)."""
    a = np.ascontiguousarray(rec)
    if a.dtype == np.uint32:
        return a
    return a.view(np.uint8).reshape(-1).view(np.uint32).reshape(a.shape[0], a.shape[1], 4)


def miss_words(rays, k):
    """uint32 (k, n, 4): k miss records per ray, {-1, the ray's tmax word, 0, 0}."""
    w = np.zeros((k, rays.shape[0], 4), np.uint32)
    w[:, :, 0] = MISS_ID
    w[:, :, 1] = ray_words(rays)[None, :, 3]
    return w


def brute(d, rays, k):
    """(a): words uint32 (k, n, 4), k up to 16."""
    v, idx = _mesh(d)
    rw = ray_words(rays)
    out = np.zeros((k, rw.shape[0], 4), np.uint32)
    lib().multihit_ref_brute(_p(v), _p(idx), idx.size // 3, _p(rw), rw.shape[0], k, _p(out))
    return out


def traverse(d, rays, k, presence=True):
    """(b): (words uint32 (k, n, 4), {overflows, inner_visits, tri_tests}, deepest int32 (n,))."""
    v, idx = _mesh(d)
    nodes = np.ascontiguousarray(d["nodes"], F32).reshape(-1, 12)
    refs = np.ascontiguousarray(d["tri_indices"], np.int32).reshape(-1)
    rw = ray_words(rays)
    n = rw.shape[0]
    out = np.zeros((k, n, 4), np.uint32)
    st = np.zeros(3, np.uint64)
    deepest = np.zeros(n, np.int32)
    lib().multihit_ref_traverse(_p(v), _p(idx), _p(nodes), nodes.shape[0], _p(refs), _p(rw), n, k, _p(out), _p(st),
                                _p(deepest), 1 if presence else 0)
    return out, {"overflows": int(st[0]), "inner_visits": int(st[1]), "tri_tests": int(st[2])}, deepest


def cut_tmax(d, o, dirs, seed=31):
    """float32 (n,): per ray the length of its direction -- the distance to the point inside the scene
    box it is aimed at -- times a factor uniform in [0.6, 1.4): about half of what lies along the ray."""
    rng = np.random.default_rng(seed + d["vertices"].shape[0])
    length = np.sqrt(np.sum(dirs.astype(np.float64) ** 2, axis=1))
    return (length * rng.uniform(0.6, 1.4, o.shape[0])).astype(F32)


def rays(name, which):
    """The 2,000 incoherent rays of a fixture (or of "tie") under a tmax, packed, computed once (shared;
    do not modify)."""
    if (name, which) not in _RAYS:
        import rtamd
        d = scene(name)
        o, dirs, _ = incoherent_rays(d)
        _RAYS[(name, which)] = rtamd.pack_rays(o, dirs, None if which == "default" else cut_tmax(d, o, dirs))
    return _RAYS[(name, which)]


def scene(name):
    """ray_query_common's scenes, "tie": rand2k's mesh with every triangle appended a second time
    (ids i and i + 3 * 2000), in the host twin's tree of build_lbvh(2, keys="extent"), and "tie_swapped"."""
    if name == "tie_swapped":   # the same tree with every reference swapped for its twin's: the higher id of a pair is met first
        if name not in _SCENES:
            d = dict(scene("tie"))
            d["tri_indices"] = ((np.asarray(d["tri_indices"], np.int32) + 6000) % 12000).astype(np.int32)
            _SCENES[name] = d
        return _SCENES[name]
    if name != "tie":
        return scene_arrays(name)
    if name not in _SCENES:
        import rtamd
        d = dict(scene_arrays("rand2k"))
        idx = np.asarray(d["indices"], np.int32).reshape(-1)
        assert idx.size == 3 * 2000
        d["indices"] = np.concatenate([idx, idx])
        d["normals_indices"] = np.concatenate([d["normals_indices"], d["normals_indices"]])
        d["tri_to_material"] = np.concatenate([d["tri_to_material"], d["tri_to_material"]])
        b = rtamd.Mesh.from_arrays(d["vertices"], d["indices"]).build_lbvh(2, keys="extent")
        d["nodes"], d["tri_indices"] = b.nodes, b.tri_indices
        _SCENES[name] = d
    return _SCENES[name]


def brute9(name, which):
    """(a) with nine planes for a fixture's rays under a tmax, computed once (shared; do not modify)."""
    if (name, which) not in _BRUTE:
        _BRUTE[(name, which)] = brute(scene(name), rays(name, which), BRUTE_K)
    return _BRUTE[(name, which)]


def traversal(name, which, k):
    """(b) for a fixture's rays under a tmax, computed once per k (shared; do not modify)."""
    if (name, which, k) not in _TRAV:
        _TRAV[(name, which, k)] = traverse(scene(name), rays(name, which), k)
    return _TRAV[(name, which, k)]


def found(w):
    """int (n,): the records of each row of words (k, n, 4) that are no miss."""
    return (w[:, :, 0] != MISS_ID).sum(axis=0)


def repeats(w):
    """bool (n,): the rows of words (k, n, 4) in which a found id appears twice."""
    ids = w[:, :, 0].view(np.int32).T                                            # (n, k)
    out = np.zeros(ids.shape[0], bool)
    for a in range(ids.shape[1]):
        for b in range(a + 1, ids.shape[1]):
            out |= (ids[:, a] >= 0) & (ids[:, a] == ids[:, b])
    return out


def multiply_referenced(d):
    """The ids (3 * index) of the triangles that d's tree references more than once, ascending."""
    ids, count = np.unique(np.asarray(d["tri_indices"]).reshape(-1), return_counts=True)
    return ids[count > 1].astype(np.int64)


def duplicate_set(name, per=16, seed=23, draws=None):
    """(packed rays with the default tmax, (a) words (8, n, 4)): `per` rays per multiply-referenced
    triangle of the fixture, each from a random origin (the scene box grown by 20 units) at a random
    point of the triangle, computed once (shared; do not modify).

    draws=None: the first `per` drawn.  Otherwise `draws` rays are drawn per triangle and yardstick (b)
    chooses `per` of them: in draw order, first those whose row repeats an id when (b) runs WITHOUT
    the presence check (a second reference shows only where the ray passes through two leaves that
    hold the triangle)."""
    key = (name, per, draws)
    if key not in _DUP:
        import rtamd
        d = scene_arrays(name)
        ids = multiply_referenced(d)
        m = draws or per
        v = d["vertices"][:, :3].astype(np.float64)
        idx = np.asarray(d["indices"]).reshape(-1)
        rng = np.random.default_rng(seed)
        t = np.repeat(ids, m)
        tri = v[np.stack([idx[t], idx[t + 1], idx[t + 2]], axis=1)]              # (n, 3 vertices, 3)
        b = rng.dirichlet((1.0, 1.0, 1.0), t.size)
        target = np.einsum("mk,mkc->mc", b, tri)
        o = rng.uniform(v.min(0) - 20.0, v.max(0) + 20.0, (t.size, 3)).astype(F32)
        cand = rtamd.pack_rays(o, (target - o).astype(F32), None)
        if draws:
            bites = repeats(traverse(d, cand, MAX_K, presence=False)[0]).reshape(ids.size, m)
            keep = np.argsort(~bites, axis=1, kind="stable")[:, :per]            # biting draws first, in draw order
            cand = np.ascontiguousarray(cand.reshape(ids.size, m)[np.arange(ids.size)[:, None], np.sort(keep, axis=1)].reshape(-1))
        _DUP[key] = (cand, brute(d, cand, MAX_K))
    return _DUP[key]


def edge_rays(d):
    """The edge set on scene d: (packed rays, what each is, whether it is valid).  An origin or direction
    component NaN or +-inf, a zero direction of either sign, tmax NaN (two payloads), 0, -1, 0.001f and
    the float below it (nothing can be accepted), the float above 0.001f, +inf, the default."""
    import rtamd
    o0, d0, _ = incoherent_rays(d, n=1)
    o, dr, tm, what, ok = [], [], [], [], []

    def add(oo, dd, t, label, valid):
        o.append(np.asarray(oo, F32)); dr.append(np.asarray(dd, F32)); tm.append(t); what.append(label); ok.append(valid)

    for bad, label in ((np.nan, "nan"), (np.inf, "+inf"), (-np.inf, "-inf")):
        for ax in range(3):
            p = o0[0].copy(); p[ax] = bad
            add(p, d0[0], TMAX_DEFAULT, f"origin {ax} {label}", False)
            q = d0[0].copy(); q[ax] = bad
            add(o0[0], q, TMAX_DEFAULT, f"direction {ax} {label}", False)
    add(o0[0], [0.0, 0.0, 0.0], TMAX_DEFAULT, "direction zero", False)
    add(o0[0], [-0.0, 0.0, -0.0], TMAX_DEFAULT, "direction signed zero", False)
    nan2 = np.array([0x7FC00000, 0xFFC12345], np.uint32).view(F32)
    add(o0[0], d0[0], nan2[0], "tmax nan", False)
    add(o0[0], d0[0], nan2[1], "tmax nan with a payload", False)
    for t, label in ((0.0, "tmax 0"), (-1.0, "tmax -1"), (-np.inf, "tmax -inf"), (F32(0.001), "tmax 0.001f"),
                     (np.nextafter(F32(0.001), F32(0)), "tmax below 0.001f")):
        add(o0[0], d0[0], F32(t), label, False)
    add(o0[0], d0[0], np.nextafter(F32(0.001), F32(1)), "tmax above 0.001f", True)
    add(o0[0], d0[0], F32(np.inf), "tmax +inf", True)
    add(o0[0], d0[0], TMAX_DEFAULT, "default", True)
    return rtamd.pack_rays(np.stack(o), np.stack(dr), np.array(tm, F32)), what, np.array(ok)


def same_planes(got, want, label):
    got, want = planes(got), planes(want)
    assert got.shape == want.shape, f"{label}: {got.shape} vs {want.shape}"
    bad = np.argwhere(np.any(got != want, axis=2))
    assert bad.shape[0] == 0, f"{label}: {bad.shape[0]} records differ, first (plane, ray) {bad[:4].tolist()}: " \
                              f"{[got[j, i].tolist() for j, i in bad[:2]]} vs {[want[j, i].tolist() for j, i in bad[:2]]}"


def check_rows(w, rays, label):
    """Rows ascend in (t, id) with the misses last, no id appears twice, a miss is the miss record."""
    ids = w[:, :, 0].view(np.int32)
    t = w[:, :, 1].view(F32)
    hit = ids >= 0
    assert np.all(hit[:-1] | ~hit[1:]), f"{label}: a miss before a found record"
    both = hit[:-1] & hit[1:]
    asc = (t[:-1] < t[1:]) | ((t[:-1] == t[1:]) & (ids[:-1] < ids[1:]))
    assert np.all(asc | ~both), f"{label}: a row is not sorted by (t, id)"
    assert not np.any(repeats(w)), f"{label}: an id twice"
    assert np.array_equal(w[~hit], miss_words(rays, w.shape[0])[~hit]), f"{label}: a miss is not the miss record"
    tmax = ray_words(rays)[:, 3].view(F32)
    assert np.all((t > F32(0.001)) & (t < tmax[None, :]) | ~hit), f"{label}: a hit outside (0.001f, tmax)"
