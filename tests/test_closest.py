"""Closest-point queries without a GPU: rt_closest_points_host, the definition in host
code, against the yardsticks of tests/closest_common.py -- (a) the brute force over all triangles and
(b) the traversal over the BVH_Node_ array, both of tests/closest_ref.c, and a float64 numpy distance.
Records are compared as words."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtamd
import closest_common as K
from ray_query_common import scene_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-opencl-raytracer_amd")
F32 = np.float32
INVALID, BAD_SCENE = -1, -5
BIG_FIXTURE = 5000   # triangles above which the float64 yardstick takes every 4th point (it costs points x triangles)


def twin(d, rec, stats=False):
    return rtamd.closest_points_host(rtamd.Scene.from_arrays(d), rec, stats=stats)


def same_words(got, want, label):
    got, want = K.words(got), K.words(want)
    assert got.shape == want.shape, f"{label}: {got.shape} vs {want.shape}"
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert bad.size == 0, f"{label}: {bad.size} records differ, first {bad[:4].tolist()}: " \
                          f"{[got[i].tolist() for i in bad[:2]]} vs {[want[i].tolist() for i in bad[:2]]}"


def f32(words_column):
    return np.ascontiguousarray(words_column).view(F32)


@pytest.mark.parametrize("name", K.FIXTURES)
def test_twin_equals_the_traversal_and_the_brute_force(name):
    """All 8 words of every record and the overflow count against (b); every word against (a): the
    result is the mesh's, whatever the tree.  No point is set aside."""
    d = scene_arrays(name)
    for which in K.RADII:
        a, b, st, _ = K.yardstick(name, which)
        got, gst = twin(d, K.records(name, which), stats=True)
        same_words(got, b, f"{name} {which} vs the traversal")
        assert gst == st, f"{name} {which}: counters {gst} vs {st}"
        same_words(got, a, f"{name} {which} vs the brute force")
        miss = np.mean(a[:, 0] == 0xFFFFFFFF)
        print(f"{name} {which}: misses {miss:.3f}, inner visits {st['inner_visits'] / a.shape[0]:.1f}, "
              f"triangle tests {st['tri_tests'] / a.shape[0]:.1f} per point")
        assert st["overflows"] == 0
        assert miss == 0.0 if which == "inf" else 0.25 <= miss <= 0.50


@pytest.mark.parametrize("name", K.FIXTURES)
def test_distance_against_float64(name):
    """|sqrt(d2) - D64| <= 1e-6 x (max|q_k| + scene diagonal), D64 the float64 minimum over all triangles."""
    d = scene_arrays(name)
    step = 4 if d["indices"].size // 3 > BIG_FIXTURE else 1
    q = K.points(name)[::step]
    got = twin(d, rtamd.pack_points(q, None))
    D = K.dist64(d, q)
    err = np.abs(np.sqrt(got["d2"].astype(np.float64)) - D)
    scale = np.abs(q.astype(np.float64)).max(axis=1) + K.diagonal(d)
    print(f"{name}: worst error {np.max(err / scale):.3g} of the scale over {q.shape[0]} points")
    assert np.all(got["id"] >= 0)
    assert np.all(err <= 1e-6 * scale)


@pytest.mark.parametrize("name", K.FIXTURES)
def test_record_words_are_consistent(name):
    """u, v >= 0 and u + v <= 1 + 2^-22; p is the fma expression of (u, v) and d2 is dot(q - p, q - p),
    word for word, evaluated here in float64 arithmetic that is exact for one float32 operation."""
    d = scene_arrays(name)
    q = K.points(name)
    got = twin(d, rtamd.pack_points(q, None))
    idx, v = d["indices"], d["vertices"][:, :3].astype(F32)
    t = got["id"]
    p0 = v[idx[t]]
    e1, e2 = (v[idx[t + 1]] - p0).astype(F32), (v[idx[t + 2]] - p0).astype(F32)
    u, w = got["u"], got["v"]
    assert np.all(u >= 0) and np.all(w >= 0) and np.all(u.astype(np.float64) + w <= 1.0 + 2.0 ** -22)

    def fma(a, b, c):   # one rounding: the float64 product of two float32 is exact, and so is what is added here
        return _round_sum(a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64))
    p = fma(w[:, None], e2, fma(u[:, None], e1, p0))
    assert np.array_equal(p.view(np.uint32), np.ascontiguousarray(got["p"]).view(np.uint32)), "p is not fma(v, e2, fma(u, e1, p0))"
    df = (q - p).astype(F32)
    d2 = fma(df[:, 2], df[:, 2], fma(df[:, 1], df[:, 1], (df[:, 0] * df[:, 0]).astype(F32)))
    assert np.array_equal(d2.view(np.uint32), got["d2"].view(np.uint32)), "d2 is not dot(q - p, q - p)"


def _round_sum(x, y):
    """fl32(x + y) for float64 x and y, rounded once.  s = fl64(x + y) and its exact error (two-sum):
    rounding s again gives the right float32 unless s lies exactly half-way between two of them while
    the exact sum does not; then the error's sign says which neighbour it is."""
    s = x + y
    bb = s - x
    err = (x - (s - bb)) + (y - bb)
    r = s.astype(F32)
    back = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > back, F32(np.inf), F32(-np.inf)).astype(F32))
    tie = (s != back) & (s == 0.5 * (back + other.astype(np.float64))) & (err != 0.0)
    hi, lo = np.maximum(r, other), np.minimum(r, other)
    return np.where(tie, np.where(err > 0.0, hi, lo), r).astype(F32)


def test_a_point_that_is_a_mesh_vertex():
    """The record's d2 is the brute force's word (0 where the vertex is its triangle's p0), and the id is
    the lowest among the triangles at the minimum."""
    for name in ("hf40k", "knot16k", "rand2k"):
        d = scene_arrays(name)
        idx = d["indices"]
        tris = np.arange(0, idx.size // 3, max(1, idx.size // 3 // 200))
        for corner in (0, 1, 2):
            q = d["vertices"][idx[3 * tris + corner], :3].astype(F32)
            rec = rtamd.pack_points(q, None)
            got = twin(d, rec)
            a = K.brute(d, rec)
            same_words(got, a, f"{name} corner {corner}")
            if corner == 0:
                # q == p0 of triangle `tris`: f gives exactly 0 for it, so the minimum is 0 ...
                assert np.all(got["d2"].view(np.uint32) == 0)
            # ... and the id is the lowest of all triangles that reach the minimum
            for i in range(0, q.shape[0], 17):
                all_d2 = np.array([K.ref_tri(q[i], *d["vertices"][idx[3 * t:3 * t + 3], :3].astype(F32))[5]
                                   for t in _tris_near(d, q[i])])
                near = _tris_near(d, q[i])
                lowest = 3 * int(near[np.flatnonzero(all_d2 == all_d2.min())[0]])
                assert got["id"][i] == lowest and got["d2"][i] == all_d2.min()
        assert np.unique(got["id"]).size > 10


def _tris_near(d, q):
    """The triangles that have q as a vertex or lie within a small box of it (ascending)."""
    v = d["vertices"][d["indices"].reshape(-1, 3), :3]
    lo, hi = v.min(axis=1), v.max(axis=1)
    pad = 1e-3 * K.diagonal(d)
    return np.flatnonzero(np.all((lo - pad <= q) & (q <= hi + pad), axis=1))


def test_edge_set_one_consequence_at_a_time():
    d = scene_arrays("rand2k")
    rec, what = K.edge_points(d)
    got = twin(d, rec)
    same_words(got, K.brute(d, rec), "edge set vs the brute force")
    same_words(got, K.traverse(d, rec)[0], "edge set vs the traversal")
    w = K.words(got)
    for i, label in enumerate(what):
        found = got["id"][i] >= 0
        if label.startswith("coordinate") or label in ("r nan", "r 0", "r -0", "r -1"):
            assert np.array_equal(w[i], K.MISS_WORDS), f"{label}: an invalid point is a miss"
        elif label in ("r subnormal", "r 1e-30"):
            assert np.array_equal(w[i], K.MISS_WORDS), f"{label}: r * r underflows to 0 and nothing is below 0"
        else:
            assert found and np.isfinite(got["d2"][i]), f"{label}: r * r = +inf bounds nothing"
    # r equal to the exact distance is exclusive: a miss; the float above it finds the triangle
    tri = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]], F32)
    s = K.two_tri_scene(tri)
    q = np.array([[1, 1, 3]] * 2, F32)                       # distance exactly 3, d2 = 9
    r = np.array([3.0, np.nextafter(F32(3.0), F32(4.0))], F32)
    got = twin(s, rtamd.pack_points(q, r))
    assert np.array_equal(K.words(got)[0], K.MISS_WORDS), "r equal to the distance is a miss"
    assert got["id"][1] == 0 and got["d2"][1] == F32(9.0) and tuple(got["p"][1]) == (1.0, 1.0, 0.0)
    # a degenerate triangle beside a proper one: three equal vertices, collinear vertices
    deg = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[9, 9, 9], [9, 9, 9], [9, 9, 9]], [[20, 0, 0], [21, 0, 0], [23, 0, 0]]], F32)
    s = K.two_tri_scene(deg)
    q = np.array([[1, 1, 1], [9, 9, 8], [22, 1, 0], [9.5, 9, 9], [100, 100, 100]], F32)
    rec = rtamd.pack_points(q, None)
    got = twin(s, rec)
    same_words(got, K.brute(s, rec), "degenerate triangles vs the brute force")
    assert got["id"].tolist()[:3] == [0, 3, 6] and not np.any(np.isnan(got["d2"]))
    # coordinates at 2^60: whatever f gives (products of 2^60-sized dots overflow to inf - inf = NaN, which
    # is never accepted) equals the brute force; at 2^64 d2 itself is +inf: a miss even with r = +inf
    big = np.array([[2.0 ** 60] * 3, [-2.0 ** 60, 0, 0], [2.0 ** 64] * 3, [0, -2.0 ** 64, 0]], F32)
    rec = rtamd.pack_points(big, None)
    got = twin(d, rec)
    same_words(got, K.brute(d, rec), "2^60 and 2^64 vs the brute force")
    same_words(got, K.traverse(d, rec)[0], "2^60 and 2^64 vs the traversal")
    assert np.array_equal(K.words(got)[2], K.MISS_WORDS) and np.array_equal(K.words(got)[3], K.MISS_WORDS)
    # a root leaf of one triangle
    s = scene_arrays("single_tri_rootleaf")
    rec = rtamd.pack_points(K.make_points(s, 256), None)
    got, st = twin(s, rec, stats=True)
    same_words(got, K.brute(s, rec), "single_tri_rootleaf")
    assert st == {"overflows": 0, "inner_visits": 0, "tri_tests": 256} and np.all(got["id"] == 0)


def test_seven_regions_of_one_triangle():
    """One point per region of f on the triangle (0,0,0) (4,0,0) (0,4,0), u and v known exactly."""
    s = K.two_tri_scene(np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]], F32))
    q = np.array([[-1, -1, 2], [6, -1, 0], [-1, 6, 0], [1, -2, 0], [-2, 3, 0], [3, 3, 1], [1, 2, -5]], F32)
    want_uv = [(0, 0), (1, 0), (0, 1), (0.25, 0), (0, 0.75), (0.5, 0.5), (0.25, 0.5)]
    want_p = [(0, 0, 0), (4, 0, 0), (0, 4, 0), (1, 0, 0), (0, 3, 0), (2, 2, 0), (1, 2, 0)]
    want_d2 = [6, 5, 5, 4, 4, 3, 25]
    got = twin(s, rtamd.pack_points(q, None))
    for i in range(7):
        assert (got["u"][i], got["v"][i]) == want_uv[i], f"region {i}: (u, v) = {(got['u'][i], got['v'][i])}"
        assert tuple(got["p"][i]) == want_p[i] and got["d2"][i] == want_d2[i] and got["id"][i] == 0, f"region {i}"
        r = K.ref_tri(q[i], *s["vertices"][:3, :3])
        assert (r[0], r[1], r[5]) == (got["u"][i], got["v"][i], got["d2"][i])


def test_overflow_comb_and_the_comb_cut_to_40_levels():
    d = scene_arrays("overflow_comb")
    rec = rtamd.pack_points(K.make_points(d, 4096), None)
    got, st = twin(d, rec, stats=True)
    b, bst, _, _ = K.traverse(d, rec)
    same_words(got, b, "overflow_comb vs the traversal")
    assert st == bst and st["overflows"] == 4096, "both children pass at every level: every query overflows"
    assert np.all(K.words(got) == K.MISS_WORDS)
    c = K.comb40()
    rec = rtamd.pack_points(K.make_points(c), None)
    got, st = twin(c, rec, stats=True)
    b, bst, _, deep = K.traverse(c, rec)
    same_words(got, b, "comb40 vs the traversal")
    same_words(got, K.brute(c, rec), "comb40 vs the brute force")
    assert st == bst and st["overflows"] == 0 and deep.max() > 16 and np.all(got["id"] >= 0)


def bad_node_points():
    """(records, visits node 375 by yardstick (b)): 512 points of seed 11 under both radii."""
    d = scene_arrays("bad_node")
    q = K.make_points(d, 512)
    rec = np.concatenate([rtamd.pack_points(q, None), rtamd.pack_points(q, K.radius(d, "r02"))])
    b, _, visits, _ = K.traverse(d, rec, watch=375)
    return d, rec, b, visits


def test_bad_node_error_misses():
    d, rec, b, visits = bad_node_points()
    ni = d["nodes"].view(np.int32)
    assert ni[375, 8] >= 0 and not (0 <= ni[375, 9] < ni.shape[0]), "node 375 is the malformed one"
    got = twin(d, rec)
    same_words(got, b, "bad_node vs the traversal")
    assert visits.sum() >= 10 and (~visits).sum() >= 10
    assert np.all(K.words(got)[visits] == K.MISS_WORDS), "a query that stands on the malformed node is an error miss"
    assert np.any(got["id"][~visits] >= 0)


def test_a_tree_with_a_wrong_box_pins_the_visit_order():
    d = K.wrong_box()
    ni = scene_arrays("rand2k")["nodes"].view(np.int32)
    assert ni[K.WRONG_BOX_NODE, 8] >= 0, "an inner node"
    rec = K.records("rand2k", "inf")
    got, st = twin(d, rec, stats=True)
    b, bst, _, _ = K.traverse(d, rec)
    same_words(got, b, "wrong box vs the traversal")
    assert st == bst
    a = K.yardstick("rand2k", "inf")[0]
    differ = int(np.any(K.words(got) != a, axis=1).sum())
    print(f"wrong box at node {K.WRONG_BOX_NODE}: {differ} records differ from the brute force")
    assert differ >= 1


def test_refusals_that_need_no_gpu():
    L = rtamd.lib()
    d = scene_arrays("cornell12")
    v = np.ascontiguousarray(d["vertices"], F32)
    idx = np.ascontiguousarray(d["indices"], np.int32)
    nodes = np.ascontiguousarray(d["nodes"], F32)
    refs = np.ascontiguousarray(d["tri_indices"], np.int32)
    rec = rtamd.pack_points(np.zeros((2, 3), F32))
    out = np.full(2 * 8, 0x5A5A5A5A, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(v_=vp(v), nv=v.shape[0], idx_=vp(idx), nidx=idx.size, nodes_=vp(nodes), nn=nodes.shape[0], refs_=vp(refs),
             nref=refs.size, pts=vp(rec), n=2, out_=vp(out)):
        return L.rt_closest_points_host(v_, nv, idx_, nidx, nodes_, nn, refs_, nref, pts, n, out_, None)
    assert L.rt_closest_points(None, vp(rec), 2, 0, vp(out)) == INVALID
    assert L.rt_closest_points_device(None, vp(rec), 2, 0, vp(out), None) == INVALID
    for n in (-1, (1 << 30) + 1, 1 << 62):
        assert call(n=n) == INVALID
    for kw in ({"v_": None}, {"idx_": None}, {"nodes_": None}, {"refs_": None}, {"pts": None}, {"out_": None}, {"nv": 0}, {"nn": 0}):
        assert call(**kw) == INVALID, kw
    assert call(nidx=idx.size - 1) == INVALID, "nidx % 3"
    bad = idx.copy()
    bad[5] = v.shape[0]
    assert call(idx_=vp(bad)) == BAD_SCENE, "an index out of range"
    assert np.all(out == 0x5A5A5A5A), "a refused call writes nothing"
    assert call(pts=None, n=0, out_=None) == 0, "n == 0 is RT_OK"
    assert call() == 0 and out.view(np.int32)[0] >= 0
    assert L.rt_abi_version() == 3
    assert rtamd.POINT_DTYPE.itemsize == C.sizeof(rtamd.rt_point) == 16
    assert rtamd.CLOSEST_DTYPE.itemsize == C.sizeof(rtamd.rt_closest) == 32


def test_twin_is_clean_under_asan_ubsan(tmp_path):
    """csrc/host/closest_points.cpp, the encoding it calls and tests/closest_sanitize_main.cpp, compiled
    together with every sanitizer report fatal and run as a program of their own."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "closest_sanitize_main")
    host = os.path.join(PKG, "csrc", "host")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                    "-I", host, "-o", exe, os.path.join(host, "closest_points.cpp"), os.path.join(host, "scene_encode.cpp"),
                    os.path.join(ROOT, "tests", "closest_sanitize_main.cpp"), "-lm"], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "ALL OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
