"""k-nearest-triangle queries without a GPU: rt_nearest_k_host, the definition in host
code, against the yardsticks of tests/nearest_common.py -- (a) f on every triangle and the k smallest
(d2, id), (b) the traversal over the BVH_Node_ array with the list, both of tests/nearest_ref.c.
Records are compared as words, plane by plane."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtamd
import closest_common as K
import nearest_common as NK
from ray_query_common import scene_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-opencl-raytracer_amd")
F32 = np.float32
INVALID, BAD_SCENE = -1, -5
KS = (1, 2, 3, 8)


def twin(d, rec, k, stats=False):
    return rtamd.nearest_k_host(rtamd.Scene.from_arrays(d), rec, k, stats=stats)


def same_planes(got, want, label):
    got, want = NK.planes(got), NK.planes(want)
    assert got.shape == want.shape, f"{label}: {got.shape} vs {want.shape}"
    bad = np.argwhere(np.any(got != want, axis=2))
    assert bad.shape[0] == 0, f"{label}: {bad.shape[0]} records differ, first (plane, point) {bad[:4].tolist()}: " \
                              f"{[got[j, i].tolist() for j, i in bad[:2]]} vs {[want[j, i].tolist() for j, i in bad[:2]]}"


def found(w):
    """int (n,): the records of each row of words (k, n, 8) that are no miss."""
    return (w[:, :, 0] != 0xFFFFFFFF).sum(axis=0)


@pytest.mark.parametrize("name", K.FIXTURES)
def test_twin_equals_the_traversal_and_the_brute_force(name):
    """Every word of every plane and the three counters against (b); every word against (a): the k
    records are the mesh's, whatever the tree.  No point is set aside."""
    d = scene_arrays(name)
    for which in K.RADII:
        a9 = NK.brute9(name, which)
        for k in KS:
            b, st, _ = NK.traversal(name, which, k)
            got, gst = twin(d, K.records(name, which), k, stats=True)
            assert got.shape == (k, K.N_POINTS) and got.dtype == rtamd.CLOSEST_DTYPE
            same_planes(got, b, f"{name} {which} k={k} vs the traversal")
            assert gst == st, f"{name} {which} k={k}: counters {gst} vs {st}"
            same_planes(got, a9[:k], f"{name} {which} k={k} vs the brute force")
            assert st["overflows"] == 0
        print(f"{name} {which}: found of 8 per row, mean {found(a9[:8]).mean():.2f}; k=8 inner visits "
              f"{st['inner_visits'] / K.N_POINTS:.1f}, triangle tests {st['tri_tests'] / K.N_POINTS:.1f} per point")


@pytest.mark.parametrize("name", K.FIXTURES)
def test_k_1_is_closest_points(name):
    d = scene_arrays(name)
    for which in K.RADII:
        rec = K.records(name, which)
        got = twin(d, rec, 1)
        one = rtamd.closest_points_host(rtamd.Scene.from_arrays(d), rec)
        assert np.array_equal(NK.planes(got)[0], K.words(one)), f"{name} {which}"
        assert np.array_equal(NK.planes(twin(d, rec, 8))[0], K.words(one)), f"{name} {which}: plane 0 of k = 8"


@pytest.mark.parametrize("name", ["rand2k", "rand4k_sbvh", "rand3k_bigleaf"])
def test_inputs_fill_rows_partly_under_the_small_radius(name):
    """From (a) alone: at r = 0.02 x diagonal and k = 8 at least 30 % of the rows hold 1 .. 7 records."""
    f = found(NK.brute9(name, "r02")[:8])
    part = np.mean((f >= 1) & (f <= 7))
    print(f"{name}: {part:.3f} of the rows partly filled, {np.mean(f == 0):.3f} empty, {np.mean(f == 8):.3f} full")
    assert part >= 0.30


@pytest.mark.parametrize("name", ["hf40k", "knot16k"])
def test_inputs_tie_at_the_last_place(name):
    """From (a) alone: in at least 5 % of the rows the 8th and the 9th smallest d2 are equal, so the id
    rule decides which triangle takes the last place of k = 8."""
    a9 = NK.brute9(name, "inf")
    tie = (a9[7, :, 1] == a9[8, :, 1]) & (a9[8, :, 0] != 0xFFFFFFFF)
    print(f"{name}: {tie.mean():.3f} of {tie.size} rows tie at the 8th place")
    assert tie.mean() >= 0.05
    assert np.all(a9[7, tie, 0].view(np.int32) < a9[8, tie, 0].view(np.int32))


@pytest.mark.parametrize("name", ["rand4k_sbvh", "cubes2_dae"])
def test_duplicate_set(name):
    """16 points on each triangle that the tree references from more than one leaf: the twin equals (a),
    and (b) restated without the presence check repeats an id in at least half of the rows."""
    d = scene_arrays(name)
    assert NK.multiply_referenced(d).size >= 30
    rec, a = NK.duplicate_set(name)
    got, st = twin(d, rec, 8, stats=True)
    same_planes(got, a, f"{name} duplicate set vs the brute force")
    b, bst, deep = NK.traverse(d, rec, 8)
    same_planes(got, b, f"{name} duplicate set vs the traversal")
    assert st == bst
    loose, _, _ = NK.traverse(d, rec, 8, presence=False)
    rep = NK.repeats(loose)
    print(f"{name}: {rec.shape[0]} points, without the presence check {rep.sum()} rows repeat an id; deepest stack {deep.max()}")
    assert rep.mean() >= 0.5
    assert not np.any(NK.repeats(NK.planes(got)))


@pytest.mark.parametrize("name", ["rand2k", "knot16k", "rand4k_sbvh"])
def test_rows_are_sorted_distinct_and_re_evaluate(name):
    """Rows ascend in (d2, id) with the misses last, no id appears twice, and u, v, p, d2 of every found
    record are f's words for that triangle (nearest_ref.c's f on the three vertices)."""
    d = scene_arrays(name)
    for which in ("r02", "inf"):
        w = NK.planes(twin(d, K.records(name, which), 8))
        ids = w[:, :, 0].view(np.int32)
        d2 = w[:, :, 1].view(F32)
        hit = ids >= 0
        assert np.all(hit[:-1] | ~hit[1:]), "a miss before a found record"
        both = hit[:-1] & hit[1:]
        asc = (d2[:-1] < d2[1:]) | ((d2[:-1] == d2[1:]) & (ids[:-1] < ids[1:]))
        assert np.all(asc | ~both), "a row is not sorted by (d2, id)"
        assert not np.any(NK.repeats(w))
        assert np.all(w[~hit] == NK.MISS_WORDS)
    q = K.points(name)
    v, idx = d["vertices"][:, :3].astype(F32), d["indices"]
    checked = 0
    for i in range(0, 512):
        for j in range(8):
            if ids[j, i] < 0:
                continue
            t = ids[j, i]
            r = NK.ref_tri(q[i], v[idx[t]], v[idx[t + 1]], v[idx[t + 2]])
            want = np.array([r[5], r[0], r[1], r[2], r[3], r[4]], F32).view(np.uint32)
            assert np.array_equal(w[j, i, 1:7], want), f"plane {j} point {i}"
            assert w[j, i, 7] == 0
            checked += 1
    assert checked > 300


def test_edge_set_at_k_8():
    d = scene_arrays("rand2k")
    rec, what = K.edge_points(d)
    got = twin(d, rec, 8)
    same_planes(got, NK.brute(d, rec, 8), "edge set vs the brute force")
    same_planes(got, NK.traverse(d, rec, 8)[0], "edge set vs the traversal")
    w = NK.planes(got)
    for i, label in enumerate(what):
        if label in ("r 1e30", "r +inf"):
            assert np.all(got["id"][:, i] >= 0), f"{label}: r * r = +inf bounds nothing"
        else:
            assert np.all(w[:, i] == NK.MISS_WORDS), f"{label}: a miss is 8 miss records"
    # r equal to the exact distance excludes that triangle and no other: two triangles at distances 3 and 2
    tris = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[0, 0, 5], [4, 0, 5], [0, 4, 5]]], F32)
    s = K.two_tri_scene(tris)
    q = np.array([[1, 1, 3]] * 3, F32)                       # d2 = 9 to triangle 0, 4 to triangle 1
    r = np.array([3.0, np.nextafter(F32(3.0), F32(4.0)), 2.0], F32)
    got = twin(s, rtamd.pack_points(q, r), 8)
    assert got["id"][:, 0].tolist() == [3] + [-1] * 7 and got["d2"][0, 0] == F32(4.0), "r equal to the distance excludes"
    assert got["id"][:, 1].tolist() == [3, 0] + [-1] * 6 and got["d2"][1, 1] == F32(9.0)
    assert np.all(NK.planes(got)[:, 2] == NK.MISS_WORDS), "r = 2 equals the nearer distance: nothing found"
    assert tuple(got["p"][1, 1]) == (1.0, 1.0, 0.0) and tuple(got["p"][0, 1]) == (1.0, 1.0, 5.0)
    # coordinates at 2^60 and 2^64
    big = rtamd.pack_points(np.array([[2.0 ** 60] * 3, [-2.0 ** 60, 0, 0], [2.0 ** 64] * 3, [0, -2.0 ** 64, 0]], F32), None)
    got = twin(d, big, 8)
    same_planes(got, NK.brute(d, big, 8), "2^60 and 2^64 vs the brute force")
    assert np.all(NK.planes(got)[:, 2:] == NK.MISS_WORDS)


def test_single_triangle_and_cornell():
    s = scene_arrays("single_tri_rootleaf")
    rec = rtamd.pack_points(K.make_points(s, 256), None)
    got, st = twin(s, rec, 8, stats=True)
    same_planes(got, NK.brute(s, rec, 8), "single_tri_rootleaf")
    assert st == {"overflows": 0, "inner_visits": 0, "tri_tests": 256}
    assert np.all(got["id"][0] == 0) and np.all(NK.planes(got)[1:] == NK.MISS_WORDS), "one found, seven misses"
    c = scene_arrays("cornell12")
    got = twin(c, K.records("cornell12", "inf"), 8)
    assert np.all(got["id"] >= 0), "8 of its 12"
    for i in range(0, K.N_POINTS, 64):
        assert np.unique(got["id"][:, i]).size == 8


def test_overflow_comb_and_the_comb_cut_to_40_levels():
    d = scene_arrays("overflow_comb")
    n = 1024
    rec = rtamd.pack_points(K.make_points(d, n), None)
    for k in (1, 8):
        got, st = twin(d, rec, k, stats=True)
        b, bst, _ = NK.traverse(d, rec, k)
        same_planes(got, b, f"overflow_comb k={k} vs the traversal")
        assert st == bst and st["overflows"] == n, "every query overflows, counted once whatever k"
        assert np.all(NK.planes(got) == NK.MISS_WORDS)
    c = K.comb40()
    rec = rtamd.pack_points(K.make_points(c), None)
    got, st = twin(c, rec, 8, stats=True)
    b, bst, deep = NK.traverse(c, rec, 8)
    same_planes(got, b, "comb40 vs the traversal")
    same_planes(got, NK.brute(c, rec, 8), "comb40 vs the brute force")
    assert st == bst and st["overflows"] == 0 and deep.max() > 16 and np.all(got["id"] >= 0)


def bad_node_points():
    """(scene, records, (b) words at k = 8): 512 points of seed 11 under both radii."""
    d = scene_arrays("bad_node")
    q = K.make_points(d, 512)
    rec = np.concatenate([rtamd.pack_points(q, None), rtamd.pack_points(q, K.radius(d, "r02"))])
    b, _, _ = NK.traverse(d, rec, 8)
    return d, rec, b


def test_bad_node_error_misses():
    d, rec, b = bad_node_points()
    got = twin(d, rec, 8)
    same_planes(got, b, "bad_node vs the traversal")
    w = NK.planes(got)
    whole_miss = np.all(w[:, :, 0] == 0xFFFFFFFF, axis=0)
    # a query that stood on the malformed node with k = 1 stands on it with k = 8 too (the bound is no smaller)
    _, _, visits, _ = K.traverse(d, rec, watch=375)
    assert visits.sum() >= 10 and np.all(whole_miss[visits]), "an error miss is 8 miss records"
    assert np.any(~whole_miss)
    assert np.all(w[:, whole_miss] == NK.MISS_WORDS)


def test_a_tree_with_a_wrong_box():
    d = K.wrong_box()
    rec = K.records("rand2k", "inf")
    differ = {}
    for k in (1, 8):
        got, st = twin(d, rec, k, stats=True)
        b, bst, _ = NK.traverse(d, rec, k)
        same_planes(got, b, f"wrong box k={k} vs the traversal")
        assert st == bst
        differ[k] = int(np.any(NK.planes(got) != NK.brute9("rand2k", "inf")[:k], axis=(0, 2)).sum())
    print(f"wrong box at node {K.WRONG_BOX_NODE}: rows that differ from the brute force {differ}")
    assert differ[1] >= 1 and differ[8] >= 1


def test_refusals_that_need_no_gpu():
    L = rtamd.lib()
    d = scene_arrays("cornell12")
    v = np.ascontiguousarray(d["vertices"], F32)
    idx = np.ascontiguousarray(d["indices"], np.int32)
    nodes = np.ascontiguousarray(d["nodes"], F32)
    refs = np.ascontiguousarray(d["tri_indices"], np.int32)
    rec = rtamd.pack_points(np.zeros((2, 3), F32))
    out = np.full(2 * 8 * 8, 0x5A5A5A5A, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(n=2, k=8, pts=vp(rec), out_=vp(out), v_=vp(v), nidx=idx.size):
        return L.rt_nearest_k_host(v_, v.shape[0], vp(idx), nidx, vp(nodes), nodes.shape[0], vp(refs), refs.size, pts, n, k,
                                   out_, None)
    assert L.rt_nearest_k(None, vp(rec), 2, 8, 0, vp(out)) == INVALID
    assert L.rt_nearest_k_device(None, vp(rec), 2, 8, 0, vp(out), None) == INVALID
    for k in (0, 9, -1, 1 << 30):
        assert call(k=k) == INVALID, k
        assert call(k=k, n=0) == INVALID, k
    for n in (-1, (1 << 30) + 1, 1 << 62):
        assert call(n=n, k=1) == INVALID, n
    for n, k in (((1 << 27) + 1, 8), ((1 << 29) + 1, 2), ((1 << 30), 2)):
        assert call(n=n, k=k) == INVALID, "n * k over 2^30"
    for kw in ({"pts": None}, {"out_": None}, {"v_": None}, {"nidx": idx.size - 1}):
        assert call(**kw) == INVALID, kw
    assert np.all(out == 0x5A5A5A5A), "a refused call writes nothing"
    assert call(pts=None, n=0, out_=None) == 0, "n == 0 is RT_OK"
    assert call() == 0 and np.all(out.view(np.int32).reshape(8, 2, 8)[:, :, 0] >= 0)
    assert L.rt_abi_version() == 3
    with pytest.raises(rtamd.RtError):
        twin(d, rec, 9)


def test_twin_is_clean_under_asan_ubsan(tmp_path):
    """csrc/host/closest_points.cpp, the encoding it calls and tests/nearest_sanitize_main.cpp, compiled
    together with every sanitizer report fatal and run as a program of their own."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "nearest_sanitize_main")
    host = os.path.join(PKG, "csrc", "host")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                    "-I", host, "-o", exe, os.path.join(host, "closest_points.cpp"), os.path.join(host, "scene_encode.cpp"),
                    os.path.join(ROOT, "tests", "nearest_sanitize_main.cpp"), "-lm"], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "ALL OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
