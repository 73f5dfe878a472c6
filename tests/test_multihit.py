"""First-k-hits ray queries without a GPU: rt_trace_rays_k_host, the definition in host
code (S_strict), against the yardsticks of tests/multihit_common.py -- (a) ray_tri on every triangle and
the k smallest (t, id) in (0.001f, tmax), (b) the traversal over the BVH_Node_ array with the list, both
of tests/multihit_ref.c.  Records are compared as words, plane by plane."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtamd
import closest_common as K
import multihit_common as M
from ray_query_common import N_RAYS, TMAX_DEFAULT, incoherent_rays, reference, scene_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-opencl-raytracer_amd")
F32 = np.float32
INVALID, BAD_SCENE = -1, -5
KS = (1, 2, 4, 8)


def twin(d, rays, k, stats=False):
    return rtamd.trace_rays_k_host(rtamd.Scene.from_arrays(d), rays, None, k, stats=stats)


def share(name, at_least, which="default"):
    """From (a) alone: the share of the fixture's rays with at least `at_least` hits."""
    return float(np.mean(M.found(M.brute9(name, which)) >= at_least))


def test_inputs_overflow_the_lists():
    """From (a) alone, before anything else is asserted: the lists overflow, so the last entry really
    bounds the traversal at k = 8, 4 and 2; and the finite tmax cuts lists short."""
    s9 = share("rand3k_bigleaf", 9)
    s5 = {n: share(n, 5) for n in ("rand3k_bigleaf", "rand4k_sbvh")}
    s3 = {n: share(n, 3) for n in ("hf40k", "knot16k")}
    print(f"9 or more hits: rand3k_bigleaf {s9:.3f}; 5 or more: {s5}; 3 or more: {s3}")
    assert s9 >= 0.08
    assert all(v >= 0.30 for v in s5.values())
    assert all(v >= 0.15 for v in s3.values())
    for name in M.FIXTURES:
        full, cut = M.found(M.brute9(name, "default")), M.found(M.brute9(name, "cut"))
        assert np.all(cut <= full)
        assert np.mean(cut < full) >= 0.10, f"{name}: the finite tmax cuts {np.mean(cut < full):.3f} of the rows short"


@pytest.mark.parametrize("name", M.FIXTURES)
def test_twin_equals_the_traversal_and_the_brute_force(name):
    """Every word of every plane and the three counters against (b); every word against (a): the k
    records are the mesh's, whatever the tree.  No ray is set aside: (a) and (b) agree on every ray of
    these fixtures (the slab test excludes no triangle that ray_tri accepts), which is asserted."""
    d = scene_arrays(name)
    for which in M.TMAXES:
        a9 = M.brute9(name, which)
        for k in KS:
            b, st, _ = M.traversal(name, which, k)
            differ = np.flatnonzero(np.any(b != a9[:k], axis=(0, 2)))
            assert differ.size == 0, f"{name} {which} k={k}: (a) and (b) differ on rays {differ[:8].tolist()}"
            got, gst = twin(d, M.rays(name, which), k, stats=True)
            assert got.shape == (k, N_RAYS) and got.dtype == rtamd.HIT_UV_DTYPE
            M.same_planes(got, b, f"{name} {which} k={k} vs the traversal")
            assert gst == st, f"{name} {which} k={k}: counters {gst} vs {st}"
            M.same_planes(got, a9[:k], f"{name} {which} k={k} vs the brute force")
            assert st["overflows"] == 0
        print(f"{name} {which}: found of 8 per row, mean {M.found(a9[:8]).mean():.2f}; k=8 inner visits "
              f"{st['inner_visits'] / N_RAYS:.1f}, triangle tests {st['tri_tests'] / N_RAYS:.1f} per ray")


@pytest.mark.parametrize("name", M.FIXTURES)
def test_k_1_is_the_oracles_closest_hit(name):
    """k = 1's t words are the oracle's closest hit (ray_query_common.reference), the id differs only
    where two triangles tie and is then the lower; plane 0 of k = 8 equals k = 1."""
    d = scene_arrays(name)
    o, dirs, ids, t, overflow, _ = reference(name)
    assert overflow == 0
    one = twin(d, M.rays(name, "default"), 1)
    assert np.array_equal(one["t"][0].view(np.uint32), t.view(np.uint32)), name
    other = one["id"][0] != ids
    assert np.all(one["id"][0][other] < ids[other]), "where the ids differ, k = 1 has the lower"
    assert np.array_equal(M.planes(twin(d, M.rays(name, "default"), 8))[0], M.planes(one)[0])


@pytest.mark.parametrize("name", ["rand2k", "knot16k", "rand4k_sbvh", "rand3k_bigleaf"])
def test_rows_are_sorted_and_distinct(name):
    d = scene_arrays(name)
    for which in M.TMAXES:
        r = M.rays(name, which)
        M.check_rows(M.planes(twin(d, r, 8)), r, f"{name} {which}")


def test_tie_scene():
    """rand2k's mesh with every triangle a second time: every hit ties bit for bit with its twin, so
    the id rule decides every pair and, where the row ends on an odd count, the last place."""
    d = M.scene("tie")
    a9 = M.brute9("tie", "default")
    ids, t = a9[:, :, 0].view(np.int32), a9[:, :, 1]
    pairs = 0
    for j in range(0, 8, 2):
        hit = ids[j] >= 0
        assert np.all(ids[j + 1][hit] == ids[j][hit] + 6000) and np.all(t[j + 1][hit] == t[j][hit]), f"plane {j}: a hit without its twin"
        pairs += int(hit.sum())
    assert pairs >= 1000
    for k in (1, 3, 8):
        got, st = twin(d, M.rays("tie", "default"), k, stats=True)
        M.same_planes(got, a9[:k], f"tie k={k} vs the brute force")
        b, bst, _ = M.traversal("tie", "default", k)
        M.same_planes(got, b, f"tie k={k} vs the traversal")
        assert st == bst
    # the same tree with every reference swapped for its twin's, so that the higher id of a pair is met
    # first: the id rule of acceptance brings the lower one in at the last place, insertion puts it in front
    sw = M.scene("tie_swapped")
    for k in (1, 3, 8):
        got, st = twin(sw, M.rays("tie", "default"), k, stats=True)
        M.same_planes(got, a9[:k], f"tie, references swapped, k={k} vs the brute force")
        b, bst, _ = M.traverse(sw, M.rays("tie", "default"), k)
        M.same_planes(got, b, f"tie, references swapped, k={k} vs the traversal")
        assert st == bst
    odd = twin(d, M.rays("tie", "default"), 3)
    both = odd["id"][2] >= 0
    assert both.sum() >= 30 and np.all(odd["id"][2][both] < 6000), "an odd k ends on the lower id of the pair"


def test_duplicate_sets():
    """16 rays per triangle that a tree references from more than one leaf: the twin equals (a), and (b)
    restated without the presence check repeats an id in >= 25 % (rand4k_sbvh; cubes2_dae: half of the
    16 that (b)-without-presence chose of 48)."""
    for name, draws, least in (("rand4k_sbvh", None, 0.25), ("cubes2_dae", 48, 0.5)):
        d = scene_arrays(name)
        assert M.multiply_referenced(d).size >= 30
        r, a = M.duplicate_set(name, draws=draws)
        assert r.shape[0] == 16 * M.multiply_referenced(d).size
        got, st = twin(d, r, 8, stats=True)
        M.same_planes(got, a, f"{name} duplicate set vs the brute force")
        b, bst, deep = M.traverse(d, r, 8)
        M.same_planes(got, b, f"{name} duplicate set vs the traversal")
        assert st == bst
        rep = M.repeats(M.traverse(d, r, 8, presence=False)[0])
        print(f"{name}: {r.shape[0]} rays, without the presence check {rep.sum()} rows repeat an id; deepest stack {deep.max()}")
        assert rep.mean() >= least
        assert not np.any(M.repeats(M.planes(got)))


def test_edge_rays():
    d = scene_arrays("rand3k_bigleaf")
    r, what, ok = M.edge_rays(d)
    for k in (1, 8):
        got = twin(d, r, k)
        M.same_planes(got, M.brute(d, r, k), f"edge set k={k} vs the brute force")
        M.same_planes(got, M.traverse(d, r, k)[0], f"edge set k={k} vs the traversal")
        w = M.planes(got)
        miss = M.miss_words(r, k)
        for i, label in enumerate(what):
            if not ok[i]:
                assert np.array_equal(w[:, i], miss[:, i]), f"{label}: an invalid ray is k miss records with its tmax word"
    i_inf, i_def = what.index("tmax +inf"), what.index("default")
    assert np.array_equal(M.planes(got)[:, i_inf, [0, 2, 3]], M.planes(got)[:, i_def, [0, 2, 3]])
    # tmax equal to a hit's exact t excludes that hit and keeps the nearer ones
    base = M.brute9("rand3k_bigleaf", "default")
    rows = np.flatnonzero(M.found(base) >= 4)[:64]
    o, dirs, _ = incoherent_rays(d)
    for j in (1, 3):
        tj = base[j, rows, 1].view(F32)
        strict = base[j - 1, rows, 1].view(F32) < tj
        rr = rtamd.pack_rays(o[rows], dirs[rows], tj)
        got = M.planes(twin(d, rr, 8))
        assert np.array_equal(got[:j][:, strict], base[:j, rows][:, strict]), "the nearer hits stay"
        assert np.all(got[j:, strict, 0] == M.MISS_ID) and np.all(got[j:, strict, 1] == tj.view(np.uint32)[strict]), "tmax is exclusive"
        assert strict.sum() >= 32


def test_special_scenes():
    s = scene_arrays("single_tri_rootleaf")
    o, dirs, _ = incoherent_rays(s, n=256)
    tri = s["vertices"][s["indices"][:3], :3].astype(F32)
    dirs[::2] = (tri.mean(0) - o[::2]).astype(F32)   # every second ray at the triangle
    r = rtamd.pack_rays(o, dirs, None)
    got, st = twin(s, r, 8, stats=True)
    M.same_planes(got, M.brute(s, r, 8), "single_tri_rootleaf")
    assert st == {"overflows": 0, "inner_visits": 0, "tri_tests": 256}
    assert np.sum(got["id"][0] == 0) >= 100 and np.all(got["id"][1:] == -1), "one found at the most"
    # both combs
    d = scene_arrays("overflow_comb")
    o, dirs, _ = incoherent_rays(d, n=512)
    r = rtamd.pack_rays(o, dirs, None)
    for k in (1, 8):
        got, st = twin(d, r, k, stats=True)
        b, bst, _ = M.traverse(d, r, k)
        M.same_planes(got, b, f"overflow_comb k={k} vs the traversal")
        assert st == bst and st["overflows"] == 512, "every ray overflows, counted once whatever k"
        assert np.array_equal(M.planes(got), M.miss_words(r, k))
    c = K.comb40()
    o, dirs, _ = incoherent_rays(c, n=512)
    r = rtamd.pack_rays(o, dirs, None)
    got, st = twin(c, r, 8, stats=True)
    b, bst, deep = M.traverse(c, r, 8)
    M.same_planes(got, b, "comb40 vs the traversal")
    M.same_planes(got, M.brute(c, r, 8), "comb40 vs the brute force")
    assert st == bst and st["overflows"] == 0 and deep.max() > 16 and np.any(got["id"] >= 0)


def test_bad_node_error_misses():
    from ray_edge_common import aimed_at_malformed
    d = scene_arrays("bad_node")
    o, dirs, _ = aimed_at_malformed(d, n=512)
    r = rtamd.pack_rays(o, dirs, None)
    got = twin(d, r, 8)
    b, _, _ = M.traverse(d, r, 8)
    M.same_planes(got, b, "bad_node vs the traversal")
    w = M.planes(got)
    whole_miss = np.all(w[:, :, 0] == M.MISS_ID, axis=0)
    differs = np.any(w != M.brute(d, r, 8), axis=(0, 2))
    assert differs.sum() >= 10 and np.all(whole_miss[differs]), "an error miss is 8 miss records"
    assert np.any(~whole_miss)


def test_big_leaves():
    """rand3k_bigleaf's leaves of up to 7 references at an odd k, and the hand-made tree whose leaf of 40
    goes through the escape table."""
    d = scene_arrays("rand3k_bigleaf")
    cnt = np.asarray(d["nodes"]).view(np.int32).reshape(-1, 12)
    assert np.any((cnt[:, 8] < 0) & (cnt[:, 11] >= 7))
    M.same_planes(twin(d, M.rays("rand3k_bigleaf", "default"), 5), M.brute9("rand3k_bigleaf", "default")[:5], "k = 5")
    e = K.escape_tree()
    o, dirs, _ = incoherent_rays(e, n=512)
    tri = e["vertices"][np.asarray(e["indices"]).reshape(-1, 3), :3].astype(F32)   # its 42 triangles
    dirs = (tri.mean(1)[np.arange(512) % 42] - o).astype(F32)                       # each ray at one's centroid
    r = rtamd.pack_rays(o, dirs, None)
    got, st = twin(e, r, 8, stats=True)
    M.same_planes(got, M.brute(e, r, 8), "escape tree vs the brute force")
    b, bst, _ = M.traverse(e, r, 8)
    M.same_planes(got, b, "escape tree vs the traversal")
    assert st == bst and np.sum(got["id"][0] >= 0) >= 256


def test_refusals_that_need_no_gpu():
    L = rtamd.lib()
    d = scene_arrays("cornell12")
    v = np.ascontiguousarray(d["vertices"], F32)
    idx = np.ascontiguousarray(d["indices"], np.int32)
    nodes = np.ascontiguousarray(d["nodes"], F32)
    refs = np.ascontiguousarray(d["tri_indices"], np.int32)
    rec = M.rays("cornell12", "default")[:2].copy()
    out = np.full(2 * 8 * 4, 0x5A5A5A5A, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(n=2, k=8, rays=vp(rec), out_=vp(out), v_=vp(v), nidx=idx.size):
        return L.rt_trace_rays_k_host(v_, v.shape[0], vp(idx), nidx, vp(nodes), nodes.shape[0], vp(refs), refs.size, rays, n, k,
                                      out_, None)
    assert L.rt_trace_rays_k(None, vp(rec), 2, 8, 0, vp(out)) == INVALID
    assert L.rt_trace_rays_k_device(None, vp(rec), 2, 8, 0, vp(out), None) == INVALID
    for k in (0, 9, -1, 1 << 30):
        assert call(k=k) == INVALID, k
        assert call(k=k, n=0) == INVALID, k
    for n in (-1, (1 << 30) + 1, 1 << 62):
        assert call(n=n, k=1) == INVALID, n
    for n, k in (((1 << 27) + 1, 8), ((1 << 29) + 1, 2), ((1 << 30), 2)):
        assert call(n=n, k=k) == INVALID, "n * k over 2^30"
    for kw in ({"rays": None}, {"out_": None}, {"v_": None}, {"nidx": idx.size - 1}):
        assert call(**kw) == INVALID, kw
    assert np.all(out == 0x5A5A5A5A), "a refused call writes nothing"
    assert call(rays=None, n=0, out_=None) == 0, "n == 0 is RT_OK"
    assert call() == 0 and not np.any(out == 0x5A5A5A5A)
    assert L.rt_abi_version() == 3
    assert C.sizeof(rtamd.rt_hit_uv) == 16 == rtamd.HIT_UV_DTYPE.itemsize
    with pytest.raises(rtamd.RtError):
        twin(d, rec, 9)


def test_twin_is_clean_under_asan_ubsan(tmp_path):
    """csrc/host/multihit.cpp, the encoding it calls and tests/multihit_sanitize_main.cpp, compiled
    together with every sanitizer report fatal and run as a program of their own."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "multihit_sanitize_main")
    host = os.path.join(PKG, "csrc", "host")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                    "-I", host, "-o", exe, os.path.join(host, "multihit.cpp"), os.path.join(host, "scene_encode.cpp"),
                    os.path.join(ROOT, "tests", "multihit_sanitize_main.cpp"), "-lm"], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "ALL OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
