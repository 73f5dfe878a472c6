"""k-nearest-triangle queries on the GPU.  Everything is exact: records are compared as
words, plane by plane, against rt_nearest_k_host (the twin, which runs the kernel's own text over the
records the device holds) and against yardstick (a), the plain-C brute force of tests/nearest_ref.c."""
import ctypes as C
import os

import numpy as np
import pytest

import rtamd
import closest_common as K
import nearest_common as NK
from conftest import load_golden
from ray_query_common import scene_arrays
from refit_common import scene_image

pytestmark = pytest.mark.gpu

F32 = np.float32
MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")
RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE = -1, -3
GUARD = 0x5A5A5A5A
HDR_CLEAN = 13
RECORD_LIMIT = 64
KS = (1, 3, 8)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def upload(r, d):
    r.upload(rtamd.Scene.from_arrays(d))
    return d


def twin(d, rec, k):
    return rtamd.nearest_k_host(rtamd.Scene.from_arrays(d), rec, k)


def same_planes(got, want, label):
    got, want = NK.planes(got), NK.planes(want)
    assert got.shape == want.shape, f"{label}: {got.shape} vs {want.shape}"
    bad = np.argwhere(np.any(got != want, axis=2))
    assert bad.shape[0] == 0, f"{label}: {bad.shape[0]} records differ, first (plane, point) {bad[:4].tolist()}: " \
                              f"{[got[j, i].tolist() for j, i in bad[:2]]} vs {[want[j, i].tolist() for j, i in bad[:2]]}"


def differing(got, want):
    return int(np.any(NK.planes(got) != NK.planes(want), axis=(0, 2)).sum())


# ---- the fixtures ----

@pytest.mark.parametrize("name", K.FIXTURES)
def test_fixture_equals_the_twin_and_the_brute_force(renderer, name):
    d = upload(renderer, scene_arrays(name))
    for which in K.RADII:
        rec = K.records(name, which)
        a9 = NK.brute9(name, which)
        for k in KS:
            got = renderer.nearest_k(rec, k)
            assert got.shape == (k, rec.shape[0])
            same_planes(got, twin(d, rec, k), f"{name} {which} k={k} vs the twin")
            same_planes(got, a9[:k], f"{name} {which} k={k} vs the brute force")
        assert np.any(got["id"][0] >= 0) and (which == "inf" or np.any(got["id"][7] < 0))
    assert renderer.last_query_ms() > 0.0 and renderer.last_deferred() == 0


def test_k_1_is_closest_points(renderer):
    for name in ("rand4k_sbvh", "knot16k"):
        upload(renderer, scene_arrays(name))
        for which in K.RADII:
            rec = K.records(name, which)
            one = K.words(renderer.closest_points(rec))
            assert np.array_equal(NK.planes(renderer.nearest_k(rec, 1))[0], one), f"{name} {which}"
            assert np.array_equal(NK.planes(renderer.nearest_k(rec, 8))[0], one), f"{name} {which}: plane 0 of k = 8"


def test_duplicate_set(renderer):
    d = upload(renderer, scene_arrays("rand4k_sbvh"))
    rec, a = NK.duplicate_set("rand4k_sbvh")
    for k in (2, 8):
        got = renderer.nearest_k(rec, k)
        same_planes(got, a[:k], f"duplicate set k={k} vs the brute force")
        same_planes(got, twin(d, rec, k), f"duplicate set k={k} vs the twin")
        assert not np.any(NK.repeats(NK.planes(got)))
    loose = NK.traverse(d, rec, 8, presence=False)[0]
    assert NK.repeats(loose).mean() >= 0.5, "the set bites"


# ---- sizes and forms ----

@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_sizes_host_and_device_form(renderer, n, k):
    import torch
    upload(renderer, scene_arrays("rand2k"))
    rec = K.records("rand2k", "r02")[:n]
    want = np.ascontiguousarray(NK.brute9("rand2k", "r02")[:k, :n])
    same_planes(renderer.nearest_k(rec, k), want, f"host form n={n} k={k}")
    # the device form on a side stream: a guard record after pts[n], four guard records after out[k * n]
    h_pts = np.concatenate([K.words(rec).reshape(-1), np.full(4, GUARD, np.uint32)])
    side = torch.cuda.Stream()
    d_pts = torch.from_numpy(h_pts.view(np.int32).copy()).cuda()
    d_out = torch.full(((k * n + 4) * 8,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        renderer.nearest_k_device(d_pts.data_ptr(), n, k, d_out.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.all(out[8 * k * n:] == GUARD), "the kernel wrote past out[k * n]"
    assert np.array_equal(d_pts.cpu().numpy().view(np.uint32), h_pts), "the points were modified"
    flat = out[:8 * k * n].reshape(k * n, 8)
    same_planes(flat.reshape(k, n, 8), want, f"device form n={n} k={k}")
    for j in range(1, k if n else 0):
        # record j * n - 1 is the last point's in plane j - 1, record j * n the first point's in plane j
        assert np.array_equal(flat[j * n - 1], want[j - 1, n - 1]) and np.array_equal(flat[j * n], want[j, 0]), f"plane {j}"
    if n:
        assert renderer.last_query_ms() > 0.0 and renderer.last_deferred() == 0


def test_grid_cap_several_groups_per_wave(renderer):
    d = upload(renderer, scene_arrays("rand2k"))
    rec = K.records("rand2k", "inf")[:1500]
    old = os.environ.get("RTAMD_CLOSEST_GRID_BLOCKS")
    os.environ["RTAMD_CLOSEST_GRID_BLOCKS"] = "2"   # 8 waves for 24 groups
    capped = rtamd.Renderer(0)
    try:
        upload(capped, d)
        for k in (1, 8):
            got = capped.nearest_k(rec, k)              # the knob is read at this context's first point query
            same_planes(got, renderer.nearest_k(rec, k), f"capped vs uncapped k={k}")
            same_planes(got, NK.brute9("rand2k", "inf")[:k, :1500], f"capped vs the brute force k={k}")
    finally:
        capped.close()
        if old is None:
            del os.environ["RTAMD_CLOSEST_GRID_BLOCKS"]
        else:
            os.environ["RTAMD_CLOSEST_GRID_BLOCKS"] = old


def test_invalid_points_at_lanes_0_31_63(renderer):
    upload(renderer, scene_arrays("rand2k"))
    n, k = 192, 8
    rec = K.records("rand2k", "inf")[:n]
    whole = NK.planes(renderer.nearest_k(rec, k))
    for what in ("nan coordinate", "inf coordinate", "zero radius", "nan radius"):
        for lane in (0, 31, 63):
            at = np.arange(lane, n, 64)
            bad = rec.copy()
            if what == "nan coordinate":
                bad["q"][at, 1] = np.nan
            elif what == "inf coordinate":
                bad["q"][at, 2] = -np.inf
            elif what == "zero radius":
                bad["r"][at] = 0.0
            else:
                bad["r"][at] = np.nan
            got = NK.planes(renderer.nearest_k(bad, k))
            keep = np.setdiff1d(np.arange(n), at)
            assert np.all(got[:, at] == NK.MISS_WORDS), f"{what} at lane {lane}: an invalid point is k miss records"
            assert np.array_equal(got[:, keep], whole[:, keep]), f"{what} at lane {lane}: the neighbours"
    assert np.all(whole[:, :, 0] != 0xFFFFFFFF)


def test_point_order_does_not_matter(renderer):
    upload(renderer, scene_arrays("knot16k"))
    rec = K.records("knot16k", "r02")
    want = NK.brute9("knot16k", "r02")[:8]
    orders = {"morton": K.morton_order(K.points("knot16k")), "permuted": np.random.default_rng(5).permutation(rec.shape[0])}
    same_planes(renderer.nearest_k(rec, 8), want, "as generated")
    for label, perm in orders.items():
        got = renderer.nearest_k(np.ascontiguousarray(rec[perm]), 8)
        same_planes(got, np.ascontiguousarray(want[:, perm]), label)


# ---- split records, malformed nodes, escape leaves, root leaves, wrong boxes ----

def test_split_records():
    """A context uploaded under RTAMD_RECORD_LIMIT=64, the split asserted as tests/test_closest_gpu.py
    asserts it: the records reach the limit, and the context refuses rt_fetch_counts."""
    r = rtamd.Renderer(0)
    try:
        name = "rand4k_sbvh"
        d = scene_arrays(name)
        old = os.environ.get("RTAMD_RECORD_LIMIT")
        os.environ["RTAMD_RECORD_LIMIT"] = str(RECORD_LIMIT)
        try:
            upload(r, d)
        finally:
            if old is None:
                del os.environ["RTAMD_RECORD_LIMIT"]
            else:
                os.environ["RTAMD_RECORD_LIMIT"] = old
        hdr = scene_image(r)[:6]
        assert 16 * (int(hdr[2]) + (int(hdr[3]) << 32) + int(hdr[4]) + (int(hdr[5]) << 32)) >= RECORD_LIMIT
        with pytest.raises(rtamd.RtError):
            r.fetch_counts(8, 8, 1, 0)
        for which in K.RADII:
            same_planes(r.nearest_k(K.records(name, which), 8), NK.brute9(name, which)[:8], f"split {name} {which}")
    finally:
        r.close()


def test_bad_node_error_misses(renderer):
    from test_nearest_k import bad_node_points
    d, rec, b = bad_node_points()
    upload(renderer, d)
    assert scene_image(renderer)[HDR_CLEAN] == 0
    before = renderer.overflow_count()
    got = renderer.nearest_k(rec, 8)
    same_planes(got, twin(d, rec, 8), "bad_node vs the twin")
    same_planes(got, b, "bad_node vs the traversal")
    whole_miss = np.all(NK.planes(got)[:, :, 0] == 0xFFFFFFFF, axis=0)
    assert whole_miss.sum() >= 10 and np.any(~whole_miss)
    assert renderer.overflow_count() == before, "an error miss is no overflow"
    upload(renderer, load_golden("cornell12"))
    assert scene_image(renderer)[HDR_CLEAN] == 1


def test_escape_leaves(renderer):
    d = upload(renderer, K.escape_tree())
    rec = rtamd.pack_points(K.make_points(d, 512), None)
    got = renderer.nearest_k(rec, 8)
    same_planes(got, twin(d, rec, 8), "escape tree vs the twin")
    same_planes(got, NK.brute(d, rec, 8), "escape tree vs the brute force")
    assert np.any(got["id"] < 120) and np.any(got["id"] >= 120), "both leaves answer"


def test_single_triangle_root_leaf(renderer):
    d = upload(renderer, scene_arrays("single_tri_rootleaf"))
    rec = rtamd.pack_points(K.make_points(d, 300), None)
    got = renderer.nearest_k(rec, 8)
    same_planes(got, NK.brute(d, rec, 8), "single_tri_rootleaf")
    assert np.all(got["id"][0] == 0) and np.all(NK.planes(got)[1:] == NK.MISS_WORDS)


def test_wrong_box_tree_follows_the_twin_not_the_mesh(renderer):
    d = upload(renderer, K.wrong_box())
    rec = K.records("rand2k", "inf")
    got = renderer.nearest_k(rec, 8)
    same_planes(got, twin(d, rec, 8), "wrong box vs the twin")
    same_planes(got, NK.traverse(d, rec, 8)[0], "wrong box vs the traversal")
    assert differing(got, NK.brute9("rand2k", "inf")[:8]) >= 1


def test_combs(renderer):
    d = upload(renderer, scene_arrays("overflow_comb"))
    n = 1000
    rec = rtamd.pack_points(K.make_points(d, n), None)
    for k in (1, 8):
        before = renderer.overflow_count()
        got = renderer.nearest_k(rec, k)
        assert np.all(NK.planes(got) == NK.MISS_WORDS)
        assert renderer.overflow_count() - before == n, "every query overflows, each counted once: n, not k * n"
        assert renderer.last_deferred() == 0
    c = upload(renderer, K.comb40())
    rec = rtamd.pack_points(K.make_points(c), None)
    before = renderer.overflow_count()
    got = renderer.nearest_k(rec, 8)
    _, st, deep = NK.traverse(c, rec, 8)
    assert st["overflows"] == 0 and deep.max() > 16, "the stack outgrows its LDS part"
    same_planes(got, NK.brute(c, rec, 8), "comb40 vs the brute force")
    same_planes(got, twin(c, rec, 8), "comb40 vs the twin")
    assert renderer.overflow_count() == before


# ---- scenes made or moved on the GPU ----

def test_built_scene(renderer):
    d = scene_arrays("rand2k")
    renderer.build_scene({key: d[key] for key in MESH_KEYS}, max_leaf=2, keys="extent")
    built = scene_arrays("rand2k_built")   # the host twin's tree of the same build
    for which in K.RADII:
        rec = K.records("rand2k", which)
        got = renderer.nearest_k(rec, 8)
        same_planes(got, twin(built, rec, 8), f"built {which} vs the twin over the LBVH")
        same_planes(got, NK.brute9("rand2k", which)[:8], f"built {which} vs the brute force")


def test_after_update_vertices(renderer):
    from refit_common import moved_vertices, with_vertices
    d = upload(renderer, scene_arrays("hf40k"))
    rec = K.records("hf40k", "r02")
    same_planes(renderer.nearest_k(rec, 8), NK.brute9("hf40k", "r02")[:8], "before the update")
    verts = moved_vertices("hf40k")
    renderer.update_vertices(verts)
    nodes = rtamd.refit_nodes(rtamd.Scene.from_arrays(d), verts)
    moved = with_vertices(d, verts, nodes)
    got = renderer.nearest_k(rec, 8)
    same_planes(got, NK.brute(moved, rec, 8), "after the update vs the brute force on the new vertices")
    same_planes(got, twin(moved, rec, 8), "after the update vs the twin on rt_refit_nodes' arrays")
    assert differing(got, NK.brute9("hf40k", "r02")[:8]) > 100


def test_scene_replacement_waits_for_a_query(renderer):
    import torch
    upload(renderer, scene_arrays("rand2k"))
    rec = K.records("rand2k", "inf")
    want = NK.brute9("rand2k", "inf")[:8]
    reps, n = 16, rec.shape[0]
    side = torch.cuda.Stream()
    d_pts = torch.from_numpy(np.tile(K.words(rec).reshape(-1), reps).view(np.int32).copy()).cuda()
    d_out = torch.full((8 * reps * n * 8,), GUARD, dtype=torch.int32, device="cuda")
    b = load_golden("cornell12")
    torch.cuda.synchronize()
    # a query of scene A, then at once, without synchronising, build_scene of scene B: the records are A's
    renderer.nearest_k_device(d_pts.data_ptr(), reps * n, 8, d_out.data_ptr(), stream=side.cuda_stream)
    renderer.build_scene({key: b[key] for key in MESH_KEYS}, max_leaf=2)
    side.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(8, reps, n, 8)
    assert np.all(got == want[:, None]), "a query in flight saw the scene that replaced its own"
    torch.cuda.synchronize()


def test_after_scene_copy_and_scene_image_load(renderer):
    import torch
    upload(renderer, scene_arrays("rand4k_sbvh"))
    rec = K.records("rand4k_sbvh", "r02")
    want = NK.brute9("rand4k_sbvh", "r02")[:8]
    n = renderer.scene_image_size()
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    renderer.pack_scene(buf.data_ptr(), n)
    c = rtamd.Renderer(0)
    try:
        c.load_scene(buf.data_ptr(), n)
        same_planes(c.nearest_k(rec, 8), want, "after scene_image_load")
        upload(c, load_golden("cornell12"))
        c.copy_scene_from(renderer)
        same_planes(c.nearest_k(rec, 8), want, "after scene_copy")
    finally:
        c.close()


# ---- the edge set ----

def test_edge_set(renderer):
    d = upload(renderer, scene_arrays("rand2k"))
    rec, what = K.edge_points(d)
    got = renderer.nearest_k(rec, 8)
    same_planes(got, twin(d, rec, 8), "edge set vs the twin")
    same_planes(got, NK.brute(d, rec, 8), "edge set vs the brute force")
    for i, label in enumerate(what):
        if label in ("r 1e30", "r +inf"):
            assert np.all(got["id"][:, i] >= 0), label
        else:
            assert np.all(NK.planes(got)[:, i] == NK.MISS_WORDS), label
    tris = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[0, 0, 5], [4, 0, 5], [0, 4, 5]]], F32)
    s = upload(renderer, K.two_tri_scene(tris))
    q = np.array([[1, 1, 3]] * 3, F32)                       # d2 = 9 to triangle 0, 4 to triangle 1
    r = np.array([3.0, np.nextafter(F32(3.0), F32(4.0)), 2.0], F32)
    rec = rtamd.pack_points(q, r)
    got = renderer.nearest_k(rec, 8)
    same_planes(got, twin(s, rec, 8), "exact radius vs the twin")
    assert got["id"][:, 0].tolist() == [3] + [-1] * 7, "r equal to the distance excludes that triangle"
    assert got["id"][:, 1].tolist() == [3, 0] + [-1] * 6
    assert np.all(NK.planes(got)[:, 2] == NK.MISS_WORDS)


# ---- refusals ----

def test_refusals_leave_the_context_usable(renderer):
    import torch
    L = rtamd.lib()
    rec = rtamd.pack_points(np.zeros((4, 3), F32))
    out = np.full(8 * 4 * 8, GUARD, np.uint32)
    pp, po = vp(rec), vp(out)
    fresh = rtamd.Renderer(0)
    try:
        assert L.rt_nearest_k(fresh._h, pp, 4, 8, 0, po) == RT_ERR_NO_SCENE
        assert L.rt_nearest_k_device(fresh._h, pp, 4, 8, 0, po, None) == RT_ERR_NO_SCENE
    finally:
        fresh.close()
    d = upload(renderer, load_golden("cornell12"))
    h = renderer._h
    d_pts = torch.zeros(4 * 16 + 16, dtype=torch.uint8, device="cuda")
    d_out = torch.full((8 * 4 * 8 + 8,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dp, do = d_pts.data_ptr(), d_out.data_ptr()
    assert dp % 16 == 0 and do % 16 == 0
    c = C.c_void_p
    for bit in range(32):
        assert L.rt_nearest_k(h, pp, 4, 8, 1 << bit, po) == RT_ERR_INVALID_ARG, bit
        assert L.rt_nearest_k_device(h, c(dp), 4, 8, 1 << bit, c(do), None) == RT_ERR_INVALID_ARG, bit
    for k in (0, 9, -1, 1 << 30, -(1 << 31)):
        for n in (0, 4):
            assert L.rt_nearest_k(h, pp, n, k, 0, po) == RT_ERR_INVALID_ARG, (n, k)
            assert L.rt_nearest_k_device(h, c(dp), n, k, 0, c(do), None) == RT_ERR_INVALID_ARG, (n, k)
    for n, k in ((-1, 1), ((1 << 30) + 1, 1), (1 << 40, 8), ((1 << 27) + 1, 8), ((1 << 29) + 1, 2), (1 << 30, 2)):
        assert L.rt_nearest_k(h, pp, n, k, 0, po) == RT_ERR_INVALID_ARG, (n, k)
        assert L.rt_nearest_k_device(h, c(dp), n, k, 0, c(do), None) == RT_ERR_INVALID_ARG, (n, k)
    assert L.rt_nearest_k(h, None, 4, 8, 0, po) == RT_ERR_INVALID_ARG
    assert L.rt_nearest_k(h, pp, 4, 8, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_nearest_k_device(h, None, 4, 8, 0, c(do), None) == RT_ERR_INVALID_ARG
    assert L.rt_nearest_k_device(h, c(dp), 4, 8, 0, None, None) == RT_ERR_INVALID_ARG
    for off in (4, 8):
        assert L.rt_nearest_k_device(h, c(dp + off), 4, 8, 0, c(do), None) == RT_ERR_INVALID_ARG
        assert L.rt_nearest_k_device(h, c(dp), 4, 8, 0, c(do + off), None) == RT_ERR_INVALID_ARG
    assert L.rt_nearest_k(h, None, 0, 8, 0, None) == 0          # n == 0: RT_OK, nothing launched
    assert L.rt_nearest_k_device(h, None, 0, 1, 0, None, None) == 0
    torch.cuda.synchronize()
    assert np.all(out == GUARD) and np.all(d_out.cpu().numpy().view(np.uint32) == GUARD), "a refused call wrote records"
    renderer.set_params(d["params"])
    frame = renderer.render(int(d["w"]), int(d["h"]), depth=int(d["depth"]), flags=0)
    assert np.array_equal(frame, d["ref_default"])
    got = renderer.nearest_k(rec, 8)
    assert np.all(got["id"] >= 0) and renderer.last_query_ms() > 0.0 and renderer.last_deferred() == 0
    assert L.rt_abi_version() == 3
