"""Closest-point queries on the GPU.  Everything is exact: records are compared as words
against rt_closest_points_host (the twin, which runs the kernel's own text over the records the device
holds) and against yardstick (a), the plain-C brute force over all triangles of tests/closest_ref.c."""
import ctypes as C
import os

import numpy as np
import pytest

import rtamd
import closest_common as K
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


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def upload(r, d):
    r.upload(rtamd.Scene.from_arrays(d))
    return d


def twin(d, rec):
    return rtamd.closest_points_host(rtamd.Scene.from_arrays(d), rec)


def same_words(got, want, label):
    got, want = K.words(got), K.words(want)
    assert got.shape == want.shape, f"{label}: {got.shape} vs {want.shape}"
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert bad.size == 0, f"{label}: {bad.size} records differ, first {bad[:4].tolist()}: " \
                          f"{[got[i].tolist() for i in bad[:2]]} vs {[want[i].tolist() for i in bad[:2]]}"


def differing(got, want):
    return int(np.any(K.words(got) != K.words(want), axis=1).sum())


# ---- the fixtures ----

@pytest.mark.parametrize("name", K.FIXTURES)
def test_fixture_equals_the_twin_and_the_brute_force(renderer, name):
    d = upload(renderer, scene_arrays(name))
    for which in K.RADII:
        rec = K.records(name, which)
        a = K.yardstick(name, which)[0]
        got = renderer.closest_points(rec)
        same_words(got, twin(d, rec), f"{name} {which} vs the twin")
        same_words(got, a, f"{name} {which} vs the brute force")
        assert np.any(got["id"] >= 0) and (which == "inf" or np.any(got["id"] < 0))
    assert renderer.last_query_ms() > 0.0 and renderer.last_deferred() == 0


# ---- sizes and forms ----

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_sizes_host_and_device_form(renderer, n):
    import torch
    d = upload(renderer, scene_arrays("rand2k"))
    rec = K.records("rand2k", "r02")[:n]
    want = K.yardstick("rand2k", "r02")[0][:n]
    same_words(renderer.closest_points(rec), want, f"host form n={n}")
    # the device form on a side stream: a guard record after pts[n], four guard records after out[n]
    h_pts = np.concatenate([K.words(rec).reshape(-1), np.full(4, GUARD, np.uint32)])
    side = torch.cuda.Stream()
    d_pts = torch.from_numpy(h_pts.view(np.int32).copy()).cuda()
    d_out = torch.full(((n + 4) * 8,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        renderer.closest_points_device(d_pts.data_ptr(), n, d_out.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.all(out[8 * n:] == GUARD), "the kernel wrote past out[n]"
    assert np.array_equal(d_pts.cpu().numpy().view(np.uint32), h_pts), "the points were modified"
    same_words(out[:8 * n].reshape(n, 8), want, f"device form n={n}")
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
        got = capped.closest_points(rec)                # the knob is read at this context's first point query
        same_words(got, renderer.closest_points(rec), "capped vs uncapped")
        same_words(got, K.yardstick("rand2k", "inf")[0][:1500], "capped vs the brute force")
    finally:
        capped.close()
        if old is None:
            del os.environ["RTAMD_CLOSEST_GRID_BLOCKS"]
        else:
            os.environ["RTAMD_CLOSEST_GRID_BLOCKS"] = old


def test_invalid_points_at_lanes_0_31_63(renderer):
    upload(renderer, scene_arrays("rand2k"))
    n = 192
    rec = K.records("rand2k", "inf")[:n]
    whole = K.words(renderer.closest_points(rec))
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
            got = K.words(renderer.closest_points(bad))
            keep = np.setdiff1d(np.arange(n), at)
            assert np.all(got[at] == K.MISS_WORDS), f"{what} at lane {lane}: an invalid point is a miss"
            assert np.array_equal(got[keep], whole[keep]), f"{what} at lane {lane}: the neighbours"
    assert np.all(whole[:, 0] != 0xFFFFFFFF)


def test_point_order_does_not_matter(renderer):
    upload(renderer, scene_arrays("knot16k"))
    rec = K.records("knot16k", "r02")
    want = K.yardstick("knot16k", "r02")[0]
    orders = {"morton": K.morton_order(K.points("knot16k")), "permuted": np.random.default_rng(5).permutation(rec.shape[0])}
    same_words(renderer.closest_points(rec), want, "as generated")
    for label, perm in orders.items():
        got = renderer.closest_points(np.ascontiguousarray(rec[perm]))
        same_words(got, want[perm], label)


# ---- split records, malformed nodes, escape leaves, root leaves, wrong boxes ----

def test_split_records(renderer):
    """A context uploaded under RTAMD_RECORD_LIMIT=64, the split asserted as tests/test_ray_query_edges_gpu.py
    asserts it: the records reach the limit, and the context refuses rt_fetch_counts."""
    r = rtamd.Renderer(0)
    try:
        for name in ("rand2k", "cubes2_obj"):
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
                same_words(r.closest_points(K.records(name, which)), K.yardstick(name, which)[0], f"split {name} {which}")
    finally:
        r.close()


def test_bad_node_error_misses(renderer):
    from test_closest import bad_node_points
    d, rec, b, visits = bad_node_points()
    upload(renderer, d)
    assert scene_image(renderer)[HDR_CLEAN] == 0
    before = renderer.overflow_count()
    got = renderer.closest_points(rec)
    same_words(got, twin(d, rec), "bad_node vs the twin")
    same_words(got, b, "bad_node vs the traversal")
    assert visits.sum() >= 10 and np.all(K.words(got)[visits] == K.MISS_WORDS)
    assert renderer.overflow_count() == before, "an error miss is no overflow"
    upload(renderer, load_golden("cornell12"))
    assert scene_image(renderer)[HDR_CLEAN] == 1


def test_escape_leaves(renderer):
    d = upload(renderer, K.escape_tree())
    rec = rtamd.pack_points(K.make_points(d, 512), None)
    got = renderer.closest_points(rec)
    same_words(got, twin(d, rec), "escape tree vs the twin")
    same_words(got, K.brute(d, rec), "escape tree vs the brute force")
    assert np.any(got["id"] < 120) and np.any(got["id"] >= 120), "both leaves answer"


def test_single_triangle_root_leaf(renderer):
    d = upload(renderer, scene_arrays("single_tri_rootleaf"))
    rec = rtamd.pack_points(K.make_points(d, 300), None)
    got = renderer.closest_points(rec)
    same_words(got, K.brute(d, rec), "single_tri_rootleaf")
    assert np.all(got["id"] == 0)


def test_wrong_box_tree_follows_the_twin_not_the_mesh(renderer):
    d = upload(renderer, K.wrong_box())
    rec = K.records("rand2k", "inf")
    got = renderer.closest_points(rec)
    same_words(got, twin(d, rec), "wrong box vs the twin")
    same_words(got, K.traverse(d, rec)[0], "wrong box vs the traversal")
    assert differing(got, K.yardstick("rand2k", "inf")[0]) >= 1


def test_combs(renderer):
    d = upload(renderer, scene_arrays("overflow_comb"))
    n = 1000
    rec = rtamd.pack_points(K.make_points(d, n), None)
    before = renderer.overflow_count()
    got = renderer.closest_points(rec)
    assert np.all(K.words(got) == K.MISS_WORDS)
    assert renderer.overflow_count() - before == n, "every query overflows, each counted once"
    assert renderer.last_deferred() == 0
    c = upload(renderer, K.comb40())
    rec = rtamd.pack_points(K.make_points(c), None)
    before = renderer.overflow_count()
    got = renderer.closest_points(rec)
    _, st, _, deep = K.traverse(c, rec)
    assert st["overflows"] == 0 and deep.max() > 16, "the stack outgrows its LDS part"
    same_words(got, K.brute(c, rec), "comb40 vs the brute force")
    same_words(got, twin(c, rec), "comb40 vs the twin")
    assert renderer.overflow_count() == before


# ---- scenes made or moved on the GPU ----

def test_built_scene(renderer):
    d = scene_arrays("rand2k")
    renderer.build_scene({key: d[key] for key in MESH_KEYS}, max_leaf=2, keys="extent")
    built = scene_arrays("rand2k_built")   # the host twin's tree of the same build
    for which in K.RADII:
        rec = K.records("rand2k", which)
        got = renderer.closest_points(rec)
        same_words(got, twin(built, rec), f"built {which} vs the twin over the LBVH")
        same_words(got, K.yardstick("rand2k", which)[0], f"built {which} vs the brute force")


def test_after_update_vertices(renderer):
    from refit_common import moved_vertices, with_vertices
    d = upload(renderer, scene_arrays("hf40k"))
    rec = K.records("hf40k", "r02")
    same_words(renderer.closest_points(rec), K.yardstick("hf40k", "r02")[0], "before the update")
    verts = moved_vertices("hf40k")
    renderer.update_vertices(verts)
    nodes = rtamd.refit_nodes(rtamd.Scene.from_arrays(d), verts)
    moved = with_vertices(d, verts, nodes)
    got = renderer.closest_points(rec)
    same_words(got, K.brute(moved, rec), "after the update vs the brute force on the new vertices")
    same_words(got, twin(moved, rec), "after the update vs the twin on rt_refit_nodes' arrays")
    assert differing(got, K.yardstick("hf40k", "r02")[0]) > 100


def test_scene_replacement_waits_for_a_point_query(renderer):
    import torch
    d = upload(renderer, scene_arrays("rand2k"))
    rec = K.records("rand2k", "inf")
    want = K.yardstick("rand2k", "inf")[0]
    reps, n = 64, rec.shape[0]
    side = torch.cuda.Stream()
    d_pts = torch.from_numpy(np.tile(K.words(rec).reshape(-1), reps).view(np.int32).copy()).cuda()
    d_out = torch.full((reps * n * 8,), GUARD, dtype=torch.int32, device="cuda")
    b = load_golden("cornell12")
    torch.cuda.synchronize()
    # a point query of scene A, then at once, without synchronising, build_scene of scene B: the records are A's
    renderer.closest_points_device(d_pts.data_ptr(), reps * n, d_out.data_ptr(), stream=side.cuda_stream)
    renderer.build_scene({key: b[key] for key in MESH_KEYS}, max_leaf=2)
    side.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(reps, n, 8)
    assert np.all(got == want[None]), "a point query in flight saw the scene that replaced its own"
    torch.cuda.synchronize()


def test_after_scene_copy_and_scene_image_load(renderer):
    import torch
    upload(renderer, scene_arrays("rand4k_sbvh"))
    rec = K.records("rand4k_sbvh", "r02")
    want = K.yardstick("rand4k_sbvh", "r02")[0]
    n = renderer.scene_image_size()
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    renderer.pack_scene(buf.data_ptr(), n)
    c = rtamd.Renderer(0)
    try:
        c.load_scene(buf.data_ptr(), n)
        same_words(c.closest_points(rec), want, "after scene_image_load")
        upload(c, load_golden("cornell12"))
        c.copy_scene_from(renderer)
        same_words(c.closest_points(rec), want, "after scene_copy")
    finally:
        c.close()


# ---- the edge set ----

def test_edge_set(renderer):
    d = upload(renderer, scene_arrays("rand2k"))
    rec, what = K.edge_points(d)
    got = renderer.closest_points(rec)
    same_words(got, twin(d, rec), "edge set vs the twin")
    same_words(got, K.brute(d, rec), "edge set vs the brute force")
    for i, label in enumerate(what):
        if label in ("r 1e30", "r +inf"):
            assert got["id"][i] >= 0, label
        else:
            assert np.array_equal(K.words(got)[i], K.MISS_WORDS), label
    big = rtamd.pack_points(np.array([[2.0 ** 60] * 3, [-2.0 ** 60, 0, 0], [2.0 ** 64] * 3, [0, -2.0 ** 64, 0]], F32), None)
    got = renderer.closest_points(big)
    same_words(got, twin(d, big), "2^60 and 2^64 vs the twin")
    assert np.all(K.words(got)[2:] == K.MISS_WORDS), "d2 overflows to +inf: a miss even with r = +inf"
    # r equal to the exact distance (a miss) and the float above it; degenerate triangles beside a proper one
    tris = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[9, 9, 9], [9, 9, 9], [9, 9, 9]], [[20, 0, 0], [21, 0, 0], [23, 0, 0]]], F32)
    s = upload(renderer, K.two_tri_scene(tris))
    q = np.array([[1, 1, 3], [1, 1, 3], [9, 9, 8], [22, 1, 0], [9.5, 9, 9], [100, 100, 100]], F32)
    r = np.array([3.0, np.nextafter(F32(3.0), F32(4.0)), np.inf, np.inf, np.inf, np.inf], F32)
    rec = rtamd.pack_points(q, r)
    got = renderer.closest_points(rec)
    same_words(got, twin(s, rec), "degenerate triangles vs the twin")
    same_words(got, K.brute(s, rec), "degenerate triangles vs the brute force")
    assert np.array_equal(K.words(got)[0], K.MISS_WORDS) and got["id"].tolist()[1:4] == [0, 3, 6]


# ---- refusals ----

def test_refusals_leave_the_context_usable(renderer):
    import torch
    L = rtamd.lib()
    rec = rtamd.pack_points(np.zeros((4, 3), F32))
    out = np.full(4 * 8, GUARD, np.uint32)
    pp, po = vp(rec), vp(out)
    fresh = rtamd.Renderer(0)
    try:
        assert L.rt_closest_points(fresh._h, pp, 4, 0, po) == RT_ERR_NO_SCENE
        assert L.rt_closest_points_device(fresh._h, pp, 4, 0, po, None) == RT_ERR_NO_SCENE
    finally:
        fresh.close()
    d = upload(renderer, load_golden("cornell12"))
    h = renderer._h
    d_pts = torch.zeros(4 * 16 + 16, dtype=torch.uint8, device="cuda")
    d_out = torch.full((4 * 8 + 8,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dp, do = d_pts.data_ptr(), d_out.data_ptr()
    assert dp % 16 == 0 and do % 16 == 0
    c = C.c_void_p
    for bit in range(32):
        assert L.rt_closest_points(h, pp, 4, 1 << bit, po) == RT_ERR_INVALID_ARG, bit
        assert L.rt_closest_points_device(h, c(dp), 4, 1 << bit, c(do), None) == RT_ERR_INVALID_ARG, bit
    for n in (-1, (1 << 30) + 1, 1 << 40):
        assert L.rt_closest_points(h, pp, n, 0, po) == RT_ERR_INVALID_ARG, n
        assert L.rt_closest_points_device(h, c(dp), n, 0, c(do), None) == RT_ERR_INVALID_ARG, n
    assert L.rt_closest_points(h, None, 4, 0, po) == RT_ERR_INVALID_ARG
    assert L.rt_closest_points(h, pp, 4, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_closest_points_device(h, None, 4, 0, c(do), None) == RT_ERR_INVALID_ARG
    assert L.rt_closest_points_device(h, c(dp), 4, 0, None, None) == RT_ERR_INVALID_ARG
    for off in (4, 8):
        assert L.rt_closest_points_device(h, c(dp + off), 4, 0, c(do), None) == RT_ERR_INVALID_ARG
        assert L.rt_closest_points_device(h, c(dp), 4, 0, c(do + off), None) == RT_ERR_INVALID_ARG
    assert L.rt_closest_points(h, None, 0, 0, None) == 0          # n == 0: RT_OK, nothing launched
    assert L.rt_closest_points_device(h, None, 0, 0, None, None) == 0
    torch.cuda.synchronize()
    assert np.all(out == GUARD) and np.all(d_out.cpu().numpy().view(np.uint32) == GUARD), "a refused call wrote records"
    renderer.set_params(d["params"])
    frame = renderer.render(int(d["w"]), int(d["h"]), depth=int(d["depth"]), flags=0)
    assert np.array_equal(frame, d["ref_default"])
    assert renderer.closest_points(rec)["id"][0] >= 0 and renderer.last_query_ms() > 0.0 and renderer.last_deferred() == 0
