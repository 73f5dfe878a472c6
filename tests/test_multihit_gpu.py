"""First-k-hits ray queries on the GPU.  Everything is exact: records are compared as
words, plane by plane.  In S_strict (with and without RT_FLAG_EXACT_DIV) against rt_trace_rays_k_host
(the twin, which runs the kernels' control flow over the records the device holds) and against yardstick
(a), the plain-C brute force of tests/multihit_ref.c; in all three arithmetics against rt_trace_rays'
closest hit, which the k = 1 bound and a peel of the k = 8 rows must reproduce."""
import ctypes as C
import os

import numpy as np
import pytest

import rtamd
import closest_common as K
import multihit_common as M
from conftest import load_golden
from ray_query_common import N_RAYS, incoherent_rays, scene_arrays
from refit_common import scene_image

pytestmark = pytest.mark.gpu

F32 = np.float32
MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")
RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE = -1, -3
GUARD = 0x5A5A5A5A
HDR_CLEAN = 13
RECORD_LIMIT = 64
STRICT, HW, EXACT, ANY = rtamd.RT_FLAG_STRICT_MATH, rtamd.RT_FLAG_HW_MATH, rtamd.RT_FLAG_EXACT_DIV, rtamd.RT_FLAG_ANY_HIT
ARITHMETICS = {"strict": STRICT, "hw": HW, "ref": 0}
ALLOWED = STRICT | HW | EXACT


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def upload(r, d):
    r.upload(rtamd.Scene.from_arrays(d))
    return d


def twin(d, rays, k):
    return rtamd.trace_rays_k_host(rtamd.Scene.from_arrays(d), rays, None, k)


def gpu(r, rays, k, flags=STRICT):
    return r.trace_rays_k(rays, None, k, flags=flags)


def differing(got, want):
    return int(np.any(M.planes(got) != M.planes(want), axis=(0, 2)).sum())


# ---- S_strict: the twin and the brute force ----

@pytest.mark.parametrize("name", M.FIXTURES)
def test_fixture_equals_the_twin_and_the_brute_force(renderer, name):
    d = upload(renderer, scene_arrays(name))
    for which in M.TMAXES:
        rays = M.rays(name, which)
        a9 = M.brute9(name, which)
        for k in (1, 4, 8):
            want = twin(d, rays, k)
            M.same_planes(want, a9[:k], f"{name} {which} k={k}: the twin vs the brute force")
            for flags in (STRICT, STRICT | EXACT):
                got = gpu(renderer, rays, k, flags)
                assert got.shape == (k, N_RAYS) and got.dtype == rtamd.HIT_UV_DTYPE
                M.same_planes(got, want, f"{name} {which} k={k} flags={flags} vs the twin")
        assert np.any(got["id"][0] >= 0) and np.any(got["id"][7] < 0)
    assert renderer.last_query_ms() > 0.0 and renderer.last_deferred() == 0


# ---- every arithmetic: the closest-hit query ----

@pytest.mark.parametrize("arith", list(ARITHMETICS))
@pytest.mark.parametrize("name", ["rand3k_bigleaf", "rand4k_sbvh", "hf40k"])
def test_k_1_and_the_peel_against_trace_rays(renderer, name, arith):
    """k = 1's t words are trace_rays' closest-hit t words for every ray (the id the lower one where they
    differ); plane 0 of k = 8 is k = 1; rows are sorted with no id twice; and the peel, on the rows
    strictly increasing in t, one trace_rays call and one trace_rays_k call per plane j >= 1:
      * trace_rays of the same ray with tmax = t_j returns plane j - 1's t word at j = 1, the one plane
        where a closest-hit query can: tmax is exclusive, so the hit at t_1 is cut off and the nearest
        left is plane 0.  For j >= 2 a closest-hit query with tmax = t_j still answers the NEAREST hit,
        which is plane 0 and not plane j - 1 (there is no per-ray TMIN to peel from the near side), so
        there it must return plane 0's t word: t_j cuts nothing in front of it.
      * trace_rays_k with tmax = t_j returns planes 0 .. j - 1 word for word and misses after them: the
        entries in front of plane j are what the query finds when plane j and all behind it are cut off."""
    flags = ARITHMETICS[arith]
    d = upload(renderer, scene_arrays(name))
    o, dirs, _ = incoherent_rays(d)
    rays = M.rays(name, "default")
    ids, t = renderer.trace_rays(o, dirs, flags=flags)
    one = gpu(renderer, rays, 1, flags)
    assert np.array_equal(one["t"][0].view(np.uint32), t.view(np.uint32)), "k = 1 t words"
    other = one["id"][0] != ids
    assert np.all(one["id"][0][other] < ids[other]) and np.all(ids[other] >= 0), "where the ids differ, k = 1 has the lower"
    eight = gpu(renderer, rays, 8, flags)
    w = M.planes(eight)
    assert np.array_equal(w[0], M.planes(one)[0]), "plane 0 of k = 8 is k = 1"
    M.check_rows(w, rays, f"{name} {arith}")
    hit = eight["id"] >= 0
    rising = np.all((eight["t"][:-1] < eight["t"][1:]) | ~hit[1:], axis=0)
    assert rising.mean() >= 0.5
    checked = 0
    for j in range(1, 8):
        at = hit[j] & rising
        _, tp = renderer.trace_rays(o, dirs, tmax=eight["t"][j], flags=flags)
        assert np.array_equal(tp[at].view(np.uint32), eight["t"][0][at].view(np.uint32)), f"peel at plane {j}: the closest hit under tmax = t_{j}"
        cut = M.planes(renderer.trace_rays_k(o, dirs, 8, tmax=eight["t"][j], flags=flags))
        assert np.array_equal(cut[:j, at], w[:j, at]), f"peel at plane {j}: the planes in front of it"
        assert np.all(cut[j:, at, 0] == M.MISS_ID) and np.array_equal(cut[j:, at, 1], np.broadcast_to(w[j, at, 1], cut[j:, at, 1].shape)), \
            f"peel at plane {j}: tmax = t_{j} is exclusive"
        checked += int(at.sum())
    print(f"{name} {arith}: {checked} peeled entries on {int(rising.sum())} rising rows, ids differ at k = 1 on {int(other.sum())}")
    assert checked >= 1000


# ---- sizes and forms ----

@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_sizes_host_and_device_form(renderer, n, k):
    import torch
    upload(renderer, scene_arrays("rand3k_bigleaf"))
    rays = M.rays("rand3k_bigleaf", "default")[:n]
    want = np.ascontiguousarray(M.brute9("rand3k_bigleaf", "default")[:k, :n])
    M.same_planes(gpu(renderer, rays, k), want, f"host form n={n} k={k}")
    # the device form on a side stream: a guard record after rays[n], four guard records after out[k * n]
    h_rays = np.concatenate([M.ray_words(rays).reshape(-1), np.full(8, GUARD, np.uint32)])
    side = torch.cuda.Stream()
    d_rays = torch.from_numpy(h_rays.view(np.int32).copy()).cuda()
    d_out = torch.full(((k * n + 4) * 4,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        renderer.trace_rays_k_device(d_rays.data_ptr(), n, k, d_out.data_ptr(), flags=STRICT, stream=side.cuda_stream)
    side.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.all(out[4 * k * n:] == GUARD), "the kernel wrote past out[k * n]"
    assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), h_rays), "the rays were modified"
    flat = out[:4 * k * n].reshape(k * n, 4)
    M.same_planes(flat.reshape(k, n, 4), want, f"device form n={n} k={k}")
    for j in range(1, k if n else 0):
        # record j * n - 1 is the last ray's in plane j - 1, record j * n the first ray's in plane j
        assert np.array_equal(flat[j * n - 1], want[j - 1, n - 1]) and np.array_equal(flat[j * n], want[j, 0]), f"plane {j}"
    if n:
        assert renderer.last_query_ms() > 0.0 and renderer.last_deferred() == 0


def test_grid_cap_several_groups_per_wave(renderer):
    d = upload(renderer, scene_arrays("rand3k_bigleaf"))
    rays = M.rays("rand3k_bigleaf", "cut")[:1500]
    old = os.environ.get("RTAMD_MULTIHIT_GRID_BLOCKS")
    os.environ["RTAMD_MULTIHIT_GRID_BLOCKS"] = "2"   # 8 waves for 24 groups
    capped = rtamd.Renderer(0)
    try:
        upload(capped, d)
        for k in (1, 8):
            for flags in (STRICT, 0):
                got = gpu(capped, rays, k, flags)       # the knob is read at this context's first such query
                M.same_planes(got, gpu(renderer, rays, k, flags), f"capped vs uncapped k={k} flags={flags}")
            M.same_planes(gpu(capped, rays, k), M.brute9("rand3k_bigleaf", "cut")[:k, :1500], f"capped vs the brute force k={k}")
    finally:
        capped.close()
        if old is None:
            del os.environ["RTAMD_MULTIHIT_GRID_BLOCKS"]
        else:
            os.environ["RTAMD_MULTIHIT_GRID_BLOCKS"] = old


def test_invalid_rays_at_lanes_0_31_63(renderer):
    upload(renderer, scene_arrays("rand3k_bigleaf"))
    n, k = 192, 8
    rays = M.rays("rand3k_bigleaf", "default")[:n]
    whole = M.planes(gpu(renderer, rays, k))
    for what in ("nan origin", "inf direction", "zero direction", "zero tmax", "nan tmax"):
        for lane in (0, 31, 63):
            at = np.arange(lane, n, 64)
            bad = rays.copy()
            if what == "nan origin":
                bad["o"][at, 1] = np.nan
            elif what == "inf direction":
                bad["d"][at, 2] = -np.inf
            elif what == "zero direction":
                bad["d"][at] = 0.0
            elif what == "zero tmax":
                bad["tmax"][at] = 0.0
            else:
                bad["tmax"].view(np.uint32)[at] = 0xFFC12345
            for flags in (STRICT, 0):
                got = M.planes(gpu(renderer, bad, k, flags))
                assert np.array_equal(got[:, at], M.miss_words(bad, k)[:, at]), f"{what} at lane {lane}: k miss records with the tmax word"
            keep = np.setdiff1d(np.arange(n), at)
            got = M.planes(gpu(renderer, bad, k))
            assert np.array_equal(got[:, keep], whole[:, keep]), f"{what} at lane {lane}: the neighbours"
    assert np.mean(whole[0, :, 0] != M.MISS_ID) >= 0.5


def test_ray_order_does_not_matter(renderer):
    upload(renderer, scene_arrays("rand4k_sbvh"))
    rays = M.rays("rand4k_sbvh", "cut")
    want = M.brute9("rand4k_sbvh", "cut")[:8]
    orders = {"morton": K.morton_order(rays["o"]), "permuted": np.random.default_rng(5).permutation(rays.shape[0])}
    M.same_planes(gpu(renderer, rays, 8), want, "as generated")
    for label, perm in orders.items():
        got = gpu(renderer, np.ascontiguousarray(rays[perm]), 8)
        M.same_planes(got, np.ascontiguousarray(want[:, perm]), label)


# ---- scenes ----

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
        for which in M.TMAXES:
            M.same_planes(gpu(r, M.rays(name, which), 8), M.brute9(name, which)[:8], f"split {name} {which}")
    finally:
        r.close()


def test_tie_scene_and_duplicate_set(renderer):
    d = upload(renderer, M.scene("tie"))
    rays = M.rays("tie", "default")
    a9 = M.brute9("tie", "default")
    for k in (1, 3, 8):
        M.same_planes(gpu(renderer, rays, k), a9[:k], f"tie k={k} vs the brute force")
    sw = upload(renderer, M.scene("tie_swapped"))   # the higher id of every pair is met first
    for k in (1, 3, 8):
        M.same_planes(gpu(renderer, rays, k), a9[:k], f"tie, references swapped, k={k} vs the brute force")
    for flags in (HW, 0):   # the id rule in the other arithmetics: twins stand side by side, the lower id first
        got = gpu(renderer, rays, 8, flags)
        hit = got["id"][0::2] >= 0
        assert np.all(got["id"][1::2][hit] == got["id"][0::2][hit] + 6000) and hit.sum() >= 1000
        assert np.array_equal(got["t"][1::2][hit].view(np.uint32), got["t"][0::2][hit].view(np.uint32))
    d = upload(renderer, scene_arrays("rand4k_sbvh"))
    rays, a = M.duplicate_set("rand4k_sbvh")
    for k in (2, 8):
        got = gpu(renderer, rays, k)
        M.same_planes(got, a[:k], f"duplicate set k={k} vs the brute force")
        M.same_planes(got, twin(d, rays, k), f"duplicate set k={k} vs the twin")
    for flags in (HW, 0):
        assert not np.any(M.repeats(M.planes(gpu(renderer, rays, 8, flags))))
    assert M.repeats(M.traverse(d, rays, 8, presence=False)[0]).mean() >= 0.25, "the set bites"


def test_bad_node_error_misses(renderer):
    from ray_edge_common import aimed_at_malformed
    d = upload(renderer, scene_arrays("bad_node"))
    assert scene_image(renderer)[HDR_CLEAN] == 0
    o, dirs, _ = aimed_at_malformed(d, n=512)
    rays = rtamd.pack_rays(o, dirs, None)
    before = renderer.overflow_count()
    got = gpu(renderer, rays, 8)
    M.same_planes(got, twin(d, rays, 8), "bad_node vs the twin")
    M.same_planes(got, M.traverse(d, rays, 8)[0], "bad_node vs the traversal")
    whole_miss = np.all(M.planes(got)[:, :, 0] == M.MISS_ID, axis=0)
    assert differing(got, M.brute(d, rays, 8)) >= 10 and np.any(~whole_miss)
    assert renderer.overflow_count() == before, "an error miss is no overflow"
    upload(renderer, load_golden("cornell12"))
    assert scene_image(renderer)[HDR_CLEAN] == 1


def aimed(d, n):
    """n rays from incoherent origins, each at the centroid of one of d's triangles in turn."""
    o, _, _ = incoherent_rays(d, n=n)
    tri = d["vertices"][np.asarray(d["indices"]).reshape(-1, 3), :3].astype(F32)
    return rtamd.pack_rays(o, (tri.mean(1)[np.arange(n) % tri.shape[0]] - o).astype(F32), None)


def test_escape_leaves_and_root_leaf(renderer):
    d = upload(renderer, K.escape_tree())
    rays = aimed(d, 512)
    got = gpu(renderer, rays, 8)
    M.same_planes(got, twin(d, rays, 8), "escape tree vs the twin")
    M.same_planes(got, M.brute(d, rays, 8), "escape tree vs the brute force")
    assert np.any((got["id"] >= 0) & (got["id"] < 120)) and np.any(got["id"] >= 120), "both leaves answer"
    s = upload(renderer, scene_arrays("single_tri_rootleaf"))
    rays = aimed(s, 300)
    for flags in ARITHMETICS.values():
        got = gpu(renderer, rays, 8, flags)
        assert np.all(got["id"][0] == 0) and np.array_equal(M.planes(got)[1:], M.miss_words(rays, 7))
    M.same_planes(gpu(renderer, rays, 8), M.brute(s, rays, 8), "single_tri_rootleaf")


def test_combs(renderer):
    d = upload(renderer, scene_arrays("overflow_comb"))
    n = 1000
    o, dirs, _ = incoherent_rays(d, n=n)
    rays = rtamd.pack_rays(o, dirs, None)
    _, st, _ = M.traverse(d, rays, 8)
    assert st["overflows"] == n
    for k in (1, 8):
        for flags in (STRICT, 0):
            before = renderer.overflow_count()
            got = gpu(renderer, rays, k, flags)
            assert np.array_equal(M.planes(got), M.miss_words(rays, k))
            assert renderer.overflow_count() - before == n, "every ray overflows, each counted once: n, not k * n"
            assert renderer.last_deferred() == 0
    c = upload(renderer, K.comb40())
    o, dirs, _ = incoherent_rays(c, n=1000)
    rays = rtamd.pack_rays(o, dirs, None)
    before = renderer.overflow_count()
    got = gpu(renderer, rays, 8)
    _, st, deep = M.traverse(c, rays, 8)
    assert st["overflows"] == 0 and deep.max() > 16, "the stack outgrows its LDS part"
    M.same_planes(got, M.brute(c, rays, 8), "comb40 vs the brute force")
    M.same_planes(got, twin(c, rays, 8), "comb40 vs the twin")
    assert renderer.overflow_count() == before and np.any(got["id"] >= 0)


# ---- scenes made or moved on the GPU ----

def test_built_scene(renderer):
    d = scene_arrays("rand2k")
    renderer.build_scene({key: d[key] for key in MESH_KEYS}, max_leaf=2, keys="extent")
    built = scene_arrays("rand2k_built")   # the host twin's tree of the same build
    for which in M.TMAXES:
        rays = M.rays("rand2k", which)
        got = gpu(renderer, rays, 8)
        M.same_planes(got, twin(built, rays, 8), f"built {which} vs the twin over the LBVH")
        M.same_planes(got, M.brute9("rand2k", which)[:8], f"built {which} vs the brute force")


def test_after_update_vertices(renderer):
    from refit_common import moved_vertices, with_vertices
    d = upload(renderer, scene_arrays("hf40k"))
    rays = M.rays("hf40k", "default")
    M.same_planes(gpu(renderer, rays, 8), M.brute9("hf40k", "default")[:8], "before the update")
    verts = moved_vertices("hf40k")
    renderer.update_vertices(verts)
    nodes = rtamd.refit_nodes(rtamd.Scene.from_arrays(d), verts)
    moved = with_vertices(d, verts, nodes)
    got = gpu(renderer, rays, 8)
    M.same_planes(got, M.brute(moved, rays, 8), "after the update vs the brute force on the new vertices")
    M.same_planes(got, twin(moved, rays, 8), "after the update vs the twin on rt_refit_nodes' arrays")
    assert differing(got, M.brute9("hf40k", "default")[:8]) > 100


def test_scene_replacement_waits_for_a_query(renderer):
    import torch
    upload(renderer, scene_arrays("rand3k_bigleaf"))
    rays = M.rays("rand3k_bigleaf", "default")
    want = M.brute9("rand3k_bigleaf", "default")[:8]
    reps, n = 16, rays.shape[0]
    side = torch.cuda.Stream()
    d_rays = torch.from_numpy(np.tile(M.ray_words(rays).reshape(-1), reps).view(np.int32).copy()).cuda()
    d_out = torch.full((8 * reps * n * 4,), GUARD, dtype=torch.int32, device="cuda")
    b = load_golden("cornell12")
    torch.cuda.synchronize()
    # a query of scene A, then at once, without synchronising, build_scene of scene B: the records are A's
    renderer.trace_rays_k_device(d_rays.data_ptr(), reps * n, 8, d_out.data_ptr(), flags=STRICT, stream=side.cuda_stream)
    renderer.build_scene({key: b[key] for key in MESH_KEYS}, max_leaf=2)
    side.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(8, reps, n, 4)
    assert np.all(got == want[:, None]), "a query in flight saw the scene that replaced its own"
    torch.cuda.synchronize()


def test_after_scene_copy_and_scene_image_load(renderer):
    import torch
    upload(renderer, scene_arrays("rand4k_sbvh"))
    rays = M.rays("rand4k_sbvh", "default")
    want = M.brute9("rand4k_sbvh", "default")[:8]
    n = renderer.scene_image_size()
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    renderer.pack_scene(buf.data_ptr(), n)
    c = rtamd.Renderer(0)
    try:
        c.load_scene(buf.data_ptr(), n)
        M.same_planes(gpu(c, rays, 8), want, "after scene_image_load")
        upload(c, load_golden("cornell12"))
        c.copy_scene_from(renderer)
        M.same_planes(gpu(c, rays, 8), want, "after scene_copy")
    finally:
        c.close()


def test_edge_rays(renderer):
    d = upload(renderer, scene_arrays("rand3k_bigleaf"))
    rays, what, ok = M.edge_rays(d)
    got = gpu(renderer, rays, 8)
    M.same_planes(got, twin(d, rays, 8), "edge set vs the twin")
    M.same_planes(got, M.brute(d, rays, 8), "edge set vs the brute force")
    for flags in (HW, 0):
        w = M.planes(gpu(renderer, rays, 8, flags))
        assert np.array_equal(w[:, ~ok], M.miss_words(rays, 8)[:, ~ok]), "an invalid ray is k miss records in every arithmetic"


# ---- refusals ----

def test_refusals_leave_the_context_usable(renderer):
    import torch
    L = rtamd.lib()
    rays = M.rays("cornell12", "default")[:4].copy()
    out = np.full(8 * 4 * 4, GUARD, np.uint32)
    pp, po = vp(rays), vp(out)
    fresh = rtamd.Renderer(0)
    try:
        assert L.rt_trace_rays_k(fresh._h, pp, 4, 8, 0, po) == RT_ERR_NO_SCENE
        assert L.rt_trace_rays_k_device(fresh._h, pp, 4, 8, 0, po, None) == RT_ERR_NO_SCENE
    finally:
        fresh.close()
    d = upload(renderer, load_golden("cornell12"))
    h = renderer._h
    d_rays = torch.zeros(4 * 32 + 16, dtype=torch.uint8, device="cuda")
    d_out = torch.full((8 * 4 * 4 + 8,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dp, do = d_rays.data_ptr(), d_out.data_ptr()
    assert dp % 16 == 0 and do % 16 == 0
    c = C.c_void_p
    for bit in range(32):
        if (1 << bit) & ALLOWED:
            continue
        assert L.rt_trace_rays_k(h, pp, 4, 8, 1 << bit, po) == RT_ERR_INVALID_ARG, bit
        assert L.rt_trace_rays_k_device(h, c(dp), 4, 8, 1 << bit, c(do), None) == RT_ERR_INVALID_ARG, bit
    assert ANY & ~ALLOWED, "RT_FLAG_ANY_HIT is among the refused"
    assert L.rt_trace_rays_k(h, pp, 4, 8, STRICT | HW, po) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_k_device(h, c(dp), 4, 8, STRICT | HW, c(do), None) == RT_ERR_INVALID_ARG
    for k in (0, 9, -1, 1 << 30, -(1 << 31)):
        for n in (0, 4):
            assert L.rt_trace_rays_k(h, pp, n, k, 0, po) == RT_ERR_INVALID_ARG, (n, k)
            assert L.rt_trace_rays_k_device(h, c(dp), n, k, 0, c(do), None) == RT_ERR_INVALID_ARG, (n, k)
    for n, k in ((-1, 1), ((1 << 30) + 1, 1), (1 << 40, 8), ((1 << 27) + 1, 8), ((1 << 29) + 1, 2), (1 << 30, 2)):
        assert L.rt_trace_rays_k(h, pp, n, k, 0, po) == RT_ERR_INVALID_ARG, (n, k)
        assert L.rt_trace_rays_k_device(h, c(dp), n, k, 0, c(do), None) == RT_ERR_INVALID_ARG, (n, k)
    assert L.rt_trace_rays_k(h, None, 4, 8, 0, po) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_k(h, pp, 4, 8, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_k_device(h, None, 4, 8, 0, c(do), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_k_device(h, c(dp), 4, 8, 0, None, None) == RT_ERR_INVALID_ARG
    for off in (4, 8):
        assert L.rt_trace_rays_k_device(h, c(dp + off), 4, 8, 0, c(do), None) == RT_ERR_INVALID_ARG
        assert L.rt_trace_rays_k_device(h, c(dp), 4, 8, 0, c(do + off), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_k(h, None, 0, 8, 0, None) == 0          # n == 0: RT_OK, nothing launched
    assert L.rt_trace_rays_k_device(h, None, 0, 1, 0, None, None) == 0
    torch.cuda.synchronize()
    assert np.all(out == GUARD) and np.all(d_out.cpu().numpy().view(np.uint32) == GUARD), "a refused call wrote records"
    renderer.set_params(d["params"])
    frame = renderer.render(int(d["w"]), int(d["h"]), depth=int(d["depth"]), flags=0)
    assert np.array_equal(frame, d["ref_default"])
    for flags in (0, STRICT, HW, EXACT, STRICT | EXACT, HW | EXACT):   # each allowed bit and combination answers
        got = gpu(renderer, rays, 8, flags)
        assert np.any(got["id"] >= 0) and renderer.last_query_ms() > 0.0 and renderer.last_deferred() == 0
    assert L.rt_abi_version() == 3
