"""Ray queries on the GPU: Renderer.trace_rays / trace_rays_device against the two
yardsticks of tests/ray_query_common.py.  Every comparison is exact: ids equal, t equal in bits.

The frame of test_more_rays_than_lanes is 1024 x 1024, not 1024 x 640: yardstick 2 needs
power-of-two sides for its rays to be exact in float32 (640 is not one: (y - 0.5) / 640 has a full
mantissa and b * yf rounds), and 1024 x 512 is exactly the 524,288 lanes of the largest resident
grid, so 1024 x 1024 is the smallest such frame in which a wave must take a second group."""
import ctypes as C

import numpy as np
import pytest

import rtamd
from conftest import load_golden
from ray_edge_common import deep_comb40   # overflow_comb cut to 40 levels: restarts without overflow, rays that hit
from ray_query_common import (N_RAYS, TMAX_DEFAULT, TMIN, oracle_closest, oracle_normalize, oracle_ray_tri,
                              quantised_frame, reference, scene_arrays)

pytestmark = pytest.mark.gpu

STRICT, HW, EXACT_DIV, NO_SHADOW = rtamd.RT_FLAG_STRICT_MATH, rtamd.RT_FLAG_HW_MATH, rtamd.RT_FLAG_EXACT_DIV, 1
RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE = -1, -3
SCENES = ["cornell12", "rand2k", "rand4k_sbvh", "rand3k_bigleaf", "single_tri_rootleaf", "rand2k_built"]
MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")
GUARD = 0x5A5A5A5A


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def put_scene(r, name):
    """The named scene in the renderer: an upload, or for rand2k_built build_scene on the GPU (the
    yardstick then runs on the host twin's arrays)."""
    d = scene_arrays(name)
    if name == "rand2k_built":
        r.build_scene({k: d[k] for k in MESH_KEYS}, max_leaf=2, keys="extent")
    else:
        r.upload(rtamd.Scene.from_arrays(d))
    return d


def same(got, ids, t, label):
    gi, gt = got
    bad = np.flatnonzero(gi != ids)
    assert bad.size == 0, f"{label}: {bad.size} ids differ, first {bad[:5]}: {gi[bad[:5]]} vs {ids[bad[:5]]}"
    bad = np.flatnonzero(bits(gt) != bits(t))
    assert bad.size == 0, f"{label}: {bad.size} t differ, first {bad[:5]}: {gt[bad[:5]]} vs {t[bad[:5]]}"


def hit_tmax(ids, t, scale=1.0):
    """Per-ray tmax: scale * t* where the oracle hits, the default elsewhere."""
    return np.where(ids >= 0, (t * np.float32(scale)).astype(np.float32), TMAX_DEFAULT).astype(np.float32)


# ---- 1: closest hit against the oracle, incoherent rays ----

@pytest.mark.parametrize("name", SCENES)
def test_closest_hit_equals_the_oracle(renderer, name):
    put_scene(renderer, name)
    o, dirs, ids, t, _, _ = reference(name)
    assert o.shape[0] == N_RAYS and np.any(ids >= 0) and np.any(ids < 0)
    got = renderer.trace_rays(o, dirs, flags=STRICT)
    same(got, ids, t, name)
    assert np.all(bits(got[1][ids < 0]) == bits(TMAX_DEFAULT)), "a miss's t is the tmax word"
    assert renderer.last_query_ms() > 0.0


# ---- 2: group edges ----

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_group_edges_write_nothing_past_n(renderer, n):
    import torch
    put_scene(renderer, "cornell12")
    o, dirs, ids, t, _, _ = reference("cornell12")
    rays = rtamd.pack_rays(o[:n + 3], dirs[:n + 3])          # more rays in memory than asked for
    # host form, straight through the C ABI into a buffer with guard records after hits[n]
    hits = np.full(2 * (n + 4), GUARD, np.uint32)
    rc = rtamd.lib().rt_trace_rays(renderer._h, rays.ctypes.data_as(C.c_void_p), n, STRICT, hits.ctypes.data_as(C.c_void_p))
    assert rc == 0
    assert np.all(hits[2 * n:] == GUARD), "the host form wrote past hits[n]"
    assert np.array_equal(hits[0:2 * n:2].view(np.int32), ids[:n]) and np.array_equal(hits[1:2 * n:2], bits(t[:n]))
    # device form: the kernel's own stores
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_hits = torch.full((2 * (n + 4),), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    renderer.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), flags=STRICT)
    torch.cuda.synchronize()
    got = d_hits.cpu().numpy().view(np.uint32)
    assert np.all(got[2 * n:] == GUARD), "the kernel wrote past hits[n]"
    assert np.array_equal(got[0:2 * n:2].view(np.int32), ids[:n]) and np.array_equal(got[1:2 * n:2], bits(t[:n]))


# ---- 3: more rays than lanes ----

def test_more_rays_than_lanes(renderer):
    from oracle import oracle
    d = put_scene(renderer, "rand2k")
    w = h = 1024                                              # see the module's docstring
    p, o, dirs = quantised_frame(d, w, h)
    assert o.shape[0] > 256 * 2048, "some wave must take a second group"
    ref = oracle.render(d, p, w, h, depth=1, flags=NO_SHADOW)
    want = ref["hits"][:, 0, 0].copy()
    assert int((want >= 0).sum()) > 100000
    want[want == -2] = -1                                     # untraced pixels count as misses, id only
    ids, t = renderer.trace_rays(o, dirs, flags=STRICT)
    bad = np.flatnonzero(ids != want)
    assert bad.size == 0, f"vs the oracle's frame: {bad.size} ids differ, first {bad[:5]}"
    traced = ref["hits"][:, 0, 0] != -2
    assert np.array_equal(bits(t[traced]), bits(ref["t"][traced, 0]))
    renderer.set_params(p)
    for flags in (0, HW, STRICT):
        g = renderer.render(w, h, depth=1, flags=flags, aux=True)
        ids, t = renderer.trace_rays(o, dirs, flags=flags)
        traced = g["hits"][:, 0, 0] != -2
        assert int(traced.sum()) > 100000
        same((ids[traced], t[traced]), g["hits"][traced, 0, 0], g["t"][traced, 0], f"vs render flags={flags}")


# ---- 4: the fast quotient ----

@pytest.mark.parametrize("name", SCENES)
def test_fast_quotient_equals_the_division_form(renderer, name):
    put_scene(renderer, name)
    o, dirs, ids, _, _, _ = reference(name)
    for flags in (0, HW, STRICT):
        for any_hit in (False, True):
            fast = renderer.trace_rays(o, dirs, any_hit=any_hit, flags=flags)
            slow = renderer.trace_rays(o, dirs, any_hit=any_hit, flags=flags | EXACT_DIV)
            same(fast, slow[0], slow[1], f"{name} flags={flags} any={any_hit}")
            assert np.any(fast[0] >= 0)


# ---- 5: tmax ----

@pytest.mark.parametrize("name", SCENES)
def test_tmax_at_the_hit_distance_misses(renderer, name):
    put_scene(renderer, name)
    o, dirs, ids, t, _, _ = reference(name)
    tm = hit_tmax(ids, t)
    gi, gt = renderer.trace_rays(o, dirs, tmax=tm, flags=STRICT)
    assert np.all(gi == -1), f"{name}: {int((gi >= 0).sum())} rays hit at or beyond their tmax"
    assert np.array_equal(bits(gt), bits(tm))
    if name == "rand2k_built":   # whole-triangle boxes: the hit's leaf is still entered with n <= 2 t*
        same(renderer.trace_rays(o, dirs, tmax=hit_tmax(ids, t, 2.0), flags=STRICT), ids, t, name + " tmax = 2 t*")


# ---- 6: any hit ----

@pytest.mark.parametrize("name", SCENES)
def test_any_hit(renderer, name):
    d = put_scene(renderer, name)
    o, dirs, ids, t, _, _ = reference(name)
    for label, tm in (("default", None), ("t*", hit_tmax(ids, t)), ("2 t*", hit_tmax(ids, t, 2.0))):
        ci, ct = renderer.trace_rays(o, dirs, tmax=tm, flags=STRICT)
        ai, at = renderer.trace_rays(o, dirs, tmax=tm, any_hit=True, flags=STRICT)
        assert np.array_equal(ai >= 0, ci >= 0), f"{name} {label}: any hit and closest hit disagree on hit / miss"
        tmv = np.full(N_RAYS, TMAX_DEFAULT, np.float32) if tm is None else tm
        miss = ai < 0
        assert np.all(ai[miss] == -1) and np.array_equal(bits(at[miss]), bits(tmv[miss]))
        if label == "default":
            same((ci, ct), ids, t, name)
        if label == "t*":
            assert np.all(miss)
        for k in np.flatnonzero(~miss):
            assert ai[k] % 3 == 0 and 0 <= ai[k] < d["indices"].size
            want = oracle_ray_tri(d, o[k], oracle_normalize(dirs[k]), int(ai[k]))
            assert bits(at[k])[0] == bits(want)[0], (name, label, k, at[k], want)
            assert TMIN < at[k] < tmv[k] and at[k] >= ct[k], (name, label, k, at[k], ct[k], tmv[k])
        for flags in (0, HW):   # the other arithmetics: the hit / miss equality alone
            ci2 = renderer.trace_rays(o, dirs, tmax=tm, flags=flags)[0]
            ai2 = renderer.trace_rays(o, dirs, tmax=tm, any_hit=True, flags=flags)[0]
            assert np.array_equal(ai2 >= 0, ci2 >= 0), f"{name} {label} flags={flags}"


# ---- 7: invalid rays ----

def test_invalid_rays_are_misses_and_leave_their_neighbours(renderer):
    put_scene(renderer, "cornell12")
    o, dirs, ids, t, _, _ = reference("cornell12")
    n, lanes = 128, (0, 31, 63)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    payload = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    cases = {                                                 # name -> (field, component or None, value)
        "nan origin": ("o", 1, nan), "inf origin": ("o", 2, inf), "-inf origin": ("o", 0, -inf),
        "nan direction": ("d", 0, nan), "inf direction": ("d", 1, inf), "zero direction": ("d", None, 0.0),
        "nan tmax": ("tmax", None, payload), "zero tmax": ("tmax", None, 0.0), "negative tmax": ("tmax", None, -5.0),
        "tmax at tmin": ("tmax", None, TMIN),
    }
    for flags in (STRICT, 0):
        base = renderer.trace_rays(o[:n], dirs[:n], flags=flags)
        if flags == STRICT:
            same(base, ids[:n], t[:n], "valid rays")
        for label, (field, comp, val) in cases.items():
            rays = rtamd.pack_rays(o[:n], dirs[:n])
            for lane in lanes:
                if field == "tmax":
                    rays["tmax"].view(np.uint32)[lane] = np.float32(val).view(np.uint32)
                elif comp is None:
                    rays[field][lane] = val
                else:
                    rays[field][lane, comp] = val
            hits = np.zeros(n, rtamd.HIT_DTYPE)
            rc = rtamd.lib().rt_trace_rays(renderer._h, rays.ctypes.data_as(C.c_void_p), n, flags, hits.ctypes.data_as(C.c_void_p))
            assert rc == 0, label
            for lane in lanes:
                assert hits["id"][lane] == -1, (label, lane)
                assert bits(hits["t"])[lane] == bits(rays["tmax"])[lane], (label, lane, "the tmax word changed")
            keep = np.setdiff1d(np.arange(n), lanes)
            same((hits["id"][keep], hits["t"][keep]), base[0][keep], base[1][keep], f"{label} flags={flags}: the neighbours")
        gi, gt = renderer.trace_rays(o[:n], dirs[:n], tmax=inf, flags=flags)
        assert np.array_equal(gi, base[0]), "+inf is a legal tmax"
        hit = gi >= 0
        assert np.array_equal(bits(gt[hit]), bits(base[1][hit])) and np.all(gt[~hit] == inf)


# ---- 8: deep stacks ----

def test_deep_stacks_overflow_and_restart(renderer):
    put_scene(renderer, "overflow_comb")
    o, dirs, ids, t, overflows, _ = reference("overflow_comb")
    before = renderer.overflow_count()
    gi, gt = renderer.trace_rays(o, dirs, flags=STRICT)
    assert np.array_equal(gi, ids), "overflow_comb: ids differ from the oracle's"
    assert np.all(gi == -1) and np.all(bits(gt) == bits(TMAX_DEFAULT))   # an overflow is a miss: t is the tmax word
    assert renderer.last_deferred() > 0
    assert renderer.overflow_count() - before == overflows and overflows > 0
    hit = ids >= 0                                            # (this comb's rays overflow or miss: none hit)
    mi = renderer.trace_rays(o[hit], dirs[hit], tmax=t[hit], flags=STRICT)[0] if np.any(hit) else np.empty(0, np.int32)
    assert np.all(mi == -1)
    # the same comb 40 levels deep: restarts without overflow, and rays that hit -- what a restart
    # that forgot the ray's tmax would get wrong
    d = deep_comb40()
    renderer.upload(rtamd.Scene.from_arrays(d))
    from ray_query_common import incoherent_rays
    o, dirs, campos = incoherent_rays(d)
    st = {}
    ids, t = oracle_closest(d, o, campos, st)
    assert st["stack_overflow"] == 0 and int((ids >= 0).sum()) > 100
    before = renderer.overflow_count()
    same(renderer.trace_rays(o, dirs, flags=STRICT), ids, t, "deep_comb40")
    assert renderer.last_deferred() > 0 and renderer.overflow_count() == before
    tm = hit_tmax(ids, t)
    gi, gt = renderer.trace_rays(o, dirs, tmax=tm, flags=STRICT)
    assert renderer.last_deferred() > 0
    assert np.all(gi == -1), f"{int((gi >= 0).sum())} restarted rays hit at their tmax"
    assert np.array_equal(bits(gt), bits(tm))
    same(renderer.trace_rays(o, dirs, tmax=hit_tmax(ids, t, 2.0), flags=STRICT), ids, t, "deep_comb40 tmax = 2 t*")
    ai = renderer.trace_rays(o, dirs, tmax=tm, any_hit=True, flags=STRICT)[0]
    assert np.all(ai == -1)
    for flags in (0, HW):
        fast = renderer.trace_rays(o, dirs, tmax=hit_tmax(ids, t, 2.0), flags=flags)
        slow = renderer.trace_rays(o, dirs, tmax=hit_tmax(ids, t, 2.0), flags=flags | EXACT_DIV)
        same(fast, slow[0], slow[1], f"deep_comb40 flags={flags}")


# ---- 9: the device form and its ordering ----

def test_device_form_and_ordering(renderer):
    import torch
    from refit_common import moved_vertices, np_refit, with_vertices
    put_scene(renderer, "rand2k")
    o, dirs, ids, t, _, _ = reference("rand2k")
    want = renderer.trace_rays(o, dirs, flags=STRICT)
    same(want, ids, t, "host form")
    rays = rtamd.pack_rays(o, dirs)
    side = torch.cuda.Stream()
    host = torch.from_numpy(rays.view(np.uint8).reshape(-1)).pin_memory()
    d_rays = torch.zeros(rays.nbytes, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((2 * N_RAYS,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_rays.copy_(host, non_blocking=True)                 # the rays are written on the side stream
        renderer.trace_rays_device(d_rays.data_ptr(), N_RAYS, d_hits.data_ptr(), flags=STRICT, stream=side.cuda_stream)
    side.synchronize()
    got = d_hits.cpu().numpy()
    same((got[0::2], got[1::2].view(np.float32)), want[0], want[1], "device form")
    assert renderer.last_query_ms() > 0.0

    # a query of scene A, then at once, without synchronising, build_scene of scene B: the hits are A's
    reps = 256
    big = torch.from_numpy(np.tile(rays, reps).view(np.uint8).reshape(-1)).cuda()
    big_hits = torch.full((2 * N_RAYS * reps,), -7, dtype=torch.int32, device="cuda")
    b = load_golden("cornell12")
    torch.cuda.synchronize()
    renderer.trace_rays_device(big.data_ptr(), N_RAYS * reps, big_hits.data_ptr(), flags=STRICT, stream=side.cuda_stream)
    renderer.build_scene({k: b[k] for k in MESH_KEYS}, max_leaf=2)
    side.synchronize()
    got = big_hits.cpu().numpy().reshape(reps, N_RAYS, 2)
    assert np.all(got[:, :, 0] == want[0][None, :]), "a query in flight saw the scene that replaced its own"
    assert np.all(got[:, :, 1].view(np.uint32) == bits(want[1])[None, :])

    # after update_vertices the query sees the refit scene: the oracle on the CPU-refit arrays
    d = put_scene(renderer, "hf40k")
    o, dirs, ids0, t0, _, campos = reference("hf40k")
    same(renderer.trace_rays(o, dirs, flags=STRICT), ids0, t0, "hf40k before the update")
    verts = moved_vertices("hf40k")
    renderer.trace_rays_device(big.data_ptr(), N_RAYS, big_hits.data_ptr(), flags=STRICT, stream=side.cuda_stream)
    renderer.update_vertices(verts)                           # waits for the query above
    nodes, _ = np_refit(d, verts)
    ids1, t1 = oracle_closest(with_vertices(d, verts, nodes), o, campos)
    assert not np.array_equal(ids1, ids0) or not np.array_equal(t1, t0)
    same(renderer.trace_rays(o, dirs, flags=STRICT), ids1, t1, "hf40k after the update")
    torch.cuda.synchronize()


# ---- 10: refusals ----

def test_refusals_leave_the_context_usable(renderer):
    import torch
    L = rtamd.lib()
    fresh = rtamd.Renderer(0)
    rays = rtamd.pack_rays(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    hits = np.full(8, GUARD, np.uint32)
    pr, ph = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    try:
        assert L.rt_trace_rays(fresh._h, pr, 4, 0, ph) == RT_ERR_NO_SCENE
        assert L.rt_trace_rays_device(fresh._h, pr, 4, 0, ph, None) == RT_ERR_NO_SCENE
    finally:
        fresh.close()
    d = put_scene(renderer, "cornell12")
    h = renderer._h
    d_rays = torch.zeros(4 * 32 + 16, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((8 + 2,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dr, dh = d_rays.data_ptr(), d_hits.data_ptr()
    assert dr % 16 == 0 and dh % 8 == 0
    for bad in (1, 8, 16, 32, 256, 1 << 31, HW | STRICT):
        assert L.rt_trace_rays(h, pr, 4, bad, ph) == RT_ERR_INVALID_ARG, bad
        assert L.rt_trace_rays_device(h, C.c_void_p(dr), 4, bad, C.c_void_p(dh), None) == RT_ERR_INVALID_ARG, bad
    assert L.rt_trace_rays(h, pr, -1, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays(h, pr, (1 << 30) + 1, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays(h, None, 4, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays(h, pr, 4, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_device(h, None, 4, 0, C.c_void_p(dh), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_device(h, C.c_void_p(dr), 4, 0, None, None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_device(h, C.c_void_p(dr + 4), 4, 0, C.c_void_p(dh), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_device(h, C.c_void_p(dr), 4, 0, C.c_void_p(dh + 4), None) == RT_ERR_INVALID_ARG
    with pytest.raises(rtamd.RtError):
        renderer.trace_rays(np.zeros((4, 3)), np.ones((4, 3)), flags=NO_SHADOW)
    assert L.rt_trace_rays(h, None, 0, 0, None) == 0          # n == 0: RT_OK, nothing launched
    torch.cuda.synchronize()
    assert np.all(hits == GUARD) and np.all(d_hits.cpu().numpy().view(np.uint32) == GUARD), "a refused call wrote hits"
    renderer.set_params(d["params"])
    out = renderer.render(int(d["w"]), int(d["h"]), depth=int(d["depth"]), flags=0)
    assert np.array_equal(out, d["ref_default"])
