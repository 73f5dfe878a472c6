"""Occlusion fans on the GPU.  Everything is exact: masks are compared as words.

Two yardsticks.  S_strict has the CPU oracle: fan_common.yardstick, oracle.trace_rays(any_hit=True)
on the rays fan_ref.c expands, packed.  All three arithmetics have the definition itself: bit (i, j)
is the `id >= 0` of rt_trace_rays(RT_FLAG_ANY_HIT | flags) for ray (i, j) of rt_fan_expand, asked of
the same context (query_masks below), which pins the per-lane ray_init, the octant loops of S_ref
and the raw-word cull in every arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

import rtamd
import fan_common as F
import ray_edge_common as E
from conftest import load_golden
from ray_query_common import quantised_frame, scene_arrays
from refit_common import scene_image

pytestmark = pytest.mark.gpu

STRICT, HW, EXACT_DIV, ANY_HIT = rtamd.RT_FLAG_STRICT_MATH, rtamd.RT_FLAG_HW_MATH, rtamd.RT_FLAG_EXACT_DIV, rtamd.RT_FLAG_ANY_HIT
ARITHMETICS = {"ref": 0, "strict": STRICT, "hw": HW}
MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")
RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE = -1, -3
GUARD = 0x5A5A5A5A
HDR_CLEAN = 13
RECORD_LIMIT = 64
SLICE = 1 << 20


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def upload(r, d):
    r.upload(rtamd.Scene.from_arrays(d))
    return d


def query_masks(r, rec, dirs, flags):
    """The definition on the GPU: rt_trace_rays(ANY_HIT | flags) of rt_fan_expand's traced rays, in
    slices of 2^20, `id >= 0` packed into the fan's layout."""
    rays, traced = rtamd.fan_expand(rec, dirs)
    n, k = rec.shape[0], len(dirs)
    hit = np.zeros(n * k, bool)
    idx = np.flatnonzero(traced)
    for s in range(0, idx.size, SLICE):
        part = np.ascontiguousarray(rays[idx[s:s + SLICE]])
        out = np.zeros(part.shape[0], rtamd.HIT_DTYPE)
        assert rtamd.lib().rt_trace_rays(r._h, vp(part), part.shape[0], flags | ANY_HIT, vp(out)) == 0
        hit[idx[s:s + SLICE]] = out["id"] >= 0
    return F.pack_bits(hit.reshape(n, k))


def same_masks(got, want, label):
    assert got.shape == want.shape and got.dtype == np.uint32, f"{label}: {got.shape} vs {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{label}: {bad.shape[0]} words differ, first (chunk, origin) {bad[:4].tolist()}: " \
                          f"{[hex(int(got[c, i])) for c, i in bad[:4]]} vs {[hex(int(want[c, i])) for c, i in bad[:4]]}"


# ---- S_strict against the oracle ----

@pytest.mark.parametrize("name", F.SCENES)
def test_strict_equals_the_oracle(renderer, name):
    x = F.inputs(name)
    upload(renderer, x["d"])
    for setting in F.SETTINGS:
        want = F.yardstick(name, setting)[0]
        got = renderer.trace_fan(F.records(name, setting), x["dirs"], flags=STRICT)
        same_masks(got, want, f"{name} {setting}")
        assert want.any() and (setting != "default" or not want.all())


# ---- all three arithmetics against the expanded query ----

@pytest.mark.parametrize("name", F.SCENES)
def test_every_arithmetic_equals_the_expanded_query(renderer, name):
    x = F.inputs(name)
    upload(renderer, x["d"])
    rec = F.records(name, "quarter")
    for mode, f in ARITHMETICS.items():
        for extra in (0, EXACT_DIV):
            got = renderer.trace_fan(rec, x["dirs"], flags=f | extra)
            same_masks(got, query_masks(renderer, rec, x["dirs"], f | extra), f"{name} {mode} extra={extra}")
            assert got.any()
    # S_ref's cull is the raw-word rule too: with culling, the fan's bits are the unculled fan's bits of the traced rays
    _, traced = rtamd.fan_expand(rec, x["dirs"])
    nocull = renderer.trace_fan(rtamd.pack_fan_origins(x["origins"], None, x["quarter"]), x["dirs"])
    culled = renderer.trace_fan(rec, x["dirs"])
    n, k = rec.shape[0], x["dirs"].shape[0]
    assert np.array_equal(rtamd.fan_bits(culled, k), rtamd.fan_bits(nocull, k) & traced.reshape(n, k))


# ---- shapes: group and chunk edges, host and device form, guards ----

@pytest.mark.parametrize("k", [1, 31, 32, 33, 64, 65])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_shapes_host_and_device_form(renderer, n, k):
    import torch
    x = F.inputs("rand2k")
    upload(renderer, x["d"])
    dirs = F.fibonacci(k)
    rec = rtamd.pack_fan_origins(x["origins"][:n], x["normals"][:n], x["quarter"])
    w = (k + 31) // 32
    want = query_masks(renderer, rec, dirs, 0)
    got = renderer.trace_fan(rec, dirs)
    same_masks(got, want, f"host form n={n} k={k}")
    if k % 32 and n:
        assert not np.any(got[-1] >> np.uint32(k % 32)), "the bits j >= k of the last word are 0"
    # the device form on a side stream: a guard record after the origins, 64 guard words after masks[W n]
    guard_rec = rtamd.pack_fan_origins(np.full((1, 3), np.nan, np.float32), np.full((1, 3), np.nan, np.float32), np.nan)
    h_org = np.concatenate([rec, guard_rec])
    side = torch.cuda.Stream()
    d_org = torch.from_numpy(h_org.view(np.uint8).reshape(-1).copy()).cuda()
    d_dirs = torch.from_numpy(rtamd.pack_fan_dirs(dirs).reshape(-1).copy()).cuda()
    d_masks = torch.full((w * n + 64,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        renderer.trace_fan_device(d_org.data_ptr(), n, d_dirs.data_ptr(), k, d_masks.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    out = d_masks.cpu().numpy().view(np.uint32)
    assert np.all(out[w * n:] == GUARD), "the kernel wrote past masks[W n]"
    same_masks(out[:w * n].reshape(w, n), want, f"device form n={n} k={k}")
    if n:
        assert renderer.last_query_ms() > 0.0


# ---- the grid cap: every wave takes several items ----

def test_grid_cap_many_items_per_wave(renderer):
    x = F.inputs("rand2k")
    upload(renderer, x["d"])
    n, k = 300, 100
    pick = np.arange(n) % x["origins"].shape[0]
    rec = rtamd.pack_fan_origins(x["origins"][pick], x["normals"][pick], x["quarter"])
    dirs = F.fibonacci(k)
    old = os.environ.get("RTAMD_FAN_GRID_BLOCKS")
    os.environ["RTAMD_FAN_GRID_BLOCKS"] = "2"   # 8 waves for 5 groups x 4 chunks = 20 items
    capped = rtamd.Renderer(0)
    try:
        upload(capped, x["d"])
        for mode, f in ARITHMETICS.items():
            got = capped.trace_fan(rec, dirs, flags=f)       # the knob is read at this context's first fan
            same_masks(got, renderer.trace_fan(rec, dirs, flags=f), f"capped vs uncapped, {mode}")
            assert got.any()
        same_masks(capped.trace_fan(rec, dirs, flags=STRICT), F.yardstick_for(x["d"], rec, dirs), "capped vs the oracle")
    finally:
        capped.close()
        if old is None:
            del os.environ["RTAMD_FAN_GRID_BLOCKS"]
        else:
            os.environ["RTAMD_FAN_GRID_BLOCKS"] = old


# ---- lanes and directions ----

def test_invalid_origins_at_lanes_0_31_63(renderer):
    x = F.inputs("rand2k")
    upload(renderer, x["d"])
    n = 192
    rec = rtamd.pack_fan_origins(x["origins"][:n], x["normals"][:n], x["quarter"])
    for mode, f in ARITHMETICS.items():
        whole = renderer.trace_fan(rec, x["dirs"], flags=f)
        for what in ("nan origin", "inf normal", "zero tmax"):
            for lane in (0, 31, 63):
                at = np.arange(lane, n, 64)
                bad = rec.copy()
                if what == "nan origin":
                    bad["o"][at, 1] = np.nan
                elif what == "inf normal":
                    bad["n"][at, 2] = np.inf
                else:
                    bad["tmax"][at] = 0.0
                got = renderer.trace_fan(bad, x["dirs"], flags=f)
                keep = np.setdiff1d(np.arange(n), at)
                assert not got[:, at].any(), f"{mode} {what} at lane {lane}: an invalid origin's words are 0"
                assert np.array_equal(got[:, keep], whole[:, keep]), f"{mode} {what} at lane {lane}: the neighbours"
        assert whole[:, np.arange(0, n, 64)].any() or whole[:, np.arange(31, n, 64)].any()


def test_direction_table_with_every_kind_in_one_chunk(renderer):
    """Zero, NaN, inf, subnormal-component, axis-aligned and opposite-octant directions in one chunk:
    each bit is what the ray gets alone (a fan of that one direction), and the expanded query's."""
    x = F.inputs("rand2k")
    d = upload(renderer, x["d"])
    sub = np.float32(1e-45)
    dirs = np.array([(1, 2, 3), (0, 0, 0), (-1, -2, -3), (np.nan, 1, 0), (0, 1, 0), (np.inf, 0, 0), (sub, 1, 1), (0, -1, 0),
                     (1, 0, 0), (-0.0, 0, -0.0), (-1, 0, 0), (0, 0, 1), (sub, sub, sub), (0, 0, -1), (1, -1, 1), (-1, 1, -1),
                     (1e30, 1e30, 1e30), (-1e-30, 2e-30, 1e-30)], np.float32)
    n = 128
    rec = rtamd.pack_fan_origins(x["origins"][:n], None, x["quarter"])
    for mode, f in ARITHMETICS.items():
        got = renderer.trace_fan(rec, dirs, flags=f)
        same_masks(got, query_masks(renderer, rec, dirs, f), f"mixed table {mode}")
        bits = rtamd.fan_bits(got, dirs.shape[0])
        for j in range(dirs.shape[0]):
            alone = rtamd.fan_bits(renderer.trace_fan(rec, dirs[j:j + 1], flags=f), 1)[:, 0]
            assert np.array_equal(bits[:, j], alone), f"{mode}: direction {j} alone"
        invalid = ~np.all(np.isfinite(dirs), axis=1) | np.all(dirs == 0, axis=1)
        assert not bits[:, invalid].any() and bits[:, ~invalid].any()
    same_masks(renderer.trace_fan(rec, dirs, flags=STRICT), F.yardstick_for(d, rec, dirs), "mixed table vs the oracle")


def test_a_direction_no_lane_faces_is_skipped(renderer):
    """Group 0: all 64 normals face away from direction 0 (the wave skips its traversal); group 1: the
    same but for lane 17, which faces it.  The other directions are traced by every lane."""
    x = F.inputs("rand2k")
    d = upload(renderer, x["d"])
    n = 128
    dirs = np.concatenate([np.array([(0, 0, 1)], np.float32), F.fibonacci(40)])
    normals = np.tile(np.array([(0.3, 0.2, -1.0)], np.float32), (n, 1))
    normals[64 + 17] = (0.3, 0.2, 1.0)
    rec = rtamd.pack_fan_origins(x["origins"][:n], normals, None)
    nocull = rtamd.pack_fan_origins(x["origins"][:n], None, None)
    _, traced = rtamd.fan_expand(rec, dirs)
    traced = traced.reshape(n, -1)
    assert not traced[:64, 0].any() and traced[64:, 0].sum() == 1 and traced[64 + 17, 0] and traced[:, 1:].any(axis=0).any()
    for mode, f in ARITHMETICS.items():
        got = renderer.trace_fan(rec, dirs, flags=f)
        same_masks(got, query_masks(renderer, rec, dirs, f), f"skip {mode}")
        bits = rtamd.fan_bits(got, dirs.shape[0])
        free = rtamd.fan_bits(renderer.trace_fan(nocull, dirs, flags=f), dirs.shape[0])
        assert not bits[:64, 0].any() and not np.delete(bits[64:, 0], 17).any()
        assert bits[64 + 17, 0] == free[64 + 17, 0]
        assert np.array_equal(bits, free & traced)
    same_masks(renderer.trace_fan(rec, dirs, flags=STRICT), F.yardstick_for(d, rec, dirs), "skip vs the oracle")


# ---- the general kernel and deep stacks ----

@pytest.fixture(scope="module")
def general():
    """A second context whose uploads take the general traversal (split records), asserted on every
    upload as tests/test_ray_query_edges_gpu.py does: the records reach the limit, and the context
    refuses rt_fetch_counts, whose counting kernels are fast-path only."""
    r = rtamd.Renderer(0)

    def put(d):
        old = os.environ.get("RTAMD_RECORD_LIMIT")
        os.environ["RTAMD_RECORD_LIMIT"] = str(RECORD_LIMIT)
        try:
            r.upload(rtamd.Scene.from_arrays(d))
        finally:
            if old is None:
                del os.environ["RTAMD_RECORD_LIMIT"]
            else:
                os.environ["RTAMD_RECORD_LIMIT"] = old
        hdr = scene_image(r)[:6]
        assert 16 * (int(hdr[2]) + (int(hdr[3]) << 32) + int(hdr[4]) + (int(hdr[5]) << 32)) >= RECORD_LIMIT
        with pytest.raises(rtamd.RtError):
            r.fetch_counts(8, 8, 1, 0)
        return r
    yield put
    r.close()


@pytest.mark.parametrize("name", ["cornell12", "rand2k", "knot16k"])
def test_general_kernel(renderer, general, name):
    x = F.inputs(name)
    upload(renderer, x["d"])
    g = general(x["d"])
    rec = F.records(name, "quarter")
    for mode, f in ARITHMETICS.items():
        got = g.trace_fan(rec, x["dirs"], flags=f)
        same_masks(got, renderer.trace_fan(rec, x["dirs"], flags=f), f"{name} {mode}: general vs fast")
        same_masks(got, query_masks(g, rec, x["dirs"], f), f"{name} {mode}: general fan vs general query")
    same_masks(g.trace_fan(rec, x["dirs"], flags=STRICT), F.yardstick(name, "quarter")[0], f"{name}: general vs the oracle")


def test_bad_node_takes_the_general_kernel(renderer):
    d = upload(renderer, E.edge_scene("bad_node"))
    assert scene_image(renderer)[HDR_CLEAN] == 0
    o, dirs, _ = E.ray_class("bad_node", "malformed")
    rec = rtamd.pack_fan_origins(o[:192], None, None)
    table = np.ascontiguousarray(dirs[1:67:2])   # the rays aimed into the malformed node's box
    want, _, hit, stats = F.yardstick_for(d, rec, table, want_stats=True)
    assert stats["error_miss"] >= 10 and hit.any() and not hit.all()
    for mode, f in ARITHMETICS.items():
        got = renderer.trace_fan(rec, table, flags=f)
        same_masks(got, query_masks(renderer, rec, table, f), f"bad_node {mode}")
        if mode == "strict":
            same_masks(got, want, "bad_node vs the oracle")
    upload(renderer, load_golden("cornell12"))
    assert scene_image(renderer)[HDR_CLEAN] == 1


def _comb_fan(name):
    o, dirs, _ = E.ray_class(name, "incoherent")
    return rtamd.pack_fan_origins(o[:128], None, None), np.ascontiguousarray(dirs[:48])


def test_overflow_comb_counts_what_the_expanded_query_counts(renderer):
    d = upload(renderer, E.edge_scene("overflow_comb"))
    rec, dirs = _comb_fan("overflow_comb")
    want, _, _, stats = F.yardstick_for(d, rec, dirs, want_stats=True)
    assert stats["stack_overflow"] > 0
    before = renderer.overflow_count()
    got = renderer.trace_fan(rec, dirs, flags=STRICT)
    rise = renderer.overflow_count() - before
    same_masks(got, want, "overflow_comb vs the oracle")
    assert rise == stats["stack_overflow"]
    before = renderer.overflow_count()
    same_masks(got, query_masks(renderer, rec, dirs, STRICT), "overflow_comb vs the expanded query")
    assert renderer.overflow_count() - before == rise, "the fan counts the overflows the expanded query counts"


def test_deep_comb_restarts_and_hits(renderer):
    d = upload(renderer, E.edge_scene("deep_comb40"))
    rec, dirs = _comb_fan("deep_comb40")
    want, _, hit, stats = F.yardstick_for(d, rec, dirs, want_stats=True)
    assert stats["stack_overflow"] == 0 and stats["max_stack"] > 16 and hit.any()
    before = renderer.overflow_count()
    for mode, f in ARITHMETICS.items():
        got = renderer.trace_fan(rec, dirs, flags=f)
        assert renderer.last_deferred() > 0, "these rays outgrow the LDS stack and restart"
        if mode == "strict":
            same_masks(got, want, "deep_comb40 vs the oracle")
        same_masks(got, query_masks(renderer, rec, dirs, f), f"deep_comb40 {mode}")
    assert renderer.overflow_count() == before


# ---- scene changes ----

def test_scene_changes_wait_for_a_fan(renderer):
    import torch
    from refit_common import moved_vertices, np_refit, with_vertices
    x = F.inputs("rand2k")
    upload(renderer, x["d"])
    rec = F.records("rand2k", "default")
    want = F.yardstick("rand2k", "default")[0]
    reps, n, k = 64, rec.shape[0], x["dirs"].shape[0]
    big = np.tile(rec, reps)
    side = torch.cuda.Stream()
    d_org = torch.from_numpy(big.view(np.uint8).reshape(-1).copy()).cuda()
    d_dirs = torch.from_numpy(rtamd.pack_fan_dirs(x["dirs"]).reshape(-1).copy()).cuda()
    d_masks = torch.full((2 * n * reps,), GUARD, dtype=torch.int32, device="cuda")
    b = load_golden("cornell12")
    torch.cuda.synchronize()
    # a fan of scene A, then at once, without synchronising, build_scene of scene B: the masks are A's
    renderer.trace_fan_device(d_org.data_ptr(), n * reps, d_dirs.data_ptr(), k, d_masks.data_ptr(), flags=STRICT,
                              stream=side.cuda_stream)
    renderer.build_scene({key: b[key] for key in MESH_KEYS}, max_leaf=2)
    side.synchronize()
    got = d_masks.cpu().numpy().view(np.uint32).reshape(2, reps, n)
    assert np.all(got == want[:, None, :]), "a fan in flight saw the scene that replaced its own"
    # after update_vertices the fan sees the refit scene: the oracle on the CPU-refit arrays
    h = F.inputs("hf40k")
    d = upload(renderer, h["d"])
    hrec = F.records("hf40k", "quarter")
    same_masks(renderer.trace_fan(hrec, h["dirs"], flags=STRICT), F.yardstick("hf40k", "quarter")[0], "hf40k before the update")
    verts = moved_vertices("hf40k")
    renderer.trace_fan_device(d_org.data_ptr(), n, d_dirs.data_ptr(), k, d_masks.data_ptr(), flags=STRICT, stream=side.cuda_stream)
    renderer.update_vertices(verts)                           # waits for the fan above
    nodes, _ = np_refit(d, verts)
    after = F.yardstick_for(with_vertices(d, verts, nodes), hrec, h["dirs"])
    assert not np.array_equal(after, F.yardstick("hf40k", "quarter")[0])
    same_masks(renderer.trace_fan(hrec, h["dirs"], flags=STRICT), after, "hf40k after the update")
    torch.cuda.synchronize()


# ---- refusals ----

def test_refusals_leave_the_context_usable(renderer):
    import torch
    L = rtamd.lib()
    rec = rtamd.pack_fan_origins(np.zeros((4, 3), np.float32))
    dirs = rtamd.pack_fan_dirs(np.ones((3, 3), np.float32))
    masks = np.full(4, GUARD, np.uint32)
    po, pd, pm = vp(rec), vp(dirs), vp(masks)
    fresh = rtamd.Renderer(0)
    try:
        assert L.rt_trace_fan(fresh._h, po, 4, pd, 3, 0, pm) == RT_ERR_NO_SCENE
        assert L.rt_trace_fan_device(fresh._h, po, 4, pd, 3, 0, pm, None) == RT_ERR_NO_SCENE
    finally:
        fresh.close()
    d = upload(renderer, load_golden("cornell12"))
    h = renderer._h
    d_org = torch.zeros(4 * 32 + 16, dtype=torch.uint8, device="cuda")
    d_dirs = torch.zeros(3 * 16 + 16, dtype=torch.uint8, device="cuda")
    d_masks = torch.full((4 + 2,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    do, dd, dm = d_org.data_ptr(), d_dirs.data_ptr(), d_masks.data_ptr()
    assert do % 16 == 0 and dd % 16 == 0 and dm % 4 == 0
    c = C.c_void_p
    for bad in (1, 8, 16, 32, 128, 256, 1 << 31, HW | STRICT, HW | ANY_HIT):
        assert L.rt_trace_fan(h, po, 4, pd, 3, bad, pm) == RT_ERR_INVALID_ARG, bad
        assert L.rt_trace_fan_device(h, c(do), 4, c(dd), 3, bad, c(dm), None) == RT_ERR_INVALID_ARG, bad
    for n in (-1, (1 << 26) + 1, 1 << 40):
        assert L.rt_trace_fan(h, po, n, pd, 3, 0, pm) == RT_ERR_INVALID_ARG, n
        assert L.rt_trace_fan_device(h, c(do), n, c(dd), 3, 0, c(dm), None) == RT_ERR_INVALID_ARG, n
    for k in (0, -1, rtamd.RT_FAN_MAX_DIRS + 1):
        assert L.rt_trace_fan(h, po, 4, pd, k, 0, pm) == RT_ERR_INVALID_ARG, k
        assert L.rt_trace_fan_device(h, c(do), 4, c(dd), k, 0, c(dm), None) == RT_ERR_INVALID_ARG, k
    assert L.rt_trace_fan(h, None, 4, pd, 3, 0, pm) == RT_ERR_INVALID_ARG
    assert L.rt_trace_fan(h, po, 4, None, 3, 0, pm) == RT_ERR_INVALID_ARG
    assert L.rt_trace_fan(h, po, 4, pd, 3, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_fan_device(h, None, 4, c(dd), 3, 0, c(dm), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_fan_device(h, c(do), 4, None, 3, 0, c(dm), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_fan_device(h, c(do), 4, c(dd), 3, 0, None, None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_fan_device(h, c(do + 4), 4, c(dd), 3, 0, c(dm), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_fan_device(h, c(do), 4, c(dd + 8), 3, 0, c(dm), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_fan_device(h, c(do), 4, c(dd), 3, 0, c(dm + 2), None) == RT_ERR_INVALID_ARG
    with pytest.raises(rtamd.RtError):
        renderer.trace_fan(np.zeros((4, 3)), np.ones((3, 3)), flags=ANY_HIT)
    assert L.rt_trace_fan(h, None, 0, None, 0, 0, None) == 0          # n == 0: RT_OK, nothing launched
    assert L.rt_trace_fan_device(h, None, 0, None, -7, 0, None, None) == 0
    torch.cuda.synchronize()
    assert np.all(masks == GUARD) and np.all(d_masks.cpu().numpy().view(np.uint32) == GUARD), "a refused call wrote masks"
    renderer.set_params(d["params"])
    out = renderer.render(int(d["w"]), int(d["h"]), depth=int(d["depth"]), flags=0)
    assert np.array_equal(out, d["ref_default"])


# ---- the tail case: more items than the grid has waves ----

def test_tail_16k_origins_256_directions(renderer):
    """cornell12's 128 x 128 quantised frame's hit points x 256 directions, 4.2 M rays, against the
    expanded query in slices of 2^20 rays; culling on, tmax a quarter of the diagonal.  12,841 of the
    frame's 16,384 pixels see the box; the others give their ray's origin on the image plane and a zero
    normal, so that the fan has the 16,384 origins (256 whole groups x 8 chunks) the case is about."""
    d = upload(renderer, scene_arrays("cornell12"))
    _, o, dirs = quantised_frame(d, 128, 128)
    origins, normals = F.hit_points(d, o, dirs, keep_misses=True)
    assert origins.shape[0] == 128 * 128 and 12000 < int(np.any(normals != 0, axis=1).sum()) < 16384
    rec = rtamd.pack_fan_origins(origins, normals, F.quarter_diagonal(d))
    table = F.fibonacci(256)
    got = renderer.trace_fan(rec, table)
    assert renderer.last_query_ms() > 0.0
    same_masks(got, query_masks(renderer, rec, table, 0), "tail")
    share = rtamd.fan_bits(got, 256).mean()
    assert 0.02 < share < 0.45
