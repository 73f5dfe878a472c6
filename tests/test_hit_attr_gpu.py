"""Ray queries with hit attributes on the GPU: Renderer.trace_rays_attr /
trace_rays_attr_device against the yardstick of tests/hit_attr_common.py (pinned to the oracle by
tests/test_hit_attr.py).  Records are compared as sixteen uint32 words; everything in S_strict is
exact.  S_ref and S_hw have no oracle: their id and t must be the plain query's, their paths (fast
quotient, division form, general kernel) must agree word for word, and their float fields are held
against S_strict's by a gross-error bound (test_ref_and_hw_against_strict)."""
import ctypes as C

import numpy as np
import pytest

import rtamd
import ray_edge_common as E
from conftest import load_golden
from hit_attr_common import (FLOAT_FIELDS, ID, T, assert_same_records, miss_words, oracle_frame, ray_words, ref_hit_attr,
                             ref_next_rays, words)
from ray_query_common import N_RAYS, TMAX_DEFAULT, quantised_frame, reference, scene_arrays
from test_ray_query_edges_gpu import general  # noqa: F401  (the split-records context, a module fixture)

pytestmark = pytest.mark.gpu

STRICT, HW, EXACT_DIV, NO_SHADOW = rtamd.RT_FLAG_STRICT_MATH, rtamd.RT_FLAG_HW_MATH, rtamd.RT_FLAG_EXACT_DIV, 1
ANY = rtamd.RT_FLAG_ANY_HIT
RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE = -1, -3
SCENES = ["cornell12", "rand2k", "rand4k_sbvh", "rand3k_bigleaf", "single_tri_rootleaf", "rand2k_built"]
MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")
GUARD = 0x5A5A5A5A
HDR_CLEAN = 13

# test_ref_and_hw_against_strict's bounds: 8 x the largest absolute difference from S_strict's field
# seen on the first GPU run over SCENES' incoherent rays, closest and any hit, S_ref and S_hw
# together (DESIGN.md 19 has the figures).  A gross-error check, not a precision claim.
MEASURED = {"t": 6.103515625e-05, "u": 8.64267349243164e-06, "v": 2.193450927734375e-05, "p": 6.866455078125e-05,
            "ndotd": 2.384185791015625e-07, "ng": 1.1920928955078125e-07, "ns": 1.7881393432617188e-07}
DEVIATION_BOUND = {k: 8.0 * v for k, v in MEASURED.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def put_scene(r, name):
    d = E.edge_scene(name)
    if name == "rand2k_built":
        r.build_scene({k: d[k] for k in MESH_KEYS}, max_leaf=2, keys="extent")
    else:
        r.upload(rtamd.Scene.from_arrays(d))
    return d


def attr(r, rays, flags=STRICT, any_hit=False):
    """rt_trace_rays_attr of packed rays through the C ABI: uint32 (n, 16)."""
    rays = np.ascontiguousarray(rays)
    n = ray_words(rays).shape[0]
    out = np.zeros((n, 16), np.uint32)
    rc = rtamd.lib().rt_trace_rays_attr(r._h, rays.ctypes.data_as(C.c_void_p), n, flags | (ANY if any_hit else 0),
                                        out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def plain(r, rays, flags=STRICT, any_hit=False):
    """rt_trace_rays of packed rays: (ids, t)."""
    rays = np.ascontiguousarray(rays)
    n = ray_words(rays).shape[0]
    hits = np.zeros(n, rtamd.HIT_DTYPE)
    rc = rtamd.lib().rt_trace_rays(r._h, rays.ctypes.data_as(C.c_void_p), n, flags | (ANY if any_hit else 0),
                                   hits.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return hits["id"].copy(), hits["t"].copy()


def yardstick(d, rays, any_hit=False):
    from oracle import oracle
    ids, t, _ = oracle.trace_rays(d, rays, any_hit=any_hit)
    return ref_hit_attr(d, rays, ids, t)


# ---- 1: incoherent rays against the yardstick ----

@pytest.mark.parametrize("name", SCENES)
def test_records_equal_the_yardstick(renderer, name):
    from oracle import oracle
    d = put_scene(renderer, name)
    o, dirs, ids, t, _, _ = reference(name)
    rays = rtamd.pack_rays(o, dirs)
    got = words(renderer.trace_rays_attr(o, dirs, flags=STRICT))
    assert got.shape == (N_RAYS, 16) and np.any(ids >= 0) and np.any(ids < 0)
    assert_same_records(got, ref_hit_attr(d, rays, ids, t), f"{name} closest")
    miss = ids < 0
    assert np.array_equal(got[miss], miss_words(rays)[miss]) and np.all(got[miss, T] == bits(TMAX_DEFAULT)[0])
    assert renderer.last_query_ms() > 0.0
    ai, at, _ = oracle.trace_rays(d, rays, any_hit=True)
    got = words(renderer.trace_rays_attr(o, dirs, any_hit=True, flags=STRICT))
    assert_same_records(got, ref_hit_attr(d, rays, ai, at), f"{name} any hit")
    assert np.array_equal(got[ai < 0], miss_words(rays)[ai < 0])


# ---- 2: id and t are the plain query's, in every arithmetic ----

@pytest.mark.parametrize("name", SCENES)
def test_id_and_t_are_the_plain_querys(renderer, name):
    put_scene(renderer, name)
    o, dirs, _, _, _, _ = reference(name)
    rays = rtamd.pack_rays(o, dirs)
    for flags in (0, HW, STRICT):
        for extra in (0, EXACT_DIV):
            for any_hit in (False, True):
                a = attr(renderer, rays, flags | extra, any_hit)
                ids, t = plain(renderer, rays, flags | extra, any_hit)
                what = f"{name} flags={flags | extra} any={any_hit}"
                assert np.array_equal(a[:, ID].view(np.int32), ids), what + ": ids"
                assert np.array_equal(a[:, T], bits(t)), what + ": t"
                assert np.any(ids >= 0)
                assert not a[:, 11].any() and not a[:, 15].any(), what + ": the reserved words are 0"


# ---- 3: sizes, guards, refusals ----

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_group_edges_write_nothing_past_n(renderer, n):
    import torch
    d = put_scene(renderer, "cornell12")
    o, dirs, ids, t, _, _ = reference("cornell12")
    rays = rtamd.pack_rays(o[:n + 3], dirs[:n + 3])           # more rays in memory than asked for
    want = ref_hit_attr(d, rays[:n], ids[:n], t[:n])
    hits = np.full((n + 2, 16), GUARD, np.uint32)             # two guard records after hits[n]
    rc = rtamd.lib().rt_trace_rays_attr(renderer._h, rays.ctypes.data_as(C.c_void_p), n, STRICT, hits.ctypes.data_as(C.c_void_p))
    assert rc == 0
    assert np.all(hits[n:] == GUARD), "the host form wrote past hits[n]"
    assert_same_records(hits[:n], want, f"host form n={n}")
    side = torch.cuda.Stream()
    host = torch.from_numpy(rays.view(np.uint8).reshape(-1)).pin_memory()
    d_rays = torch.zeros(rays.nbytes, dtype=torch.uint8, device="cuda")
    d_hits = torch.full(((n + 2) * 16,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_rays.copy_(host, non_blocking=True)                 # the rays are written on the side stream
        renderer.trace_rays_attr_device(d_rays.data_ptr(), n, d_hits.data_ptr(), flags=STRICT, stream=side.cuda_stream)
    side.synchronize()
    got = d_hits.cpu().numpy().view(np.uint32).reshape(n + 2, 16)
    assert np.all(got[n:] == GUARD), "the kernel wrote past hits[n]"
    assert_same_records(got[:n], want, f"device form n={n}")


def test_refusals_leave_the_context_usable(renderer):
    import torch
    L = rtamd.lib()
    fresh = rtamd.Renderer(0)
    rays = rtamd.pack_rays(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    hits = np.full((4, 16), GUARD, np.uint32)
    pr, ph = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    try:
        assert L.rt_trace_rays_attr(fresh._h, pr, 4, 0, ph) == RT_ERR_NO_SCENE
        assert L.rt_trace_rays_attr_device(fresh._h, pr, 4, 0, ph, None) == RT_ERR_NO_SCENE
    finally:
        fresh.close()
    d = put_scene(renderer, "cornell12")
    h = renderer._h
    d_rays = torch.zeros(4 * 32 + 16, dtype=torch.uint8, device="cuda")
    d_hits = torch.full((5 * 16,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dr, dh = d_rays.data_ptr(), d_hits.data_ptr()
    assert dr % 16 == 0 and dh % 16 == 0
    for bad in (1, 8, 16, 32, 256, 1 << 31, HW | STRICT):
        assert L.rt_trace_rays_attr(h, pr, 4, bad, ph) == RT_ERR_INVALID_ARG, bad
        assert L.rt_trace_rays_attr_device(h, C.c_void_p(dr), 4, bad, C.c_void_p(dh), None) == RT_ERR_INVALID_ARG, bad
    assert L.rt_trace_rays_attr(h, pr, -1, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_attr(h, pr, (1 << 30) + 1, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_attr(h, None, 4, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_attr(h, pr, 4, 0, None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_attr_device(h, None, 4, 0, C.c_void_p(dh), None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_attr_device(h, C.c_void_p(dr), 4, 0, None, None) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_attr_device(h, C.c_void_p(dr + 4), 4, 0, C.c_void_p(dh), None) == RT_ERR_INVALID_ARG
    for off in (4, 8):                                        # d_hits must be 16-byte aligned: 8 is rt_hit's, not this record's
        assert L.rt_trace_rays_attr_device(h, C.c_void_p(dr), 4, 0, C.c_void_p(dh + off), None) == RT_ERR_INVALID_ARG
    with pytest.raises(rtamd.RtError):
        renderer.trace_rays_attr(np.zeros((4, 3)), np.ones((4, 3)), flags=NO_SHADOW)
    assert L.rt_trace_rays_attr(h, None, 0, 0, None) == 0     # n == 0: RT_OK, nothing launched
    assert L.rt_trace_rays_attr_device(h, None, 0, 0, None, None) == 0
    torch.cuda.synchronize()
    assert np.all(hits == GUARD) and np.all(d_hits.cpu().numpy().view(np.uint32) == GUARD), "a refused call wrote hits"
    renderer.set_params(d["params"])
    out = renderer.render(int(d["w"]), int(d["h"]), depth=int(d["depth"]), flags=0)
    assert np.array_equal(out, d["ref_default"])


# ---- 4: more rays than the grid has lanes ----

def test_more_rays_than_lanes(renderer):
    """1024 x 1024 (power-of-two sides keep the rays exact; more than the 524,288 lanes of the largest
    resident grid): some wave takes a second group, after its LDS rows staged the first group's records."""
    d = put_scene(renderer, "cornell12")
    _, o, dirs = quantised_frame(d, 1024, 1024)
    assert o.shape[0] > 256 * 2048, "some wave must take a second group"
    rays = rtamd.pack_rays(o, dirs)
    want = yardstick(d, rays)
    assert int((want[:, ID].view(np.int32) >= 0).sum()) > 100000
    assert_same_records(attr(renderer, rays), want, "1024 x 1024")
    perm = np.random.default_rng(19).permutation(rays.shape[0])
    assert_same_records(attr(renderer, rays[perm]), want[perm], "1024 x 1024 permuted")


# ---- 5: continuing the frame's path from the GPU's records ----

@pytest.mark.parametrize("name", ["cornell12", "rand2k"])
def test_records_continue_the_gpu_frame(renderer, name):
    f = oracle_frame(name)
    d, p, rays = f["d"], f["params"], f["rays"]
    put_scene(renderer, name)
    renderer.set_params(p)
    g = renderer.render(64, 64, depth=2, flags=STRICT, aux=True)
    a = attr(renderer, rays)
    traced = g["hits"][:, 0, 0] != -2
    hit = g["hits"][:, 0, 0] >= 0
    assert np.array_equal(a[traced, ID].view(np.int32), g["hits"][traced, 0, 0])
    assert np.array_equal(a[hit, T], bits(g["t"][hit, 0]))
    only = a.copy()
    only[~hit] = miss_words(rays)[~hit]                       # continue the frame's pixels only
    refl, shadow = ref_next_rays(rays, only, p[16:19])
    ids1, t1 = plain(renderer, refl)
    assert int((g["hits"][hit, 1, 0] >= 0).sum()) >= 100
    assert np.array_equal(ids1[hit], g["hits"][hit, 1, 0]), f"{name}: bounce-1 ids"
    assert np.array_equal(bits(t1[hit]), bits(g["t"][hit, 1])), f"{name}: bounce-1 t"
    sid, _ = plain(renderer, shadow, any_hit=True)
    assert int((g["hits"][hit, 0, 1] >= 0).sum()) >= 100
    assert np.array_equal(sid[hit], g["hits"][hit, 0, 1]), f"{name}: bounce-0 shadow ids"


# ---- 6: invalid and barred rays ----

def test_invalid_rays_get_the_miss_record_and_leave_their_neighbours(renderer):
    d = put_scene(renderer, "cornell12")
    o, dirs, ids, t, _, _ = reference("cornell12")
    n, lanes = 128, (0, 31, 63)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    payload = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    cases = {                                                 # name -> (field, component or None, value)
        "nan origin": ("o", 1, nan), "inf origin": ("o", 2, inf), "-inf origin": ("o", 0, -inf),
        "nan direction": ("d", 0, nan), "inf direction": ("d", 1, inf), "zero direction": ("d", None, 0.0),
        "nan tmax": ("tmax", None, payload), "zero tmax": ("tmax", None, 0.0), "negative tmax": ("tmax", None, -5.0),
        "tmax at tmin": ("tmax", None, np.float32(0.001)),
    }
    assert all(ids[lane] >= 0 for lane in lanes), "the barred lanes would have hit"
    keep = np.setdiff1d(np.arange(n), lanes)
    for flags in (STRICT, 0):
        base = attr(renderer, rtamd.pack_rays(o[:n], dirs[:n]), flags)
        if flags == STRICT:
            assert_same_records(base, ref_hit_attr(d, rtamd.pack_rays(o[:n], dirs[:n]), ids[:n], t[:n]), "valid rays")
        for label, (field, comp, val) in cases.items():
            rays = rtamd.pack_rays(o[:n], dirs[:n])
            for lane in lanes:
                if field == "tmax":
                    rays["tmax"].view(np.uint32)[lane] = np.float32(val).view(np.uint32)
                elif comp is None:
                    rays[field][lane] = val
                else:
                    rays[field][lane, comp] = val
            got = attr(renderer, rays, flags)
            assert np.array_equal(got[list(lanes)], miss_words(rays)[list(lanes)]), f"{label} flags={flags}: not the miss record"
            assert_same_records(got[keep], base[keep], f"{label} flags={flags}: the neighbours")
        # tmax = t*: the hit itself is barred
        rays = rtamd.pack_rays(o[:n], dirs[:n])
        tstar = base[list(lanes), T]
        rays["tmax"].view(np.uint32)[list(lanes)] = tstar
        got = attr(renderer, rays, flags)
        assert np.array_equal(got[list(lanes)], miss_words(rays)[list(lanes)]), f"tmax = t* flags={flags}"
        assert np.array_equal(got[list(lanes), T], tstar)
        assert_same_records(got[keep], base[keep], f"tmax = t* flags={flags}: the neighbours")


# ---- 7: the general kernel ----

def three_paths(renderer, g, rays, flags, any_hit):
    return [("fast", attr(renderer, rays, flags, any_hit)), ("EXACT_DIV", attr(renderer, rays, flags | EXACT_DIV, any_hit)),
            ("general", attr(g, rays, flags, any_hit))]


@pytest.mark.parametrize("name", ["rand2k", "rand3k_bigleaf", "bad_node"])
def test_general_kernel(renderer, general, name):  # noqa: F811
    """query_attr_kernel<ANY, false>: on the split-records context (its fixture asserts the split), and
    for bad_node, which is not clean, on the normal context too."""
    from refit_common import scene_image
    d = put_scene(renderer, name)
    g = general(d)
    if name == "bad_node":
        assert scene_image(renderer)[HDR_CLEAN] == 0
        o, dirs, tm = E.ray_class("bad_node", "malformed")
    else:
        o, dirs, tm = E.ray_class(name, "incoherent")
    rays = rtamd.pack_rays(o, dirs, tm)
    for any_hit in (False, True):
        want = yardstick(d, rays, any_hit)
        assert int((want[:, ID].view(np.int32) >= 0).sum()) > 100
        for label, got in three_paths(renderer, g, rays, STRICT, any_hit):
            assert_same_records(got, want, f"{name} strict any={any_hit} {label}")
        for flags in (0, HW):
            paths = three_paths(renderer, g, rays, flags, any_hit)
            for label, got in paths[1:]:
                assert_same_records(got, paths[0][1], f"{name} flags={flags} any={any_hit} {label} vs fast")
    if name == "bad_node":
        put_scene(renderer, "cornell12")


# ---- 8: restarted rays ----

def test_restarted_rays(renderer):
    d = E.deep_comb40()
    renderer.upload(rtamd.Scene.from_arrays(d))
    o, dirs, tm = E.ray_class("deep_comb40", "incoherent")
    rays = rtamd.pack_rays(o, dirs, tm)
    want = yardstick(d, rays)
    assert int((want[:, ID].view(np.int32) >= 0).sum()) > 100
    before = renderer.overflow_count()
    assert_same_records(attr(renderer, rays), want, "deep_comb40")
    assert renderer.last_deferred() > 0 and renderer.overflow_count() == before
    assert_same_records(attr(renderer, rays, any_hit=True), yardstick(d, rays, True), "deep_comb40 any hit")
    assert renderer.last_deferred() > 0


# ---- 9: after update_vertices; a scene replaced behind a query ----

def test_after_update_vertices_and_before_a_scene_replacement(renderer):
    import torch
    from refit_common import moved_vertices, np_refit, with_vertices
    d = put_scene(renderer, "hf40k")
    o, dirs, _, _, _, _ = reference("hf40k")
    rays = rtamd.pack_rays(o, dirs)
    assert_same_records(attr(renderer, rays), yardstick(d, rays), "hf40k before the update")
    verts = moved_vertices("hf40k")
    rng = np.random.default_rng(9)
    normals = np.array(d["normals"], np.float32, copy=True)
    normals[:, :3] += rng.uniform(-0.3, 0.3, (normals.shape[0], 3)).astype(np.float32)
    renderer.update_vertices(verts, normals)
    nodes, _ = np_refit(d, verts)
    e = with_vertices(d, verts, nodes)
    e["normals"] = normals
    want = yardstick(e, rays)
    assert not np.array_equal(want, yardstick(d, rays))
    assert_same_records(attr(renderer, rays), want, "hf40k after the update")
    # a query of this scene, then at once, without synchronising, build_scene of another: the records are this scene's
    reps = 64
    side = torch.cuda.Stream()
    big = torch.from_numpy(np.tile(rays, reps).view(np.uint8).reshape(-1)).cuda()
    big_hits = torch.full((16 * N_RAYS * reps,), -7, dtype=torch.int32, device="cuda")
    b = load_golden("cornell12")
    torch.cuda.synchronize()
    renderer.trace_rays_attr_device(big.data_ptr(), N_RAYS * reps, big_hits.data_ptr(), flags=STRICT, stream=side.cuda_stream)
    renderer.build_scene({k: b[k] for k in MESH_KEYS}, max_leaf=2)
    side.synchronize()
    got = big_hits.cpu().numpy().view(np.uint32).reshape(reps, N_RAYS, 16)
    assert np.all(got == want[None, :, :]), "a query in flight saw the scene that replaced its own"
    torch.cuda.synchronize()


# ---- 10: S_ref and S_hw against S_strict ----

def deviations(renderer, name):
    """Per float field, the largest absolute difference of S_ref's and S_hw's records from S_strict's on
    `name`'s incoherent rays (closest and any hit) where the ids agree, and the largest share of rays
    left out because they do not."""
    put_scene(renderer, name)
    o, dirs, _, _, _, _ = reference(name)
    rays = rtamd.pack_rays(o, dirs)
    worst = {k: 0.0 for k in FLOAT_FIELDS}
    left_out = 0.0
    for any_hit in (False, True):
        s = attr(renderer, rays, STRICT, any_hit)
        for flags in (0, HW):
            a = attr(renderer, rays, flags, any_hit)
            both = (a[:, ID] == s[:, ID]) & (s[:, ID].view(np.int32) >= 0)
            left_out = max(left_out, float(np.mean(a[:, ID] != s[:, ID])))
            assert np.array_equal(a[(a[:, ID] == s[:, ID]) & ~both], s[(a[:, ID] == s[:, ID]) & ~both]), "misses are the same words"
            for k, cols in FLOAT_FIELDS.items():
                if np.any(both):
                    diff = np.abs(a[both][:, cols].view(np.float32).astype(np.float64) - s[both][:, cols].view(np.float32).astype(np.float64))
                    worst[k] = max(worst[k], float(diff.max()))
    return worst, left_out


@pytest.mark.parametrize("name", SCENES)
def test_ref_and_hw_against_strict(renderer, name):
    worst, left_out = deviations(renderer, name)
    print(name, "largest |S_ref or S_hw - S_strict| per field:", worst, "share of ids that differ:", left_out)
    assert left_out <= 0.01, f"{name}: {left_out:.4f} of the ids differ between arithmetics"
    for k, v in worst.items():
        assert np.isfinite(v) and v <= DEVIATION_BOUND[k], f"{name}: {k} differs from S_strict's by {v} > {DEVIATION_BOUND[k]}"
