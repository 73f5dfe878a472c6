"""The trimmed traversal trip: the wave-uniform prologue whose slab test reads the
record from SGPR pairs and whose loop is uniform, the main loop's offset select next to the leaf
compare, the child-ref load inside the inner step's region, and the decode's 32-bit shift-adds.
None of it may change a lane's arithmetic, visit order or fetches, so every comparison is exact.

The shapes stand where the changed code branches:
  rand2k at 13 x 7 and 8 x 8     partial waves and exactly full ones (a tile is 8 x 8)
  single_tri_rootleaf            the prologue ends before its first trip (the root is a leaf)
  two_far_leaves                 one inner node whose two leaf boxes lie behind every ray: each lane
                                 misses both in the prologue's first trip and is done, the main loop
                                 runs no trip
  rand3k_bigleaf                 (its largest leaf has 7 triangles, see test_trip_paths_gpu.py)
  escape40                       refit_common's big-leaf tree: leaves of 40 and 35 triangles through
                                 the decode's table path, one of 3, and an EMPTY leaf
  degenerate_leaf1               mesh_edge_common's degenerate mesh (a third of its triangles points,
                                 a third segments) on the host twin's tree at max_leaf 1: every leaf
                                 holds one triangle, many of them of no area
  overflow_comb, bad_node        restart with the general traversal; the general path from the start
  rand2k_axis_33x33              an axis-aligned camera: column and row 17 have a direction component
                                 of exactly 0: MODE 1 in S_strict / S_hw, and the division form under
                                 RT_FLAG_EXACT_DIV (a case like the others, plus a test of its own)
  four cameras in one batch

Per case: S_strict equals the CPU oracle in every word (packed pixels, hit ids, t, rgb) through the
single-frame, batch, wavefront (depth 2, where the bounce kernels run) and query kernels; S_ref and
S_hw give the same frame single, batched and on the wavefront path, and S_ref equals the general
traversal of a split-records context, which shares none of the fast loops; rt_fetch_counts equals the
oracle's visits; and, where the reference kernel's code objects travelled with the snapshot
(oracle/_ref), the depth-3 frame (the depth the reference is compiled at) in S_ref equals the reference
kernel as its host builds it and in S_hw its correctly rounded build, run live, fused and wavefront
(every case but the axis-aligned camera, on which the reference kernel does not reproduce itself: LIVE).
(The empty leaf and the escape leaves come from refit_common's tree: mesh_edge_common.py has one-triangle
leaves and triangles of no area, but no leaf without a triangle.)
Restarted traversals are not counted and an unclean scene has no counting kernel: overflow_comb's
counts are bounded by the oracle's, bad_node's are refused."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

STRICT, HW, EXACT_DIV, NO_SHADOW, WAVEFRONT, WF_SORT = 64, 2, 4, 1, 8, 32
MODES = {"ref": 0, "hw": HW, "strict": STRICT}
CASES = {"rand2k_13x7": (13, 7), "rand2k_8x8": (8, 8), "single_tri_rootleaf": (32, 32), "two_far_leaves": (16, 16),
         "rand3k_bigleaf": (64, 64), "escape40": (64, 64), "degenerate_leaf1": (64, 64), "overflow_comb": (64, 64),
         "bad_node": (64, 64), "rand2k_axis_33x33": (33, 33)}
RESTARTS = ("overflow_comb",)
UNCLEAN = ("bad_node",)

_SCENES = {}
_ORACLE = {}


def _axis_params(d):
    """The eye on the z axis looking down it, image plane 100 x 100 at z = 120: with an odd frame
    size the middle column and row have image_pos.x == campos.x (y) exactly."""
    p = np.zeros((8, 4), np.float32)
    p[:, 3] = 1
    p[0, :3] = [100, 0, 0]
    p[1, :3] = [0, 100, 0]
    p[2, :3] = [-50, -50, 120]
    p[3, :3] = [0, 0, 220]
    p[4, :3] = [-23, 200, 3]
    p[5, :3] = [1, 1, 1]
    p[6, :3] = d["scene_min"]
    p[7, :3] = d["scene_max"]
    return p.reshape(-1)


def _scene_dict(name):
    """Scene arrays and params of a case (shared; do not modify)."""
    if name in _SCENES:
        return _SCENES[name]
    import rtamd
    if name == "rand2k_axis_33x33":
        d = load_golden("rand2k")
        d["params"] = _axis_params(d)
    elif name.startswith("rand2k_"):
        d = load_golden("rand2k")
    elif name == "two_far_leaves":
        # two small triangles behind the eye of the axis-aligned camera, which looks down -z from z = 220
        v = np.array([[10, 10, 300, 1], [12, 10, 300, 1], [10, 12, 300, 1],
                      [-30, -20, 320, 1], [-28, -20, 320, 1], [-30, -18, 321, 1]], np.float32)
        m = rtamd.Mesh.from_arrays(v, np.arange(6, dtype=np.int32))
        d = rtamd.Scene.from_mesh(m, m.build_bvh(1)).arrays()
        ni = np.asarray(d["nodes"]).view(np.int32).reshape(-1, 12)
        assert ni.shape[0] == 3 and ni[0, 8] >= 0 and np.all(ni[1:, 8] < 0), "one inner node over two leaves"
        p = _axis_params(d)
        p[24:27], p[28:31] = (-400, -400, -400), (400, 400, 400)   # the scene box every ray enters
        d["params"] = p
    elif name == "escape40":
        from refit_common import scene_arrays
        d = dict(scene_arrays("bigleaf"))
        m = rtamd.Mesh.from_arrays(d["vertices"], d["indices"])
        d["params"] = rtamd.params_to_array(m.camera_params(64, 64, radius=90.0))   # every ray enters the tree
        ni = np.asarray(d["nodes"]).view(np.int32).reshape(-1, 12)
        assert sorted(ni[ni[:, 8] < 0][:, 11].tolist()) == [0, 3, 35, 40]
    elif name == "degenerate_leaf1":
        from mesh_edge_common import arrays, mesh, twin
        nodes, refs = twin("degenerate", 1)
        d = dict(arrays("degenerate"), nodes=nodes, tri_indices=refs)
        ni = np.asarray(nodes).view(np.int32).reshape(-1, 12)
        assert np.all(ni[ni[:, 8] < 0][:, 11] == 1), "every leaf holds one triangle"
        d["scene_min"], d["scene_max"] = nodes[0, 0:3].copy(), nodes[0, 4:7].copy()
        # the orbit camera far enough to see all of the mesh, the scene box the root's (as test_mesh_edges_gpu.py)
        v, i = mesh("degenerate")
        m = rtamd.Mesh.from_arrays(v, i)
        p = rtamd.params_to_array(m.camera_params(64, 64, radius=max(200.0, 1.5 * float(np.ptp(v[:, :3], axis=0).max()))))
        p = np.array(p, np.float32, copy=True)
        p[24:27], p[28:31] = nodes[0, 0:3], nodes[0, 4:7]
        d["params"] = p
    else:
        d = load_golden(name)
    _SCENES[name] = d
    return d


def _oracle(name, params, w, h, depth, flags=0):
    """The oracle's frame, computed once per (case, camera, size, depth) (shared; do not modify)."""
    from oracle import oracle
    key = (name, np.asarray(params, np.float32).tobytes(), w, h, depth, flags)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.render(_scene_dict(name), params, w, h, depth=depth, flags=flags)
    return _ORACLE[key]


def _cams(d, k):
    """k distinct cameras: the case's own, moved sideways (eye and image plane together)."""
    cams = []
    for i in range(k):
        p = np.array(d["params"], np.float32, copy=True).reshape(8, 4)
        shift = np.array([3.0 * i, -2.0 * i, 1.5 * i], np.float32)
        p[2, :3] += shift
        p[3, :3] += shift
        cams.append(p.reshape(-1))
    return cams


def _compare(got, ref, label):
    assert np.array_equal(got["hits"], ref["hits"]), f"{label}: hit ids differ at " \
        f"{np.argwhere(got['hits'] != ref['hits'])[:5].tolist()}"
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)), f"{label}: t differs"
    assert np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), f"{label}: rgb not bitwise"
    assert np.array_equal(got["out"], ref["out"]), f"{label}: packed pixels differ"


def _batch(r, cams, w, h, flags):
    import torch
    out = torch.full((len(cams) * w * h,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.render_device_batch(w, h, 1, flags, cams, out.data_ptr(), w * h)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(len(cams), w * h)


def _put(r, name):
    import rtamd
    d = _scene_dict(name)
    r.upload(rtamd.Scene.from_arrays(d))
    return d


@pytest.fixture(scope="module")
def general():
    """A second context whose uploads take the general traversal (split records)."""
    import os
    import rtamd
    r = rtamd.Renderer(0)

    def upload(d):
        old = os.environ.get("RTAMD_RECORD_LIMIT")
        os.environ["RTAMD_RECORD_LIMIT"] = "64"
        try:
            r.upload(rtamd.Scene.from_arrays(d))
        finally:
            if old is None:
                del os.environ["RTAMD_RECORD_LIMIT"]
            else:
                os.environ["RTAMD_RECORD_LIMIT"] = old
        return r
    yield upload
    r.close()


@pytest.mark.parametrize("name", list(CASES))
def test_strict_frames_equal_the_oracle_on_every_path(renderer, name):
    """Single frame at depth 1 (first_bounce_kernel) and 2 (the fused kernel), the wavefront path at
    depth 2 with and without the bounce sort, and a batch of four distinct cameras."""
    d = _put(renderer, name)
    w, h = CASES[name]
    p = d["params"]
    renderer.set_params(p)
    ref1 = _oracle(name, p, w, h, 1)
    if name == "two_far_leaves":
        assert np.all(ref1["hits"][:, 0, 0] == -1), "every ray enters the scene box and misses"
    elif name == "overflow_comb":
        assert ref1["stats"]["stack_overflow"] > 0   # every traversal restarts and then overflows: no hit
    else:
        assert int((ref1["hits"][:, 0, 0] >= 0).sum()) > 0, "the camera sees nothing"
    _compare(renderer.render(w, h, depth=1, flags=STRICT, aux=True), ref1, f"{name} depth 1")
    restarts = renderer.last_deferred()
    assert (restarts > 0) == (name in RESTARTS), restarts
    ref2 = _oracle(name, p, w, h, 2)
    _compare(renderer.render(w, h, depth=2, flags=STRICT, aux=True), ref2, f"{name} depth 2 fused")
    for sort in (0, WF_SORT):
        _compare(renderer.render(w, h, depth=2, flags=STRICT | WAVEFRONT | sort, aux=True), ref2,
                 f"{name} depth 2 wavefront sort {sort}")
    _compare(renderer.render(w, h, depth=1, flags=STRICT | WAVEFRONT, aux=True), ref1, f"{name} depth 1 wavefront")
    cams = _cams(d, 4)
    frames = _batch(renderer, cams, w, h, STRICT)
    for i, c in enumerate(cams):
        assert np.array_equal(frames[i], _oracle(name, c, w, h, 1)["out"]), f"{name}: batch frame {i} vs the oracle"


@pytest.mark.parametrize("name", list(CASES))
def test_ref_and_hw_agree_across_kernels_and_with_the_general_traversal(renderer, general, name):
    """S_ref and S_hw: single == batch == wavefront at depth 1, fused == wavefront at depth 2, and
    every S_ref and S_hw frame equals the split-records context's (the general traversal's)."""
    d = _put(renderer, name)
    g = general(d)
    w, h = CASES[name]
    cams = _cams(d, 4)
    for mode in ("ref", "hw"):
        f = MODES[mode]
        singles = []
        for i, c in enumerate(cams):
            renderer.set_params(c)
            g.set_params(c)
            one = renderer.render(w, h, depth=1, flags=f, aux=True)
            _compare(one, g.render(w, h, depth=1, flags=f, aux=True), f"{name} {mode} cam {i} vs the general traversal")
            _compare(renderer.render(w, h, depth=1, flags=f | WAVEFRONT, aux=True), one, f"{name} {mode} cam {i} wavefront")
            singles.append(one["out"])
        for call in range(2):   # the static block order, then the adaptive one
            frames = _batch(renderer, cams, w, h, f)
            for i in range(4):
                assert np.array_equal(frames[i], singles[i]), (name, mode, call, i)
        renderer.set_params(cams[0])
        g.set_params(cams[0])
        fused = renderer.render(w, h, depth=2, flags=f, aux=True)
        _compare(fused, g.render(w, h, depth=2, flags=f, aux=True), f"{name} {mode} depth 2 vs the general traversal")
        for sort in (0, WF_SORT):
            _compare(renderer.render(w, h, depth=2, flags=f | WAVEFRONT | sort, aux=True), fused,
                     f"{name} {mode} depth 2 wavefront sort {sort}")


def _query_rays(d):
    """130 coherent rays (two full waves and two lanes: neighbouring origins, one target, so a wave
    shares the top of the tree and its octant), 66 incoherent ones and 192 with a zero component."""
    import rtamd
    from ray_query_common import incoherent_rays, scene_box
    lo, hi = scene_box(d)
    mid, ext = (lo + hi) * np.float32(0.5), float(np.max(hi - lo)) + 1.0
    k = np.arange(130)
    o = (mid + np.array([0.9, 0.7, 1.3], np.float32) * np.float32(ext)).astype(np.float32)[None, :] + \
        np.stack([(k % 8) * 0.25, (k // 8) * 0.25, np.zeros(130)], 1).astype(np.float32) * np.float32(ext / 64)
    o = o.astype(np.float32)
    dirs = (mid[None, :] - o).astype(np.float32)
    io, idirs, _ = incoherent_rays(d, n=66)
    # 3 x 64 rays along an axis plane: one direction component exactly 0 in every lane of a wave (x, y,
    # z in turn), the other two aimed through the box
    zo, zd = [], []
    for axis in range(3):
        for j in range(64):
            t = mid + (np.array([(j % 8) - 3.5, (j // 8) - 3.5, ((j * 5) % 8) - 3.5], np.float32) * np.float32(ext / 24))
            dv = np.array([0.7, -0.5, 0.6], np.float32) * np.float32(ext)
            dv[axis] = 0.0
            zo.append((t - dv).astype(np.float32))
            zd.append(dv)
    zo, zd = np.array(zo, np.float32), np.array(zd, np.float32)
    assert np.all((zd == 0.0).sum(1) == 1)
    return rtamd.pack_rays(np.concatenate([o, io, zo]), np.concatenate([dirs, idirs, zd]))


@pytest.mark.parametrize("name", list(CASES))
def test_queries_equal_the_oracle(renderer, general, name):
    """query_kernel, closest and any hit: S_strict equals the oracle; S_ref and S_hw equal the
    general kernel of the split-records context."""
    from oracle import oracle
    d = _put(renderer, name)
    g = general(d)
    rays = _query_rays(d)
    o, dirs, tmax = rays["o"], rays["d"], rays["tmax"]
    for any_hit in (False, True):
        oi, ot, _ = oracle.trace_rays(d, rays, any_hit=any_hit)
        assert name in ("two_far_leaves", "overflow_comb") or np.any(oi >= 0)
        gi, gt = renderer.trace_rays(o, dirs, tmax=tmax, any_hit=any_hit, flags=STRICT)
        assert np.array_equal(gi, oi), f"{name} any_hit {any_hit}: ids differ at {np.flatnonzero(gi != oi)[:5]}"
        assert np.array_equal(gt.view(np.uint32), ot.view(np.uint32)), f"{name} any_hit {any_hit}: t differs"
        for mode in ("ref", "hw"):
            a = renderer.trace_rays(o, dirs, tmax=tmax, any_hit=any_hit, flags=MODES[mode])
            b = g.trace_rays(o, dirs, tmax=tmax, any_hit=any_hit, flags=MODES[mode])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (name, mode, any_hit)


@pytest.mark.parametrize("name", list(CASES))
def test_fetch_counts_are_the_oracles_visits(renderer, name):
    """As test_render_gpu.py asserts for its fixtures: in S_strict the inner-record fetches are exactly
    the oracle's inner visits and the triangle-record fetches its triangle tests plus at most one per
    leaf visit (an empty leaf's one dropped test), at depth 1 and on the wavefront path at depth 2."""
    import rtamd
    d = _put(renderer, name)
    w, h = CASES[name]
    renderer.set_params(d["params"])
    if name in UNCLEAN:
        with pytest.raises(rtamd.RtError):
            renderer.fetch_counts(w, h, 1, STRICT)
        return
    for depth, flags in ((1, STRICT), (2, STRICT | WAVEFRONT), (2, STRICT | WAVEFRONT | WF_SORT)):
        fr = renderer.fetch_counts(w, h, depth, flags)
        st = _oracle(name, d["params"], w, h, depth)["stats"]
        kinds = ("primary", "shadow", "secondary")
        inner = sum(st[k]["inner"] for k in kinds)
        tris = sum(st[k]["tris"] for k in kinds)
        leaves = sum(st[k]["leaf"] for k in kinds)
        print(f"{name} depth {depth} flags {flags}: inner {fr['inner']} / {inner}, tri {fr['tri']} / {tris} + {leaves} leaves, "
              f"restarts {renderer.last_deferred()}")
        if name in RESTARTS:   # a restarted traversal's fetches are not counted
            assert renderer.last_deferred() > 0 and fr["inner"] <= inner and fr["tri"] <= tris + leaves
            continue
        assert renderer.last_deferred() == 0
        assert fr["inner"] == inner, (depth, flags)
        assert tris <= fr["tri"] <= tris + leaves, (depth, flags)
        # (a prologue fetch is a lane fetch and a wave-distinct record but no quad request)
        assert fr["quad_inner"] <= fr["inner"] and fr["distinct_inner"] <= fr["inner"]
        assert fr["distinct_tri"] <= fr["quad_tri"] <= fr["tri"]
        assert fr["mixed_instructions"] <= fr["wave_instructions"]
        if name == "two_far_leaves":   # prologue only: the vector path fetched nothing
            assert fr["quad_inner"] == 0 and fr["tri"] == 0 and fr["inner"] == w * h, fr


def test_axis_aligned_camera_runs_mode_1_and_the_division_form(renderer):
    """rand2k_axis_33x33 beyond what every case gets: the division form.  S_strict under
    RT_FLAG_EXACT_DIV equals the oracle, single frame, batch and queries (the zero-component rays
    among them); in S_ref and S_hw the fast quotient equals RT_FLAG_EXACT_DIV (every traversal through
    the division form), single frame, wavefront, batch and queries.  The counting kernels are about
    the fast quotient's loops: rt_fetch_counts refuses RT_FLAG_EXACT_DIV (the case's counts without it
    are in test_fetch_counts_are_the_oracles_visits)."""
    import rtamd
    from oracle import oracle
    name = "rand2k_axis_33x33"
    d = _put(renderer, name)
    w, h = CASES[name]
    p = d["params"]
    renderer.set_params(p)
    ref = _oracle(name, p, w, h, 1)
    assert int((ref["hits"][:, 0, 0] >= 0).sum()) > 0
    _compare(renderer.render(w, h, depth=1, flags=STRICT | EXACT_DIV, aux=True), ref, "axis-aligned S_strict, division form")
    assert renderer.last_deferred() == 0
    ref2 = _oracle(name, p, w, h, 2)
    _compare(renderer.render(w, h, depth=2, flags=STRICT | EXACT_DIV | WAVEFRONT, aux=True), ref2,
             "axis-aligned S_strict wavefront, division form")
    cams = _cams(d, 4)
    frames = _batch(renderer, cams, w, h, STRICT | EXACT_DIV)
    for i, c in enumerate(cams):
        assert np.array_equal(frames[i], _oracle(name, c, w, h, 1)["out"]), f"batch frame {i}, division form, vs the oracle"
    with pytest.raises(rtamd.RtError):
        renderer.fetch_counts(w, h, 1, STRICT | EXACT_DIV)
    rays = _query_rays(d)
    o, dirs, tmax = rays["o"], rays["d"], rays["tmax"]
    for any_hit in (False, True):
        oi, ot, _ = oracle.trace_rays(d, rays, any_hit=any_hit)
        assert np.any(oi[-192:] >= 0), "some zero-component ray hits"
        gi, gt = renderer.trace_rays(o, dirs, tmax=tmax, any_hit=any_hit, flags=STRICT | EXACT_DIV)
        assert np.array_equal(gi, oi) and np.array_equal(gt.view(np.uint32), ot.view(np.uint32)), f"queries, division form, any_hit {any_hit}"
        for flags in (0, HW):
            a = renderer.trace_rays(o, dirs, tmax=tmax, any_hit=any_hit, flags=flags)
            b = renderer.trace_rays(o, dirs, tmax=tmax, any_hit=any_hit, flags=flags | EXACT_DIV)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (flags, any_hit)
    for flags in (0, HW):
        renderer.set_params(p)
        fast = renderer.render(w, h, depth=1, flags=flags, aux=True)
        _compare(fast, renderer.render(w, h, depth=1, flags=flags | EXACT_DIV, aux=True), f"axis-aligned flags {flags}")
        fast2 = renderer.render(w, h, depth=2, flags=flags | WAVEFRONT, aux=True)
        _compare(fast2, renderer.render(w, h, depth=2, flags=flags | WAVEFRONT | EXACT_DIV, aux=True), f"axis-aligned wavefront flags {flags}")
        frames = _batch(renderer, [p, p], w, h, flags)
        assert np.array_equal(frames[0], fast["out"]) and np.array_equal(frames[1], fast["out"])
        frames = _batch(renderer, [p, p], w, h, flags | EXACT_DIV)
        assert np.array_equal(frames[0], fast["out"]) and np.array_equal(frames[1], fast["out"])


# The reference kernel does not reproduce ITSELF on the axis-aligned camera: three live runs of it on
# rand2k_axis_33x33 disagree with each other on 11 of the 1,089 pixels (default build) and on 30 (strict
# build), other pixels from run to run, and a frame of this library, which is the same every run, then
# differs from one reference run in 9 to 22 pixels -- the parent library's frame exactly as this one's.
# A frame that changes from run to run is no yardstick for a pixel-exact comparison, so that camera's
# S_ref and S_hw frames are held to the general traversal and to RT_FLAG_EXACT_DIV (above) and to the
# oracle in S_strict; every other case is compared with the reference here.
LIVE = [n for n in CASES if n != "rand2k_axis_33x33"]


@pytest.mark.parametrize("name", LIVE)
def test_ref_and_hw_equal_the_reference_kernel_run_live(renderer, name, tmp_path):
    """The depth-3 frame (the reference kernel's compiled-in depth, with its shadow ray) in S_ref against
    the reference kernel as its host builds it, and in S_hw against its correctly rounded build, run
    live in a process of its own: no differing pixel, through the fused kernel and the wavefront path."""
    from oracle import ref_ocl
    if not ref_ocl.available():
        pytest.skip("oracle/_ref (the reference kernel's code objects) not in this snapshot")
    d = _put(renderer, name)
    w, h = CASES[name]
    renderer.set_params(d["params"])
    for mode, f, variant in (("S_ref", 0, "default"), ("S_hw", HW, "strict")):
        ref = ref_ocl.render_subprocess(d, d["params"], w, h, variant, str(tmp_path), timeout=120)
        for what, extra in (("fused", 0), ("wavefront", WAVEFRONT)):
            out = renderer.render(w, h, depth=3, flags=f | extra)
            nd = int(np.sum(out != ref))
            print(f"{name} {mode} {what} vs the reference kernel ({variant}): {nd} of {out.size} pixels differ")
            assert nd == 0, f"{name} {mode} {what}: first at {np.flatnonzero(out != ref)[:5]}"


def test_a_leaf_past_2_to_the_24_records(renderer):
    """The decode multiplies a 26-bit reference offset by 48: a 24-bit multiply is wrong from 2^24
    records on.  The 8 x 8 frame of rand2k with 2^24 + 5 padding references in front of every leaf
    range (about 0.8 GB of triangle records, one allocation) equals the unpadded scene's in every
    arithmetic, and the oracle's in S_strict."""
    import rtamd
    d = _scene_dict("rand2k_8x8")
    w, h = 8, 8
    base = rtamd.Scene.from_arrays(d)
    renderer.upload(base)
    renderer.set_params(d["params"])
    want = {m: renderer.render(w, h, depth=1, flags=f, aux=True) for m, f in MODES.items()}
    pad = (1 << 24) + 5
    big = rtamd.Scene.from_arrays(d)
    big.tri_indices = np.concatenate([np.full(pad, base.tri_indices[0], np.int32), base.tri_indices])
    big.nodes = np.array(big.nodes, copy=True)
    ni = big.nodes.view(np.int32)
    ni[ni[:, 8] < 0, 10] += pad
    renderer.upload(big)
    renderer.set_params(d["params"])
    try:
        for m, f in MODES.items():
            _compare(renderer.render(w, h, depth=1, flags=f, aux=True), want[m], f"padded refs {m}")
        _compare(want["strict"], _oracle("rand2k_8x8", d["params"], w, h, 1), "unpadded vs the oracle")
    finally:
        renderer.upload(base)
