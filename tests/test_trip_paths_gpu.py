"""Every path through the depth-1 traversal trip's bookkeeping: the leaf decode
at the top of a trip, with and without escape leaves and for a root that is a leaf, through every
way a scene reaches a context, the LDS stack's guard rows and its deep exit, and the three quotient
variants that share the loop.

Bar: S_strict frames equal the CPU oracle in packed pixels and aux planes, as test_render_gpu.py
compares its fixtures.  The oracle has no S_ref, so an S_ref frame is compared, planes and all,
with the same scene rendered by the general traversal (RTAMD_RECORD_LIMIT: split records), which
shares none of the fast loop's bookkeeping; both reproduce the reference kernel's stored frames
in test_reference_pin_gpu.py.  Every frame is 64 x 64.

The fixture rand3k_bigleaf, for all its name, holds no escape leaf (its largest leaf has 7
triangles: _has_escape_leaves below checks each scene), so the escape table is exercised by
refit_common's big-leaf tree: leaves of 40 and 35 triangles through the escape table, one of 3,
and an empty one."""
import numpy as np
import pytest

from conftest import load_golden
from refit_common import scene_arrays

pytestmark = pytest.mark.gpu

W = H = 64
STRICT, HW, EXACT_DIV = 64, 2, 4
LDS_STACK = 16   # rtk::kLdsStack (RTK_LDS_STACK)
PLAIN = ["rand3k_bigleaf", "rand2k", "hf40k", "cornell12", "single_tri_rootleaf"]


def _has_escape_leaves(d):
    """Whether the encoding needs the escape table: a leaf of >= 31 references (rt_records.h)."""
    ni = np.asarray(d["nodes"]).view(np.int32).reshape(-1, 12)
    return bool(np.any((ni[:, 8] < 0) & (ni[:, 11] >= 31)))


_SCENES = {}


def _scene_dict(name):
    """Scene arrays with params for a 64 x 64 frame (shared; do not modify)."""
    if name not in _SCENES:
        import rtamd
        if name == "escape40":
            d = dict(scene_arrays("bigleaf"))
            m = rtamd.Mesh.from_arrays(d["vertices"], d["indices"])
            d["params"] = rtamd.params_to_array(m.camera_params(W, H, radius=90.0))   # every ray enters the tree
        else:
            d = load_golden(name)
        _SCENES[name] = d
    return _SCENES[name]


def _cams(d, k):
    """k distinct cameras: the scene's own, moved sideways (eye and image plane together)."""
    cams = []
    for i in range(k):
        p = np.array(d["params"], np.float32, copy=True).reshape(8, 4)
        shift = np.array([3.0 * i, -2.0 * i, 1.5 * i], np.float32)
        p[2, :3] += shift
        p[3, :3] += shift
        cams.append(p.reshape(-1))
    return cams


def _device_render(r, params, flags, depth=1):
    """One frame through rt_render_device with aux planes, as the dict rt_render returns."""
    import torch
    r.set_params(params)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    hits = torch.zeros(W * H * depth * 2, dtype=torch.int32, device="cuda")
    t = torch.zeros(W * H * depth, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # the fills run on torch's stream, the frame on the context's own
    r.render_device(W, H, depth, flags, out.data_ptr(), aux_ptrs=(hits.data_ptr(), t.data_ptr(), rgb.data_ptr()))
    torch.cuda.synchronize()
    return {"out": out.cpu().numpy().view(np.uint32), "hits": hits.cpu().numpy().reshape(W * H, depth, 2),
            "t": t.cpu().numpy().reshape(W * H, depth), "rgb": rgb.cpu().numpy().reshape(W * H, 3)}


def _batch_render(r, cams, flags):
    import torch
    out = torch.full((len(cams) * W * H,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.render_device_batch(W, H, 1, flags, cams, out.data_ptr(), W * H)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(len(cams), W * H)


def _compare(got, ref, label):
    assert np.array_equal(got["hits"], ref["hits"]), f"{label}: hit ids differ at " \
        f"{np.argwhere(got['hits'] != ref['hits'])[:5].tolist()}"
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)), f"{label}: t differs"
    assert np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), f"{label}: rgb not bitwise"
    assert np.array_equal(got["out"], ref["out"]), f"{label}: packed pixels differ"


def _oracle(d, params, depth=1):
    from oracle import oracle
    return oracle.render(d, params, W, H, depth=depth)


@pytest.fixture(scope="module")
def general(renderer):
    """A second context whose uploads take the general traversal (split records), and the way to
    bring it to a scene: the S_ref reference."""
    import rtamd
    r = rtamd.Renderer(0)

    def upload(d):
        import os
        old = os.environ.get("RTAMD_RECORD_LIMIT")
        os.environ["RTAMD_RECORD_LIMIT"] = "1024"
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


def _check_scene(renderer, general, d, label, k=3):
    """d, on `renderer`: single renders of k cameras in S_strict (vs the oracle) and S_ref (vs the
    general traversal), then the k-frame batch in both, every frame equal to its single render."""
    cams = _cams(d, k)
    g = general(d)
    singles = {STRICT: [], 0: []}
    for i, p in enumerate(cams):
        s = _device_render(renderer, p, STRICT)
        ref = _oracle(d, p)
        assert i > 0 or int((ref["hits"][:, 0, 0] >= 0).sum()) > 0, f"{label}: the camera sees nothing"
        _compare(s, ref, f"{label} cam {i} S_strict vs oracle")
        singles[STRICT].append(s["out"])
        f = _device_render(renderer, p, 0)
        _compare(f, _device_render(g, p, 0), f"{label} cam {i} S_ref vs general traversal")
        singles[0].append(f["out"])
    for flags in (STRICT, 0):
        for call in range(2):   # the static block order, then the adaptive one
            frames = _batch_render(renderer, cams, flags)
            for i in range(k):
                assert np.array_equal(frames[i], singles[flags][i]), (label, flags, call, i)


def test_fixtures_are_what_the_cases_need():
    """(No GPU work.)  Which scenes hold escape leaves, and that the root-leaf scene is one."""
    assert _has_escape_leaves(_scene_dict("escape40"))
    for name in PLAIN:
        assert not _has_escape_leaves(_scene_dict(name)), name
    ni = _scene_dict("single_tri_rootleaf")["nodes"].view(np.int32).reshape(-1, 12)
    assert ni[0, 8] < 0 and ni[0, 11] == 1
    ni = _scene_dict("escape40")["nodes"].view(np.int32).reshape(-1, 12)
    assert sorted(ni[ni[:, 8] < 0][:, 11].tolist()) == [0, 3, 35, 40]   # an empty leaf among them


@pytest.mark.parametrize("name", ["escape40"] + PLAIN)
def test_escape_and_plain_scenes(renderer, general, name):
    """escape40's big leaves decode through the escape table, the others' from the reference itself;
    a root that is a leaf is decoded by the loop's first trip like any other."""
    import rtamd
    d = _scene_dict(name)
    renderer.upload(rtamd.Scene.from_arrays(d))
    _check_scene(renderer, general, d, name)
    assert renderer.last_deferred() == 0


def test_the_decode_follows_the_scene(general):
    """One context through every way a scene comes into being, alternating scenes with and without
    escape leaves; after each step it renders what a fresh context brought to that scene renders
    (_check_scene's references are the oracle and the general traversal).  Kernels specialised to
    scenes without escape leaves were measured and dropped; anything per-scene that
    the launch may come to depend on has to follow the scene through these steps, or a stale value
    would read triangle ranges out of the wrong place."""
    import rtamd
    import torch
    ctx = rtamd.Renderer(0)
    holders, images = [], []

    def holder(name):
        r = rtamd.Renderer(0)
        holders.append(r)
        r.upload(rtamd.Scene.from_arrays(_scene_dict(name)))
        return r

    def image_of(name):
        r = holder(name)
        n = r.scene_image_size()
        img = torch.zeros(n, dtype=torch.uint8, device="cuda")
        r.pack_scene(img.data_ptr(), n)
        images.append(img)   # alive until the load has copied it
        return img.data_ptr(), n

    try:
        steps = [
            ("upload rand2k", "rand2k", lambda: ctx.upload(rtamd.Scene.from_arrays(_scene_dict("rand2k")))),
            ("upload rand3k_bigleaf", "rand3k_bigleaf",
             lambda: ctx.upload(rtamd.Scene.from_arrays(_scene_dict("rand3k_bigleaf")))),
            ("upload escape40", "escape40", lambda: ctx.upload(rtamd.Scene.from_arrays(_scene_dict("escape40")))),
            ("load rand2k", "rand2k", lambda: ctx.load_scene(*image_of("rand2k"))),
            ("copy rand3k_bigleaf", "rand3k_bigleaf", lambda: ctx.copy_scene_from(holder("rand3k_bigleaf"))),
            ("load escape40", "escape40", lambda: ctx.load_scene(*image_of("escape40"))),
            ("build cornell12", "cornell12", lambda: ctx.build_scene(_scene_dict("cornell12"))),
            ("copy escape40", "escape40", lambda: ctx.copy_scene_from(holder("escape40"))),
            ("load rand2k again", "rand2k", lambda: ctx.load_scene(*image_of("rand2k"))),
        ]
        for label, name, step in steps:
            step()
            d = _scene_dict(name)
            if label.startswith("build"):
                # the on-GPU build makes its own tree: its reference is a fresh context's build
                fresh = rtamd.Renderer(0)
                holders.append(fresh)
                fresh.build_scene(d)
                cams = _cams(d, 2)
                for flags in (STRICT, 0):
                    want = [_device_render(fresh, p, flags) for p in cams]
                    for i, p in enumerate(cams):
                        _compare(_device_render(ctx, p, flags), want[i], f"{label} cam {i} flags {flags}")
                    frames = _batch_render(ctx, cams, flags)
                    for i in range(2):
                        assert np.array_equal(frames[i], want[i]["out"]), (label, flags, i)
            else:
                _check_scene(ctx, general, d, label, k=2)
    finally:
        ctx.close()
        for r in holders:
            r.close()


def _comb(levels):
    """A comb of `levels` inner nodes, every box the scene's, so every level pushes (the way
    tests/golden/make_golden.py builds overflow_comb): a ray's stack count reaches levels + 1."""
    import rtamd
    m = rtamd.Mesh.random(80, extent=40.0, size=8.0, seed=7)
    a = m.arrays()
    ntri = a["indices"].size // 3
    lo = np.append(a["scene_min"], 1.0).astype(np.float32)
    hi = np.append(a["scene_max"], 1.0).astype(np.float32)

    def node(l, r, off, cnt):
        rec = np.zeros(12, np.float32)
        rec[0:4] = lo
        rec[4:8] = hi
        rec[8:12] = np.array([l, r, off, cnt], np.int32).view(np.float32)
        return rec
    nodes, refs = [], []
    for k in range(levels):
        nodes.append(node(2 * (k + 1) if k + 1 < levels else 2 * k + 1, 2 * k + 1, -1, 0))
        nodes.append(node(-1, -1, len(refs), 1))
        refs.append(3 * (k % ntri))
    d = {k: a[k] for k in ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material",
                           "scene_min", "scene_max")}
    d["nodes"] = np.stack(nodes).astype(np.float32)
    d["tri_indices"] = np.array(refs, np.int32)
    d["params"] = rtamd.params_to_array(m.camera_params(W, H))
    return d


@pytest.mark.parametrize("over", [1, 2, 3])
def test_stack_depths_around_the_lds_part(renderer, over):
    """Deepest stack count kLdsStack + 1 (the last the LDS column holds), + 2 (the first that
    restarts with the general traversal) and + 3."""
    import rtamd
    d = _comb(LDS_STACK + over - 1)
    ref = _oracle(d, d["params"])
    assert ref["stats"]["max_stack"] == LDS_STACK + over and ref["stats"]["stack_overflow"] == 0   # the oracle alone
    assert int((ref["hits"][:, 0, 0] >= 0).sum()) > 0
    renderer.upload(rtamd.Scene.from_arrays(d))
    got = _device_render(renderer, d["params"], STRICT)
    restarts = renderer.last_deferred()
    _compare(got, ref, f"comb +{over}")
    assert (restarts == 0) if over == 1 else (restarts > 0), restarts
    frames = _batch_render(renderer, [d["params"]] * 2, STRICT)
    assert np.array_equal(frames[0], ref["out"]) and np.array_equal(frames[1], ref["out"])


def test_overflow_comb_at_depth_1(renderer):
    """The stored comb of 70 levels: every traversal restarts, and the general code overflows."""
    import rtamd
    d = load_golden("overflow_comb")
    ref = _oracle(d, d["params"])
    assert ref["stats"]["stack_overflow"] > 0
    renderer.upload(rtamd.Scene.from_arrays(d))
    before = renderer.overflow_count()
    _compare(_device_render(renderer, d["params"], STRICT), ref, "overflow_comb")
    assert renderer.last_deferred() > 0
    assert renderer.overflow_count() > before


def test_zero_direction_rays_take_marksteins_variant(renderer):
    """An axis-aligned camera, and a frame 65 pixels wide (the only case here that is not 64), so
    that column 33 has image_pos.x == campos.x exactly: rays with a direction component of 0 run
    the traversal's MODE 1 in S_strict and S_hw, the same bookkeeping around another slab test."""
    import rtamd
    d = _scene_dict("rand2k")
    renderer.upload(rtamd.Scene.from_arrays(d))
    w, h = 65, 64
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
    p = p.reshape(-1)
    renderer.set_params(p)
    from oracle import oracle
    ref = oracle.render(d, p, w, h, depth=1)
    assert int((ref["hits"][:, 0, 0] >= 0).sum()) > 0
    got = renderer.render(w, h, depth=1, flags=STRICT, aux=True)
    _compare(got, ref, "axis-aligned camera")
    assert renderer.last_deferred() == 0
    for flags in (0, HW):
        fast = renderer.render(w, h, depth=1, flags=flags, aux=True)
        slow = renderer.render(w, h, depth=1, flags=flags | EXACT_DIV, aux=True)
        _compare(fast, slow, f"axis-aligned camera flags {flags}")


def test_a_scene_outside_the_fast_quotients_domain_takes_the_division_form(renderer, general):
    """rand2k with one vertex coordinate of 1e-25 (below 2^-66), one triangle per leaf so that the
    coordinate is a box bound: the scene's every traversal runs MODE 2."""
    import rtamd
    src = _scene_dict("rand2k")
    v = np.array(src["vertices"], np.float32, copy=True)
    v[int(src["indices"][0]), 2] = np.float32(1e-25)
    m = rtamd.Mesh.from_arrays(v, src["indices"])
    s = rtamd.Scene.from_mesh(m, m.build_bvh(1))
    d = s.arrays()
    boxes = np.asarray(d["nodes"], np.float32).reshape(-1, 12)[:, [0, 1, 2, 4, 5, 6]]
    assert np.any(boxes == np.float32(1e-25))
    d["params"] = rtamd.params_to_array(m.camera_params(W, H))
    renderer.upload(s)
    _check_scene(renderer, general, d, "tiny coordinate", k=2)
