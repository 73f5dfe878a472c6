"""The extent-aware Morton keys and rt_scene_sah on the GPU.  Renderer.build_bvh and
Renderer.build_scene with keys="extent" must give, byte for byte, what the host twin
(rt_bvh_build_lbvh with RT_BUILD_EXTENT_KEYS) and an upload of its arrays give; the built scene
renders as the CPU oracle renders the twin; Renderer.scene_sah equals the numpy evaluation of its
definition over the host nodes of whatever was uploaded, built or refitted, and reports on the
flat heightfield the gain the CPU test demands of the definition."""
import ctypes as C

import numpy as np
import pytest

import rtamd
from conftest import load_golden
from lbvh_common import cornell_first, twin
from lbvh_keys_common import EXTENT, SMALL, mesh, np_scene_sah, twin_extent
from refit_common import np_refit, scene_image

pytestmark = pytest.mark.gpu

STRICT = rtamd.RT_FLAG_STRICT_MATH
RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE = -1, -3
MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")
# double sums of at most 2^22 exactly known float terms, all of one sign: n * 2^-53 ~ 5e-10
SAH_RTOL = 1e-9


@pytest.fixture(scope="module")
def pair():
    a, b = rtamd.Renderer(0), rtamd.Renderer(0)
    yield a, b
    a.close()
    b.close()


def _same(got, want, label):
    nodes, refs = got
    assert nodes.shape == want[0].shape and refs.shape == want[1].shape, label
    assert np.array_equal(refs, want[1]), f"{label}: references"
    assert np.array_equal(nodes.view(np.uint32), want[0].view(np.uint32)), f"{label}: nodes"


def _device_build(r, v, i, max_leaf):
    import torch
    d_v, d_i = torch.from_numpy(v).to("cuda:0"), torch.from_numpy(i).to("cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    return r.build_bvh((d_v.data_ptr(), side.cuda_stream), (d_i.data_ptr(), side.cuda_stream), max_leaf,
                       num_vertices=v.shape[0], num_indices=i.size, keys="extent")


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
@pytest.mark.parametrize("name", SMALL + ["hf40k"])
def test_build_with_extent_keys_equals_the_host_twin(pair, name, max_leaf):
    """The host form and the device form.  copies70: no extent, the cap alone decides the plan;
    grid16: y gets no bit; needle: the 20-bit cap binds; nonfinite: an infinite extent; cubes2_obj
    and hf40k: three different bit counts, many workgroups."""
    r = pair[0]
    v, i = mesh(name)
    want = twin_extent(name, max_leaf)
    _same(r.build_bvh(v, i, max_leaf, keys="extent"), want, f"{name} max_leaf {max_leaf}, host form")
    _same(_device_build(r, v, i, max_leaf), want, f"{name} max_leaf {max_leaf}, device form")
    if name in ("hf40k", "cubes2_obj"):
        assert not np.array_equal(want[1], twin(name, max_leaf)[1])      # not the per-axis order


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
def test_root_leaf_then_the_smallest_kept_tree(pair, max_leaf):
    for k in (max_leaf, max_leaf + 1):
        v, i = cornell_first(k)
        got = pair[0].build_bvh(v, i, max_leaf, keys="extent")
        assert got[0].shape[0] == (1 if k == max_leaf else 3)
        _same(got, twin_extent((v, i), max_leaf), f"first {k} of cornell12, max_leaf {max_leaf}")


def arrays(name):
    d = load_golden(name)
    return {k: d[k] for k in MESH_KEYS}


def uploaded(d, tree, verts=None):
    """The Scene the second renderer uploads: the mesh arrays with the twin's tree."""
    nodes, refs = tree
    v = d["vertices"] if verts is None else verts
    return rtamd.Scene.from_arrays(dict(d, vertices=v, nodes=nodes, tri_indices=refs, scene_min=v[:, :3].min(0),
                                        scene_max=v[:, :3].max(0)))


def _assert_same_records(ia, ib, label):
    """test_refit_gpu's rule: word for word, but for the sign of a zero."""
    assert ia.shape == ib.shape, label
    k = np.flatnonzero(ia != ib)
    bad = k[((ia[k] | ib[k]) != 0x80000000) | ((ia[k] & ib[k]) != 0)]
    assert bad.size == 0, f"{label}: {bad.size} words differ, first at {bad[:8]}: {ia[bad[:8]]} vs {ib[bad[:8]]}"


def _close(got, want, label):
    for g, w, what in zip(got[:3], want, ("inner_area", "leaf_area_tris", "root_area")):
        print(f"{label}: {what} {g!r} vs {w!r}")
        assert abs(g - w) <= SAH_RTOL * abs(w), f"{label}: {what} {g!r} vs {w!r}"


def _moved(v, seed):
    v2 = np.array(v, np.float32, copy=True)
    v2[:, :3] += np.random.default_rng(seed).uniform(-1.5, 1.5, (v.shape[0], 3)).astype(np.float32)
    return v2


@pytest.mark.parametrize("name", ["cornell12", "rand2k", "hf40k"])
def test_built_scene_equals_an_upload_of_the_twin_and_refits(pair, name):
    """The scene image word for word, the bounds, the refit plan; then update_vertices on the
    built scene against an upload of the CPU refit; scene_sah at both stages."""
    a, b = pair
    d, tree = arrays(name), twin_extent(name, 2)
    a.build_scene(d, 2, keys="extent")
    b.upload(uploaded(d, tree))
    ia, ib = scene_image(a), scene_image(b)
    assert ia.shape == ib.shape
    k = np.flatnonzero(ia != ib)
    assert k.size == 0, f"{name}: {k.size} words differ, first at {k[:8]}"
    (amn, amx), (bmn, bmx) = a.scene_bounds(), b.scene_bounds()
    assert np.array_equal(amn.view(np.uint32), bmn.view(np.uint32)) and np.array_equal(amx.view(np.uint32), bmx.view(np.uint32))
    assert np.array_equal(a.refit_level_counts(), b.refit_level_counts())
    built = a.scene_sah()
    _close(built, np_scene_sah(tree[0]), f"{name}: built")
    v2 = _moved(d["vertices"], len(name))
    a.update_vertices(v2)
    want, _ = np_refit({"nodes": tree[0], "tri_indices": tree[1], "indices": d["indices"]}, v2)
    b.upload(uploaded(d, (want, tree[1]), v2))
    _assert_same_records(scene_image(a), scene_image(b), f"{name}: after update_vertices")
    mn, mx = a.scene_bounds()
    assert np.array_equal(mn, want[0, 0:3]) and np.array_equal(mx, want[0, 4:7])
    _close(a.scene_sah(), np_scene_sah(want), f"{name}: refitted")
    assert a.scene_sah().inner_area != built.inner_area              # the query follows the refit


def test_refused_values_leave_the_previous_scene(pair):
    a, _ = pair
    g = load_golden("cornell12")
    d = arrays("cornell12")
    a.build_scene(d, 4, keys="extent")
    a.set_params(g["params"])
    before = a.render(64, 64, depth=3)
    assert np.count_nonzero(before) > 0
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    n = d["indices"].size // 3
    nodes, refs, nn = np.zeros((2 * n - 1, 12), np.float32), np.zeros(n, np.int32), C.c_int32(-7)
    for bad in (EXTENT | 0, EXTENT | 9, 0x200 | 4):
        rc = rtamd.lib().rt_build_scene(a._h, p(d["vertices"]), d["vertices"].shape[0], p(d["indices"]), d["indices"].size, bad,
                                        p(d["normals"]), d["normals"].shape[0], p(d["normals_indices"]), p(d["materials"]),
                                        d["materials"].shape[0], p(d["tri_to_material"]))
        assert rc == RT_ERR_INVALID_ARG, hex(bad)
        rc = rtamd.lib().rt_build_bvh(a._h, p(d["vertices"]), d["vertices"].shape[0], p(d["indices"]), d["indices"].size, bad,
                                      p(nodes), nodes.shape[0], p(refs), refs.size, C.byref(nn))
        assert rc == RT_ERR_INVALID_ARG and nn.value == -7 and not nodes.any() and not refs.any(), hex(bad)
        with pytest.raises(rtamd.RtError) as e:
            a.build_bvh(d["vertices"], d["indices"], bad)
        assert e.value.code == RT_ERR_INVALID_ARG
        assert np.array_equal(a.render(64, 64, depth=3), before), hex(bad)
    with pytest.raises(ValueError):
        a.build_scene(d, 4, keys="morton")
    _same(a.build_bvh(d["vertices"], d["indices"], 4, keys="extent"), twin_extent("cornell12", 4), "a valid build afterwards")


def _boxed(params, nodes):
    p = np.array(params, np.float32, copy=True)
    p[24:27], p[28:31] = nodes[0, 0:3], nodes[0, 4:7]
    return p


@pytest.mark.parametrize("name", ["hf40k", "cornell12"])
def test_extent_keys_scene_renders_as_the_oracle_renders_the_twin(pair, name):
    from oracle import oracle
    a, _ = pair
    g = load_golden(name)
    w, h = int(g["w"]), int(g["h"])
    tree = twin_extent(name, 2)
    a.build_scene(arrays(name), 2, keys="extent")
    e = dict(g, nodes=tree[0], tri_indices=tree[1])
    p = _boxed(g["params"], tree[0])
    a.set_params(p)
    gpu = a.render(w, h, depth=3, flags=STRICT, aux=True)
    ref = oracle.render(e, p, w, h, depth=3)
    assert ref["stats"]["stack_overflow"] == 0 and a.overflow_count() == 0
    assert np.array_equal(gpu["hits"], ref["hits"]), "hits"
    assert np.array_equal(gpu["t"].view(np.uint32), ref["t"].view(np.uint32)), "t"
    assert np.array_equal(gpu["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), "rgb"
    assert np.array_equal(gpu["out"], ref["out"]), "packed pixels"
    assert np.count_nonzero(ref["hits"][:, 0, 0] >= 0) > 0


@pytest.mark.parametrize("name", ["cornell12", "rand4k_sbvh", "rand3k_bigleaf", "bad_node", "overflow_comb"])
def test_scene_sah_of_an_uploaded_scene_equals_its_definition(pair, name):
    """rand3k_bigleaf: the widest leaves of the golden scenes (7 references; escape leaves are
    test_scene_sah_reads_escape_leaves'); bad_node: a malformed reference adds nothing;
    overflow_comb: a node with two parents counts once per child slot."""
    _, b = pair
    d = load_golden(name)
    b.upload(rtamd.Scene.from_arrays(d))
    got = b.scene_sah()
    want = np_scene_sah(d["nodes"])
    _close(got, want, name)
    assert got.cost == pytest.approx((want[0] + want[1]) / want[2], rel=SAH_RTOL) and got.cost > 1.0
    ni = d["nodes"].view(np.int32)
    if name == "bad_node":
        assert ((ni[:, 8] >= 0) & (ni[:, 9] < 0)).any()
    if name == "overflow_comb":
        kids = np.concatenate([ni[ni[:, 8] >= 0, 8], ni[ni[:, 8] >= 0, 9]])
        assert np.unique(kids).size < kids.size


def test_scene_sah_reads_escape_leaves(pair):
    """A count of 31 or more does not fit the reference: it comes from the escape table.  A hand-made
    tree over the first 42 triangles of rand2k -- leaves of 40 and 2 -- and one root leaf of all 42."""
    _, b = pair
    d = load_golden("rand2k")
    refs = 3 * np.arange(42, dtype=np.int32)
    for words in ([[1, 2, -1, 0], [-1, -1, 0, 40], [-1, -1, 40, 2]], [[-1, -1, 0, 42]]):
        nodes = np.zeros((len(words), 12), np.float32)
        nodes[:, 3] = nodes[:, 7] = 1.0
        nodes.view(np.int32)[:, 8:12] = words
        nodes, _ = np_refit({"nodes": nodes, "tri_indices": refs, "indices": d["indices"]}, d["vertices"])
        b.upload(rtamd.Scene.from_arrays(dict(d, nodes=nodes, tri_indices=refs)))
        want = np_scene_sah(nodes)
        _close(b.scene_sah(), want, f"escape leaves, {len(words)} nodes")
        assert want[1] > 0.0


def test_scene_sah_of_a_root_leaf_scene(pair):
    a, b = pair
    d = arrays("single_tri_rootleaf")
    a.build_scene(d, 4, keys="extent")
    g = load_golden("single_tri_rootleaf")
    b.upload(rtamd.Scene.from_arrays(g))
    for r, nodes in ((a, twin_extent("single_tri_rootleaf", 4)[0]), (b, g["nodes"])):
        got, want = r.scene_sah(), np_scene_sah(nodes)
        _close(got, want, "root leaf")
        assert got.inner_area == 0.0 and got.leaf_area_tris == got.root_area * 1


def test_scene_sah_through_a_scene_image_and_a_copy(pair):
    """A scene image carries no root box: the root record's own box stands in, which for a built
    tree is the same box."""
    import torch
    a, _ = pair
    a.build_scene(arrays("hf40k"), 2, keys="extent")
    want = a.scene_sah()
    n = a.scene_image_size()
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a.pack_scene(buf.data_ptr(), n)
    c = rtamd.Renderer(0)
    try:
        c.load_scene(buf.data_ptr(), n)
        assert c.scene_sah() == want
        c.copy_scene_from(a)
        assert c.scene_sah() == want
    finally:
        c.close()


def test_scene_sah_reports_the_gain_on_the_flat_heightfield(pair):
    """The CPU condition (test_lbvh_keys.py), seen through the GPU: extent-aware cost <= 0.75 x per-axis."""
    a, _ = pair
    d = arrays("hf40k")
    for max_leaf in (1, 4):
        a.build_scene(d, max_leaf)
        axis = a.scene_sah().cost
        a.build_scene(d, max_leaf, keys="extent")
        extent = a.scene_sah().cost
        print(f"hf40k max_leaf {max_leaf}: per-axis {axis:.2f}, extent-aware {extent:.2f}, ratio {extent / axis:.3f}")
        assert extent <= 0.75 * axis


def test_scene_sah_without_a_scene():
    c = rtamd.Renderer(0)
    try:
        with pytest.raises(rtamd.RtError) as e:
            c.scene_sah()
        assert e.value.code == RT_ERR_NO_SCENE
    finally:
        c.close()


def test_frameloop_extent_keys_matches_the_oracle(tmp_path):
    """rt_frameloop --gpu-scene --extent-keys: frame 0 equals the oracle's frame over
    Mesh.cornell().build_lbvh(2, keys="extent"); the option alone is refused."""
    import json
    import os
    import subprocess
    from conftest import ROOT
    from oracle import oracle
    tool = os.path.join(ROOT, "real-time-opencl-raytracer_amd", "lib", "rt_frameloop")
    w, h, depth = 96, 64, 3
    run = subprocess.run([tool, "--scene", "cornell", "--width", str(w), "--height", str(h), "--depth", str(depth),
                          "--frames", "1", "--ppm-dir", str(tmp_path), "--ppm-every", "1", "--flags", str(STRICT),
                          "--gpu-scene", "--max-leaf", "2", "--extent-keys"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert json.loads(run.stdout.strip().splitlines()[-1])["scene_build_ms"] > 0.0
    m = rtamd.Mesh.cornell()
    scene = rtamd.Scene.from_mesh(m, m.build_lbvh(2, keys="extent"))
    p = rtamd.params_to_array(rtamd.Camera().params(m, w, h))
    ref = oracle.render(scene, p, w, h, depth=depth, aux=False)["out"].reshape(h, w)
    rgb = np.stack([ref & 0xFF, (ref >> 8) & 0xFF, (ref >> 16) & 0xFF], -1).astype(np.uint8)
    with open(tmp_path / "frame_00000.ppm", "rb") as f:
        parts = f.read().split(b"\n", 3)
    assert np.array_equal(np.frombuffer(parts[3], np.uint8).reshape(h, w, 3), rgb) and np.count_nonzero(rgb) > 0
    run = subprocess.run([tool, "--scene", "cornell", "--frames", "1", "--extent-keys"], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 2
