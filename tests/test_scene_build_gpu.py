"""rt_build_scene on the GPU: Renderer.build_scene must leave exactly the scene
rt_upload_scene builds from the same mesh arrays and the host twin's tree (rt_bvh_build_lbvh):
the same scene image word for word, header included, the same bounds, the same refit plan, the
same pixels as the CPU oracle -- on the smallest meshes at which each stage can go wrong.  Two
renderers: A calls build_scene, B uploads the twin's arrays.  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import rtamd
from conftest import ROOT, load_golden
from lbvh_common import mesh, twin
from refit_common import np_refit, scene_image

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "real-time-opencl-raytracer_amd", "lib", "rt_frameloop")
STRICT = rtamd.RT_FLAG_STRICT_MATH
RT_ERR_INVALID_ARG, RT_ERR_BAD_SCENE = -1, -5
HDR_WORDS = 64             # the image header's section (256 B)
HDR_ROOT, HDR_N_INNER, HDR_FAST_DIV, HDR_CLEAN = 10, 11, 12, 13   # ImageHeader, in words
GOLDEN = ("single_tri_rootleaf", "cornell12", "rand2k", "hf40k")
MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")


@pytest.fixture(scope="module")
def pair():
    a, b = rtamd.Renderer(0), rtamd.Renderer(0)
    yield a, b
    a.close()
    b.close()


_ARRAYS = {}


def arrays(name):
    """The mesh arrays of a named mesh (shared; do not modify): from the golden file or the
    generator where it has normals and materials, otherwise a seeded made-up set."""
    if name not in _ARRAYS:
        if name in GOLDEN:
            d = load_golden(name)
            _ARRAYS[name] = {k: d[k] for k in MESH_KEYS}
        elif name == "hf320":
            d = rtamd.Mesh.heightfield(320, 320).arrays()
            _ARRAYS[name] = {k: d[k] for k in MESH_KEYS}
        else:
            v, i = mesh(name)
            rng = np.random.default_rng(len(name) + i.size)
            mats = load_golden("cornell12")["materials"]
            nrm = rng.uniform(-1.0, 1.0, (17, 4)).astype(np.float32)
            nrm[:, 3] = 0.0
            _ARRAYS[name] = {"vertices": v, "indices": i, "normals": nrm,
                             "normals_indices": rng.integers(0, 17, i.size).astype(np.int32), "materials": mats,
                             "tri_to_material": rng.integers(0, mats.shape[0], i.size // 3).astype(np.int32)}
    return _ARRAYS[name]


def first(d, k):
    """The first k triangles of a mesh."""
    return dict(d, indices=d["indices"][:3 * k], normals_indices=d["normals_indices"][:3 * k],
                tri_to_material=d["tri_to_material"][:k])


def case(name, max_leaf):
    """(mesh arrays, (twin nodes, twin references)) of a test mesh."""
    if name == "cornell_first":
        d = first(arrays("cornell12"), max_leaf + 1)
        return d, twin((d["vertices"], d["indices"]), max_leaf)
    if name.startswith("rand2k_first"):
        d = first(arrays("rand2k"), int(name[len("rand2k_first"):]))
        return d, twin((d["vertices"], d["indices"]), max_leaf)
    return arrays(name), twin(name, max_leaf)


def uploaded(d, tree, verts=None):
    """The Scene B uploads: the mesh arrays with the twin's tree."""
    nodes, refs = tree
    v = d["vertices"] if verts is None else verts
    e = dict(d, vertices=v, nodes=nodes, tri_indices=refs, scene_min=v[:, :3].min(0), scene_max=v[:, :3].max(0))
    return rtamd.Scene.from_arrays(e)


def _assert_equal_images(ia, ib, label):
    assert ia.shape == ib.shape, f"{label}: image sizes {ia.shape} vs {ib.shape}"
    assert np.array_equal(ia[:HDR_WORDS], ib[:HDR_WORDS]), f"{label}: headers differ: {ia[:16]} vs {ib[:16]}"
    k = np.flatnonzero(ia != ib)
    assert k.size == 0, f"{label}: {k.size} words differ, first at {k[:8]}: {ia[k[:8]]} vs {ib[k[:8]]}"


def _assert_same_records(ia, ib, label):
    """test_refit_gpu's rule: word for word, but for the sign of a zero; the header equal."""
    assert ia.shape == ib.shape, label
    assert np.array_equal(ia[:HDR_WORDS], ib[:HDR_WORDS]), f"{label}: headers differ"
    k = np.flatnonzero(ia != ib)
    bad = k[((ia[k] | ib[k]) != 0x80000000) | ((ia[k] & ib[k]) != 0)]
    assert bad.size == 0, f"{label}: {bad.size} words differ, first at {bad[:8]}: {ia[bad[:8]]} vs {ib[bad[:8]]}"


def _both(pair, d, tree, max_leaf, label):
    """A builds, B uploads; the images and the bounds must be equal.  Returns A's image."""
    a, b = pair
    a.build_scene(d, max_leaf)
    b.upload(uploaded(d, tree))
    ia, ib = scene_image(a), scene_image(b)
    _assert_equal_images(ia, ib, label)
    (amn, amx), (bmn, bmx) = a.scene_bounds(), b.scene_bounds()
    assert np.array_equal(amn.view(np.uint32), bmn.view(np.uint32)), f"{label}: bounds min {amn} vs {bmn}"
    assert np.array_equal(amx.view(np.uint32), bmx.view(np.uint32)), f"{label}: bounds max {amx} vs {bmx}"
    assert ia[HDR_CLEAN] == 1
    return ia


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
@pytest.mark.parametrize("name", ["single_tri_rootleaf", "cornell_first", "cornell12", "deep40", "copies70", "grid16",
                                  "rand2k", "hf40k", "hf320"])
def test_built_scene_image_equals_an_upload_of_the_twin(pair, name, max_leaf):
    """single_tri_rootleaf: no inner record; cornell_first (max_leaf + 1 triangles): one inner
    record; cornell12: one workgroup; deep40: a breadth-first order with one node per level,
    pre-order equal to depth order; copies70: no axis has extent; grid16: one axis without extent;
    rand2k: K = 1,999 at max_leaf 1, mixing breadth-first and pre-order ids, K < 1,024 at 8; hf40k:
    many workgroups, scans across blocks; hf320 (204,800 triangles): multi-pass sort and scan."""
    d, tree = case(name, max_leaf)
    ia = _both(pair, d, tree, max_leaf, f"{name} max_leaf {max_leaf}")
    assert ia[HDR_N_INNER] == (tree[0].shape[0] - 1) // 2
    if name == "single_tri_rootleaf":
        assert ia[HDR_N_INNER] == 0
    if name == "cornell_first":
        assert ia[HDR_N_INNER] == 1
    if name == "rand2k" and max_leaf == 1:
        assert ia[HDR_N_INNER] == 1999
    if name == "rand2k" and max_leaf == 8:
        assert 0 < ia[HDR_N_INNER] < 1024
    assert pair[0].last_scene_build_ms() > 0.0


@pytest.mark.parametrize("ntri", [1024, 1025, 1026])
def test_ids_at_the_1024_boundary(pair, ntri):
    """K = ntri - 1 inner records at max_leaf 1: 1,023 (all ids breadth-first), 1,024 (exactly
    full), 1,025 (one id past the top)."""
    d, tree = case(f"rand2k_first{ntri}", 1)
    ia = _both(pair, d, tree, 1, f"first {ntri} of rand2k")
    assert ia[HDR_N_INNER] == ntri - 1


def _moved(d, name):
    """refit_common.moved_vertices' displacement for a mesh of this module."""
    v = np.array(d["vertices"], np.float32, copy=True)
    rng = np.random.default_rng(len(name) + v.shape[0])
    v[:, :3] += rng.uniform(-1.5, 1.5, (v.shape[0], 3)).astype(np.float32)
    return v


@pytest.mark.parametrize("name", ["hf40k", "deep40", "rand2k"])
def test_refit_plan_counts_and_an_update_afterwards(pair, name):
    a, b = pair
    d, tree = case(name, 2)
    _both(pair, d, tree, 2, name)
    ca, cb = a.refit_level_counts(), b.refit_level_counts()
    assert np.array_equal(ca, cb), f"{name}: records per height {ca} vs {cb}"
    assert ca.sum() == (tree[0].shape[0] - 1) // 2 and (np.diff(ca.astype(np.int64)) <= 0).all()
    v2 = _moved(d, name)
    base = scene_image(a)
    a.update_vertices(v2)
    b.update_vertices(v2)
    ia, ib = scene_image(a), scene_image(b)
    assert not np.array_equal(ia, base), "the update changed nothing"
    _assert_same_records(ia, ib, f"{name}: after update_vertices")
    # and both are the upload of the CPU refit
    want, _ = np_refit({"nodes": tree[0], "tri_indices": tree[1], "indices": d["indices"]}, v2)
    b.upload(uploaded(d, (want, tree[1]), v2))
    _assert_same_records(ia, scene_image(b), f"{name}: against an upload of the CPU refit")
    mn, mx = a.scene_bounds()
    assert np.array_equal(mn, want[0, 0:3]) and np.array_equal(mx, want[0, 4:7])


def _boxed(params, nodes):
    p = np.array(params, np.float32, copy=True)
    p[24:27], p[28:31] = nodes[0, 0:3], nodes[0, 4:7]
    return p


def test_built_scene_renders_as_the_oracle_renders_the_twin(pair):
    from oracle import oracle
    a, _ = pair
    g = load_golden("hf40k")
    w, h = int(g["w"]), int(g["h"])
    d, tree = case("hf40k", 2)
    a.build_scene(d, 2)
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


def test_fast_quotient_flag_follows_the_coordinates_both_ways(pair):
    a, b = pair
    d = arrays("rand2k")
    v2 = np.array(d["vertices"], np.float32, copy=True)
    v2[0, 0] = np.float32(2.0 ** 61)          # outside the fast quotient's domain [2^-66, 2^60]
    e = dict(d, vertices=v2)
    ia = _both(pair, e, twin((v2, d["indices"]), 2), 2, "2^61")
    assert ia[HDR_FAST_DIV] == 0 and scene_image(b)[HDR_FAST_DIV] == 0
    ia = _both(pair, d, twin("rand2k", 2), 2, "back to the base vertices")
    assert ia[HDR_FAST_DIV] == 1 and scene_image(b)[HDR_FAST_DIV] == 1


def _device_scene(d, side, spare=0):
    """The mesh on the device: (the dict build_scene takes, the tensors to keep alive).  `spare`
    rows past the end of the vertex and normal arrays keep a missed index check in defined memory."""
    import torch
    keep, out = {}, {"materials": d["materials"]}
    for k in MESH_KEYS:
        if k == "materials":
            continue
        x = d[k]
        if spare and k in ("vertices", "normals"):
            x = np.concatenate([x, np.tile(x[:1], (spare, 1))])
        keep[k] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
        out[k] = (keep[k].data_ptr(), side.cuda_stream)
    return out, keep


def _counts(d):
    return {"num_vertices": d["vertices"].shape[0], "num_indices": d["indices"].size, "num_normals": d["normals"].shape[0]}


def test_device_form_takes_vertices_written_on_a_side_stream(pair):
    import torch
    a, _ = pair
    d = arrays("hf40k")
    rng = np.random.default_rng(41)
    delta = np.zeros_like(d["vertices"])
    delta[:, :3] = rng.uniform(-2.0, 2.0, (delta.shape[0], 3)).astype(np.float32)
    side = torch.cuda.Stream(device="cuda:0")
    dev, keep = _device_scene(d, side)
    dlt = torch.from_numpy(delta).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dv = keep["vertices"] + dlt                    # the caller's animation kernel, on its own stream
    dev["vertices"] = (dv.data_ptr(), side.cuda_stream)
    a.build_scene(dev, 4, **_counts(d))
    device_form = scene_image(a)
    side.synchronize()
    moved = dv.cpu().numpy()                           # what that kernel wrote
    assert not np.array_equal(moved, d["vertices"])
    a.build_scene(dict(d, vertices=moved), 4)
    host_form = scene_image(a)
    _assert_equal_images(device_form, host_form, "device form against host form")
    a.build_scene(d, 4)
    assert not np.array_equal(scene_image(a), device_form)   # the moved vertices mattered
    a.update_vertices(moved)                            # and the device form left a refittable scene
    mixed = dict(dev, indices=d["indices"])             # numpy indices join the device arrays
    a.build_scene(mixed, 4, **_counts(d))
    _assert_equal_images(scene_image(a), host_form, "device vertices, host indices")


def _raw(r, d, max_leaf, nidx=None, nnorm=None):
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    return rtamd.lib().rt_build_scene(
        r._h, p(d["vertices"]), d["vertices"].shape[0], p(d["indices"]), d["indices"].size if nidx is None else nidx,
        max_leaf, p(d["normals"]), d["normals"].shape[0] if nnorm is None else nnorm, p(d["normals_indices"]),
        p(d["materials"]), d["materials"].shape[0], p(d["tri_to_material"]))


def test_refusals_leave_the_previous_scene(pair):
    import torch
    a, b = pair
    g = load_golden("cornell12")
    d = arrays("cornell12")
    w, h = 64, 64
    a.build_scene(d, 4)
    a.set_params(g["params"])
    before = a.render(w, h, depth=3)
    assert np.count_nonzero(before) > 0
    image = scene_image(a)

    def unchanged(label):
        assert np.array_equal(a.render(w, h, depth=3), before), label
        assert np.array_equal(scene_image(a), image), label

    for kw in ({"max_leaf": 0}, {"max_leaf": 9}, {"max_leaf": 4, "nidx": 4}, {"max_leaf": 4, "nnorm": 0}):
        assert _raw(a, d, **kw) == RT_ERR_INVALID_ARG, kw
        unchanged(kw)
    bad = {}
    for key, bound, word in (("indices", d["vertices"].shape[0], "mesh_indices"),
                             ("normals_indices", d["normals"].shape[0], "mesh_normals_indices"),
                             ("tri_to_material", d["materials"].shape[0], "tri_to_material")):
        x = np.array(d[key], np.int32, copy=True)
        x[7] = bound                                  # an index equal to its array's size
        bad[key] = (dict(d, **{key: x}), word)
    side = torch.cuda.Stream(device="cuda:0")
    for key, (e, word) in bad.items():
        assert _raw(a, e, 4) == RT_ERR_BAD_SCENE, key
        with pytest.raises(rtamd.RtError) as err:
            a.build_scene(e, 4)
        assert err.value.code == RT_ERR_BAD_SCENE and word in str(err.value), (key, str(err.value))
        unchanged(f"host form, bad {key}")
        dev, keep = _device_scene(e, side, spare=8)
        torch.cuda.synchronize()
        with pytest.raises(rtamd.RtError) as err:
            a.build_scene(dev, 4, **_counts(d))
        assert err.value.code == RT_ERR_BAD_SCENE and word in str(err.value), (key, str(err.value))
        unchanged(f"device form, bad {key}")
    _both(pair, arrays("rand2k"), twin("rand2k", 4), 4, "a valid build after the refusals")
    c = rtamd.Renderer(0)                             # no build yet: no timing, no plan
    try:
        with pytest.raises(rtamd.RtError) as err:
            c.last_scene_build_ms()
        assert err.value.code == RT_ERR_INVALID_ARG
        with pytest.raises(rtamd.RtError):
            c.refit_level_counts()
    finally:
        c.close()


def test_a_frame_in_flight_keeps_the_old_scene(pair):
    import torch
    a, _ = pair
    g = load_golden("rand2k")
    w, h = int(g["w"]), int(g["h"])
    old, new = arrays("rand2k"), first(arrays("rand2k"), 700)
    a.build_scene(new, 2)
    a.set_params(g["params"])
    want_new = a.render(w, h, depth=3)
    a.build_scene(old, 2)
    want_old = a.render(w, h, depth=3)
    assert not np.array_equal(want_old, want_new)
    side = torch.cuda.Stream(device="cuda:0")
    buf = torch.zeros(w * h, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    a.render_device(w, h, 3, 0, buf.data_ptr(), stream=side.cuda_stream)
    a.build_scene(new, 2)                             # at once: the frame may still be running
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), want_old)
    assert np.array_equal(a.render(w, h, depth=3), want_new)


def _read_ppm(path):
    with open(path, "rb") as f:
        parts = f.read().split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def test_frameloop_gpu_scene_matches_the_oracle(tmp_path):
    """rt_frameloop --gpu-scene: frame 0 equals the oracle's frame over Mesh.cornell().build_lbvh(2);
    the summary carries scene_build_ms, and only with the flag."""
    from oracle import oracle
    w, h, depth = 96, 64, 3
    run = subprocess.run([TOOL, "--scene", "cornell", "--width", str(w), "--height", str(h), "--depth", str(depth),
                          "--frames", "1", "--ppm-dir", str(tmp_path), "--ppm-every", "1", "--flags", str(STRICT),
                          "--gpu-scene", "--max-leaf", "2"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["frames"] == 1 and summary["scene_build_ms"] > 0.0
    m = rtamd.Mesh.cornell()
    scene = rtamd.Scene.from_mesh(m, m.build_lbvh(2))
    p = rtamd.params_to_array(rtamd.Camera().params(m, w, h))
    ref = oracle.render(scene, p, w, h, depth=depth, aux=False)["out"].reshape(h, w)
    rgb = np.stack([ref & 0xFF, (ref >> 8) & 0xFF, (ref >> 16) & 0xFF], -1).astype(np.uint8)
    assert np.array_equal(_read_ppm(tmp_path / "frame_00000.ppm"), rgb)
    assert np.count_nonzero(rgb) > 0
    run = subprocess.run([TOOL, "--scene", "cornell", "--width", "32", "--height", "32", "--frames", "1"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "scene_build_ms" not in run.stdout
