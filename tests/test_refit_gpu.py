"""Animated geometry on the GPU: Renderer.update_vertices rewrites the uploaded
scene's records in place -- triangle and shading records, and the inner records' boxes by a
bottom-up refit -- and must leave exactly what rt_upload_scene builds from the new vertices and
the CPU-refit nodes (rtamd.refit_nodes): the same device records word for word (a refit has no
freedom but the sign of a zero), the same fast-quotient flag, the same pixels as the CPU oracle."""
import json
import os
import subprocess

import numpy as np
import pytest

import rtamd
from conftest import ROOT, load_golden
from refit_common import FIXTURES, SYNTHETIC, moved_vertices, np_refit, scene_arrays, scene_image, with_vertices

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "real-time-opencl-raytracer_amd", "lib", "rt_frameloop")
STRICT = rtamd.RT_FLAG_STRICT_MATH
HDR_WORDS = 64             # the image header's section (256 B)
HDR_FAST_DIV = 12          # ImageHeader::fast_div, in words


@pytest.fixture(scope="module")
def pair():
    """A: uploads the base scene and is updated; B: uploads the CPU-refit arrays."""
    a, b = rtamd.Renderer(0), rtamd.Renderer(0)
    yield a, b
    a.close()
    b.close()


def _scene(d, verts=None, nodes=None, normals=None):
    e = dict(d)
    if verts is not None:
        e["vertices"] = verts
    if nodes is not None:
        e["nodes"] = nodes
    if normals is not None:
        e["normals"] = normals
    return rtamd.Scene.from_arrays(e)


def _assert_same_records(ia, ib, label):
    """Word for word, but for the sign of a zero; the header (fast_div in it) equal."""
    assert ia.shape == ib.shape, label
    assert np.array_equal(ia[:HDR_WORDS], ib[:HDR_WORDS]), f"{label}: headers differ"
    k = np.flatnonzero(ia != ib)
    bad = k[((ia[k] | ib[k]) != 0x80000000) | ((ia[k] & ib[k]) != 0)]
    assert bad.size == 0, f"{label}: {bad.size} words differ, first at {bad[:8]}: {ia[bad[:8]]} vs {ib[bad[:8]]}"


def _refit_scene(name):
    d = scene_arrays(name)
    v2 = moved_vertices(name)
    return d, v2, rtamd.refit_nodes(_scene(d), v2)


@pytest.mark.parametrize("name", FIXTURES + SYNTHETIC)
def test_updated_records_equal_an_upload_of_the_cpu_refit(pair, name):
    """hf40k: 13 k inner records, many workgroups per height; comb60: every height one node, all in
    the single-workgroup kernel; bigleaf: escape-table leaves and an empty leaf."""
    a, b = pair
    d, v2, nodes2 = _refit_scene(name)
    a.upload(_scene(d))
    base = scene_image(a)
    mn0, mx0 = a.scene_bounds()
    assert np.array_equal(mn0, d["nodes"][0, 0:3]) and np.array_equal(mx0, d["nodes"][0, 4:7])   # before any update
    a.update_vertices(v2)
    b.upload(_scene(d, v2, nodes2))
    ia, ib = scene_image(a), scene_image(b)
    assert not np.array_equal(ia, base), "the update changed nothing"
    _assert_same_records(ia, ib, name)
    want, _ = np_refit(d, v2)
    mn, mx = a.scene_bounds()
    assert np.array_equal(mn, want[0, 0:3]) and np.array_equal(mx, want[0, 4:7]), (mn, mx, want[0])
    assert a.last_update_ms() > 0.0


def test_fast_quotient_flag_follows_the_coordinates_both_ways(pair):
    a, b = pair
    d = load_golden("rand2k")
    a.upload(_scene(d))
    assert scene_image(a)[HDR_FAST_DIV] == 1
    v2 = np.array(d["vertices"], np.float32, copy=True)
    v2[0, 0] = np.float32(2.0 ** 61)          # outside the fast quotient's domain [2^-66, 2^60]
    a.update_vertices(v2)
    b.upload(_scene(d, v2, rtamd.refit_nodes(_scene(d), v2)))
    ia, ib = scene_image(a), scene_image(b)
    assert ib[HDR_FAST_DIV] == 0 and ia[HDR_FAST_DIV] == 0
    _assert_same_records(ia, ib, "2^61")
    a.update_vertices(d["vertices"])         # and back
    b.upload(_scene(d))
    ia, ib = scene_image(a), scene_image(b)
    assert ib[HDR_FAST_DIV] == 1 and ia[HDR_FAST_DIV] == 1
    _assert_same_records(ia, ib, "back to the base vertices")


def _boxed(params, mn, mx):
    """The params with the scene box the kernel's early-out reads."""
    p = np.array(params, np.float32, copy=True)
    p[24:27], p[28:31] = mn, mx
    return p


def _same_frame(g, r, label):
    assert np.array_equal(g["hits"], r["hits"]), f"{label}: hits"
    assert np.array_equal(g["t"].view(np.uint32), r["t"].view(np.uint32)), f"{label}: t"
    assert np.array_equal(g["rgb"].view(np.uint32), r["rgb"].view(np.uint32)), f"{label}: rgb"
    assert np.array_equal(g["out"], r["out"]), f"{label}: packed pixels"


@pytest.mark.parametrize("name", ["hf40k", "rand4k_sbvh", "cornell12", "single_tri_rootleaf"])
def test_updated_scene_renders_as_the_oracle_renders_the_cpu_refit(pair, name):
    from oracle import oracle
    a, b = pair
    d, v2, nodes2 = _refit_scene(name)
    w, h = int(d["w"]), int(d["h"])
    a.upload(_scene(d))
    a.update_vertices(v2)
    p = _boxed(d["params"], *a.scene_bounds())
    a.set_params(p)
    gpu = a.render(w, h, depth=3, flags=STRICT, aux=True)
    moved = oracle.render(with_vertices(d, v2, nodes2), p, w, h, depth=3)
    assert moved["stats"]["stack_overflow"] == 0
    _same_frame(gpu, moved, name)
    # nothing passes vacuously: the frame moved, and the boxes mattered
    base = oracle.render(d, d["params"], w, h, depth=3, aux=False)
    assert np.count_nonzero(moved["out"] != base["out"]) > 0
    if d["nodes"].shape[0] > 1:
        stale = oracle.render(with_vertices(d, v2, d["nodes"]), p, w, h, depth=3, aux=False)
        assert np.count_nonzero(moved["out"] != stale["out"]) > 0
    if name == "rand4k_sbvh":
        b.upload(_scene(d, v2, nodes2))
        b.set_params(p)
        for flags in (0, rtamd.RT_FLAG_HW_MATH, rtamd.RT_FLAG_WAVEFRONT | rtamd.RT_FLAG_WF_SORT):
            _same_frame(a.render(w, h, depth=3, flags=flags, aux=True), b.render(w, h, depth=3, flags=flags, aux=True),
                        f"{name} flags {flags}")
    # back to the base vertices, with new normals: as an upload of those arrays renders
    rng = np.random.default_rng(7)
    n2 = np.array(d["normals"], np.float32, copy=True)
    n2[:, :3] += rng.uniform(-0.3, 0.3, (n2.shape[0], 3)).astype(np.float32)
    a.update_vertices(d["vertices"], n2)
    b.upload(_scene(d, d["vertices"], rtamd.refit_nodes(_scene(d), d["vertices"]), n2))
    _assert_same_records(scene_image(a), scene_image(b), f"{name}: base vertices, new normals")
    p0 = _boxed(d["params"], *a.scene_bounds())
    a.set_params(p0)
    b.set_params(p0)
    back = a.render(w, h, depth=3, flags=STRICT, aux=True)
    _same_frame(back, b.render(w, h, depth=3, flags=STRICT, aux=True), f"{name}: base vertices, new normals")
    assert not np.array_equal(back["rgb"], gpu["rgb"])


def test_refusals_leave_the_scene_as_it_was(pair):
    a, _ = pair
    for name in ("overflow_comb", "bad_node"):       # uploaded and rendered as ever, but not refittable
        d = load_golden(name)
        w, h = int(d["w"]), int(d["h"])
        a.upload(_scene(d))
        a.set_params(d["params"])
        before = a.render(w, h, depth=int(d["depth"]))
        assert np.array_equal(before, d["ref_default"]), name
        with pytest.raises(rtamd.RtError) as e:
            a.update_vertices(d["vertices"])
        assert e.value.code == -5 and "node" in str(e.value), str(e.value)
        assert np.array_equal(a.render(w, h, depth=int(d["depth"])), before), name
    d = load_golden("cornell12")
    w, h = 64, 64
    a.upload(_scene(d))
    a.set_params(d["params"])
    before = a.render(w, h, depth=3)
    for bad in (d["vertices"][:-1], np.concatenate([d["vertices"], d["vertices"][:1]])):   # a wrong nv
        with pytest.raises(rtamd.RtError) as e:
            a.update_vertices(bad)
        assert e.value.code == -1
        assert np.array_equal(a.render(w, h, depth=3), before)
    with pytest.raises(rtamd.RtError) as e:                                               # a wrong nnorm
        a.update_vertices(d["vertices"], d["normals"][:-1])
    assert e.value.code == -1
    assert np.array_equal(a.render(w, h, depth=3), before)
    with pytest.raises(rtamd.RtError) as e:
        a.last_update_ms()                            # no update since the upload
    assert e.value.code == -1
    # a context filled from a scene image keeps no refit data
    import torch
    n = a.scene_image_size()
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a.pack_scene(buf.data_ptr(), n)
    c = rtamd.Renderer(0)
    try:
        c.load_scene(buf.data_ptr(), n)
        c.set_params(d["params"])
        assert np.array_equal(c.render(w, h, depth=3), before)
        with pytest.raises(rtamd.RtError) as e:
            c.update_vertices(d["vertices"])
        assert e.value.code == -5 and "rt_scene_image_load" in str(e.value)
        assert np.array_equal(c.render(w, h, depth=3), before)
    finally:
        c.close()
    c = rtamd.Renderer(0)                             # and one without a scene
    try:
        with pytest.raises(rtamd.RtError) as e:
            c.update_vertices(d["vertices"])
        assert e.value.code == -3
    finally:
        c.close()


def test_device_form_takes_vertices_written_on_a_side_stream(pair):
    import torch
    a, _ = pair
    d, v2, _ = _refit_scene("hf40k")
    a.upload(_scene(d))
    base = scene_image(a)
    side = torch.cuda.Stream(device="cuda:0")
    src = torch.from_numpy(d["vertices"]).to("cuda:0")
    delta = torch.from_numpy(v2 - d["vertices"]).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dv = src + delta                              # the caller's animation kernel, on its own stream
    a.update_vertices((dv.data_ptr(), side.cuda_stream))
    device_form = scene_image(a)
    side.synchronize()
    moved = dv.cpu().numpy()                          # what that kernel wrote
    assert not np.array_equal(moved, d["vertices"]) and not np.array_equal(device_form, base)
    a.upload(_scene(d))
    a.update_vertices(moved)
    assert np.array_equal(scene_image(a), device_form)


def _read_ppm(path):
    with open(path, "rb") as f:
        parts = f.read().split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def test_frameloop_animate_matches_the_oracle(tmp_path):
    """rt_frameloop --animate: before frame f the vertices are base * (1 + f / 64) (one float
    multiply per coordinate) and the params carry rt_scene_bounds' box; frames 0, 2, 4 equal the
    oracle's frames of the scaled, CPU-refit scene."""
    from oracle import oracle
    w, h, depth, frames, dx, dy = 96, 64, 3, 5, 7.0, -3.0
    r = subprocess.run([TOOL, "--scene", "cornell", "--width", str(w), "--height", str(h), "--depth", str(depth),
                        "--frames", str(frames), "--drag", str(dx), str(dy), "--ppm-dir", str(tmp_path),
                        "--ppm-every", "2", "--flags", str(STRICT), "--animate"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["frames"] == frames and summary["update_ms_mean"] > 0.0
    m = rtamd.Mesh.cornell()
    scene = rtamd.Scene.from_mesh(m, m.build_sbvh())
    cam = rtamd.Camera()
    for f in range(frames):
        if f > 0:
            cam.add_rotate(dx * 0.25 / 100.0, dy * 0.25 / 100.0)
        if f % 2:
            continue
        s = np.float32(1.0) + np.float32(f) * np.float32(0.015625)
        v = np.array(scene.vertices, np.float32, copy=True)
        v[:, :3] *= s
        nodes = rtamd.refit_nodes(scene, v)
        p = _boxed(rtamd.params_to_array(cam.params(m, w, h)), nodes[0, 0:3], nodes[0, 4:7])
        ref = oracle.render(with_vertices(scene.arrays(), v, nodes), p, w, h, depth=depth, aux=False)["out"].reshape(h, w)
        rgb = np.stack([ref & 0xFF, (ref >> 8) & 0xFF, (ref >> 16) & 0xFF], -1).astype(np.uint8)
        assert np.array_equal(_read_ppm(tmp_path / f"frame_{f:05d}.ppm"), rgb), f"frame {f}"
    # without the flag the summary is as ever
    r = subprocess.run([TOOL, "--scene", "cornell", "--width", "32", "--height", "32", "--frames", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "update_ms_mean" not in r.stdout
