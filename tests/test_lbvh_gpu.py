"""The on-GPU LBVH build: Renderer.build_bvh (rt_build_bvh / rt_build_bvh_device)
must write, byte for byte, the arrays of its host twin rt_bvh_build_lbvh -- every node word, every
reference -- on the smallest meshes at which each stage can go wrong; the built arrays upload,
render as the CPU oracle renders them and refit; and every refusal leaves the context usable."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import rtamd
from conftest import ROOT, load_golden
from lbvh_common import ALL, cornell_first, mesh, twin

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "real-time-opencl-raytracer_amd", "lib", "rt_frameloop")
STRICT = rtamd.RT_FLAG_STRICT_MATH
RT_ERR_INVALID_ARG, RT_ERR_BAD_SCENE = -1, -5


@pytest.fixture(scope="module")
def r():
    x = rtamd.Renderer(0)
    yield x
    x.close()


def _same(got, want, label):
    nodes, refs = got
    assert nodes.shape == want[0].shape and refs.shape == want[1].shape, label
    assert np.array_equal(refs, want[1]), f"{label}: references"
    assert np.array_equal(nodes.view(np.uint32), want[0].view(np.uint32)), f"{label}: nodes"


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
@pytest.mark.parametrize("name", ALL)
def test_device_build_equals_the_host_twin(r, name, max_leaf):
    """single_tri_rootleaf: a root leaf, no inner node; cornell12: one workgroup; copies70: no axis
    has extent, order from the index bits alone; deep40: a one-sided tree, many depths of one node
    (the single-workgroup path); grid16: one axis without extent; rand2k: several workgroups;
    hf40k: many workgroups per depth, the scan across blocks; hf320 (204,800 triangles): the
    multi-pass paths of the device sort and scan."""
    v, i = mesh(name)
    _same(r.build_bvh(v, i, max_leaf), twin(name, max_leaf), f"{name} max_leaf {max_leaf}")
    assert r.last_build_ms() > 0.0


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
def test_root_leaf_then_the_smallest_kept_tree(r, max_leaf):
    for k in (max_leaf, max_leaf + 1):
        v, i = cornell_first(k)
        got = r.build_bvh(v, i, max_leaf)
        assert got[0].shape[0] == (1 if k == max_leaf else 3)
        _same(got, twin((v, i), max_leaf), f"first {k} of cornell12, max_leaf {max_leaf}")


def _boxed(params, nodes):
    """The params with the scene box taken from node 0."""
    p = np.array(params, np.float32, copy=True)
    p[24:27], p[28:31] = nodes[0, 0:3], nodes[0, 4:7]
    return p


@pytest.mark.parametrize("name", ["hf40k", "rand2k"])
def test_built_scene_renders_as_the_oracle_and_refits(r, name):
    from oracle import oracle
    d = load_golden(name)
    w, h = int(d["w"]), int(d["h"])
    nodes, refs = r.build_bvh(d["vertices"], d["indices"], 4)
    e = dict(d, nodes=nodes, tri_indices=refs)
    p = _boxed(d["params"], nodes)
    r.upload(rtamd.Scene.from_arrays(e))
    r.set_params(p)
    gpu = r.render(w, h, depth=3, flags=STRICT, aux=True)
    ref = oracle.render(e, p, w, h, depth=3)
    assert ref["stats"]["stack_overflow"] == 0 and r.overflow_count() == 0
    assert np.array_equal(gpu["hits"], ref["hits"]), "hits"
    assert np.array_equal(gpu["t"].view(np.uint32), ref["t"].view(np.uint32)), "t"
    assert np.array_equal(gpu["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), "rgb"
    assert np.array_equal(gpu["out"], ref["out"]), "packed pixels"
    assert np.count_nonzero(ref["hits"][:, 0, 0] >= 0) > 0
    # the builder's output is refittable, and building does not disturb the uploaded scene
    v2 = np.array(d["vertices"], np.float32, copy=True)
    v2[:, :3] *= np.float32(1.125)
    r.update_vertices(v2)
    mn, mx = r.scene_bounds()
    want = rtamd.refit_nodes(rtamd.Scene.from_arrays(e), v2)
    assert np.array_equal(mn, want[0, 0:3]) and np.array_equal(mx, want[0, 4:7])
    r.update_vertices(d["vertices"])
    other = mesh("grid16")
    r.build_bvh(other[0], other[1], 2)
    again = r.render(w, h, depth=3, flags=STRICT, aux=True)
    assert np.array_equal(again["out"], gpu["out"]) and np.array_equal(again["hits"], gpu["hits"])


def test_device_form_takes_vertices_written_on_a_side_stream(r):
    import torch
    v, i = mesh("hf40k")
    rng = np.random.default_rng(40)
    delta = np.zeros_like(v)
    delta[:, :3] = rng.uniform(-2.0, 2.0, (v.shape[0], 3)).astype(np.float32)
    side = torch.cuda.Stream(device="cuda:0")
    src = torch.from_numpy(v).to("cuda:0")
    dlt = torch.from_numpy(delta).to("cuda:0")
    d_idx = torch.from_numpy(i).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dv = src + dlt                                 # the caller's animation kernel, on its own stream
    dev = r.build_bvh((dv.data_ptr(), side.cuda_stream), (d_idx.data_ptr(), side.cuda_stream), 4,
                      num_vertices=v.shape[0], num_indices=i.size)
    side.synchronize()
    moved = dv.cpu().numpy()                           # what that kernel wrote
    assert not np.array_equal(moved, v)
    host = r.build_bvh(moved, i, 4)
    _same(dev, host, "device form against host form")
    _same(dev, twin((moved, i), 4), "device form against the twin")
    assert not np.array_equal(dev[0], twin("hf40k", 4)[0])
    mixed = r.build_bvh((dv.data_ptr(), side.cuda_stream), i, 4, num_vertices=v.shape[0])   # numpy indices join
    _same(mixed, host, "device vertices, host indices")


def _raw(r, v, i, max_leaf, node_cap=None, nidx=None, nv=None):
    n = i.size // 3
    nodes = np.zeros((max(2 * n - 1, 1), 12), np.float32)
    refs = np.zeros(max(n, 1), np.int32)
    nn = C.c_int32(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = rtamd.lib().rt_build_bvh(r._h, p(v), v.shape[0] if nv is None else nv, p(i), i.size if nidx is None else nidx,
                                  max_leaf, p(nodes), nodes.shape[0] if node_cap is None else node_cap, p(refs),
                                  refs.size, C.byref(nn))
    return rc, nn.value, nodes, refs


def test_refusals_leave_the_context_usable(r):
    import torch
    v, i = mesh("cornell12")
    want = twin("cornell12", 4)

    def still_works():
        _same(r.build_bvh(v, i, 4), want, "a valid build after a refusal")

    for kw in ({"max_leaf": 0}, {"max_leaf": 9}, {"max_leaf": 4, "node_cap": 2 * 12 - 2}, {"max_leaf": 4, "nidx": 4}):
        rc, nn, nodes, refs = _raw(r, v, i, **kw)
        assert rc == RT_ERR_INVALID_ARG, kw
        assert nn == -7 and not nodes.any() and not refs.any(), kw      # nothing written
        still_works()
    bad = np.array(i, np.int32, copy=True)
    bad[7] = v.shape[0]                                                   # an index equal to nv
    rc, nn, nodes, refs = _raw(r, v, bad, 4)
    assert rc == RT_ERR_BAD_SCENE and nn == -7 and not nodes.any()
    with pytest.raises(rtamd.RtError) as e:
        r.build_bvh(v, bad, 4)
    assert e.value.code == RT_ERR_BAD_SCENE
    still_works()
    # device form: the vertex buffer has spare rows past nv, so even a missed check would read
    # defined memory; the check itself must refuse
    spare = np.concatenate([v, np.tile(v[:1], (8, 1))])
    d_v = torch.from_numpy(spare).to("cuda:0")
    d_i = torch.from_numpy(bad).to("cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(rtamd.RtError) as e:
        r.build_bvh((d_v.data_ptr(), side.cuda_stream), (d_i.data_ptr(), side.cuda_stream), 4,
                    num_vertices=v.shape[0], num_indices=bad.size)
    assert e.value.code == RT_ERR_BAD_SCENE
    still_works()
    d_ok = torch.from_numpy(i).to("cuda:0")
    torch.cuda.synchronize()
    _same(r.build_bvh((d_v.data_ptr(), side.cuda_stream), (d_ok.data_ptr(), side.cuda_stream), 4,
                      num_vertices=v.shape[0], num_indices=i.size), want, "device form after a refusal")
    c = rtamd.Renderer(0)                                                 # no build yet: no timing
    try:
        with pytest.raises(rtamd.RtError) as e:
            c.last_build_ms()
        assert e.value.code == RT_ERR_INVALID_ARG
    finally:
        c.close()


def _read_ppm(path):
    with open(path, "rb") as f:
        parts = f.read().split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def test_frameloop_gpu_build_matches_the_oracle(tmp_path):
    """rt_frameloop --gpu-build: frame 0 equals the oracle's frame over Mesh.cornell().build_lbvh;
    the summary carries build_ms, and only with the flag."""
    from oracle import oracle
    w, h, depth = 96, 64, 3
    run = subprocess.run([TOOL, "--scene", "cornell", "--width", str(w), "--height", str(h), "--depth", str(depth),
                          "--frames", "1", "--ppm-dir", str(tmp_path), "--ppm-every", "1", "--flags", str(STRICT),
                          "--gpu-build", "--max-leaf", "2"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    m = rtamd.Mesh.cornell()
    bvh = m.build_lbvh(2)
    assert summary["frames"] == 1 and summary["build_ms"] > 0.0 and summary["bvh_nodes"] == bvh.nodes.shape[0]
    scene = rtamd.Scene.from_mesh(m, bvh)
    p = rtamd.params_to_array(rtamd.Camera().params(m, w, h))
    ref = oracle.render(scene, p, w, h, depth=depth, aux=False)["out"].reshape(h, w)
    rgb = np.stack([ref & 0xFF, (ref >> 8) & 0xFF, (ref >> 16) & 0xFF], -1).astype(np.uint8)
    assert np.array_equal(_read_ppm(tmp_path / "frame_00000.ppm"), rgb)
    assert np.count_nonzero(rgb) > 0
    run = subprocess.run([TOOL, "--scene", "cornell", "--width", "32", "--height", "32", "--frames", "1"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "build_ms" not in run.stdout
