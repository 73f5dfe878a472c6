"""The GPU builds and the refit at the edges of mesh space, on the meshes of
mesh_edge_common.py: rt_build_bvh (host and device form) against the host twin; rt_build_scene
against an upload of the twin's arrays -- scene image, bounds, the refit plan's lists, which prove
the launch schedule each lattice mesh is made for; rt_update_vertices on the built scene against an
upload of rt_refit_nodes' arrays; a strict frame of every finite mesh against the CPU oracle;
rt_scene_sah against its definition; and the reuse of one context's build scratch in a large,
small, large order.  Two renderers: A builds, B uploads.  Every comparison is byte equality, headers
included; on the meshes with zeros of both signs the zero rule (mesh_edge_common.excused).  A scene
that holds a NaN, an infinity or a coordinate outside [2^-66, 2^60] is compared and never rendered."""
import numpy as np
import pytest

import rtamd
from lbvh_keys_common import np_scene_sah
from mesh_edge_common import (ALL, FINITE, HEIGHTS, LATTICE, ZEROS, F, arrays, base_vertices, excused, flipped, height_counts, mesh,
                              moved_vertices, tree, twin, zero_mask)
from refit_common import scene_image
from test_scene_build_gpu import HDR_CLEAN, HDR_FAST_DIV, HDR_N_INNER, uploaded

pytestmark = pytest.mark.gpu

STRICT = rtamd.RT_FLAG_STRICT_MATH
SAH_RTOL = 1e-9            # double sums of at most 2^22 exactly known float terms of one sign
KEYS = ["axis", "extent"]


@pytest.fixture(scope="module")
def pair():
    a, b = rtamd.Renderer(0), rtamd.Renderer(0)
    yield a, b
    a.close()
    b.close()


def _mask(name, nodes, refs, verts=None):
    """The excusable node words, on the meshes with zeros of both signs; None elsewhere (plain equality)."""
    if name not in ZEROS:
        return None
    return zero_mask(tree(name, nodes, refs), mesh(name)[0] if verts is None else verts)


def _same_tree(got, want, mask, label):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, label
    assert np.array_equal(got[1], want[1]), f"{label}: references"
    return excused(got[0], want[0], mask, f"{label}: nodes")


def _device_build(r, v, i, max_leaf, keys):
    import torch
    d_v, d_i = torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(i)).to("cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    return r.build_bvh((d_v.data_ptr(), side.cuda_stream), (d_i.data_ptr(), side.cuda_stream), max_leaf,
                       num_vertices=v.shape[0], num_indices=i.size, keys=keys)


@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("max_leaf", [1, 4])
@pytest.mark.parametrize("name", ALL)
def test_build_bvh_equals_the_twin(pair, name, max_leaf, keys):
    """Nodes and references, host form and device form."""
    r = pair[0]
    v, i = mesh(name)
    want = twin(name, max_leaf, keys == "extent")
    mask = _mask(name, *want)
    n1 = _same_tree(r.build_bvh(v, i, max_leaf, keys=keys), want, mask, f"{name} max_leaf {max_leaf} {keys}, host form")
    n2 = _same_tree(_device_build(r, v, i, max_leaf, keys), want, mask, f"{name} max_leaf {max_leaf} {keys}, device form")
    print(f"{name} max_leaf {max_leaf} {keys}: words excused by the zero rule: host form {n1}, device form {n2}")


def _compare_scenes(a, b, d, nodes, refs, verts, mask, label):
    """A's scene against B's upload of (nodes, refs, verts): image, header, bounds.  Returns the words excused."""
    ia = scene_image(a)
    if mask is None:
        b.upload(uploaded(d, (nodes, refs), verts))
        ib, im = scene_image(b), None
    else:                                              # the image words an excusable node word reaches
        b.upload(uploaded(d, (flipped(nodes, mask), refs), verts))
        other = scene_image(b)
        b.upload(uploaded(d, (nodes, refs), verts))
        ib = scene_image(b)
        im = ib != other
    assert ia[HDR_FAST_DIV] == ib[HDR_FAST_DIV], f"{label}: fast_div {ia[HDR_FAST_DIV]} vs {ib[HDR_FAST_DIV]}"
    n = excused(ia, ib, im, f"{label}: scene image")
    (amn, amx), (bmn, bmx) = a.scene_bounds(), b.scene_bounds()
    n += excused(amn, bmn, None if mask is None else mask[0, 0:3], f"{label}: bounds min {amn} vs {bmn}")
    n += excused(amx, bmx, None if mask is None else mask[0, 4:7], f"{label}: bounds max {amx} vs {bmx}")
    return n


def _refit(d, nodes, refs, verts):
    """rt_refit_nodes of the tree to other vertices."""
    return rtamd.refit_nodes(uploaded(d, (nodes, refs)), verts)


@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("max_leaf", [1, 4])
@pytest.mark.parametrize("name", ALL)
def test_build_scene_equals_an_upload_of_the_twin_and_refits(pair, name, max_leaf, keys):
    """The built scene; then update_vertices to the seeded displacement, to the vertices scaled by
    1.125 and back to the mesh's own, each against an upload of rt_refit_nodes' arrays; for a mesh
    that is an edge transform of a tame one, the tame mesh built and updated to the edge vertices
    and back."""
    a, b = pair
    d = arrays(name)
    v = d["vertices"]
    nodes, refs = twin(name, max_leaf, keys == "extent")
    label = f"{name} max_leaf {max_leaf} {keys}"
    a.build_scene(d, max_leaf, keys=keys)
    counts = [_compare_scenes(a, b, d, nodes, refs, None, _mask(name, nodes, refs), f"{label}: built")]
    ia = scene_image(a)
    assert ia[HDR_N_INNER] == (nodes.shape[0] - 1) // 2 and ia[HDR_CLEAN] == 1
    ca, cb = a.refit_level_counts(), b.refit_level_counts()
    assert np.array_equal(ca, cb) and ca.tolist() == height_counts(nodes), f"{label}: records per height {ca} vs {cb}"
    if name in LATTICE and max_leaf == 1 and keys == "axis":
        assert ca[:3].tolist() == HEIGHTS[name]
    if name in FINITE:
        got, want = a.scene_sah(), np_scene_sah(nodes)
        for g, w, what in zip(got[:3], want, ("inner_area", "leaf_area_tris", "root_area")):
            print(f"{label}: {what} {g!r} vs {w!r}")
            assert abs(g - w) <= SAH_RTOL * abs(w), f"{label}: {what} {g!r} vs {w!r}"
    with np.errstate(all="ignore"):
        scaled = np.array(v, F, copy=True)
        scaled[:, :3] *= F(1.125)
    for what, v2 in (("moved", moved_vertices(name)), ("scaled", scaled), ("back", v)):
        a.update_vertices(v2)
        want = _refit(d, nodes, refs, v2)
        counts.append(_compare_scenes(a, b, d, want, refs, v2, _mask(name, want, refs, v2), f"{label}: {what}"))
    base = base_vertices(name)
    if base is not None:
        tame = dict(d, vertices=base)
        t = rtamd.Mesh.from_arrays(base, d["indices"]).build_lbvh(max_leaf, keys=keys)
        a.build_scene(tame, max_leaf, keys=keys)
        _compare_scenes(a, b, tame, t.nodes, t.tri_indices, None, None, f"{label}: tame build")
        for what, v2 in (("tame build to the edge vertices", v), ("tame build back", base)):
            a.update_vertices(v2)
            want = _refit(tame, t.nodes, t.tri_indices, v2)
            counts.append(_compare_scenes(a, b, tame, want, t.tri_indices, v2, _mask(name, want, t.tri_indices, v2),
                                          f"{label}: {what}"))
    print(f"{label}: words excused by the zero rule per comparison {counts}")


def _boxed(params, nodes):
    p = np.array(params, np.float32, copy=True)
    p[24:27], p[28:31] = nodes[0, 0:3], nodes[0, 4:7]
    return p


FOCUS = {"chain52": (0.08, 0.08, -1.1), "lattice_chain": (0.08, 0.08, -1.1), "two_scale": (0.3, 0.3, -1.6)}   # the eye


def camera(name):
    """The orbit camera, far enough to see all of the mesh.  A lattice mesh's triangles are 0.25 wide
    in a box of 8,192 and nothing nearer than the image plane (1 from the eye) is seen: there the eye
    looks along +z at the triangles at the origin (chain52's deepest leaves) from just over 1 away."""
    v, i = mesh(name)
    m = rtamd.Mesh.from_arrays(v, i)
    if name not in FOCUS:
        return rtamd.params_to_array(m.camera_params(64, 64, radius=max(200.0, 1.5 * float(np.ptp(v[:, :3], axis=0).max()))))
    p = rtamd.params_to_array(m.camera_params(64, 64))
    half = np.float32(np.tan(np.pi / 6))               # the 60 degree field of view of rt_camera_params
    eye = np.array(FOCUS[name], np.float32)
    p[0:3], p[4:7] = (2 * half, 0, 0), (0, 2 * half, 0)
    p[8:11] = eye + np.array([-half, -half, 1], np.float32)
    p[12:15] = eye
    return p


@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("max_leaf", [1, 4])
@pytest.mark.parametrize("name", FINITE)
def test_finite_meshes_render_as_the_oracle_renders_the_twin(pair, name, max_leaf, keys):
    """One 64 x 64 depth-3 strict frame: hits, t, rgb and packed pixels; no stack overflow (chain52
    is 52 deep, the stack holds 64)."""
    from oracle import oracle
    a, b = pair
    d = arrays(name)
    nodes, refs = twin(name, max_leaf, keys == "extent")
    a.build_scene(d, max_leaf, keys=keys)
    # only a scene found equal to the upload is traversed
    _compare_scenes(a, b, d, nodes, refs, None, _mask(name, nodes, refs), f"{name} max_leaf {max_leaf} {keys}: built")
    p = _boxed(camera(name), nodes)
    a.set_params(p)
    gpu = a.render(64, 64, depth=3, flags=STRICT, aux=True)
    e = dict(d, nodes=nodes, tri_indices=refs)
    ref = oracle.render(e, p, 64, 64, depth=3)
    assert ref["stats"]["stack_overflow"] == 0 and a.overflow_count() == 0
    hit = int(np.count_nonzero(ref["hits"][:, 0, 0] >= 0))
    print(f"{name} max_leaf {max_leaf} {keys}: {hit} hit pixels")
    assert np.array_equal(gpu["hits"], ref["hits"]), "hits"
    assert np.array_equal(gpu["t"].view(np.uint32), ref["t"].view(np.uint32)), "t"
    assert np.array_equal(gpu["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), "rgb"
    assert np.array_equal(gpu["out"], ref["out"]), "packed pixels"
    assert hit >= 64


def test_scratch_reuse_large_small_large():
    """One context builds two_scale, rand2k_first255, two_scale at another max_leaf and chain52; after
    each, its build_bvh and its built scene equal a fresh context's."""
    r = rtamd.Renderer(0)
    try:
        for name, max_leaf in (("two_scale", 1), ("rand2k_first255", 4), ("two_scale", 4), ("chain52", 1)):
            v, i = mesh(name)
            d = arrays(name)
            got = r.build_bvh(v, i, max_leaf)
            r.build_scene(d, max_leaf)
            image, counts, bounds = scene_image(r), r.refit_level_counts(), r.scene_bounds()
            fresh = rtamd.Renderer(0)
            try:
                _same_tree(got, fresh.build_bvh(v, i, max_leaf), None, f"{name} max_leaf {max_leaf}: build_bvh after reuse")
                fresh.build_scene(d, max_leaf)
                excused(image, scene_image(fresh), None, f"{name} max_leaf {max_leaf}: built scene after reuse")
                assert np.array_equal(counts, fresh.refit_level_counts())
                assert np.array_equal(np.concatenate(bounds), np.concatenate(fresh.scene_bounds()))
            finally:
                fresh.close()
            _same_tree(got, twin(name, max_leaf), None, f"{name} max_leaf {max_leaf}: against the twin")
    finally:
        r.close()
