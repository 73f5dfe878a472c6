"""The context's scene has one owner.  Two pins across every way a scene is
put on the GPU or replaced: the bytes of the scene image against digests recorded before the
ownership was reworked (tests/golden/scene_image_digests.json), and one context walked through
every replacement in turn, compared after each step with a fresh context brought to the same
scene directly."""
import hashlib
import json
import os

import numpy as np
import pytest

import rtamd
from conftest import GOLDEN, load_golden
from refit_common import scene_image

pytestmark = pytest.mark.gpu

MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")
UPLOADS = ("cornell12", "rand2k", "rand3k_bigleaf", "rand4k_sbvh", "bad_node")
W = H = 64


def _mesh(d, ntri=None):
    e = {k: d[k] for k in MESH_KEYS}
    if ntri is not None:
        e.update(indices=d["indices"][:3 * ntri], normals_indices=d["normals_indices"][:3 * ntri],
                 tri_to_material=d["tri_to_material"][:ntri])
    return e


def image_digests():
    """SHA-256 of the scene image of each pinned scene: the goldens uploaded with their stored
    BVHs (rand3k_bigleaf: escape leaves, rand4k_sbvh: duplicated references, bad_node: an unclean
    tree), and cornell12 and its first triangle alone (a root that is a leaf) built at max_leaf 4."""
    out = {}
    r = rtamd.Renderer(0)
    try:
        for name in UPLOADS:
            r.upload(rtamd.Scene.from_arrays(load_golden(name)))
            out[f"upload:{name}"] = hashlib.sha256(scene_image(r).tobytes()).hexdigest()
        d = load_golden("cornell12")
        for label, ntri in (("cornell12", None), ("cornell12_first1", 1)):
            r.build_scene(_mesh(d, ntri), 4)
            out[f"build4:{label}"] = hashlib.sha256(scene_image(r).tobytes()).hexdigest()
    finally:
        r.close()
    return out


def test_scene_images_keep_their_recorded_bytes():
    with open(os.path.join(GOLDEN, "scene_image_digests.json")) as f:
        want = json.load(f)["sha256"]
    got = image_digests()
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k


def _state(r, params):
    r.set_params(params)
    return scene_image(r), r.render(W, H, depth=3)


def _device(d, side):
    """The mesh on the device: (the dict build_scene takes, its counts, the tensors to keep)."""
    import torch
    keep = {k: torch.from_numpy(np.ascontiguousarray(d[k])).to("cuda:0") for k in MESH_KEYS if k != "materials"}
    dev = {k: (t.data_ptr(), side.cuda_stream) for k, t in keep.items()}
    dev["materials"] = d["materials"]
    counts = {"num_vertices": d["vertices"].shape[0], "num_indices": d["indices"].size,
              "num_normals": d["normals"].shape[0]}
    return dev, counts, keep


def test_one_context_through_every_replacement_of_its_scene():
    """build (host form), upload, build (device form), host-form update_vertices (its staging is
    allocated then), build again, pack_scene, load_scene, copy_scene_from, build, upload -- between
    two meshes of different sizes, so that every step replaces arrays of another size and origin."""
    import torch
    g = {n: load_golden(n) for n in ("cornell12", "rand2k")}
    m = {n: _mesh(g[n]) for n in g}
    side = torch.cuda.Stream(device="cuda:0")
    dev, counts, keep = _device(m["rand2k"], side)
    torch.cuda.synchronize()

    fresh = {}

    def want(key, name, bring):
        """(image, frame) of a fresh context that `bring` takes to the scene directly."""
        if key not in fresh:
            f = rtamd.Renderer(0)
            try:
                bring(f)
                fresh[key] = _state(f, g[name]["params"])
            finally:
                f.close()
        return fresh[key]

    def built(name, max_leaf):
        return lambda f: f.build_scene(m[name], max_leaf)

    def uploaded(name):
        return lambda f: f.upload(rtamd.Scene.from_arrays(g[name]))

    def built_on_device(f):
        f.build_scene(dev, 2, **counts)

    def built_and_updated(f):
        built_on_device(f)
        f.update_vertices(g["rand2k"]["vertices"])

    a, src = rtamd.Renderer(0), rtamd.Renderer(0)
    try:
        def check(step, key, name, bring):
            wi, wf = want(key, name, bring)
            gi, gf = _state(a, g[name]["params"])
            assert gi.shape == wi.shape and np.array_equal(gi, wi), f"step {step}: scene image"
            assert np.array_equal(gf, wf), f"step {step}: frame"
            assert np.count_nonzero(wf) > 0

        a.build_scene(m["cornell12"], 4)
        check(1, "built cornell12", "cornell12", built("cornell12", 4))
        a.upload(rtamd.Scene.from_arrays(g["rand2k"]))
        check(2, "uploaded rand2k", "rand2k", uploaded("rand2k"))
        a.build_scene(dev, 2, **counts)
        check(3, "device rand2k", "rand2k", built_on_device)
        a.update_vertices(g["rand2k"]["vertices"])
        check(4, "updated rand2k", "rand2k", built_and_updated)
        a.build_scene(m["cornell12"], 4)
        check(5, "built cornell12", "cornell12", built("cornell12", 4))
        n = a.scene_image_size()
        buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        a.pack_scene(buf.data_ptr(), n)
        torch.cuda.synchronize()
        check(6, "built cornell12", "cornell12", built("cornell12", 4))
        a.load_scene(buf.data_ptr(), n)
        torch.cuda.synchronize()
        check(7, "built cornell12", "cornell12", built("cornell12", 4))
        src.build_scene(m["rand2k"], 8)
        a.copy_scene_from(src)
        check(8, "built rand2k 8", "rand2k", built("rand2k", 8))
        a.build_scene(m["rand2k"], 2)
        check(9, "built rand2k 2", "rand2k", built("rand2k", 2))
        a.upload(rtamd.Scene.from_arrays(g["cornell12"]))
        check(10, "uploaded cornell12", "cornell12", uploaded("cornell12"))
        assert np.array_equal(fresh["device rand2k"][0], fresh["built rand2k 2"][0])   # the two forms agree
    finally:
        a.close()
        src.close()
    del keep
