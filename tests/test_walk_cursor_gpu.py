"""The depth-1 kernels' cursor loop and the walk references it walks by (DESIGN.md 7.1,
csrc/rt_records.h), on hand-built trees at the edges of what a walk reference can say: leaves of 1, 2, 15
and 16 references and an empty leaf (one trip on the all-zero pad record, which must never hit), and the
same tree with a leaf of 17, which has no walk references and renders by the general traversal.  Every
frame is 64 x 64.

- The derived array: after every way a scene comes onto the device (upload, image load, scene copy,
  rt_build_scene) the array read back from the device (rt_scene_walk_refs) equals, word for word, what
  the deriving kernel's host twin makes of the same records; rt_update_vertices leaves it as it is;
  walk16 has one and nowalk17 has none, so the frame tests below do run the loop they are about.
- Frames: the CPU oracle (S_strict, bitwise: hit ids, t, rgb, packed pixels); for S_ref and S_hw the same
  scene on a context whose records are split (RTAMD_RECORD_LIMIT: the general traversal) and on a
  context installed without walk references (RTAMD_NO_WALK: the other form of the same loop); single
  launches with aux planes and batches of 4 (a batch launch has no aux planes: its frames are compared
  with the single launches' packed pixels); before and after a refit.  walk16's shadow rays include
  ten whose first accepted hit is the last record of a 16-reference leaf.
- rt_fetch_counts: all eight counters equal the other loop form's in the three arithmetics, and in
  S_strict the oracle's visit counts.
Both comparisons also run on the fixtures the other depth-1 tests use (SCENES below): a deep-stack
restart, a root that is a leaf, rand3k_bigleaf, the escape tree and a kRefError child; each test first
asserts whether the scene has walk references, so it is known which loop it ran."""
import os

import numpy as np
import pytest

from refit_common import _finish, _node, _triangles, moved_vertices, np_refit, scene_arrays, with_vertices
from test_trip_paths_gpu import (H, HW, STRICT, W, _batch_render, _cams, _compare, _device_render, _oracle, _scene_dict,
                                 general)  # noqa: F401  (general: a fixture)

pytestmark = pytest.mark.gpu

_TREES = {}
COUNTS = {"walk16": [1, 16, 2, 0, 15, 16], "nowalk17": [1, 16, 2, 0, 15, 17]}
LAST_OF_16 = 3 * 16   # walk16: the id of reference 16, the last of the first 16-reference leaf (references 1..16)


def _comb(counts, seed=11):
    """Inner node i = node 2i: left = leaf 2i+1 with counts[i] references, right = inner i+1 or, for the
    last inner node, the last leaf.  Triangles in reference order inside a 40-unit cube."""
    ntri = max(sum(counts), 1)
    verts = _triangles(np.random.default_rng(seed), ntri, 20.0)
    n = len(counts)
    nodes = np.zeros((2 * n - 1, 12), np.float32)
    off = 0
    for i, c in enumerate(counts[:-1]):
        _node(nodes, 2 * i, 2 * i + 1, 2 * i + 2, -1, 0)
        _node(nodes, 2 * i + 1, -1, -1, off if c else -1, c)
        off += c
    _node(nodes, 2 * n - 2, -1, -1, off if counts[-1] else -1, counts[-1])
    for k, c in enumerate(counts):   # an empty leaf keeps a box of its own (refit_common.bigleaf), among the triangles
        if c == 0:
            j = 2 * k + 1 if k < n - 1 else 2 * n - 2
            nodes[j, 0:3] = (-6.0, -6.0, -6.0)
            nodes[j, 4:7] = (6.0, 6.0, 6.0)
    return _finish(verts, nodes, 3 * np.arange(ntri))


def _tree(name):
    if name not in _TREES:
        import rtamd
        d = _comb(COUNTS[name])
        m = rtamd.Mesh.from_arrays(d["vertices"], d["indices"])
        d["params"] = rtamd.params_to_array(m.camera_params(W, H, radius=70.0))
        _TREES[name] = d
    return _TREES[name]


# The fixtures of the frame and fetch-count comparisons: the two hand-built trees, and overflow_comb (a
# stack deeper than the LDS part: the traversal restarts in the general code), single_tri_rootleaf (the
# root is a leaf), rand3k_bigleaf, escape40 (refit_common's leaves of 40 and 35 through the escape table)
# and bad_node (a reachable kRefError child: an unclean scene).
SCENES = ["walk16", "nowalk17", "overflow_comb", "single_tri_rootleaf", "rand3k_bigleaf", "escape40", "bad_node"]
WALK = {"walk16", "overflow_comb", "single_tri_rootleaf", "rand3k_bigleaf", "rand2k"}   # scenes with walk references
RESTARTS = {"overflow_comb"}
NOT_REFITTABLE = {"overflow_comb", "bad_node"}   # a node with two parents; a malformed inner node
UNCLEAN = {"bad_node"}


def _scene(name):
    return _tree(name) if name in COUNTS else _scene_dict(name)


def _moved(name, d):
    """The scene after a refit: moved vertices (a seeded displacement) and the refit's nodes."""
    if name in COUNTS:
        v = np.array(d["vertices"], np.float32, copy=True)
        v[:, :3] += np.random.default_rng(3).uniform(-0.5, 0.5, (v.shape[0], 3)).astype(np.float32)
    else:
        v = moved_vertices("bigleaf" if name == "escape40" else name)
    nodes, _ = np_refit(d, v)
    return v, with_vertices(d, v, nodes)


def _steps(renderer, name):
    """The scene as uploaded and, where it can be refitted, after rt_update_vertices; a scene that
    cannot must refuse and stay as it was.  Yields (label, the scene dict the renderer now holds)."""
    import rtamd
    d0 = _scene(name)
    renderer.upload(rtamd.Scene.from_arrays(d0))
    assert (renderer.walk_refs()[0].size > 0) == (name in WALK), name
    yield "as uploaded", d0
    if name in NOT_REFITTABLE:
        with pytest.raises(rtamd.RtError):
            renderer.update_vertices(d0["vertices"])
        return
    v, d1 = _moved(name, d0)
    renderer.update_vertices(v)
    assert (renderer.walk_refs()[0].size > 0) == (name in WALK), name
    yield "after a refit", d1


@pytest.fixture(scope="module")
def plain():
    """A context whose scenes are installed without walk references (RTAMD_NO_WALK): its depth-1 frames
    and fetch counts come from the other form of the loop, the parent's."""
    import rtamd
    r = rtamd.Renderer(0)

    def upload(d):
        old = os.environ.get("RTAMD_NO_WALK")
        os.environ["RTAMD_NO_WALK"] = "1"
        try:
            r.upload(rtamd.Scene.from_arrays(d))
        finally:
            if old is None:
                del os.environ["RTAMD_NO_WALK"]
            else:
                os.environ["RTAMD_NO_WALK"] = old
        assert r.walk_refs()[0].size == 0
        return r
    yield upload
    r.close()


def _same_as_twin(r, label, want):
    words, root = r.walk_refs()
    twin, twin_root = r.walk_refs(host_twin=True)
    assert (words.size > 0) == want, f"{label}: walk references {'missing' if want else 'present'}"
    assert np.array_equal(words, twin) and root == twin_root, f"{label}: the device array is not the host twin's"
    return words, root


def test_the_derived_array_is_the_host_twins_on_every_install_path():
    import rtamd
    import torch
    ctx, src = rtamd.Renderer(0), rtamd.Renderer(0)
    images = []
    try:
        d = _tree("walk16")
        ctx.upload(rtamd.Scene.from_arrays(d))
        words, root = _same_as_twin(ctx, "upload walk16", True)
        assert words.size == 2 * 5 and root == 0   # five inner records; the root is record 0
        # leaves in record order: 1, 16, 2, 0, 15 on the left, the next record (or the last leaf) on the right
        assert [int(w >> 27) & 15 for w in words[0::2]] == [0, 15, 1, 0, 14] and all(int(w) >> 31 for w in words[0::2])
        assert int(words[9]) >> 31 and (int(words[9]) >> 27) & 15 == 15
        assert [int(w) for w in words[1:9:2]] == [4, 8, 12, 16]
        v, _ = _moved("walk16", d)
        ctx.update_vertices(v)
        again, root2 = _same_as_twin(ctx, "walk16 after rt_update_vertices", True)
        assert np.array_equal(again, words) and root2 == root

        ctx.upload(rtamd.Scene.from_arrays(_tree("nowalk17")))
        _same_as_twin(ctx, "upload nowalk17", False)

        g = scene_arrays("rand2k")
        src.upload(rtamd.Scene.from_arrays(g))
        up, up_root = _same_as_twin(src, "upload rand2k", True)
        n = src.scene_image_size()
        img = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        src.pack_scene(img.data_ptr(), n)
        images.append(img)
        ctx.load_scene(img.data_ptr(), n)
        w2, r2 = _same_as_twin(ctx, "image load rand2k", True)
        assert np.array_equal(w2, up) and r2 == up_root
        ctx.upload(rtamd.Scene.from_arrays(_tree("nowalk17")))
        ctx.copy_scene_from(src)
        w3, r3 = _same_as_twin(ctx, "scene copy rand2k", True)
        assert np.array_equal(w3, up) and r3 == up_root

        c = scene_arrays("cornell12")
        ctx.build_scene(c)
        built, broot = _same_as_twin(ctx, "rt_build_scene cornell12", True)
        ctx.update_vertices(np.array(c["vertices"], np.float32) * np.float32(1.25))
        b2, broot2 = _same_as_twin(ctx, "built cornell12 after rt_update_vertices", True)
        assert np.array_equal(b2, built) and broot2 == broot
    finally:
        ctx.close()
        src.close()


@pytest.mark.parametrize("name", SCENES)
def test_cursor_frames_equal_the_oracle_and_both_other_traversals(renderer, general, plain, name):
    """S_strict against the oracle, S_ref and S_hw against the general traversal and against the other form
    of the loop, aux planes bitwise; batches of 4 against the single launches; as uploaded and after a
    refit.  A scene without walk references (nowalk17, escape40, bad_node) takes the host's fallback."""
    for step, d in _steps(renderer, name):
        g, p0 = general(d), plain(d)
        cams = _cams(d, 4)
        singles = {}
        for i, p in enumerate(cams):
            ref = _oracle(d, p)
            if i == 0 and step == "as uploaded" and name in COUNTS:
                assert int((ref["hits"][:, 0, 0] >= 0).sum()) > 100, "the camera sees the triangles"
                if name == "walk16":   # any-hit: 15 misses, then the first accepted hit on the leaf's last record
                    assert int((ref["hits"][:, 0, 1] == LAST_OF_16).sum()) >= 5
            s = _device_render(renderer, p, STRICT)
            _compare(s, ref, f"{name} {step} cam {i} S_strict vs the oracle")
            if i == 0 and name in RESTARTS:
                assert renderer.last_deferred() > 0, "the deep stack restarts in the general code"
            singles[(STRICT, i)] = s["out"]
            for flags in (0, HW):
                f = _device_render(renderer, p, flags)
                if i == 0 and name in RESTARTS:
                    assert renderer.last_deferred() > 0
                _compare(f, _device_render(g, p, flags), f"{name} {step} cam {i} flags {flags} vs the general traversal")
                _compare(f, _device_render(p0, p, flags), f"{name} {step} cam {i} flags {flags} vs the loop without walk references")
                singles[(flags, i)] = f["out"]
        if name not in RESTARTS:
            assert renderer.last_deferred() == 0
        for flags in (STRICT, 0, HW):
            frames = _batch_render(renderer, cams, flags)
            for i in range(4):
                assert np.array_equal(frames[i], singles[(flags, i)]), (name, step, flags, i)


@pytest.mark.parametrize("name", SCENES + ["rand2k"])
def test_fetch_counts_of_the_cursor_loop_are_the_other_forms(renderer, plain, name):
    """All eight counters, word for word, against the same kernel's loop without walk references
    (an empty leaf's trip is keyed as that form keys it: the record its reference names), in S_strict,
    S_ref and S_hw, as uploaded and after a refit; across a deep-stack restart the counts up to the
    overflow must agree too.  S_strict also against the oracle: inner fetches == its inner visits,
    triangle fetches == its triangle tests plus at most one per leaf visit (an empty leaf's dropped
    test); a restarted traversal's fetches are not counted, so overflow_comb stays below.  An unclean
    scene has no counting kernel in either form."""
    import rtamd
    for step, d in _steps(renderer, name):
        p0 = plain(d)
        for r in (renderer, p0):
            r.set_params(d["params"])
        if name in UNCLEAN:
            for r in (renderer, p0):
                with pytest.raises(rtamd.RtError):
                    r.fetch_counts(W, H, 1, STRICT)
            continue
        for flags in (STRICT, 0, HW):
            fr, other = renderer.fetch_counts(W, H, 1, flags), p0.fetch_counts(W, H, 1, flags)
            assert (renderer.last_deferred() > 0) == (name in RESTARTS)
            print(name, step, flags, fr)
            assert fr == other, (name, step, flags, fr, other)
        fr = renderer.fetch_counts(W, H, 1, STRICT)
        st = _oracle(d, d["params"])["stats"]
        kinds = ("primary", "shadow", "secondary")
        inner = sum(st[k]["inner"] for k in kinds)
        tris = sum(st[k]["tris"] for k in kinds)
        leaves = sum(st[k]["leaf"] for k in kinds)
        if name in RESTARTS:
            assert fr["inner"] <= inner and fr["tri"] <= tris + leaves
        else:
            assert fr["inner"] == inner, (name, step)
            assert tris <= fr["tri"] <= tris + leaves, (name, step)
