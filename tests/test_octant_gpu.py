"""The octant loops of the fast traversal: a wave whose active rays share their
three direction signs, none zero, runs a copy of the loop in which the slab test's near and far
planes are picked by name.  RT_FLAG_EXACT_DIV forces the generic division form, so a frame with
flags f must equal the frame with f | RT_FLAG_EXACT_DIV in hits, t, rgb and packed pixels, and in
S_strict also the CPU oracle, for cameras in each octant, on an axis and across a sign change;
rt_loop_variant_counts says which loop the waves took; a scene with an inverted child box is kept
out of the fast quotient altogether."""
import numpy as np
import pytest

from conftest import load_golden
from octant_common import (H, W, axis_params, octant_of, octant_params, ray_dirs, straddle_params, two_leaf_scene)

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4
STRICT, WAVEFRONT, EXACT_DIV = 64, 8, 4
MODES = {"ref": 0, "strict": STRICT, "hw": 2}
HDR_FAST_DIV = 12   # ImageHeader::fast_div, in words
SCENES = ["knot16k", "hf40k"]
CAMERAS = [f"oct{k}" for k in range(8)] + ["axis", "straddle"]


def _compare(gpu, ref, label):
    assert np.array_equal(gpu["hits"], ref["hits"]), f"{label}: hit ids differ at " \
        f"{np.argwhere(gpu['hits'] != ref['hits'])[:5].tolist()}"
    assert np.array_equal(gpu["t"].view(np.uint32), ref["t"].view(np.uint32)), f"{label}: t differs"
    assert np.max(np.abs(gpu["rgb"] - ref["rgb"])) <= RGB_TOL, f"{label}: rgb beyond 1e-4"
    assert np.array_equal(gpu["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), f"{label}: rgb not bitwise"
    assert np.array_equal(gpu["out"], ref["out"]), f"{label}: packed pixels differ"


def _camera(d, name, cam):
    """(params, w, h) of camera `cam`, its rays checked on the host to be what its name says."""
    if cam == "axis":
        w = h = 65
        p = axis_params(d, name)
        dirs = ray_dirs(p, w, h)
        assert np.all(dirs[:, 33, 0] == 0.0) and np.all(dirs[33, :, 1] == 0.0)
        return p, w, h
    if cam == "straddle":
        p = straddle_params(d)
        dirs = ray_dirs(p, W, H)
        assert np.any(dirs[..., 0] < 0) and np.any(dirs[..., 0] > 0)
        return p, W, H
    k = int(cam[3:])
    p = octant_params(d, k)
    assert octant_of(ray_dirs(p, W, H)) == k
    return p, W, H


def _upload(renderer, name):
    import rtamd
    d = load_golden(name)
    renderer.upload(rtamd.Scene.from_arrays(d))
    return d


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("name", SCENES)
def test_octant_cameras_equal_the_division_form(renderer, name, cam):
    from oracle import oracle
    d = _upload(renderer, name)
    p, w, h = _camera(d, name, cam)
    renderer.set_params(p)
    for depth in (1, 3):
        ref = oracle.render(d, p, w, h, depth=depth)
        assert np.any(ref["hits"][:, 0, 0] >= 0), "the camera sees nothing"
        for wf in (0, WAVEFRONT):
            for mode, mflag in MODES.items():
                f = mflag | wf
                fast = renderer.render(w, h, depth=depth, flags=f, aux=True)
                slow = renderer.render(w, h, depth=depth, flags=f | EXACT_DIV, aux=True)
                label = f"{name} {cam} depth={depth} wavefront={bool(wf)} {mode}"
                _compare(fast, slow, label + " vs EXACT_DIV")
                if mode == "strict":
                    _compare(fast, ref, label + " vs oracle")


@pytest.mark.parametrize("name", SCENES)
def test_loop_variant_counts(renderer, name):
    d = _upload(renderer, name)
    for k in range(8):
        p, w, h = _camera(d, name, f"oct{k}")
        renderer.set_params(p)
        c = renderer.loop_variant_counts(w, h, 1, 0)
        assert c["closest"][1 + k] > 0, (k, c)
        assert all(c["closest"][1 + j] == 0 for j in range(8) if j != k), (k, c)
        assert sum(c["closest"]) <= (w // 8) * (h // 8) and sum(c["any"]) <= sum(c["closest"]), (k, c)
        e = renderer.loop_variant_counts(w, h, 1, EXACT_DIV)
        assert e["closest"][0] == sum(c["closest"]) and e["any"][0] == sum(c["any"]), (k, c, e)
        assert not any(e["closest"][1:]) and not any(e["any"][1:]), (k, e)
    p, w, h = _camera(d, name, "axis")
    renderer.set_params(p)
    c = renderer.loop_variant_counts(w, h, 1, 0)
    assert c["closest"][0] > 0, c
    p, w, h = _camera(d, name, "straddle")
    renderer.set_params(p)
    c = renderer.loop_variant_counts(w, h, 1, 0)
    assert c["closest"][0] > 0 and sum(c["closest"][1:]) > 0, c   # the middle tiles straddle, the others do not
    # the fetch counters keep their meaning (and their refusal of the division form)
    import rtamd
    with pytest.raises(rtamd.RtError):
        renderer.fetch_counts(w, h, 1, EXACT_DIV)


@pytest.mark.parametrize("name", SCENES)
def test_one_batch_launch_of_four_octants(renderer, name):
    import torch
    d = _upload(renderer, name)
    cams = [_camera(d, name, f"oct{k}")[0] for k in (0, 3, 5, 6)]
    for flags in (0, STRICT, 2):
        want = []
        for p in cams:
            renderer.set_params(p)
            dev = torch.full((W * H,), -1, dtype=torch.int32, device="cuda")
            renderer.render_device(W, H, 1, flags, dev.data_ptr())
            torch.cuda.synchronize()
            want.append(dev.cpu().numpy().view(np.uint32).copy())
        out = torch.full((4 * W * H,), -7, dtype=torch.int32, device="cuda")
        renderer.render_device_batch(W, H, 1, flags, cams, out.data_ptr(), W * H)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32).reshape(4, W * H)
        for i in range(4):
            assert np.array_equal(got[i], want[i]), (name, flags, i, int(np.sum(got[i] != want[i])))
        assert len({w_.tobytes() for w_ in want}) == 4, "the four cameras should give four different frames"


def test_inverted_child_box_takes_the_division_form(renderer):
    from oracle import oracle
    from refit_common import scene_image
    for inverted in (True, False):
        s, p = two_leaf_scene(inverted)
        renderer.upload(s)
        renderer.set_params(p)
        assert scene_image(renderer)[HDR_FAST_DIV] == (0 if inverted else 1)
        for depth in (1, 3):
            ref = oracle.render(s, p, W, H, depth=depth)
            assert np.any(ref["hits"][:, 0, 0] >= 0)
            _compare(renderer.render(W, H, depth=depth, flags=STRICT, aux=True), ref, f"inverted={inverted} strict")
            for mode in ("ref", "hw"):
                fast = renderer.render(W, H, depth=depth, flags=MODES[mode], aux=True)
                slow = renderer.render(W, H, depth=depth, flags=MODES[mode] | EXACT_DIV, aux=True)
                _compare(fast, slow, f"inverted={inverted} {mode} depth={depth}")
