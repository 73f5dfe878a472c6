"""Shading at its edges on the GPU: every case of tests/shading_edge_common.py (lights,
normals, Cramer determinants, albedo, the pixel pack, depth 5 and 8, the scene box in the params)
through every kernel that shades.  tests/test_shading_edges.py shows on the CPU that the cases reach
their edges and pins the oracle's shading to a float64 restatement.

S_strict (RT_FLAG_STRICT_MATH) against the oracle, no pixel excluded: hits and t bit for bit, packed
pixels equal, rgb bit for bit -- where the oracle's value is NaN the GPU's must be NaN too and its
payload and sign are not compared (x86 and gfx950 produce different default NaNs).  The kernels: the
fused one (depth >= 2), the wavefront ones with and without the ray sort, the depth-1 one with and
without the shadow ray, and the depth-1 batch kernel with four lights in one launch.

S_ref (flags 0) and S_hw (RT_FLAG_HW_MATH) have no CPU oracle: their fused and wavefront frames equal
each other word for word, and on one case of each class the depth-3 frame equals the reference kernel
run live (oracle/_ref, a child process per run, one after another) with no differing pixel."""
import numpy as np
import pytest

import shading_edge_common as S

pytestmark = pytest.mark.gpu

NO_SHADOW, HW, WAVEFRONT, WF_SORT, STRICT = 1, 2, 8, 32, 64
# (name, depth of the frame or None for the case's own, flags, the oracle frame it must equal)
PATHS = [("fused", None, 0, "d"), ("wavefront", None, WAVEFRONT, "d"), ("wavefront sorted", None, WAVEFRONT | WF_SORT, "d"),
         ("depth 1", 1, 0, "d1"), ("depth 1 no shadow", 1, NO_SHADOW, "d1ns")]
BATCH_LIGHTS = ["light/below_floor", "light/skims_floor", "light/at_camera", "light/distance_1e30"]
# One case of each class against the reference kernel (two of det: a zero determinant and the 1e4
# offset), then normalize's copysign branch and an infinite colour.  (All 40 cases were run once against
# both builds of the reference kernel: no differing pixel; DESIGN.md 3.1.  A run starts two child
# processes, which is what its second or so goes to, hence not all of them every time.)
LIVE = ["light/distance_1e30", "normals/nan_component", "det/floor_y0", "det/offset_1e4", "albedo/nan", "pack/negative",
        "depth/room_8", "box/nan_word", "normals/inf_component", "albedo/3e38"]


def put(renderer, c):
    import rtamd
    renderer.upload(rtamd.Scene.from_arrays(c.scene))
    renderer.set_params(c.params)


def same_rgb(got, want):
    """Bit for bit; where `want` is NaN, `got` is NaN (payload and sign not compared)."""
    nan = np.isnan(want)
    return np.where(nan, np.isnan(got), S.bits(got) == S.bits(want))


def same_frame(got, want, label):
    bad = np.argwhere(got["hits"] != want["hits"])
    assert bad.size == 0, f"{label}: {len(bad)} hit ids differ, first at {bad[:3].tolist()}"
    bad = np.argwhere(S.bits(got["t"]) != S.bits(want["t"]))
    assert bad.size == 0, f"{label}: {len(bad)} t differ, first at {bad[:3].tolist()}"
    bad = np.argwhere(~same_rgb(got["rgb"], want["rgb"]))
    assert bad.size == 0, (f"{label}: {len(bad)} rgb words differ, first at {bad[:3].tolist()}: "
                           f"{got['rgb'][bad[0, 0]]} vs {want['rgb'][bad[0, 0]]}")
    bad = np.flatnonzero(got["out"] != want["out"])
    assert bad.size == 0, f"{label}: {bad.size} packed pixels differ, first {bad[:3]}: " \
                          f"{[hex(v) for v in got['out'][bad[:3]]]} vs {[hex(v) for v in want['out'][bad[:3]]]}"


def test_the_lists_name_cases():
    assert set(BATCH_LIGHTS + LIVE) <= set(S.LABELS)
    assert {label.split("/")[0] for label in LIVE} == set(S.CLASSES)


@pytest.mark.parametrize("label", S.LABELS)
def test_strict_equals_the_oracle(renderer, label):
    """S_strict, aux on, through the five paths: every word of hits, t, rgb and the packed pixels is the
    oracle's on every pixel, and no traversal overflows its stack where the oracle's does not."""
    c = S.case(label)
    want = S.frames(c)
    assert c.depth >= 2
    put(renderer, c)
    before = renderer.overflow_count()
    for name, depth, flags, key in PATHS:
        depth = c.depth if depth is None else depth
        got = renderer.render(c.w, c.h, depth=depth, flags=flags | STRICT, aux=True)
        same_frame(got, want[key], f"{label} {name} (depth {depth})")
        assert want[key]["stats"]["stack_overflow"] == 0 and renderer.overflow_count() == before, f"{label} {name}"


def test_four_lights_in_one_batch_launch(renderer):
    """At depth 1 a batch launch carries each frame's own light: four cases of the light class that share
    the stage and the camera in ONE render_device_batch launch.  Each frame equals its own single render,
    in all three arithmetics, and in S_strict the oracle's packed pixels."""
    import torch
    cs = [S.case(label) for label in BATCH_LIGHTS]
    for c in cs[1:]:
        assert all(c.scene[k].tobytes() == cs[0].scene[k].tobytes() for k in S.MESH_KEYS)
        assert np.array_equal(np.delete(c.params, np.arange(16, 20)), np.delete(cs[0].params, np.arange(16, 20)))
    assert len({c.params[16:19].tobytes() for c in cs}) == len(cs)
    w, h = cs[0].w, cs[0].h
    put(renderer, cs[0])
    for flags in (STRICT, 0, HW, STRICT | NO_SHADOW):
        out = torch.full((len(cs) * w * h,), -7, dtype=torch.int32, device="cuda")
        renderer.render_device_batch(w, h, 1, flags, [c.params for c in cs], out.data_ptr(), w * h)
        torch.cuda.synchronize()
        frames = out.cpu().numpy().view(np.uint32).reshape(len(cs), w * h)
        for c, frame in zip(cs, frames):
            renderer.set_params(c.params)
            single = renderer.render(w, h, depth=1, flags=flags)
            assert np.array_equal(frame, single), f"{c.label} flags {flags}: {int(np.sum(frame != single))} pixels differ"
            if flags & STRICT:
                assert np.array_equal(frame, S.frames(c)["d1ns" if flags & NO_SHADOW else "d1"]["out"]), c.label


@pytest.mark.parametrize("label", S.LABELS)
def test_ref_and_hw_paths_agree(renderer, label):
    """S_ref and S_hw: the fused frame and the wavefront frames (sorted and not) at the case's depth are
    equal word for word -- packed pixels, hits, t and rgb (a NaN against a NaN) -- and the depth-1 frame's
    first ray is the fused frame's.  Their clamp is v_med3_f32, which for a NaN returns the smallest of
    the other two as fmin(fmax(x, lo), hi) does: a NaN or negative channel packs 0 and +inf packs 255, as
    in S_strict, and a channel is NaN, +inf or negative where the oracle's is (the cases make those from
    the albedo alone, which every arithmetic treats alike)."""
    c = S.case(label)
    put(renderer, c)
    want = S.frames(c)["d"]
    for mode, f in (("S_ref", 0), ("S_hw", HW)):
        fused = renderer.render(c.w, c.h, depth=c.depth, flags=f, aux=True)
        with np.errstate(invalid="ignore"):
            for ch in range(3):
                byte, v, o = (fused["out"] >> (8 * ch)) & 0xFF, fused["rgb"][:, ch], want["rgb"][:, ch]
                assert np.all(byte[np.isnan(v) | (v <= 0)] == 0) and np.all(byte[v >= 1] == 255), f"{label} {mode}: the pack"
                if c.cls in ("albedo", "pack"):
                    assert np.array_equal(np.isnan(v), np.isnan(o)), f"{label} {mode}: the NaN channels are the oracle's"
        if label == "albedo/3e38":
            assert int(np.isposinf(fused["rgb"][:, 0]).sum()) >= S.MIN_PIXELS, f"{mode}: +inf reaches the pack"
        for name, extra in (("wavefront", WAVEFRONT), ("wavefront sorted", WAVEFRONT | WF_SORT)):
            same_frame(renderer.render(c.w, c.h, depth=c.depth, flags=f | extra, aux=True), fused,
                       f"{label} {mode} {name} vs fused")
        d1 = renderer.render(c.w, c.h, depth=1, flags=f, aux=True)
        assert np.array_equal(d1["hits"][:, 0], fused["hits"][:, 0]), f"{label} {mode}: depth 1 vs fused, bounce 0"
        assert np.array_equal(S.bits(d1["t"][:, 0]), S.bits(fused["t"][:, 0])), f"{label} {mode}: depth 1 vs fused, t"


@pytest.mark.parametrize("label", LIVE)
def test_ref_and_hw_equal_the_reference_kernel(renderer, label, tmp_path):
    """The depth-3 frame (the reference kernel's compiled-in depth, with its shadow ray) in S_ref against
    the reference kernel as its host builds it, and in S_hw against its correctly rounded build, run live:
    no differing pixel, fused and wavefront."""
    from oracle import ref_ocl
    if not ref_ocl.available():
        pytest.skip("oracle/_ref (the reference kernel's code objects) not in this snapshot")
    c = S.case(label)
    put(renderer, c)
    for mode, f, variant in (("S_ref", 0, "default"), ("S_hw", HW, "strict")):
        ref = ref_ocl.render_subprocess(c.scene, c.params, c.w, c.h, variant, str(tmp_path), timeout=120)
        for name, extra in (("fused", 0), ("wavefront", WAVEFRONT)):
            out = renderer.render(c.w, c.h, depth=3, flags=f | extra)
            nd = int(np.sum(out != ref))
            print(f"{label} {mode} {name} vs the reference kernel ({variant}): {nd} of {out.size} pixels differ")
            assert nd == 0, f"{label} {mode} {name}: first at {np.flatnonzero(out != ref)[:5]}"
