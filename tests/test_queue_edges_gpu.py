"""The wavefront ray queues at their edges on the GPU: every case of tests/queue_edge_common.py
-- empty queues, queues of one ray, of exactly one segment, chunk and super-chunk, sparse queues across the
super-chunk boundary, queues alive at bounce 7, every path of the sort key -- through seg_close,
wf_compact_sort_kernel and wf_bounce_kernel.  tests/test_queue_edges.py shows on the CPU that the cases
reach their edges.

S_strict (RT_FLAG_STRICT_MATH) against the oracle, aux planes included, every word: the fused kernel, the
wavefront path unsorted and sorted, each wavefront frame twice (in the static block order, then in the
adaptive one) and the wavefront path without the shadow ray.  Every output buffer is filled with a sentinel
first, so a ray that never finishes shows.  The oracle has S_strict only: in S_ref (flags 0) and S_hw
(RT_FLAG_HW_MATH) the fused frame is the truth and the wavefront frames equal it bit for bit.

On top of that, in S_strict and S_ref: bands of a tiling (their local tile grid, so their segments, differ
from the frame's), batch launches whose frames are different populations under one camera set (K = 4 and 8
take the 16-bucket key; 256 x 48 x 8 crosses a super-chunk boundary with the tile-major interleave),
rt_render_tiled over three contexts, and rt_fetch_counts on the wavefront path."""
import numpy as np
import pytest

import queue_edge_common as Q

pytestmark = pytest.mark.gpu

NO_SHADOW, HW, WAVEFRONT, STATIC_ORDER, WF_SORT, STRICT = 1, 2, 8, 16, 32, 64
# (name, flags on top of the arithmetic, the oracle frame it must equal)
# The fused frame comes first: on the stream's slot it times its blocks, so every later frame of the same size
# without RT_FLAG_STATIC_ORDER runs the longest-first order built from a frame before it.
PATHS = [("fused", 0, "d"), ("wavefront (static order)", WAVEFRONT | STATIC_ORDER, "d"),
         ("wavefront (adaptive order)", WAVEFRONT, "d"),
         ("wavefront sorted (static order)", WAVEFRONT | WF_SORT | STATIC_ORDER, "d"),
         ("wavefront sorted (adaptive order)", WAVEFRONT | WF_SORT, "d"),
         ("wavefront without shadow rays", WAVEFRONT | NO_SHADOW, "ns")]
BAND_CASES = ["pop/lane_counts@super", "pop/super_ends@super", "depth/thinning@super"]
TILINGS = [(1, 3, 8), (0, 2, 16)]   # (rank, nranks, band_rows)
BATCHES = [Q.G_SMALL + (2,), Q.G_SMALL + (4,), Q.G_SMALL + (8,), (256, 48, 8)]


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream()


def test_the_lists_name_cases():
    assert set(BAND_CASES) <= set(Q.LABELS)


@pytest.mark.parametrize("label", Q.LABELS)
def test_strict_equals_the_oracle(renderer, stream, label):
    """S_strict, aux on, through the six paths: every word of hits, t, rgb and the packed pixels is the
    oracle's on every pixel, and no traversal overflows its stack (the oracle's does not)."""
    c = Q.case(label)
    want = Q.frames(c)
    assert c.depth >= 2
    Q.put(renderer, c.scene, c.params)
    before = renderer.overflow_count()
    for name, flags, key in PATHS:
        got = Q.render(renderer, c.w, c.h, c.depth, flags | STRICT, stream)
        Q.same_frame(got, want[key], f"{label} {name} (depth {c.depth})")
    assert want["d"]["stats"]["stack_overflow"] == 0 and renderer.overflow_count() == before, label


@pytest.mark.parametrize("label", Q.LABELS)
def test_ref_and_hw_paths_agree(renderer, stream, label):
    """S_ref and S_hw, for which there is no CPU oracle: the fused frame and the wavefront frames (unsorted,
    sorted, each in the static and in the adaptive order) are equal word for word, aux planes included (a NaN
    against a NaN).  The queues need not be the oracle's S_strict ones (printed, not asserted): a ray within a
    rounding error of a panel's edge or diagonal hits in one arithmetic and misses in another."""
    c = Q.case(label)
    Q.put(renderer, c.scene, c.params)
    want = Q.frames(c)["d"]
    for mode, f in (("S_ref", 0), ("S_hw", HW)):
        fused = Q.render(renderer, c.w, c.h, c.depth, f, stream)
        assert not np.any(fused["hits"] == Q.SENTINEL), f"{label} {mode}: the fused frame left hits unwritten"
        print(f"{label} {mode}: {int(np.sum((fused['hits'][:, :, 0] != Q.NOT_TRACED) != (want['hits'][:, :, 0] != Q.NOT_TRACED)))} "
              f"of {want['hits'][:, :, 0].size} rays are traced in one of {mode} and the oracle's S_strict alone")
        for name, extra in (("wavefront (static order)", WAVEFRONT | STATIC_ORDER), ("wavefront (adaptive order)", WAVEFRONT),
                            ("wavefront sorted (static order)", WAVEFRONT | WF_SORT | STATIC_ORDER),
                            ("wavefront sorted (adaptive order)", WAVEFRONT | WF_SORT)):
            Q.same_frame(Q.render(renderer, c.w, c.h, c.depth, f | extra, stream), fused, f"{label} {mode} {name} vs fused")


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("label", BAND_CASES)
def test_bands_equal_the_rows_of_the_whole_frame(renderer, stream, label, tiling):
    """A rank's bands of a tiling, rendered into the band's own tile grid: in S_strict the oracle's rows, in
    S_ref the rows of the whole fused frame; unsorted and sorted, aux planes included."""
    import rtamd
    c = Q.case(label)
    Q.put(renderer, c.scene, c.params)
    t = rtamd.rt_tiling(*tiling, 0)
    idx = Q.band_pixels(c.w, c.h, t)
    assert 0 < idx.size < c.w * c.h
    whole = {STRICT: Q.frames(c)["d"], 0: Q.render(renderer, c.w, c.h, c.depth, 0, stream)}
    for math, frame in whole.items():
        for extra in (WAVEFRONT, WAVEFRONT | WF_SORT, WAVEFRONT | WF_SORT):
            got = Q.render(renderer, c.w, c.h, c.depth, math | extra, stream, tiling=t)
            Q.same_frame(got, Q.rows_of(frame, idx), f"{label} rank {tiling[0]} of {tiling[1]}, band_rows {tiling[2]}, flags {math | extra}")


def _batch(renderer, stream, w, h, depth, flags, cams, stride):
    import torch
    with torch.cuda.stream(stream):
        out = torch.full((len(cams) * stride,), Q.SENTINEL, dtype=torch.int32, device="cuda")
    renderer.render_device_batch(w, h, depth, flags, cams, out.data_ptr(), stride, stream=stream.cuda_stream)
    stream.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    frames = [o[i * stride:i * stride + w * h] for i in range(len(cams))]
    gaps = [o[i * stride + w * h:(i + 1) * stride] for i in range(len(cams))]
    return frames, all(bool(np.all(g == Q.SENTINEL)) for g in gaps)


@pytest.mark.parametrize("depth", [3, 8])
@pytest.mark.parametrize("w,h,k", BATCHES)
def test_batch_frames_of_different_populations(renderer, stream, w, h, k, depth):
    """One launch, k frames, k different queues (empty, full, one ray, lane counts, ...): every frame equals
    its own single render, and in S_strict the oracle's packed pixels (a batch has no aux planes); sorted and
    not, contiguous and a stride apart (the gaps untouched)."""
    scene, cams, names = Q.batch_stage(w, h, k)
    want = Q.batch_frames(w, h, k, depth)
    Q.put(renderer, scene, cams[0])
    for flags in (STRICT | WAVEFRONT, STRICT | WAVEFRONT | WF_SORT, WAVEFRONT, WAVEFRONT | WF_SORT):
        singles = []
        for p in cams:
            renderer.set_params(p)
            singles.append(Q.render(renderer, w, h, depth, flags, stream, aux=False)["out"])
        for stride in (w * h, w * h + 37):
            got, gaps_ok = _batch(renderer, stream, w, h, depth, flags, cams, stride)
            assert gaps_ok, (w, h, k, depth, flags, stride)
            for i, name in enumerate(names):
                label = f"{w}x{h} K={k} depth {depth} flags {flags} stride {stride} frame {i} ({name})"
                assert not np.any(got[i] == Q.SENTINEL), label
                assert np.array_equal(got[i], singles[i]), f"{label}: {int(np.sum(got[i] != singles[i]))} pixels differ from the single render"
                if flags & STRICT:
                    assert np.array_equal(got[i], want[i]["out"]), f"{label}: {int(np.sum(got[i] != want[i]['out']))} pixels differ from the oracle"


@pytest.mark.parametrize("label", ["depth/thinning@super", "pop/super_ends@super"])
def test_tiled_over_three_contexts(renderer, stream, label):
    """rt_render_tiled over three contexts on device 0 at depth 8: each context renders its 8-row bands with
    its own queues.  In S_strict the frame is the oracle's, fused, wavefront and wavefront sorted, twice each;
    in S_ref, through the same three paths, it is the session renderer's whole fused frame.  The contexts' band buffers and the staging frame outlive a
    call, so a ray that never finishes would leave the pixel of the call before: before every frame the same
    call renders another view (the camera moved half a screen pitch to the right, where no panel stands),
    whose pixels are all different."""
    import rtamd
    c = Q.case(label)
    aside = Q.camera_params(c.params, c.w, c.h, dx=Q.PITCH / 2)
    hit = Q.oracle_frame(c, 8)["hits"][:, 0, 0] >= 0
    truth = {STRICT: (Q.render_oracle(c.scene, aside, c.w, c.h, 8)["out"], Q.oracle_frame(c, 8)["out"])}
    Q.put(renderer, c.scene, aside)
    blank_ref = Q.render(renderer, c.w, c.h, 8, STATIC_ORDER, stream, aux=False)["out"]
    renderer.set_params(c.params)
    truth[0] = (blank_ref, Q.render(renderer, c.w, c.h, 8, STATIC_ORDER, stream, aux=False)["out"])
    for blank, want in truth.values():
        assert np.all(blank[hit] != want[hit]) and hit.any()
    rs = [rtamd.Renderer(0) for _ in range(3)]
    try:
        Q.put(rs[0], c.scene, c.params)
        for r in rs[1:]:
            r.copy_scene_from(rs[0])
        for math, paths in ((STRICT, (0, WAVEFRONT, WAVEFRONT | WF_SORT)), (0, (0, WAVEFRONT, WAVEFRONT | WF_SORT))):
            blank, want = truth[math]
            for flags in paths:
                for again in range(2):
                    for params, frame, what in ((aside, blank, "the view aside"), (c.params, want, "the frame")):
                        rs[0].set_params(params)
                        got = np.full(c.w * c.h, Q.SENTINEL, np.uint32)
                        rtamd.render_tiled(rs, c.w, c.h, 8, math | flags, out=got)
                        assert np.array_equal(got, frame), \
                            f"{label} flags {math | flags} call {again}, {what}: {int(np.sum(got != frame))} pixels differ"
    finally:
        for r in rs:
            r.close()


@pytest.mark.parametrize("label", ["pop/full@super", "pop/chunk_checker@super"])
def test_fetch_counts_on_the_wavefront_path(renderer, label):
    """rt_fetch_counts at depth 3 on the wavefront path, sorted and not: the counting kernels run the same
    queues, and their inner-record fetches are the oracle's inner visits, their triangle-record fetches its
    triangle tests plus at most one per visited leaf (as test_render_gpu.py compares them)."""
    c = Q.case(label)
    Q.put(renderer, c.scene, c.params)
    st = Q.frames(c)["d"]["stats"]
    kinds = ("primary", "shadow", "secondary")
    inner, tris, leaves = (sum(st[k][what] for k in kinds) for what in ("inner", "tris", "leaf"))
    assert st["secondary"]["rays"] > 0
    for flags in (STRICT | WAVEFRONT, STRICT | WAVEFRONT | WF_SORT):
        fr = renderer.fetch_counts(c.w, c.h, 3, flags)
        assert renderer.last_deferred() == 0
        print(f"{label} flags {flags}: inner {fr['inner']} (oracle {inner}), tri {fr['tri']} (oracle {tris} + up to {leaves})")
        assert fr["inner"] == inner, (label, flags)
        assert tris <= fr["tri"] <= tris + leaves, (label, flags)
