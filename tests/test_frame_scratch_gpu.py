"""The life cycle of the per-stream frame scratch (rt_render.hip: rt_ctx::FrameSlot, slot_for,
render_frames): what a frame inherits from the frames before it on its slot, more streams than slots, more
block grids than order tables, and the row groups of rt_render.  The frames are those of
tests/queue_edge_common.py, whose queues the caller chooses.

A context of its own, not the session's, so that its slots and tables are known: `ctx` is shared by the
tests that walk one context through a long life (each of them brings its own streams), `fresh_ctx` is new
for a test that speaks of a state before anything else has used the context.  The truth for
every S_strict frame is the oracle, aux planes included; for an S_ref frame it is the same frame from the
session's `renderer`: the fused kernel with RT_FLAG_STATIC_ORDER on a stream of its own.  Every output
buffer is filled with a sentinel before its frame.  The two limits are restated here; the tests use 20 of
each, so they stay valid if a limit shrinks."""
import numpy as np
import pytest

import queue_edge_common as Q

pytestmark = pytest.mark.gpu

NO_SHADOW, HW, WAVEFRONT, STATIC_ORDER, WF_SORT, STRICT = 1, 2, 8, 16, 32, 64
SORTED = WAVEFRONT | WF_SORT
MAX_SLOTS = 16    # rt_render.hip:1089  static constexpr int kMaxSlots = 16
MAX_ORDERS = 16   # rt_render.hip:1097  static constexpr size_t kMaxOrders = 16
MANY = 20


@pytest.fixture(scope="module")
def ctx():
    import rtamd
    r = rtamd.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def fresh_ctx():
    import rtamd
    r = rtamd.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def ref_stream():
    import torch
    return torch.cuda.Stream()


def _streams(n):
    import torch
    return [torch.cuda.Stream() for _ in range(n)]


def _closed(geo):
    w, h = Q.GEOMETRIES[geo]
    return Q.extra_case("closed", w, h, Q.pop_empty, depth=8, front="closed")


def _truth(renderer, ref_stream, c, depth, math):
    """The frame every path must give: the oracle's in S_strict; else the session renderer's fused (depth 0
    and 1: its only) kernel in the static order."""
    if math == STRICT:
        return Q.oracle_frame(c, depth)
    Q.put(renderer, c.scene, c.params)
    return Q.render(renderer, c.w, c.h, depth, math | STATIC_ORDER, ref_stream)


def _sequence():
    """(case, depth, path flags): each frame inherits counter sets laid out for another nchunk + nsuper, a
    d_seg and a d_perm full of another frame's entries, and queues full of another frame's rays."""
    case = Q.case
    return [(case("depth/closed@super"), 8, SORTED),                         # the largest queue at every bounce
            (case("pop/empty@super"), 8, SORTED),                   # then none, at the same geometry
            (case("pop/one_last@super"), 3, SORTED),
            (case("pop/full@small"), 2, WAVEFRONT),                 # smaller: 1 chunk, the sums move up
            (case("pop/empty@small"), 8, SORTED),                   # deeper than the frame before
            (_closed("exact"), 8, WAVEFRONT),                       # grows again: exactly one super-chunk
            (case("depth/dies_at_2@super"), 8, SORTED),
            (case("depth/thinning@super"), 0, 0),                   # a depth-0 frame
            (case("depth/thinning@super"), 3, 0),                   # a fused frame
            (case("depth/thinning@super"), 1, 0),                   # a depth-1 frame
            (case("depth/thinning@super"), 8, SORTED)]


@pytest.mark.parametrize("math", [STRICT, 0], ids=["strict", "ref"])
def test_stale_state_after_a_bigger_frame(ctx, renderer, ref_stream, math):
    """One stream, one slot: a frame after a larger, deeper, fuller one equals the truth in every word, no
    traversal restarts (rt_last_deferred stays 0) and none overflows (rt_overflow_count unchanged), as the
    oracle's stack_overflow says."""
    stream = _streams(1)[0]
    before = ctx.overflow_count()
    for i, (c, depth, flags) in enumerate(_sequence()):
        want = _truth(renderer, ref_stream, c, depth, math)
        Q.put(ctx, c.scene, c.params)
        got = Q.render(ctx, c.w, c.h, depth, math | flags, stream)
        Q.same_frame(got, want, f"frame {i}: {c.label} depth {depth} flags {math | flags}")
        assert ctx.last_deferred() == 0, (i, c.label)
        assert Q.oracle_frame(c, depth)["stats"]["stack_overflow"] == 0 and ctx.overflow_count() == before, (i, c.label)


def test_queries_and_batches_in_between(ctx, renderer, ref_stream):
    """The same kind of sequence with other work on the same stream between the frames: a ray query (checked
    against oracle.trace_rays), a wavefront batch of three frames (the oracle's pixels), and an update of the
    vertices to the same vertices, after which the frame is unchanged."""
    import rtamd
    import torch
    from oracle import oracle
    stream = _streams(1)[0]
    seq = [(Q.case("depth/thinning@super"), 8), (Q.case("pop/lane_counts@super"), 3), (Q.case("pop/full@small"), 3),
           (Q.case("pop/super_ends@super"), 3), (Q.case("pop/empty@super"), 3), (Q.case("pop/segment_checker@super"), 3)]
    bw, bh = Q.G_SMALL
    bscene, bcams, _ = Q.batch_stage(bw, bh, 3)
    for i, (c, depth) in enumerate(seq):
        want = Q.oracle_frame(c, depth)
        Q.put(ctx, c.scene, c.params)
        Q.same_frame(Q.render(ctx, c.w, c.h, depth, STRICT | SORTED, stream), want, f"frame {i}: {c.label}")
        if i % 3 == 0:     # a ray query: the frame's own primary rays, a count that is no multiple of 64
            n = min(c.w * c.h, 5003)
            o, d = Q.primary_rays(c.params, c.w, c.h)
            rays = rtamd.pack_rays(o[:n].astype(np.float32), d[:n].astype(np.float32))
            ids, t, _ = oracle.trace_rays(c.scene, rays)
            with torch.cuda.stream(stream):
                d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
                d_hits = torch.full((2 * n,), Q.SENTINEL, dtype=torch.int32, device="cuda")
            stream.synchronize()
            ctx.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), flags=STRICT, stream=stream.cuda_stream)
            stream.synchronize()
            got = d_hits.cpu().numpy()
            assert np.array_equal(got[0::2], ids), f"after frame {i}: query ids"
            assert np.array_equal(got[1::2].view(np.uint32), Q.bits(t)), f"after frame {i}: query t"
        elif i % 3 == 1:   # a batch of three frames of another scene and size
            Q.put(ctx, bscene, bcams[0])
            with torch.cuda.stream(stream):
                out = torch.full((3 * bw * bh,), Q.SENTINEL, dtype=torch.int32, device="cuda")
            ctx.render_device_batch(bw, bh, 3, STRICT | SORTED, bcams, out.data_ptr(), bw * bh, stream=stream.cuda_stream)
            stream.synchronize()
            got = out.cpu().numpy().view(np.uint32).reshape(3, bw * bh)
            for k, f in enumerate(Q.batch_frames(bw, bh, 3, 3)):
                assert np.array_equal(got[k], f["out"]), f"after frame {i}: batch frame {k}"
            Q.put(ctx, c.scene, c.params)
        else:              # the same vertices again: a refit that changes nothing
            ctx.update_vertices(c.scene["vertices"])
        Q.same_frame(Q.render(ctx, c.w, c.h, depth, STRICT | SORTED, stream), want, f"frame {i} again: {c.label}")
        assert ctx.last_deferred() == 0


# twenty frames of twenty sizes and populations from ONE uploaded scene: a screen per frame
_MANY_POPS = [Q.pop_full, Q.pop_lane_counts, Q.pop_one_last, Q.pop_empty, Q.pop_every_other_tile,
              Q.pop_segments(range(1, 1088, 2)), Q.pop_centre_quadrant, Q.pop_one_first, Q.pop_chunks(range(1, 34, 2)),
              Q.pop_chunks([0])]
_MANY_SIZES = [Q.G_SUPER, Q.G_SMALL, Q.G_RAGGED, Q.G_CHUNK, Q.G_EXACT, Q.G_CHUNK_PLUS, (100, 60)]
SHIFT = 3   # round 3: stream i renders screen i + SHIFT; no multiple of the 7 sizes' period, see the assertion
_MANY = {}


def _many():
    """(scene, [(params, w, h)] of MANY screens, their oracle frames at depth 3)."""
    if not _MANY:
        sizes = [_MANY_SIZES[i % len(_MANY_SIZES)] for i in range(MANY)]
        pops = [_MANY_POPS[i % len(_MANY_POPS)] for i in range(MANY)]
        scene, cams = Q.stage([p(w, h) for p, (w, h) in zip(pops, sizes)], [s[0] for s in sizes], [s[1] for s in sizes])
        views = [(p, w, h) for p, (w, h) in zip(cams, sizes)]
        _MANY["v"] = (scene, views, [Q.render_oracle(scene, p, w, h, 3) for p, w, h in views])
    return _MANY["v"]


def test_more_streams_than_slots(ctx):
    """MANY streams on a context of MAX_SLOTS slots, every stream a frame of its own population and size, all
    enqueued before any is read back: a round in order, a round in reverse (the recycled slot is not the one
    just used), a round in which every stream renders another screen, of another size and another tile grid
    than before (asserted), so that a slot its stream still owns is reused for another nchunk + nsuper while
    other streams' frames are in flight; then rt_last_deferred; then six streams with three tilings each (18
    slots from 6 streams).  Every frame equals the oracle."""
    import rtamd
    assert MANY > MAX_SLOTS
    scene, views, want = _many()
    assert len({(w, h) for _, w, h in views}) >= 6 and len({f["hits"][:, 0, 0].tobytes() for f in want}) >= 10
    Q.put(ctx, scene, views[0][0])
    streams = _streams(MANY)
    flags = STRICT | SORTED
    for i in range(MANY):   # round 3: no stream keeps its size or its tile grid
        (_, w0, h0), (_, w1, h1) = views[i], views[(i + SHIFT) % MANY]
        assert (w0, h0) != (w1, h1) and Q.tiles(w0, h0) != Q.tiles(w1, h1), (i, (w0, h0), (w1, h1))
    for rnd, order, shift in ((1, range(MANY), 0), (2, range(MANY - 1, -1, -1), 0), (3, range(MANY), SHIFT)):
        pend = []
        for i in order:
            j = (i + shift) % MANY
            p, w, h = views[j]
            ctx.set_params(p)
            pend.append((i, j, Q.enqueue(ctx, w, h, 3, flags, streams[i])))
        for i, j, pd in pend:
            Q.same_frame(pd.get(), want[j], f"round {rnd}: stream {i}, screen {j} ({views[j][1]}x{views[j][2]})")
    assert ctx.last_deferred() == 0
    tilings = [None, rtamd.rt_tiling(0, 2, 16, 0), rtamd.rt_tiling(1, 3, 8, 0)]
    for rnd in range(2):
        pend = []
        for i in range(6):
            for k in range(3):
                j = (3 * i + k + 5 * rnd) % MANY
                p, w, h = views[j]
                ctx.set_params(p)
                pend.append((i, j, tilings[k], Q.enqueue(ctx, w, h, 3, flags, streams[i], tiling=tilings[k])))
        for i, j, t, pd in pend:
            _, w, h = views[j]
            rows = want[j] if t is None else Q.rows_of(want[j], Q.band_pixels(w, h, t))
            Q.same_frame(pd.get(), rows, f"tilings round {rnd}: stream {i}, screen {j}, rank {t.rank if t else '-'}")
    assert ctx.last_deferred() == 0


def _grids():
    """MANY frame sizes of distinct (tiles_x, tiles_y), none a multiple of the tile."""
    sizes = [(16 * (i % 5 + 2) + 5, 16 * (i // 5 + 1) + 3) for i in range(MANY)]
    assert len({Q.tiles(w, h) for w, h in sizes}) == MANY
    return sizes


@pytest.mark.parametrize("in_flight", [False, True], ids=["alone", "frames_in_flight"])
def test_more_block_grids_than_tables(fresh_ctx, in_flight):
    """MANY distinct block grids on one stream, twice round, every fourth a K = 2 batch (a table of its own),
    in the static and in the adaptive order: the static order tables are dropped when the seventeenth arrives.
    Once alone; once with depth-8 frames in flight on three other streams while the new grids arrive.  Every
    frame, those in flight included, equals the oracle.  A new context each time: it starts with no table."""
    import torch
    ctx = fresh_ctx
    assert MANY > MAX_ORDERS
    c = Q.case("depth/thinning@super")
    Q.put(ctx, c.scene, c.params)
    main = _streams(1)[0]
    others = _streams(3) if in_flight else []
    big = Q.oracle_frame(c, 8)
    oracle_of = {}

    def truth(w, h, dx):
        if (w, h, dx) not in oracle_of:
            oracle_of[(w, h, dx)] = Q.render_oracle(c.scene, Q.camera_params(c.params, w, h, dx), w, h, 3)["out"]
        return oracle_of[(w, h, dx)]
    for rnd in range(2):
        for i, (w, h) in enumerate(_grids()):
            flags = STRICT | SORTED | (STATIC_ORDER if (i + rnd) % 2 else 0)
            pend = []
            for s in others:
                ctx.set_params(c.params)
                pend.append(Q.enqueue(ctx, c.w, c.h, 8, STRICT | SORTED, s, aux=False))
            label = f"round {rnd}, grid {i} ({w}x{h}), flags {flags}"
            if i % 4 == 3:
                cams = [Q.camera_params(c.params, w, h, dx) for dx in (0.0, 3.0)]
                with torch.cuda.stream(main):
                    out = torch.full((2 * w * h,), Q.SENTINEL, dtype=torch.int32, device="cuda")
                ctx.render_device_batch(w, h, 3, flags, cams, out.data_ptr(), w * h, stream=main.cuda_stream)
                main.synchronize()
                got = out.cpu().numpy().view(np.uint32).reshape(2, w * h)
                for k, dx in enumerate((0.0, 3.0)):
                    assert np.array_equal(got[k], truth(w, h, dx)), f"{label}: batch frame {k}"
            else:
                ctx.set_params(Q.camera_params(c.params, w, h))
                got = Q.render(ctx, w, h, 3, flags, main, aux=False)
                assert np.array_equal(got["out"], truth(w, h, 0.0)), f"{label}: {int(np.sum(got['out'] != truth(w, h, 0.0)))} pixels differ"
            for k, pd in enumerate(pend):
                Q.same_frame(pd.get(), big, f"{label}: the frame in flight on stream {k}")


def test_grouped_rt_render(fresh_ctx):
    """rt_render of a 512 x 528 frame (at least 512 x 512 pixels: four row groups on the context's group
    streams, each with its own slot) into pageable memory with aux planes, wavefront sorted at depth 3, before
    and after other streams have taken all the context's slots: the oracle's frame, and rt_last_deferred,
    which reads through the groups' slots, returns.  A new context: in the first round the four groups' slots
    are its first, in the second all sixteen have been taken by other streams in between."""
    ctx = fresh_ctx
    w, h = 512, 528
    c = Q.extra_case("lane_counts", w, h, Q.pop_lane_counts)
    want = Q.oracle_frame(c, 3)
    q = Q.segment_counts(want["hits"][:, 0, 0] >= 0, w, h)
    assert len(q) == 4224 and len(set(q.tolist())) >= 24 and w * h >= 512 * 512
    small = Q.case("pop/full@small")
    # rt_render's device frame and aux planes outlive a call: before every frame the same call renders
    # another view (the camera half a screen pitch to the right, no panel in sight), so that a ray that
    # never finishes leaves another frame's words behind, not this one's
    aside = Q.camera_params(c.params, w, h, dx=Q.PITCH / 2)
    blank = Q.render_oracle(c.scene, aside, w, h, 3)
    hit = want["hits"][:, 0, 0] >= 0
    assert np.all(blank["out"][hit] != want["out"][hit]) and np.all(blank["hits"][:, 0, 0] == -1)
    for rnd in range(2):
        Q.put(ctx, c.scene, c.params)
        for again in range(2):
            ctx.set_params(aside)
            Q.same_frame(ctx.render(w, h, depth=3, flags=STRICT | SORTED, aux=True), blank, f"the view aside, round {rnd}, call {again}")
            ctx.set_params(c.params)
            got = ctx.render(w, h, depth=3, flags=STRICT | SORTED, aux=True)
            Q.same_frame(got, want, f"grouped rt_render, round {rnd}, call {again}")
            assert ctx.last_deferred() == 0
        Q.put(ctx, small.scene, small.params)
        for i, s in enumerate(_streams(MAX_SLOTS)):   # every slot goes to another stream
            Q.same_frame(Q.render(ctx, small.w, small.h, 3, STRICT | SORTED, s), Q.oracle_frame(small, 3), f"round {rnd}: stream {i}")
        assert ctx.last_deferred() == 0
