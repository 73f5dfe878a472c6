"""The wavefront ray queues at their edges, on the CPU: every case of
tests/queue_edge_common.py reaches its edge by the oracle's own output -- how many rays each bounce traces,
which bounce-1 segments hold them, which sort buckets they fall into.  A case whose predicate fails is a
broken case, not a finding.  tests/test_queue_edges_gpu.py and tests/test_frame_scratch_gpu.py then hold
the kernels and the frame scratch to the oracle on the same cases.  Run with -s for the measured n_k."""
import numpy as np
import pytest

import queue_edge_common as Q


def test_the_case_list_is_the_static_one():
    assert Q.LABELS == Q.labels()
    assert sorted({c.cls for c in Q.cases()}) == sorted(Q.CLASSES)
    assert all(c.scene["indices"].size // 3 <= 2500 for c in Q.cases())


def test_the_geometries_are_the_edges_they_are_named_for():
    """Segments, chunks and super-chunks of each frame geometry, from the segment formula."""
    def shape(geo):
        n = Q.num_segments(*Q.GEOMETRIES[geo])
        return n, -(-n // Q.CHUNK_SEGS), -(-n // Q.SUPER_SEGS)
    assert shape("super") == (1088, 34, 2) and Q.tiles(*Q.G_SUPER) == (16, 17)
    assert shape("exact") == (1024, 32, 1)
    assert shape("ragged") == (1088, 34, 2) and Q.G_RAGGED[0] % 16 and Q.G_RAGGED[1] % 16
    assert shape("chunk") == (32, 1, 1)
    assert shape("chunk+") == (36, 2, 1)
    assert shape("small") == (24, 1, 1)
    assert shape("one") == (4, 1, 1)
    # the formula: every pixel of a frame has one segment, a segment at most 64 pixels, 8 x 8 of one tile
    for w, h in Q.GEOMETRIES.values():
        whole = Q.segment_counts(np.ones(w * h, bool), w, h)
        assert whole.sum() == w * h and whole.max() <= 64
        for seg in (0, len(whole) // 2, len(whole) - 1):
            x0, y0, x1, y1 = Q.segment_rect(seg, w, h)
            ys, xs = np.mgrid[y0:max(y1, y0), x0:max(x1, x0)]
            assert np.all(Q.segment_of(xs, ys, w) == seg) and xs.size == whole[seg]


@pytest.mark.parametrize("label", Q.LABELS)
def test_every_case_reaches_its_edge(label):
    """The case's predicate on the oracle's aux output holds, every primary ray passes the box test, no
    traversal overflows its stack, and the frame without shadow rays traces the same rays."""
    c = Q.case(label)
    f = Q.frames(c)
    n = Q.n_of(c)
    q = Q.queue1(c)
    print(f"{label}: n_k = {n}; {int(np.count_nonzero(q))} of {len(q)} bounce-1 segments hold rays, "
          f"{len(set(q.tolist()))} distinct counts; {c.scene['indices'].size // 3} triangles")
    assert n[0] == c.w * c.h, "a primary ray failed the box test"
    assert c.predicate(c), label
    assert f["d"]["stats"]["stack_overflow"] == 0 and f["ns"]["stats"]["stack_overflow"] == 0
    assert np.array_equal(f["d"]["hits"][:, :, 0], f["ns"]["hits"][:, :, 0])
    assert f["d"]["hits"].shape[1] == c.depth


def test_nan_keys_is_the_only_case_with_nan_directions():
    """Pitfall 1.  keys/nan_keys is keys/one_bucket's stage moved so that the front wall lies in z = 0: every
    triangle of it has a zero Cramer determinant, every bounce-1 ray a NaN direction, so all of them miss
    although the back wall stands behind the eye as it does in one_bucket, where all of them hit.  The
    oracle's colours stay NaN-free in every case (the BRDF's max(0, .) and the clamp swallow the NaN)."""
    nan, reg = Q.case("keys/nan_keys@super"), Q.case("keys/one_bucket@super")
    assert nan.back and reg.back and nan.scene["indices"].size == reg.scene["indices"].size
    assert Q.n_of(nan)[1:3] == [nan.w * nan.h, 0] and Q.n_of(reg)[1:3] == [reg.w * reg.h, reg.w * reg.h]
    front = np.flatnonzero(nan.scene["tri_to_material"] == 0)[:-2]   # the panels (the anchors come last)
    assert np.all(nan.scene["vertices"][np.repeat(3 * front, 3) + np.tile(np.arange(3), front.size), 2] == 0.0)
    for c in Q.cases():
        f = Q.frames(c)["d"]
        assert not np.isnan(f["rgb"]).any() and not np.isnan(f["t"]).any(), c.label


def test_key_axes_and_buckets():
    """The sort key's axis follows the caller's box (x, y, z, and y on a tie), and the restated keys of the
    bucket cases: one bucket, all 8 and all 16, and one ray past the last bucket."""
    assert [Q.thin_axis(Q.case(f"keys/{n}@super").params) for n in ("axis_x", "axis_y", "axis_z", "axis_tie")] == [0, 1, 2, 1]
    assert Q.thin_axis(Q.case("keys/one_bucket@super").params) == 2
    assert Q.thin_axis(Q.case("keys/all_buckets@super").params) == 0
    for scale in (4, 8):
        k, raw = Q.keys_of_queue1(Q.case("keys/all_buckets@super"), scale)
        print(f"all_buckets, scale {scale}: rays per bucket {np.bincount(k).tolist()}")
        assert np.bincount(k, minlength=2 * scale).min() > 0
        k, raw = Q.keys_of_queue1(Q.case("keys/key_clamp@exact"), scale)
        assert raw.max() == 2 * scale and int(np.sum(raw == 2 * scale)) == 1 and k.max() == 2 * scale - 1


@pytest.mark.parametrize("w,h,k", [Q.G_SMALL + (2,), Q.G_SMALL + (4,), Q.G_SMALL + (8,), (256, 48, 8)])
def test_a_batch_holds_different_populations(w, h, k):
    """The frames of one batch launch share the scene, the light and the box, differ in the camera alone,
    and their bounce-1 queues differ: empty, full, one ray, ...; 256 x 48 x 8 has 1536 segments."""
    scene, cams, names = Q.batch_stage(w, h, k)
    for p in cams[1:]:
        assert np.array_equal(p[16:32], cams[0][16:32]) and np.array_equal(p[0:8], cams[0][0:8])
        assert not np.array_equal(p[8:16], cams[0][8:16])
    n3 = [Q.n_traced(f) for f in Q.batch_frames(w, h, k, 3)]
    n8 = [Q.n_traced(f) for f in Q.batch_frames(w, h, k, 8)]
    print(f"{w}x{h} K={k}: " + ", ".join(f"{nm} {n}" for nm, n in zip(names, n8)))
    assert all(n[0] == w * h for n in n3)
    assert n3[0][1] == 0 and n3[1][1] == w * h
    assert len({f["hits"][:, 0, 0].tobytes() for f in Q.batch_frames(w, h, k, 3)}) == k
    if k == 8:
        assert [n[1] for n in n3][2] == 1 and [n[1] for n in n3][5] == 1
    assert any(n[7] > 0 for n in n8), "a queue alive at bounce 7"
    if (w, h, k) == (256, 48, 8):
        assert Q.num_segments(w, h, k) == 1536 > Q.SUPER_SEGS
