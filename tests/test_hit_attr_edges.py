"""The yardstick of the attribute ray query at the edges of normal, ray and mesh space,
pinned on the CPU where tests/test_hit_attr.py had not pinned it: the inputs of
tests/hit_attr_edge_common.py, on which tests/test_hit_attr_edges_gpu.py compares the GPU's records
with tests/hit_attr_ref.c's.

 - The frame continued from the yardstick's records is the oracle's own frame on the thirteen
   quantisable normal-space inputs, NaN and zero shading normals included: that ties p and ns at the
   edges to the oracle, which test_shading_edges_gpu.py ties to the reference kernel.
 - Moller-Trumbore's t by the yardstick's lines is the traversal's in every bit on every input.
 - Each input reaches the edge it is made for (NaN and zero ns, on-edge barycentrics, normalize's
   branches, degenerate triangles never reported, enough hits), asserted from the oracle and the
   yardstick alone, with the counts printed.
 - u, v, p, ng and ndotd against float64 on every input: a gross-error check."""
import numpy as np
import pytest

import hit_attr_edge_common as X
import mesh_edge_common as M
import ray_edge_common as E
import shading_edge_common as S
from hit_attr_common import ID, T, TMAX_WORD, U, V, miss_words, ray_words, ref_next_rays, words

bits = X.bits


# ---- the lists and the rule ----

def test_the_lists_name_what_the_issue_names():
    assert X.NORMAL_LABELS == [l for l in S.LABELS if l.startswith("normals/")] + [l for l in S.LABELS if l.startswith("det/")]
    assert len(X.NORMAL_LABELS) == 14 and len(X.FRAME_LABELS) == 13 and len(E.CLASSES) == 14
    assert X.RAY_SCENES == ["cornell12", "rand2k", "rand2k_built", "hf40k", "single_tri_rootleaf"]
    assert set(X.SWEEP_CLASS) == set(X.RAY_SCENES) and set(X.SWEEP_CLASS.values()) <= set(E.CLASSES)
    assert set(X.NAN_MAKING) <= set(X.NORMAL_LABELS + X.MESH_LABELS)
    assert len(X.CASES) == len(set(X.CASES)) == 14 + 5 + 9


@pytest.mark.parametrize("case", X.CASES)
def test_sizes(case):
    """At most 2,048 rays or a 64 x 64 frame per input; at most 4,096 triangles per tree, but for the
    golden hf40k, which the issue names as it is."""
    inputs = X.inputs_of(case)
    assert len(inputs) == (15 if case in X.RAY_SCENES else 1)
    for inp in inputs:
        n = inp.rays.shape[0]
        assert n == 64 * 64 if inp.group == "normal" else n <= 2048, (inp.label, n)
        assert case == "hf40k" or inp.d["indices"].size // 3 <= 4096
        assert X.get(inp.label) is inp


def test_the_nan_rule():
    inp = X.get("normals/nan_component")
    want = inp.want()[0]
    nan = X.nan_words(want)
    assert nan.any() and X.assert_same_records_nan(want, want, "itself") == 0
    other = want.copy()
    other[nan] ^= np.uint32(0x80000001)                       # another payload and sign: still a NaN
    assert np.isnan(other[nan].view(np.float32)).all()
    assert X.assert_same_records_nan(other, want, "another NaN") == int(nan.sum())
    k, c = np.argwhere(nan)[0]
    for bad in (np.float32(0.0), np.float32(np.inf)):
        other = want.copy()
        other[k, c] = bits(bad)[0]
        with pytest.raises(AssertionError):
            X.assert_same_records_nan(other, want, "a number for a NaN")
    with pytest.raises(AssertionError):                       # a NaN where the yardstick has a number
        X.assert_same_records_nan(want, other, "a NaN for a number")
    hit = np.flatnonzero(want[:, ID].view(np.int32) >= 0)
    for col in (0, 1, 2, 6, 11, 15):                          # any other word: one bit is a difference
        clean = hit[~nan[hit].any(axis=1)][0]
        other = want.copy()
        other[clean, col] ^= np.uint32(1)
        with pytest.raises(AssertionError):
            X.assert_same_records_nan(other, want, f"word {col}")
    miss = np.flatnonzero(want[:, ID].view(np.int32) < 0)[0]
    other = want.copy()
    other[miss, 12] = bits(np.float32(np.nan))[0]
    with pytest.raises(AssertionError):
        X.assert_same_records_nan(other, want, "a NaN in a miss record")
    with pytest.raises(AssertionError):                       # a miss record of the yardstick is never excused
        X.assert_same_records_nan(want, other, "a miss record with a NaN as the yardstick")


# ---- the frame continued from the yardstick's records ----

@pytest.mark.parametrize("label", X.FRAME_LABELS)
def test_records_continue_the_oracles_frame(label):
    """Fed the bounce-0 ids and t of oracle.render(depth=2), the yardstick's records alone rebuild the
    frame's reflection and shadow rays: oracle.trace_rays returns the frame's bounce-1 ids, every bit of
    its bounce-1 t and its bounce-0 shadow ids.  Where ns is NaN the reflected ray is NaN, an invalid ray
    and a miss; the frame traced it and found nothing, (-1, 2^32), the same two words."""
    from oracle import oracle
    inp = X.get(label)
    ref = X.oracle_frame(label)
    ids0, t0 = ref["hits"][:, 0, 0].copy(), ref["t"][:, 0].copy()
    hit = ids0 >= 0
    traced = ids0 != -2
    qi, qt = inp.hits()
    assert np.array_equal(qi[traced], ids0[traced]) and np.array_equal(bits(qt[hit]), bits(t0[hit])), "the frame's rays are the query's"
    ids0[~hit] = -1
    from hit_attr_common import ref_hit_attr
    with np.errstate(all="ignore"):
        attrs = ref_hit_attr(inp.d, inp.rays, ids0, t0)
    assert np.array_equal(attrs[~hit], miss_words(inp.rays)[~hit])
    assert np.array_equal(attrs[hit], inp.want()[0][hit]), "the same records as on the query's ids and t"
    refl, shadow = ref_next_rays(inp.rays, attrs, inp.params[16:19])
    ids1, t1, _ = oracle.trace_rays(inp.d, refl)
    want1, want_t1 = ref["hits"][hit, 1, 0], ref["t"][hit, 1]
    assert int(hit.sum()) >= 2000 and not np.any(want1 == -2), "every pixel that hit traced its reflected ray"
    assert np.array_equal(ids1[hit], want1), f"{label}: {int((ids1[hit] != want1).sum())} bounce-1 ids differ"
    assert np.array_equal(bits(t1[hit]), bits(want_t1)), f"{label}: bounce-1 t differs"
    nan_ray = np.isnan(refl[:, 4:7]).any(axis=1) | np.isnan(refl[:, 0:3]).any(axis=1)
    assert np.all(ids1[nan_ray] == -1) and np.all(bits(t1[nan_ray]) == TMAX_WORD)
    sid, _, _ = oracle.trace_rays(inp.d, shadow, any_hit=True)
    assert np.array_equal(sid[hit], ref["hits"][hit, 0, 1]), f"{label}: shadow ids differ"
    h, n_nan, n_zero = X.ns_counts(attrs)
    print(f"{label}: {h} hits, {n_nan} NaN ns, {n_zero} zero ns, {int(nan_ray.sum())} NaN reflected rays, "
          f"{int((want1 >= 0).sum())} bounce-1 hits, {int((ref['hits'][hit, 0, 1] >= 0).sum())} shadowed")
    if label in X.NAN_MAKING and X.NAN_MAKING[label][0] == "nan":
        assert int(nan_ray.sum()) == n_nan >= 64, "a NaN ns makes a NaN reflected ray"
    else:
        assert not nan_ray.any()


# ---- every input: t, hits, NaN shares, float64 ----

@pytest.mark.parametrize("case", X.CASES)
def test_yardstick_on_every_input(case):
    for inp in X.inputs_of(case):
        for any_hit in (False, True):
            what = f"{inp.label} any={any_hit}"
            ids, t = inp.hits(any_hit)
            rec, t_mt = inp.want(any_hit)
            hit = ids >= 0
            n_hit = int(hit.sum())
            # ids, t, misses, and Moller-Trumbore's own t
            assert np.array_equal(rec[:, ID].view(np.int32), ids) and np.array_equal(rec[hit, T], bits(t[hit])), what
            assert np.array_equal(rec[~hit], miss_words(inp.rays)[~hit]), what + ": a miss is -1, the tmax word, 14 zero words"
            assert np.array_equal(bits(t_mt[hit]), bits(t[hit])), what + ": the recomputed t differs from the traversal's"
            assert not rec[:, 11].any() and not rec[:, 15].any()
            # enough hits
            if inp.label.endswith("/tmax"):
                unbarred = (inp.tstar_ids < 0) | (inp.turn >= 3)
                assert n_hit >= 0.1 * int(unbarred.sum()), what + ": the sweep's unbarred rays hit too rarely"
                assert not np.any(hit & ~unbarred), what + ": a ray barred by tmax hit"
            elif inp.label != "rand512*2^40":
                assert n_hit >= 0.1 * ids.size, what + f": only {n_hit} of {ids.size} rays hit"
            # NaN and zero ns
            _, n_nan, n_zero = X.ns_counts(rec)
            n_words = int(X.nan_words(rec).sum())
            print(f"{what}: {n_hit} of {ids.size} hit, ns NaN {n_nan}, ns zero {n_zero}, NaN words {n_words}")
            if inp.label in X.NAN_MAKING:
                kind, least = X.NAN_MAKING[inp.label]
                least = least * n_hit if isinstance(least, float) else least
                assert (n_nan if kind == "nan" else n_zero) >= least, what
                assert kind == "nan" or n_words == 0, what
            else:
                assert n_words == 0, what + ": a NaN word in an input that is not NaN-making"
            # float64
            e = X.float64_errors(inp.d, inp.rays, rec)
            print(f"   float64: {e}")
            assert e["bary"] <= 1e-5, what + ": u, v do not give the hit point"
            assert e["p"] <= 1e-5, what + ": p is not 0.001 short of the surface"
            assert e["ng"] <= 1e-4 and e["ndotd"] <= 1e-4, what + ": ng is not the winding's unit normal"
            assert e["unit"] <= 1e-6, what + ": ng is not a unit vector"
            u, v = rec[hit, U].view(np.float32), rec[hit, V].view(np.float32)
            assert np.all(u >= 0) and np.all(v >= 0) and np.all(u + v <= 1), what + ": an accepted hit passed ray_tri's tests"


# ---- per-input predicates ----

@pytest.mark.parametrize("scene", X.RAY_SCENES)
def test_snapped_rays_land_on_edges(scene):
    for any_hit in (False, True):
        n = X.on_edge(X.get(f"{scene}/snapped").want(any_hit)[0])
        print(f"{scene}/snapped any={any_hit}: {n} hits with u == 0, v == 0 or u + v == 1")
        assert n >= 3


def test_tmax_sweep_bars_what_it_must():
    """In a sweep input a ray with tmax <= t* misses with its own tmax word; above t* the hit comes back
    (one ulp above, by the reference's box test, not always: test_ray_query_edges_gpu.test_tmax_edges)."""
    for scene in X.RAY_SCENES:
        inp = X.get(f"{scene}/tmax")
        ids, t = inp.hits()
        would = inp.tstar_ids >= 0
        barred = would & (inp.turn <= 2)
        assert int(barred.sum()) >= 20 and np.all(ids[barred] == -1)
        assert np.array_equal(bits(t[barred]), bits(inp.rays["tmax"][barred]))
        at = would & (inp.turn == 2)
        assert np.array_equal(bits(inp.rays["tmax"][at]), bits(inp.tstar[at])), "tmax = t* itself"
        far = would & (inp.turn >= 4)
        assert np.array_equal(ids[far], inp.tstar_ids[far]) and np.array_equal(bits(t[far]), bits(inp.tstar[far]))
        up = would & (inp.turn == 3)
        assert float(np.mean(ids[up] == inp.tstar_ids[up])) >= 0.9
        assert np.isinf(inp.rays["tmax"][would & (inp.turn == 5)]).all()


def test_degenerate_triangles_are_never_reported():
    inp = X.get("degenerate")
    tri = np.asarray(inp.d["indices"]).reshape(-1, 3)
    flat = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    assert int(flat.sum()) >= 300 and int((~flat).sum()) >= 100
    for any_hit in (False, True):
        ids, _ = inp.hits(any_hit)
        assert not np.any(flat[ids[ids >= 0] // 3]), "a point or segment triangle was hit"


def test_signed_zero_meshes_hold_both_zeros():
    for name in ("signed_zeros_grid16", "signed_zeros_rand512"):
        v = X.get(name).d["vertices"][:, :3]
        zero = v == 0
        assert int(np.sum(zero & np.signbit(v))) >= 16 and int(np.sum(zero & ~np.signbit(v))) >= 16
        assert np.array_equal(v, M.mesh(name)[0][:, :3])


def test_tiny_tris_take_normalizes_branches():
    """From a float64 evaluation: l2 = |cross(e1, e2)|^2 = 2^-4e (1 + 2^-7)^2 is a normal float32 at
    e = 20, below FLT_MIN from e = 35 (normalize rescales by 2^86) -- where it has more bits than a
    subnormal of its size holds, so the rescale shows in ng -- and below the smallest subnormal, 0 in
    float32, at e = 50 and 62; after the rescale it is normal again.  1 / det, about 2^2e, is finite up
    to e = 63.  Each ray hits its own triangle at t = 2 with u, v = 1/4, 1/2 (or the reverse, by the
    winding), all to a rounding."""
    inp = X.get("tiny_tris")
    p0, p1, p2 = X.triangles64(inp.d, inp.own)
    g = np.cross(p1 - p0, p2 - p0)
    l2 = np.sum(g * g, axis=1)
    e = inp.exponents
    assert np.array_equal(l2, np.ldexp(X.TINY_SECOND_LEG ** 2, -4 * e)) and sorted(set(e)) == X.TINY_EXPONENTS
    at35 = float(l2[e == 35][0])
    assert at35 != float(np.float32(at35)), "l2 at e = 35 is exact as a subnormal: the rescale would not show"
    flt_min, least = np.ldexp(1.0, -126), np.ldexp(1.0, -149)
    assert np.all(l2[e == 20] >= flt_min) and np.all(l2[e >= 35] < flt_min)
    assert np.all(l2[e == 35] >= least) and np.all(l2[e >= 50] < least / 2) and np.all(l2[e >= 50].astype(np.float32) == 0)
    rescaled = l2 * np.ldexp(1.0, 172)
    assert np.all((rescaled[e >= 35] >= flt_min) & (rescaled[e >= 35] < np.ldexp(1.0, 128)))
    assert np.all(np.ldexp(1.0, 2 * e) < np.ldexp(1.0, 128)) and np.ldexp(1.0, 2 * 64) >= np.ldexp(1.0, 128)
    v = inp.d["vertices"][:, :3]
    assert np.all(v != 0), "a vertex lies in a coordinate plane"
    det = np.abs(np.einsum("ij,ij->i", p0, np.cross(p1, p2)))
    assert np.all(det >= flt_min), "the Cramer determinant is not a normal float32"
    for any_hit in (False, True):
        ids, t = inp.hits(any_hit)
        assert np.array_equal(ids, inp.own) and np.all(np.abs(t - 2.0) <= 1e-6)
        rec = inp.want(any_hit)[0]
        uv = np.sort(rec[:, [U, V]].view(np.float32), axis=1)
        assert np.all(np.abs(uv - np.array([0.25, 0.5], np.float32)) <= 1e-6)
        assert np.any(rec[:, U].view(np.float32) < 0.3) and np.any(rec[:, U].view(np.float32) > 0.4), "both windings"
        ng = rec[:, 8:11].view(np.float32)
        assert np.all(np.abs(np.abs(ng) - np.abs(ray_words(inp.rays)[:, 4:7])) <= 1e-6), "ng is the axis"
        assert np.all(np.abs(np.linalg.norm(ng.astype(np.float64), axis=1) - 1.0) <= 1e-6)
        nd = rec[:, 7].view(np.float32)
        assert np.all(np.abs(np.abs(nd) - 1) <= 1e-6) and np.any(nd < 0) and np.any(nd > 0), "front and back faces"
        ns = rec[:, 12:15].view(np.float32).astype(np.float64)
        assert np.all(np.abs(np.linalg.norm(ns, axis=1) - 1.0) <= 1e-6)
        # the corner normals differ by up to 0.3 a component, so a corner taken for another moves ns by a
        # tenth; the Cramer weights' own error here is some 1e-3 (p is 0.001 short of a plane 4 to 19 away,
        # and the weights are differences of products 2j + 1 times the leg): 5e-3 tells the two apart
        n = inp.d["normals"][:, :3].reshape(64, 3, 3).astype(np.float64)
        u, v = (rec[:, c].view(np.float32).astype(np.float64) for c in (U, V))
        mix = (1 - u - v)[:, None] * n[:, 0] + u[:, None] * n[:, 1] + v[:, None] * n[:, 2]
        mix /= np.linalg.norm(mix, axis=1)[:, None]
        assert np.abs(ns - mix).max() <= 5e-3, "ns is not the corner normals' interpolation"
        swapped = (1 - u - v)[:, None] * n[:, 0] + u[:, None] * n[:, 2] + v[:, None] * n[:, 1]
        swapped /= np.linalg.norm(swapped, axis=1)[:, None]
        assert np.abs(ns - swapped).max(axis=1).min() > 5e-3, "n1 and n2 can be told apart on every triangle"


def test_what_overflows_at_2_to_the_40():
    """Scaling a mesh and its rays' origins by 2^k is exact, so every hit is the unscaled one with t times
    2^k, until something overflows.  The first to do so is ray_tri's last line, dot(e2, qvec) with
    qvec = cross(tvec, e1): a product of three lengths, which grows as 2^3k, where every other line grows
    as 2^2k at most.  An infinite dot(e2, qvec) times det is an infinite t, and `t < tHit` rejects it.
    From a float64 evaluation on the oracle's unscaled hits: at 2^37 no product of that line reaches
    2^128 and every hit is kept; at 2^40 every kept hit stays below it, and all but a few of the lost
    hits have a product or the sum at or above it (the others sit within a rounding of it)."""
    base = X.get("rand512*2^20")
    ids0, t0 = base.hits()
    hit0 = ids0 >= 0
    top = np.ldexp(1.0, 128)
    for k in (37, 38, 40):
        inp = X.get(f"rand512*2^{k}")
        ids, t = inp.hits()
        r = ray_words(inp.rays).astype(np.float64)
        p0, p1, p2 = X.triangles64(inp.d, np.where(hit0, ids0, 0))
        qvec = np.cross(r[:, 0:3] - p0, p1 - p0)
        terms = (p2 - p0) * qvec
        reach = np.maximum(np.abs(terms).max(axis=1), np.abs(terms.sum(axis=1)))
        kept = hit0 & (ids == ids0)
        lost = hit0 & ~kept
        print(f"2^{k}: {int(hit0.sum())} unscaled hits, {int(kept.sum())} kept, {int(lost.sum())} lost, "
              f"{int(np.sum(lost & (reach >= top)))} of them with dot(e2, qvec) at or above 2^128; largest 2^{np.log2(reach[hit0].max()):.1f}")
        assert np.all(ids[~hit0] == -1) and np.all(ids[lost] == -1), "a lost hit is a miss, not another triangle"
        assert np.array_equal(bits(t[kept]), bits(np.ldexp(t0[kept], k - 20).astype(np.float32))), "a kept hit is the unscaled one"
        assert not np.any(kept & (reach >= top))
        if k == 37:
            assert not lost.any() and reach[hit0].max() < top
        if k == 40:
            assert int(kept.sum()) >= 4 and int(lost.sum()) >= 100
            assert int(np.sum(lost & (reach >= top))) >= 0.95 * int(lost.sum())
            assert np.all(reach[lost] >= top / 4)
