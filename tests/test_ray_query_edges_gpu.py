"""Ray queries at the edges of ray space and on the general kernel.  Every comparison
is exact: ids equal, t equal in bits, a miss's t the ray's tmax word; no tolerance anywhere.

The yardstick is oracle.trace_rays (oracle_trace_rays of oracle/rt_oracle.c, pinned on the CPU in
tests/test_ray_query.py); the rays are the classes of tests/ray_edge_common.py, whose properties are
asserted on the host there.

"Three code paths" of a flag word f: f on the normal context (the fast kernel, query_kernel<ANY, true>),
f | RT_FLAG_EXACT_DIV on it (the division form of the same loop), and f on a second context whose
upload ran under RTAMD_RECORD_LIMIT=64 (split records: query_kernel<ANY, false>, the general
traversal, which shares none of the fast loop; 64 bytes is below the smallest fixture's 128, and the
`general` fixture asserts after every upload that the records did split).  S_ref and S_hw have no CPU oracle: their bar is that
the three paths are equal, closest and any hit.  S_strict's bar is the same and equality with the
oracle, any-hit ids included.

The five gaps this module closes, and the test that closes each:
 1. query_kernel<ANY, false> was never launched: test_general_kernel (every scene on the split-records
    context, and an escape-leaf tree on both), test_the_smallest_scenes_split_too (that context really
    splits a scene of 128 bytes), test_bad_node_takes_the_general_kernel (an unclean scene
    on the normal context, rays that leave through the malformed node), test_general_kernel_group_edge
    (n = 65, guard records), test_general_kernel_deep_stacks (the full stack's overflow, per-ray tmax
    as the start value).
 2. The yardstick could not express most rays: test_tmax_edges (tmax at, one ulp around and far from
    t*, closest and any hit with the any-hit id compared) and every other test here through
    oracle.trace_rays.
 3. The ray side of the quotient's domain: test_edge_classes on near_axis and origin_domain, with the
    host assertion that whole groups lie inside and outside the domain of the arithmetic under test.
 4. Zero and near-zero direction components, rays in box and wall planes and through shared vertices,
    normalize's rescaling branches: test_edge_classes on axis1, axis2, snapped, scaled.
 5. The octant loops and their ballots over exec: test_octant_groups (whole sign-coherent groups, a
    tail, and lanes that sit out or break the coherence), test_neighbour_independence."""
import ctypes as C
import os

import numpy as np
import pytest

import rtamd
import ray_edge_common as E
from ray_query_common import TMAX_DEFAULT, TMIN
from refit_common import scene_image

pytestmark = pytest.mark.gpu

STRICT, HW, EXACT_DIV = rtamd.RT_FLAG_STRICT_MATH, rtamd.RT_FLAG_HW_MATH, rtamd.RT_FLAG_EXACT_DIV
ARITHMETICS = {"ref": 0, "strict": STRICT, "hw": HW}
QUERY_SCENES = ["cornell12", "rand2k", "rand4k_sbvh", "rand3k_bigleaf", "single_tri_rootleaf", "rand2k_built"]
MESH_KEYS = ("vertices", "indices", "normals", "normals_indices", "materials", "tri_to_material")
HDR_FAST_DIV, HDR_CLEAN = 12, 13   # ImageHeader::fast_div and ::clean, in words
GUARD = 0x5A5A5A5A
MAX_LAUNCH = 2048


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


RECORD_LIMIT = 64   # bytes; the smallest scene's records (single_tri_rootleaf: one inner record, one triangle) are 128


def records_bytes(r):
    """Bytes of the context's inner + triangle records, from its scene image's header (n_wnodes4 and
    n_tris4, two 64-bit counts of 16-byte units at words 2..5): what the upload compares with the limit."""
    hdr = scene_image(r)[:6]
    return 16 * (int(hdr[2]) + (int(hdr[3]) << 32) + int(hdr[4]) + (int(hdr[5]) << 32))


@pytest.fixture(scope="module")
def general(renderer):
    """A second context whose uploads take the general traversal (split records), whatever the scene's
    size.  Every upload is checked to have split: the records reach the limit, and a clean scene's
    context refuses rt_fetch_counts, whose counting kernels are fast-path only (an unclean scene is
    refused for that already; its queries run the general kernel on any context)."""
    r = rtamd.Renderer(0)

    def upload(d):
        old = os.environ.get("RTAMD_RECORD_LIMIT")
        os.environ["RTAMD_RECORD_LIMIT"] = str(RECORD_LIMIT)
        try:
            r.upload(rtamd.Scene.from_arrays(d))
        finally:
            if old is None:
                del os.environ["RTAMD_RECORD_LIMIT"]
            else:
                os.environ["RTAMD_RECORD_LIMIT"] = old
        assert records_bytes(r) >= RECORD_LIMIT, "the records are below the limit: this upload did not split"
        with pytest.raises(rtamd.RtError):
            r.fetch_counts(8, 8, 1, 0)
        return r
    yield upload
    r.close()


def test_the_scene_list_is_the_query_tests():
    from test_ray_query_gpu import SCENES
    assert QUERY_SCENES == SCENES


@pytest.mark.parametrize("name", ["cornell12", "single_tri_rootleaf"])
def test_the_smallest_scenes_split_too(renderer, general, name):
    """cornell12's records are 720 bytes and single_tri_rootleaf's 128: the normal context holds them
    unsplit and counts a frame's fetches; the second context, brought to the same scene, refuses to (the
    fixture asserts it on every upload), so the refusal is the split's and its queries run
    query_kernel<ANY, false>."""
    d = put_scene(renderer, name)
    assert scene_image(renderer)[HDR_CLEAN] == 1 and RECORD_LIMIT <= records_bytes(renderer) < 1024
    renderer.set_params(d["params"])
    assert renderer.fetch_counts(8, 8, 1, 0)["wave_instructions"] > 0
    g = general(d)
    assert records_bytes(g) == records_bytes(renderer)


def put_scene(r, name):
    """The named scene in the renderer: an upload, or for rand2k_built build_scene on the GPU (the
    oracle then runs on the host twin's arrays, which the split-records context uploads)."""
    d = E.edge_scene(name)
    if name == "rand2k_built":
        r.build_scene({k: d[k] for k in MESH_KEYS}, max_leaf=2, keys="extent")
    else:
        r.upload(rtamd.Scene.from_arrays(d))
    return d


def trace(r, rays, flags, any_hit=False, n=None):
    """rt_trace_rays of packed rays (at most MAX_LAUNCH per launch): (ids, t)."""
    n = rays.shape[0] if n is None else n
    hits = np.zeros(n, rtamd.HIT_DTYPE)
    for s in range(0, n, MAX_LAUNCH):
        m = min(MAX_LAUNCH, n - s)
        part = np.ascontiguousarray(rays[s:s + m])
        out = np.zeros(m, rtamd.HIT_DTYPE)
        rc = rtamd.lib().rt_trace_rays(r._h, part.ctypes.data_as(C.c_void_p), m,
                                       flags | (rtamd.RT_FLAG_ANY_HIT if any_hit else 0), out.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc
        hits[s:s + m] = out
    return hits["id"].copy(), hits["t"].copy()


def same(got, want, label):
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, f"{label}: {bad.size} ids differ, first {bad[:5]}: {got[0][bad[:5]]} vs {want[0][bad[:5]]}"
    bad = np.flatnonzero(bits(got[1]) != bits(want[1]))
    assert bad.size == 0, f"{label}: {bad.size} t differ, first {bad[:5]}: {got[1][bad[:5]]} vs {want[1][bad[:5]]}"


def check_paths(paths, d, rays, label, arithmetics=ARITHMETICS):
    """The bars of the module's docstring for one ray buffer.  `paths`: (label, renderer, extra flags)
    triples.  Returns the S_strict closest hits."""
    from oracle import oracle
    strict = None
    for mode, f in arithmetics.items():
        for any_hit in (False, True):
            got = [(pl, trace(r, rays, f | extra, any_hit)) for pl, r, extra in paths]
            what = f"{label} {mode} {'any' if any_hit else 'closest'}"
            for pl, g in got[1:]:
                same(g, got[0][1], f"{what}: {pl} vs {got[0][0]}")
            ids, t = got[0][1]
            miss = ids < 0
            assert np.all(ids[miss] == -1) and np.array_equal(bits(t[miss]), bits(rays["tmax"][miss])), \
                f"{what}: a miss is -1 and the tmax word"
            if mode == "strict":
                oi, ot, _ = oracle.trace_rays(d, rays, any_hit=any_hit)
                same(got[0][1], (oi, ot), f"{what}: {got[0][0]} vs the oracle")
                if not any_hit:
                    strict = (oi, ot)
    return strict


def three_paths(renderer, g):
    return [("fast", renderer, 0), ("EXACT_DIV", renderer, EXACT_DIV), ("general", g, 0)]


def uniform_tmax(ids, t, seed):
    """Per ray, uniform in (0.001, 2 t*) -- in (0.001, 200) where the ray misses."""
    rng = np.random.default_rng(seed)
    top = np.where(ids >= 0, 2.0 * t.astype(np.float64), 200.0)
    tm = (0.001 + rng.uniform(0.0, 1.0, ids.size) * (top - 0.001)).astype(np.float32)
    return np.maximum(tm, np.nextafter(TMIN, np.float32(1)))


def incoherent(name, n=MAX_LAUNCH):
    o, dirs, tm = E.ray_class(name, "incoherent")
    return o[:n], dirs[:n], tm[:n]


# ---- gap 1: the general kernel ----

@pytest.mark.parametrize("name", QUERY_SCENES + ["bigleaf"])
def test_general_kernel(renderer, general, name):
    """Incoherent rays, default tmax and per-ray tmax uniform in (0.001, 2 t*), on the normal and on the
    split-records context, whose queries run query_kernel<ANY, false>: pointer loads, the ray's own tmax
    as the start value, any hit.  bigleaf holds escape leaves of 40 and 35 triangles and an empty leaf."""
    d = put_scene(renderer, name)
    g = general(d)
    o, dirs, tm = incoherent(name)
    rays = rtamd.pack_rays(o, dirs, tm)
    ids, t = check_paths(three_paths(renderer, g), d, rays, name)
    assert np.any(ids >= 0) and np.any(ids < 0)
    tm = uniform_tmax(ids, t, 21)
    cut = check_paths(three_paths(renderer, g), d, rtamd.pack_rays(o, dirs, tm), name + " per-ray tmax")
    assert np.any((ids >= 0) & (cut[0] < 0)) and np.any(cut[0] >= 0), "tmax should fall on both sides of t*"


def test_bad_node_takes_the_general_kernel(renderer, general):
    """bad_node is not clean (the scene image's header says so), so the NORMAL context runs the general
    kernel too; half the rays are aimed into the malformed node's box, and the oracle counts at least 10
    traversals that leave through it: misses with the tmax word."""
    d = put_scene(renderer, "bad_node")
    assert scene_image(renderer)[HDR_CLEAN] == 0
    g = general(d)
    o, dirs, tm = E.ray_class("bad_node", "malformed")
    for any_hit in (False, True):
        assert E.oracle_hits("bad_node", "malformed", any_hit)[2]["error_miss"] >= 10
    ids, t = check_paths(three_paths(renderer, g), d, rtamd.pack_rays(o, dirs, tm), "bad_node")
    assert int((ids >= 0).sum()) > 100
    check_paths(three_paths(renderer, g), d, rtamd.pack_rays(o, dirs, uniform_tmax(ids, t, 22)), "bad_node per-ray tmax")
    put_scene(renderer, "cornell12")
    assert scene_image(renderer)[HDR_CLEAN] == 1


@pytest.mark.parametrize("name", ["cornell12", "bad_node"])
def test_general_kernel_group_edge(renderer, general, name):
    """n = 65 through the device form with guard records after hits[n]: the general kernel's own stores
    in all three arithmetics (cornell12 on the split-records context, whose fixture asserts the split;
    bad_node, unclean, on the normal one)."""
    import torch
    d = E.edge_scene(name)
    if name == "bad_node":
        put_scene(renderer, name)
        r = renderer
    else:
        r = general(d)
    n = 65
    o, dirs, tm = incoherent(name, n + 3)
    rays = rtamd.pack_rays(o, dirs, tm)                       # more rays in memory than asked for
    from oracle import oracle
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    for any_hit in (False, True):
        oi, ot, _ = oracle.trace_rays(d, rays[:n], any_hit=any_hit)
        d_hits = torch.full((2 * (n + 4),), GUARD, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for mode, f in ARITHMETICS.items():   # each arithmetic has its own instantiation of the kernel
            d_hits.fill_(GUARD)
            torch.cuda.synchronize()
            r.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), any_hit=any_hit, flags=f)
            torch.cuda.synchronize()
            got = d_hits.cpu().numpy().view(np.uint32)
            assert np.all(got[2 * n:] == GUARD), f"{mode}: the kernel wrote past hits[n]"
            gi, gt = got[0:2 * n:2].view(np.int32), got[1:2 * n:2]
            miss = gi < 0
            assert np.all(gi[miss] == -1) and np.array_equal(gt[miss], bits(rays["tmax"][:n][miss])), mode
            assert np.all((gi[~miss] % 3 == 0) & (gi[~miss] < d["indices"].size)), mode
            if mode == "strict":
                assert np.array_equal(gi, oi) and np.array_equal(gt, bits(ot))
            else:
                assert np.array_equal(gi, trace(r, rays[:n], f, any_hit)[0]), f"{mode}: device form vs host form"


def test_general_kernel_deep_stacks(renderer, general):
    """overflow_comb and the same comb cut to 40 levels on the split-records context: no LDS stack and
    no restart, the general traversal's 65 entries from the start.  ids and t are the oracle's, the
    overflow count grows by the oracle's, tmax = t* misses there and on the normal context (where these
    rays restart: the restart value), and with tmax = 2 t* the three paths agree in every arithmetic."""
    from oracle import oracle
    for name in ("overflow_comb", "deep_comb40"):
        d = put_scene(renderer, name)
        g = general(d)
        o, dirs, tm = incoherent(name)
        rays = rtamd.pack_rays(o, dirs, tm)
        oi, ot, stats = oracle.trace_rays(d, rays)
        assert (stats["stack_overflow"] > 0) == (name == "overflow_comb")
        assert name == "overflow_comb" or int((oi >= 0).sum()) > 100
        before = g.overflow_count()
        same(trace(g, rays, STRICT), (oi, ot), name)
        assert g.overflow_count() - before == stats["stack_overflow"]
        assert g.last_deferred() == 0, "the general kernel has nothing to restart"
        tstar = np.where(oi >= 0, ot, TMAX_DEFAULT).astype(np.float32)
        for any_hit in (False, True):
            for which, r in (("general", g), ("restarted", renderer)):
                gi, gt = trace(r, rtamd.pack_rays(o, dirs, tstar), STRICT, any_hit)
                assert np.all(gi == -1) and np.array_equal(bits(gt), bits(tstar)), f"{name} {which}: tmax = t* must miss"
            assert renderer.last_deferred() > 0, "on the normal context these rays restart"
        two = np.where(oi >= 0, np.float32(2) * ot, TMAX_DEFAULT).astype(np.float32)
        check_paths(three_paths(renderer, g), d, rtamd.pack_rays(o, dirs, two), f"{name} tmax = 2 t*")


# ---- gap 2: arbitrary tmax and exact any hit, fast path ----

@pytest.mark.parametrize("name", QUERY_SCENES)
def test_tmax_edges(renderer, name):
    """tmax = 0.5 t*, nextafter(t*, 0), t*, nextafter(t*, inf), 2 t*, +inf by turns, and uniform in
    (0.001, 2 t*): S_strict equals the oracle, closest and any hit, ids included.  The strict `<` at one
    ulp: nextafter(t*, inf) returns the oracle's hit for that tmax, t* misses."""
    from oracle import oracle
    d = put_scene(renderer, name)
    o, dirs, tm = incoherent(name)
    ids, t, _ = oracle.trace_rays(d, rtamd.pack_rays(o, dirs, tm))
    turn = np.arange(ids.size) % 6
    inf = np.float32(np.inf)
    choices = np.stack([(np.float32(0.5) * t).astype(np.float32), np.nextafter(t, np.float32(0)), t, np.nextafter(t, inf),
                        (np.float32(2) * t).astype(np.float32), np.full(t.size, inf, np.float32)])
    by_turns = np.where(ids >= 0, choices[turn, np.arange(ids.size)], TMAX_DEFAULT).astype(np.float32)
    for label, tmv in (("by turns", by_turns), ("uniform", uniform_tmax(ids, t, 23))):
        rays = rtamd.pack_rays(o, dirs, tmv)
        for any_hit in (False, True):
            oi, ot, _ = oracle.trace_rays(d, rays, any_hit=any_hit)
            got = trace(renderer, rays, STRICT, any_hit)
            same(got, (oi, ot), f"{name} tmax {label} any={any_hit}")
            same(trace(renderer, rays, STRICT | EXACT_DIV, any_hit), (oi, ot), f"{name} tmax {label} any={any_hit} EXACT_DIV")
            if label == "by turns":
                hit = ids >= 0
                up, at = hit & (turn == 3), hit & (turn == 2)
                assert int(up.sum()) > 100 and int(at.sum()) > 100
                assert np.all(got[0][at] == -1) and np.array_equal(bits(got[1][at]), bits(t[at])), "tmax = t* must miss"
                assert np.all(got[0][hit & (turn < 2)] == -1), "tmax below t* must miss"
                # One ulp above t* the hit comes back -- or, by the reference's own box test, a miss: a leaf
                # box's near distance is a rounded quotient and can exceed t* by an ulp where the box is as
                # flat as its triangle (18 of cornell12's 1,871 wall hits, none elsewhere, by the oracle).
                # `same` above has compared every one of them; these are conditions on the oracle's answer.
                back = oi[up] == ids[up]
                assert np.all(oi[up][~back] == -1) and float(back.mean()) >= 0.9, "one ulp above t* the hit comes back"
                assert any_hit or np.array_equal(bits(ot[up][back]), bits(t[up][back]))


# ---- gaps 3 and 4: the edge classes ----

EDGE_CASES = ["axis1", "axis2", "snapped", "near_axis", "origin_domain", "scaled", "octants"]


@pytest.mark.parametrize("cls", EDGE_CASES)
@pytest.mark.parametrize("name", E.EDGE_SCENES)
def test_edge_classes(renderer, general, name, cls):
    """Each class of tests/ray_edge_common.py through the three code paths, the three arithmetics, closest
    and any hit.  For near_axis and origin_domain, whose rays come in runs of 64 = the kernel's groups:
    by the rule of DESIGN.md 7.2 restated in ray_edge_common.axis_ok, some groups lie wholly inside the
    quotient's domain of the arithmetic (the fast quotient runs) and some hold rays outside it (their
    wave takes the division form)."""
    d = put_scene(renderer, name)
    g = general(d)
    assert scene_image(renderer)[HDR_FAST_DIV] == 1, "the scene itself must allow the fast quotient"
    for c in ([f"octant{k}" for k in range(8)] if cls == "octants" else [cls]):
        o, dirs, tm = E.ray_class(name, c)
        if c in ("near_axis", "origin_domain"):
            for mode in ARITHMETICS:
                ok = E.in_domain(o, dirs, mode).reshape(-1, 64)
                assert np.any(np.all(ok, axis=1)) and np.any(~np.any(ok, axis=1)), (c, mode)
        ids, _ = check_paths(three_paths(renderer, g), d, rtamd.pack_rays(o, dirs, tm), f"{name} {c}")
        assert np.any(ids >= 0)


# ---- gap 5: octant groups and the ballots ----

def _replacements(name, k):
    """Rays to put into a sign-coherent group of octant k: three invalid ones (which sit the traversal
    out), an axis1 ray, an origin_domain ray outside the domain, and a ray of octant k ^ 7."""
    base = rtamd.pack_rays(*E.ray_class(name, f"octant{k}"))[:1]
    reps = {}
    r = base.copy(); r["o"][0, 1] = np.nan; reps["nan origin"] = r
    r = base.copy(); r["d"][0] = 0.0; reps["zero direction"] = r
    r = base.copy(); r["tmax"][0] = 0.0; reps["zero tmax"] = r
    reps["axis1"] = rtamd.pack_rays(*E.ray_class(name, "axis1"))[5:6]
    o, dirs, tm = E.ray_class(name, "origin_domain")
    j = 64 * E.ORIGIN_VALUES.index(E.p2(-67)) + 7
    assert not E.in_domain(o[j:j + 1], dirs[j:j + 1], "ref")[0]
    reps["outside the domain"] = rtamd.pack_rays(o[j:j + 1], dirs[j:j + 1], tm[j:j + 1])
    reps["opposite octant"] = rtamd.pack_rays(*E.ray_class(name, f"octant{k ^ 7}"))[3:4]
    return reps


@pytest.mark.parametrize("k", range(8))
def test_octant_groups(renderer, k):
    """Whole sign-coherent 64-ray groups of octant k on rand2k; the same buffer with n cut to 64 m - 17
    (lanes past n sit out of the ballots); and with lane 0, 31 or 63 of every group replaced by a ray
    that sits out (invalid) or that must move the wave off the octant loop (a zero component, outside
    the domain, the opposite octant).  Every untouched ray's hit is unchanged bit for bit and every
    replaced ray's hit is what it gets traced alone (n = 1).  S_ref is the arithmetic with the octant
    loops.  A query has no counting instantiation, so which loop ran cannot be observed: by
    traverse_fast's rule a whole valid sign-uniform in-domain group on a fast_div scene (the header word
    is asserted to be 1) takes the octant copy, and such groups are what the first launch holds."""
    name = "rand2k"
    d = put_scene(renderer, name)
    assert scene_image(renderer)[HDR_FAST_DIV] == 1
    rays = rtamd.pack_rays(*E.ray_class(name, f"octant{k}"))
    n = rays.shape[0]
    reps = _replacements(name, k)
    paths = [("fast", renderer, 0), ("EXACT_DIV", renderer, EXACT_DIV)]
    check_paths(paths, d, rays, f"octant {k}")
    for mode, f in ARITHMETICS.items():
        for any_hit in (False, True):
            whole = trace(renderer, rays, f, any_hit)
            # the tail: lanes past n sit out
            cut = n - 17
            hits = np.full(2 * (n + 1), GUARD, np.uint32)
            rc = rtamd.lib().rt_trace_rays(renderer._h, rays.ctypes.data_as(C.c_void_p), cut,
                                           f | (rtamd.RT_FLAG_ANY_HIT if any_hit else 0), hits.ctypes.data_as(C.c_void_p))
            assert rc == 0 and np.all(hits[2 * cut:] == GUARD)
            assert np.array_equal(hits[0:2 * cut:2].view(np.int32), whole[0][:cut])
            assert np.array_equal(hits[1:2 * cut:2], bits(whole[1][:cut]))
            for label, rep in reps.items():
                alone = trace(renderer, rep, f, any_hit)
                for lane in (0, 31, 63):
                    mixed = rays.copy()
                    at = np.arange(lane, n, 64)
                    mixed[at] = rep[0]
                    got = trace(renderer, mixed, f, any_hit)
                    keep = np.setdiff1d(np.arange(n), at)
                    what = f"octant {k} {mode} any={any_hit} {label} at lane {lane}"
                    same((got[0][keep], got[1][keep]), (whole[0][keep], whole[1][keep]), what + ": the neighbours")
                    assert np.all(got[0][at] == alone[0][0]) and np.all(bits(got[1][at]) == bits(alone[1])[0]), what


# ---- gap 5 (and 3): neighbour independence ----

@pytest.mark.parametrize("name", E.EDGE_SCENES)
def test_neighbour_independence(renderer, name):
    """All classes and the incoherent rays in one buffer, traced in that order and under a seeded
    permutation (launches of 2,048 rays each, so the permutation also changes which rays share a
    launch): after un-permuting the results are equal bit for bit, in all three arithmetics, closest and
    any.  A lane's fallback moves its wave to another loop but changes no lane's result."""
    d = put_scene(renderer, name)
    rays = np.concatenate([rtamd.pack_rays(*E.ray_class(name, c)) for c in E.CLASSES + ["incoherent"]])
    perm = np.random.default_rng(31).permutation(rays.shape[0])
    shuffled = np.ascontiguousarray(rays[perm])
    from oracle import oracle
    for mode, f in ARITHMETICS.items():
        for any_hit in (False, True):
            a = trace(renderer, rays, f, any_hit)
            b = trace(renderer, shuffled, f, any_hit)
            back = (np.empty_like(b[0]), np.empty_like(b[1]))
            back[0][perm], back[1][perm] = b[0], b[1]
            same(back, a, f"{name} {mode} any={any_hit}: permuted vs in order")
            if mode == "strict":
                oi, ot, _ = oracle.trace_rays(d, rays, any_hit=any_hit)
                same(a, (oi, ot), f"{name} any={any_hit}: vs the oracle")
