"""Ray queries, the part that needs no GPU: the two records' sizes, the exported
symbols, the refusals made before any GPU work, and the self-checks of the yardsticks the GPU
tests are measured with (tests/ray_query_common.py)."""
import ctypes as C

import numpy as np
import pytest

import rtamd
from ray_query_common import (TMAX_DEFAULT, brute_force_closest, incoherent_rays, oracle_closest, quantised_frame,
                              scene_arrays)

RT_ERR_INVALID_ARG = -1


def test_record_sizes_and_constants():
    assert C.sizeof(rtamd.rt_ray) == 32 and C.sizeof(rtamd.rt_hit) == 8
    assert rtamd.RAY_DTYPE.itemsize == 32 and rtamd.HIT_DTYPE.itemsize == 8
    assert [rtamd.RAY_DTYPE.fields[k][1] for k in ("o", "tmax", "d", "reserved")] == [0, 12, 16, 28]
    assert [getattr(rtamd.rt_ray, k).offset for k in ("ox", "tmax", "dx", "reserved")] == [0, 12, 16, 28]
    assert rtamd.rt_hit.id.offset == 0 and rtamd.rt_hit.t.offset == 4
    assert rtamd.RT_FLAG_ANY_HIT == 128
    assert np.float32(rtamd.RT_RAY_TMAX_DEFAULT) == TMAX_DEFAULT == np.float32(np.uint32(0xFFFFFFFF))


def test_symbols_exported():
    L = rtamd.lib()
    for name in ("rt_trace_rays", "rt_trace_rays_device", "rt_last_query_timing"):
        assert name in rtamd.ABI_SYMBOLS
        assert hasattr(L, name), name
    assert L.rt_abi_version() == 3


def test_refusals_without_a_context():
    L = rtamd.lib()
    rays = np.zeros(4, rtamd.RAY_DTYPE)
    hits = np.zeros(4, rtamd.HIT_DTYPE)
    pr, ph = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    assert L.rt_trace_rays(None, pr, 4, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays(None, pr, 0, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_device(None, pr, 4, 0, ph, None) == RT_ERR_INVALID_ARG
    ms = C.c_float()
    assert L.rt_last_query_timing(None, C.byref(ms)) == RT_ERR_INVALID_ARG
    assert not np.any(hits.view(np.uint32)), "a refused call wrote hits"


def test_pack_rays_keeps_the_tmax_bits():
    o = np.arange(9, dtype=np.float32).reshape(3, 3)
    d = -o
    nan = np.array([0x7FC12345, 0xFFA00001, 0x7F800000], np.uint32).view(np.float32)
    r = rtamd.pack_rays(o, d, nan)
    assert np.array_equal(r["tmax"].view(np.uint32), nan.view(np.uint32))
    assert np.array_equal(r["o"], o) and np.array_equal(r["d"], d) and not np.any(r["reserved"])
    assert np.all(rtamd.pack_rays(o, d)["tmax"] == TMAX_DEFAULT)
    assert np.all(rtamd.pack_rays(o, d, 2.5)["tmax"] == np.float32(2.5))
    with pytest.raises(ValueError):
        rtamd.pack_rays(o, d[:2])


def test_yardstick_1_equals_a_brute_force_minimum():
    """One ray through the oracle's 1 x 1 frame is the closest hit of exactly that ray: id and every
    bit of t equal a minimum over ALL triangles of the oracle's own ray-triangle test."""
    d = scene_arrays("rand2k")
    o, dirs, campos = incoherent_rays(d, n=50)
    ids, t = oracle_closest(d, o, campos)
    assert 10 < int((ids >= 0).sum()) < 50, "the rays should both hit and miss"
    assert np.all(t[ids < 0] == TMAX_DEFAULT)
    for k in range(50):
        bid, bt = brute_force_closest(d, o[k], dirs[k])
        assert np.float32(bt).view(np.uint32) == t[k].view(np.uint32), (k, bt, t[k])
        assert (bid >= 0) == (ids[k] >= 0), (k, bid, ids[k])
        if bid != ids[k]:   # two triangles at the same distance: the traversal may meet the other first
            from ray_query_common import oracle_normalize, oracle_ray_tri
            assert oracle_ray_tri(d, o[k], oracle_normalize(dirs[k]), int(ids[k])) == bt, (k, bid, ids[k])


def test_yardstick_2_rays_are_exact_and_are_the_frame_s():
    """The quantised frame's rays are exact in float32 (asserted inside the helper), and tracing them
    one by one through yardstick 1 gives the oracle's own frame at those pixels."""
    from oracle import oracle
    d = scene_arrays("rand2k")
    w, h = 64, 32
    p, o, dirs = quantised_frame(d, w, h)
    assert o.shape == (w * h, 3) and np.all(np.any(dirs != 0.0, axis=1))
    frame = oracle.render(d, p, w, h, depth=1, flags=1)
    traced = frame["hits"][:, 0, 0] != -2
    assert int((frame["hits"][:, 0, 0] >= 0).sum()) > 50, "the quantised camera sees too little"
    pix = np.arange(0, w * h, 13)
    campos = np.broadcast_to(p[12:15], (pix.size, 3))
    # yardstick 1 rebuilds the direction as fl(o - campos): the frame's own subtraction
    ids, t = oracle_closest(d, o[pix], campos)
    for j, k in enumerate(pix):
        if traced[k]:
            assert ids[j] == frame["hits"][k, 0, 0], (k, ids[j], frame["hits"][k, 0, 0])
            assert t[j].view(np.uint32) == frame["t"][k, 0].view(np.uint32), k
        else:   # outside the golden's scene box the frame traces nothing; such a ray can hit nothing
            assert ids[j] == -1, k


# ---- the arbitrary-ray entry of the oracle (oracle.trace_rays), pinned before the GPU tests trust it ----

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _query_scenes():
    from test_ray_query_gpu import SCENES
    return SCENES + ["overflow_comb", "deep_comb40"]


@pytest.mark.parametrize("name", ["cornell12", "rand2k", "rand4k_sbvh", "rand3k_bigleaf", "single_tri_rootleaf",
                                  "rand2k_built", "overflow_comb", "deep_comb40"])
def test_oracle_trace_rays_equals_yardstick_1(name):
    """Where yardstick 1 can express a ray -- (o, fl(o - campos)), the default tmax, closest hit -- the new
    entry gives its ids, every bit of its t and its overflow count.  Were they to differ, the new entry
    would be the wrong one."""
    from oracle import oracle
    from ray_edge_common import edge_scene
    assert name in _query_scenes() and len(_query_scenes()) == 8
    d = edge_scene(name)
    o, dirs, campos = incoherent_rays(d)
    st = {}
    ids, t = oracle_closest(d, o, campos, st)
    gi, gt, stats = oracle.trace_rays(d, rtamd.pack_rays(o, dirs))
    assert np.array_equal(gi, ids) and np.array_equal(_bits(gt), _bits(t))
    assert stats["stack_overflow"] == st["stack_overflow"] and stats["error_miss"] == 0
    assert (st["stack_overflow"] > 0) == (name == "overflow_comb")
    assert stats["inner"] > 0 or name == "single_tri_rootleaf"
    assert 1 <= stats["max_stack"] <= 65
    assert (stats["leaf"] > 0 and stats["tris"] > 0) or name == "overflow_comb"   # (its rays overflow or miss the box)


def _tmax_rays(d, n, seed):
    """n incoherent rays, their closest hits by yardstick 1 and a per-ray tmax uniform in (0.001, 2 t*)
    (in (0.001, 200) where the ray misses)."""
    o, dirs, campos = incoherent_rays(d, n=n)
    ids, t = oracle_closest(d, o, campos)
    rng = np.random.default_rng(seed)
    top = np.where(ids >= 0, 2.0 * t.astype(np.float64), 200.0)
    tm = (0.001 + rng.uniform(0.0, 1.0, n) * (top - 0.001)).astype(np.float32)
    tm = np.maximum(tm, np.nextafter(np.float32(0.001), np.float32(1)))
    return o, dirs, ids, t, tm


def test_oracle_trace_rays_per_ray_tmax_equals_a_brute_force_minimum():
    from oracle import oracle
    from ray_query_common import TMIN, oracle_normalize, oracle_ray_tri
    d = scene_arrays("rand2k")
    o, dirs, ids, t, tm = _tmax_rays(d, 50, 11)
    cut = (ids >= 0) & (tm <= t)
    assert 5 < int(cut.sum()) and 5 < int(((ids >= 0) & (tm > t)).sum()), "tmax should fall on both sides of t*"
    rays = rtamd.pack_rays(o, dirs, tm)
    ci, ct, _ = oracle.trace_rays(d, rays)
    ai, at, _ = oracle.trace_rays(d, rays, any_hit=True)
    assert np.array_equal(ai >= 0, ci >= 0), "any hit and closest hit disagree on hit / miss"
    for k in range(50):
        bid, bt = brute_force_closest(d, o[k], dirs[k], tm[k])
        assert _bits(bt)[0] == _bits(ct[k])[0], (k, bt, ct[k])
        assert (bid >= 0) == (ci[k] >= 0), (k, bid, ci[k])
        dirn = oracle_normalize(dirs[k])
        if bid != ci[k]:   # two triangles at the same distance: the traversal may meet the other first
            assert oracle_ray_tri(d, o[k], dirn, int(ci[k])) == bt, (k, bid, ci[k])
        if ci[k] < 0:
            assert ci[k] == -1 and ai[k] == -1
            assert _bits(ct[k])[0] == _bits(tm[k])[0] == _bits(at[k])[0], "a miss's t is the tmax word"
        else:
            assert ai[k] % 3 == 0 and 0 <= ai[k] < d["indices"].size
            assert _bits(at[k])[0] == _bits(oracle_ray_tri(d, o[k], dirn, int(ai[k])))[0], k
            assert TMIN < at[k] < tm[k] and at[k] >= ct[k], (k, at[k], ct[k], tm[k])


def test_oracle_trace_rays_invalid_rays_are_untraversed_misses():
    """test_invalid_rays_are_misses_and_leave_their_neighbours' ten cases: id -1, the tmax word unchanged
    (a NaN's payload too), no traversal work counted; +inf is a legal tmax."""
    from oracle import oracle
    d = scene_arrays("cornell12")
    o, dirs, _ = incoherent_rays(d, n=16)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    payload = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    cases = {
        "nan origin": ("o", 1, nan), "inf origin": ("o", 2, inf), "-inf origin": ("o", 0, -inf),
        "nan direction": ("d", 0, nan), "inf direction": ("d", 1, inf), "zero direction": ("d", None, 0.0),
        "nan tmax": ("tmax", None, payload), "zero tmax": ("tmax", None, 0.0), "negative tmax": ("tmax", None, -5.0),
        "tmax at tmin": ("tmax", None, np.float32(0.001)),
    }
    assert len(cases) == 10
    base = oracle.trace_rays(d, rtamd.pack_rays(o, dirs))
    assert base[0][3] >= 0, "the ray the cases are made from hits when left alone"
    for label, (field, comp, val) in cases.items():
        rays = rtamd.pack_rays(o, dirs)
        for any_hit in (False, True):
            one = rays[3:4].copy()
            if field == "tmax":
                one["tmax"].view(np.uint32)[0] = np.float32(val).view(np.uint32)
            elif comp is None:
                one[field][0] = val
            else:
                one[field][0, comp] = val
            gi, gt, stats = oracle.trace_rays(d, one, any_hit=any_hit)
            assert gi[0] == -1 and _bits(gt)[0] == _bits(one["tmax"])[0], label
            assert stats["inner"] == stats["leaf"] == stats["tris"] == stats["max_stack"] == 0, label
    gi, gt, _ = oracle.trace_rays(d, rtamd.pack_rays(o, dirs, inf))
    hit = gi >= 0
    assert np.array_equal(gi, base[0]) and np.array_equal(_bits(gt[hit]), _bits(base[1][hit])), "+inf is a legal tmax"
    assert np.all(gt[~hit] == inf)
    gi, gt, _ = oracle.trace_rays(scene_arrays("single_tri_rootleaf"), rtamd.pack_rays(o, dirs, inf))
    assert np.any(gi < 0) and np.all(gt[gi < 0] == inf)


def test_oracle_trace_rays_counts_error_misses():
    """bad_node's malformed inner node: rays aimed into its box leave the traversal through the
    malformed-node exits; they are misses with the tmax word, counted, and a scene without such a node
    counts none."""
    from oracle import oracle
    from ray_edge_common import edge_scene, malformed_nodes, oracle_hits, ray_class
    d = edge_scene("bad_node")
    assert malformed_nodes(d).size == 1
    o, dirs, tm = ray_class("bad_node", "malformed")
    for any_hit in (False, True):
        ids, t, stats = oracle_hits("bad_node", "malformed", any_hit)
        assert stats["error_miss"] >= 10 and stats["stack_overflow"] == 0, stats
        assert int((ids >= 0).sum()) > 100 and np.array_equal(_bits(t[ids < 0]), _bits(tm[ids < 0]))
        # without the defect the same rays hit more: the error misses are rays that would have gone on
        ni = np.array(d["nodes"], np.float32, copy=True)
        good = dict(d, nodes=ni)
        w = ni.view(np.int32).reshape(-1, 12)
        w[malformed_nodes(d)[0], 9] = w[malformed_nodes(d)[0], 8]   # the left child twice: no longer an error exit
        assert oracle.trace_rays(good, rtamd.pack_rays(o, dirs, tm), any_hit=any_hit)[2]["error_miss"] == 0


# ---- the ray classes of tests/ray_edge_common.py: what each is, and that they hit and miss ----

def test_ray_class_properties():
    import ray_edge_common as E
    from octant_common import octant_of
    for name in E.EDGE_SCENES:
        d = E.edge_scene(name)
        lo, hi = E.scene_box(d)
        for cls in E.CLASSES:
            o, dirs, tm = E.ray_class(name, cls)
            assert o.shape == dirs.shape and o.shape[0] == tm.shape[0] <= 2048 and o.shape[0] % 64 == 0, (name, cls)
            assert np.all(np.isfinite(o)) and np.all(np.isfinite(dirs)) and np.all(np.any(dirs != 0, axis=1)), (name, cls)
            assert np.all(tm > np.float32(0.001)), (name, cls)
        o, dirs, _ = E.ray_class(name, "axis1")
        assert np.all((dirs != 0).sum(axis=1) == 1)
        ax = np.argmax(dirs != 0, axis=1)
        k = np.arange(o.shape[0])
        out = np.where(dirs[k, ax] > 0, lo[ax] - o[k, ax], o[k, ax] - hi[ax])
        assert np.all(out == 20.0) and np.all(np.signbit(dirs).any(axis=0)) and np.all((~np.signbit(dirs)).any(axis=0))
        inside = (o >= lo) & (o <= hi)
        assert np.all(inside.sum(axis=1) == 2)
        o, dirs, _ = E.ray_class(name, "axis2")
        assert np.all((dirs == 0).sum(axis=1) == 1)
        assert np.all((E.normalised(dirs) == 0).sum(axis=1) == 1)
        # snapped: the coordinates that make the ray pass through a vertex are that vertex's, bit for bit
        o, dirs, _, pick = E.snapped(d)
        v = np.asarray(d["vertices"], np.float32)[np.unique(d["indices"]), :3][pick]
        h = o.shape[0] // 2
        zero = dirs == 0
        assert np.all(zero[:h].sum(axis=1) == 2) and np.all(zero[h:].sum(axis=1) == 1)
        assert np.array_equal(o[zero], v[zero]), "a snapped coordinate is not the vertex's"
        assert np.array_equal(dirs[h:], (v[h:] - o[h:]).astype(np.float32)), "axis2 snapped rays aim at their vertex"
        za = np.argmax(zero[h:], axis=1)
        kk = np.arange(h)
        on_plane = (o[h:][kk, za] == lo[za]) | (o[h:][kk, za] == hi[za])
        assert int(on_plane.sum()) >= h // 4, "rays lying in the scene box's planes"
        # near_axis: the normalised direction IS the input, and holds every magnitude with both signs
        o, dirs, _ = E.ray_class(name, "near_axis")
        assert np.array_equal(_bits(E.normalised(dirs)), _bits(dirs))
        assert np.all((np.abs(dirs) == 1.0).sum(axis=1) == 1)
        for g, m in enumerate(E.NEAR_AXIS_MAGNITUDES):
            a, b = dirs[128 * g:128 * g + 64], dirs[128 * g + 64:128 * g + 128]
            assert m > 0 and np.all((np.abs(a) == m).sum(axis=1) == 2), m
            assert np.all((np.abs(b) == m).sum(axis=1) == 1) and np.all((b == 0).sum(axis=1) == 1), m
            small = a[np.abs(a) == m]
            assert np.any(small > 0) and np.any(small < 0)
        # origin_domain: one run of 64 per value, the value on one axis, tmax = +inf
        o, dirs, tm = E.ray_class(name, "origin_domain")
        assert np.all(tm == np.inf) and o.shape[0] == 64 * len(E.ORIGIN_VALUES)
        for g, val in enumerate(E.ORIGIN_VALUES):
            run = o[64 * g:64 * g + 64]
            assert np.array_equal(_bits(run[kk[:64], kk[:64] % 3]), np.full(64, _bits(val)[0], np.uint32)), val
        # scaled: which normalize branch each third takes; every component finite, non-zero and normal
        o, dirs, _ = E.ray_class(name, "scaled")
        n3 = o.shape[0] // 3
        assert np.all(np.abs(dirs) >= np.finfo(np.float32).tiny)
        for g, branch in enumerate(E.SCALE_EXPONENTS):
            assert np.all(E.normalize_branch(dirs[n3 * g:n3 * g + n3]) == branch), branch
            assert np.array_equal(o[n3 * g:n3 * g + n3], o[:n3])
        for k8 in range(8):
            o, dirs, _ = E.ray_class(name, f"octant{k8}")
            assert o.shape[0] % 64 == 0 and octant_of(dirs) == k8 and octant_of(E.normalised(dirs)) == k8
            for arithmetic in ("ref", "strict", "hw"):
                assert np.all(E.in_domain(o, dirs, arithmetic)), (name, k8, arithmetic)


@pytest.mark.parametrize("arithmetic", ["ref", "strict", "hw"])
def test_ray_classes_lie_on_both_sides_of_the_quotient_domain(arithmetic):
    """near_axis and origin_domain hold, for each bound of axis_ok that a ray can cross (a normalised
    component never exceeds 1, so the direction's upper bound of 2 has no other side), whole 64-ray
    groups inside the domain and groups with rays outside it."""
    import ray_edge_common as E
    for name in E.EDGE_SCENES:
        o, dirs, _ = E.ray_class(name, "near_axis")
        ok = E.in_domain(o, dirs, arithmetic).reshape(-1, 64)
        lower = E.p2(-126) if arithmetic == "ref" else E.p2(-64)
        for g, m in enumerate(E.NEAR_AXIS_MAGNITUDES):
            assert np.all(ok[2 * g] == (m >= lower)) and np.all(ok[2 * g + 1] == (m >= lower)), (name, m)
        assert lower in E.NEAR_AXIS_MAGNITUDES and np.nextafter(lower, np.float32(0)) in E.NEAR_AXIS_MAGNITUDES \
            or arithmetic == "ref" and E.p2(-127) in E.NEAR_AXIS_MAGNITUDES
        o, dirs, _ = E.ray_class(name, "origin_domain")
        ok = E.in_domain(o, dirs, arithmetic).reshape(-1, 64)
        for g, val in enumerate(E.ORIGIN_VALUES):
            a = abs(val)
            inside = a == 0 or E.p2(-66) <= a <= E.p2(60)
            if inside:
                assert np.all(ok[g]), (name, val)
            else:
                assert not np.any(ok[g]), (name, val)
        both = [abs(v) for v in E.ORIGIN_VALUES]
        assert E.p2(-66) in both and E.p2(-67) in both and E.p2(60) in both and np.nextafter(E.p2(60), np.float32(np.inf)) in both


def test_ray_classes_hit_and_miss():
    """Conditions on the inputs, with the oracle alone: in every (scene, class) at least 10 % of the rays
    hit; in every scene but the closed cornell12 at least 5 % of all classes' rays together miss."""
    import ray_edge_common as E
    for name in E.EDGE_SCENES:
        hits = total = 0
        for cls in E.CLASSES:
            ids, t, stats = E.oracle_hits(name, cls)
            share = float((ids >= 0).mean())
            print(f"{name:20s} {cls:14s} hit share {share:.2f} of {ids.size}")
            assert share >= 0.10, (name, cls, share)
            assert stats["error_miss"] == 0 and stats["stack_overflow"] == 0
            hits += int((ids >= 0).sum())
            total += ids.size
        if name != "cornell12":
            assert (total - hits) >= 0.05 * total, (name, hits, total)
