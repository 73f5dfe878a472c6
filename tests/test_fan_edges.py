"""The inputs of tests/test_fan_edges_gpu.py reach the edges they are made for ("Tests at
the edges"): every condition is asserted here from the oracle, tests/fan_ref.c and
ray_edge_common's restatement of the quotient's domain alone, with the measured figure in the
message.  No GPU."""
import numpy as np
import pytest

import rtamd
import fan_common as F
import fan_edge_common as Z
import hit_attr_edge_common as X
import ray_edge_common as E
from ray_query_common import TMAX_DEFAULT

F32 = np.float32


def expand_equals_ref(fan):
    """rt_fan_expand and fan_ref.c agree on a fan in every ray word and traced flag."""
    rays, traced = rtamd.fan_expand(fan.rec, fan.dirs)
    want_rays, want_traced = F.ref_expand(fan.rec, fan.dirs)
    assert np.array_equal(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).view(np.uint32).reshape(-1, 8), want_rays), fan.label
    assert np.array_equal(traced, want_traced), fan.label


# ---- A ----

def test_cull_edge_set_shows_every_consequence_as_a_bit():
    fan = Z.cull_edge()
    assert fan.n == 105 + 3 and fan.k == 22
    assert np.array_equal(fan.rec["o"][:105], np.tile(np.array([(0.5, -0.25, 2.0)], F32), (105, 1)))
    assert E.normalize_branch(fan.dirs[20:21])[0] == "below FLT_MIN"          # the replaced direction keeps the margin
    expand_equals_ref(fan)
    _, traced, hit, stats = fan.yard()
    valid = np.flatnonzero(np.all(np.isfinite(fan.dirs), axis=1) & np.any(fan.dirs != 0, axis=1))
    per_dir = [int(hit[:, j].sum()) for j in valid]
    print(f"cull edge set: {int(traced.sum())} rays traced, {int(hit.sum())} hit, per valid direction {per_dir}")
    assert valid.size == 16 and not traced[:, np.setdiff1d(np.arange(fan.k), valid)].any()
    assert min(per_dir) >= 8, f"traced rays that hit, per valid direction: {per_dir}"
    assert stats["stack_overflow"] == 0
    plain = Z.plain_hits(fan)
    assert plain[valid].all(), "every valid direction hits the box from the edge set's origin"
    for name, rows, cols, is_traced in Z.cull_consequences(fan):
        sub_t, sub_h = traced[np.ix_(rows, cols)], hit[np.ix_(rows, cols)]
        print(f"{name}: {rows.size} origins x {cols.size} directions, {int(sub_t.sum())} traced, {int(sub_h.sum())} hit")
        assert rows.size >= 1 and plain[cols].any(), f"{name}: no ray that hits by the oracle"
        assert sub_t.all() if is_traced else not sub_t.any(), name
        if name == "the float above 0.001 is traced":
            # traced, but (0.001, the float above it] holds no hit: the flag shows on the CPU alone
            assert not sub_h.any(), name
        elif is_traced:
            assert sub_h.sum() >= 1 and np.array_equal(sub_h, np.broadcast_to(plain[cols], sub_h.shape)), f"{name}: {int(sub_h.sum())} hit"
    rec, dirs = Z.with_reserved_and_w(fan)
    assert np.all(rec["reserved"] == 0xFFFFFFFF) and np.isnan(dirs[0, 3]) and np.isinf(dirs[1, 3]) and dirs[2, 3] == F32(-1e30) and dirs[3, 3] == 1
    want_rays, want_traced = F.ref_expand(fan.rec, fan.dirs)
    got_rays, got_traced = F.ref_expand(rec, dirs)
    assert np.array_equal(got_rays, want_rays) and np.array_equal(got_traced, want_traced), "fan_ref.c ignores reserved and w"
    r2, t2 = rtamd.fan_expand(rec, dirs)
    assert np.array_equal(t2, want_traced) and not r2["reserved"].any(), "rt_fan_expand ignores reserved and w"


# ---- B ----

def test_origin_groups_lie_on_both_sides_of_the_domain():
    g = Z.origin_groups()
    assert g.n == 704 and g.k == 64 and len(E.ORIGIN_VALUES) == 11
    o = g.rec["o"].reshape(11, 64, 3)
    lane = np.arange(64)
    for r, val in enumerate(E.ORIGIN_VALUES):
        assert np.array_equal(o[r, lane, lane % 3].view(np.uint32), np.full(64, val, F32).view(np.uint32))
    assert sorted(Z.RUNS_INSIDE + Z.RUNS_OUTSIDE) == list(range(11)) == sorted(Z.RUNS_SMALL + Z.RUNS_LARGE)
    assert [E.ORIGIN_VALUES[r] for r in Z.RUNS_OUTSIDE] == [E.p2(-67), -E.p2(-67), F32(1e-25), np.nextafter(E.p2(60), F32(np.inf)), E.p2(61), F32(1e30)]
    nonzero = np.all(E.normalised(g.dirs) != 0, axis=1)
    assert nonzero.sum() >= 60
    for a in Z.ARITHMETICS:
        dom = Z.rays_in_domain(g, a).reshape(11, 64, 64)
        for r in Z.RUNS_INSIDE:
            assert dom[r].all(), f"{a}: run {r} ({E.ORIGIN_VALUES[r]}) has {int((~dom[r]).sum())} rays outside the domain"
        for r in Z.RUNS_OUTSIDE:
            assert not dom[r][:, nonzero].any(), f"{a}: run {r} ({E.ORIGIN_VALUES[r]}) has {int(dom[r][:, nonzero].sum())} rays inside the domain"
    _, traced, hit, stats = g.yard()
    share = hit.reshape(11, 64, 64).mean(axis=(1, 2))
    print("origin groups: share of bits set per run", np.round(share, 3))
    assert traced.all() and stats["stack_overflow"] == 0
    assert np.all(share[Z.RUNS_SMALL] > 0.20), f"bits set per small-value run: {share[Z.RUNS_SMALL]}"
    assert not hit.reshape(11, 64, 64)[Z.RUNS_LARGE].any(), f"bits set per large-value run: {share[Z.RUNS_LARGE]}"


@pytest.mark.parametrize("value", list(Z.LANE_VALUES))
@pytest.mark.parametrize("lane", Z.LANES)
def test_one_lane_leaves_the_domain(lane, value):
    whole, f, at = Z.one_lane(lane, value)
    assert whole.n == f.n == 192 and at.tolist() == [lane, 64 + lane, 128 + lane]
    keep = np.setdiff1d(np.arange(f.n), at)
    assert np.array_equal(f.rec[keep], whole.rec[keep]) and np.all(f.rec["o"][at, 0] == Z.LANE_VALUES[value])
    nonzero = np.all(E.normalised(f.dirs) != 0, axis=1)
    for a in Z.ARITHMETICS:
        dom = Z.rays_in_domain(f, a)
        assert dom[keep].all() and not dom[at][:, nonzero].any(), f"{a}: the replaced lane alone is outside the domain"
    assert np.array_equal(f.want[:, keep], whole.want[:, keep]), "the oracle's words of the other 63 lanes"
    share = whole.yard()[2].mean()
    assert share > 0.20, f"bits set in the whole fan: {share:.3f}"


# ---- C ----

def test_edge_table_holds_every_class_in_every_chunk():
    dirs, names = Z.edge_table()
    cls = Z.direction_classes()
    assert dirs.shape == (96, 3) and {k: v.shape[0] for k, v in cls.items()} == {"octant": 20, "axis1": 18, "axis2": 24, "near_axis": 28, "scaled": 6}
    assert np.unique(dirs.view(np.uint32), axis=0).shape[0] == 96, "no direction twice"
    zeros = np.sum(dirs == 0, axis=1)
    by = lambda c: np.array([n == c for n in names])
    assert np.all(zeros[by("octant")] == 0) and np.all(zeros[by("axis1")] == 2) and np.all(zeros[by("axis2")] == 1)
    assert np.signbit(dirs[by("axis1")][dirs[by("axis1")] == 0]).any() and not np.signbit(dirs[by("axis1")][dirs[by("axis1")] == 0]).all()
    assert np.signbit(dirs[by("axis2")][dirs[by("axis2")] == 0]).any() and not np.signbit(dirs[by("axis2")][dirs[by("axis2")] == 0]).all()
    assert len({tuple(np.signbit(v)) for v in dirs[by("octant")]}) == 8
    near = dirs[by("near_axis")]
    small = np.sort(np.abs(near), axis=1)
    assert np.all(small[:, 2] == 1)
    for m in E.NEAR_AXIS_MAGNITUDES:
        assert np.sum((small[:, 1] == m) & (small[:, 0] == m)) == 2 and np.sum((small[:, 1] == m) & (small[:, 0] == 0)) == 2, m
    same = sum(a == b for a, b in zip(names, names[1:]))
    assert same <= 1, f"{same} neighbouring directions of one class"
    branch = E.normalize_branch(dirs)          # asserts its own margin for every direction
    counts = {b: int((branch == b).sum()) for b in ("normal", "below FLT_MIN", "inf")}
    assert min(counts.values()) >= 3, f"normalize's branches: {counts}"
    for a in Z.ARITHMETICS:
        ok = Z.domain_table(dirs, a)
        per_chunk = [(int(ok[c:c + 32].sum()), int((~ok[c:c + 32]).sum())) for c in (0, 32, 64)]
        print(f"{a}: directions (inside, outside) the domain per chunk {per_chunk}")
        assert all(i >= 1 and o >= 1 for i, o in per_chunk), f"{a}: {per_chunk}"


def test_edge_table_fans_see_the_scene():
    free, culled = Z.table_fan(False), Z.table_fan(True)
    assert free.n == culled.n == 192 and free.k == 96
    expand_equals_ref(free)
    expand_equals_ref(culled)
    _, traced, hit, stats = free.yard()
    assert traced.all() and stats["stack_overflow"] == 0
    assert hit.mean() > 0.15, f"unculled bits set: {hit.mean():.3f}"
    assert hit.any(axis=0).all(), "every direction hits from some origin"
    _, ctraced, chit, _ = culled.yard()
    print(f"edge table: unculled {hit.mean():.3f} set; culled {ctraced.mean():.3f} traced, {chit[ctraced].mean():.3f} of those set")
    assert 0.3 < ctraced.mean() < 0.7 and np.array_equal(chit, hit & ctraced)


# ---- D ----

def test_tmax_sweep_brackets_each_lanes_own_hit():
    f, jstar, turn, (ids, t) = Z.tmax_sweep()
    assert f.n == 192 and np.array_equal(jstar, np.arange(192) % 64) and np.array_equal(turn, np.arange(192) % 6)
    hits = ids >= 0
    assert hits.sum() >= 96, f"rays (i, j*) that hit: {int(hits.sum())}"
    tm = f.rec["tmax"]
    assert np.all(tm[~hits] == TMAX_DEFAULT)
    for k, want in enumerate([F32(0.5) * t, np.nextafter(t, F32(0)), t, np.nextafter(t, F32(np.inf)), F32(2) * t, np.full(192, np.inf, F32)]):
        pick = hits & (turn == k)
        assert pick.sum() >= 10 and np.array_equal(tm[pick], want.astype(F32)[pick])
    _, traced, hit, _ = f.yard()
    own = hit[np.arange(192), jstar]
    # (an origin lies 0.001 short of its surface, so a t* can be near 0.001 and a swept tmax at or below it)
    assert np.array_equal(traced, np.broadcast_to((tm > F32(0.001))[:, None], traced.shape))
    assert traced.mean() > 0.90, f"origins whose swept tmax stays above 0.001: {int(traced[:, 0].sum())} of 192"
    assert not own[hits & (turn <= 2)].any(), "tmax <= t*: the ray's own hit is out of reach"
    assert own[hits & (turn >= 4)].all(), "tmax = 2 t* and +inf: the ray hits"
    above = hits & (turn == 3)
    back = int(own[above].sum())
    print(f"tmax sweep: {int(hits.sum())} of 192 rays hit; {back} of {int(above.sum())} come back with the float above t*")
    assert back >= 0.9 * above.sum(), f"{back} of {int(above.sum())}"
    # the per-lane tmax matters to the other 63 directions too: the words differ from one tmax for all
    assert not np.array_equal(f.want, F.yardstick_for(f.d, rtamd.pack_fan_origins(f.rec["o"], None, None), f.dirs))


def test_comb_restarts_lose_hits_to_the_short_tmax():
    quarter, default, turns = Z.comb_tmax("quarter"), Z.comb_tmax("default"), Z.comb_tmax("turns")
    assert quarter.n == 128 and quarter.k == 48
    q = F.quarter_diagonal(quarter.d)
    assert np.array_equal(turns.rec["tmax"], np.array([TMAX_DEFAULT, F32(2) * q, q], F32)[np.arange(128) % 3])
    hq, hd, ht = quarter.yard()[2], default.yard()[2], turns.yard()[2]
    for f in (quarter, default, turns):
        st = f.yard()[3]
        assert st["stack_overflow"] == 0 and st["max_stack"] > 16, f"{f.label}: {st}"
    lost = int((hd & ~hq).sum())
    print(f"deep_comb40: {int(hd.sum())} hit with the default tmax, {int(hq.sum())} with a quarter of the diagonal, {int(ht.sum())} by turns")
    assert lost >= 30 and not (hq & ~hd).any(), f"rays that hit under the default tmax and miss under the quarter: {lost}"
    rows = np.arange(128) % 3
    assert np.array_equal(ht[rows == 0], hd[rows == 0]) and np.array_equal(ht[rows == 2], hq[rows == 2])
    assert (hd & ~ht).any() and (ht & ~hq).any(), "the three tmax values by turns differ from either single one"


# ---- E ----

@pytest.mark.parametrize("name,origins", zip(Z.TREES, (253, 474, 474)))
def test_tree_fans(name, origins):
    f = Z.tree_fan(name)
    expand_equals_ref(f)
    _, traced, hit, stats = f.yard()
    share = hit[traced].mean()
    print(f"{name}: {f.n} origins, {traced.mean():.3f} traced, {share:.4f} of those set")
    assert f.n == origins and f.k == 64
    assert 0.45 < traced.mean() < 0.55, f"{name}: traced {traced.mean():.3f}"
    assert 0.23 <= share <= 0.65, f"{name}: traced bits set {share:.4f}"
    assert stats["stack_overflow"] == 0


def test_the_trees_are_what_their_names_say():
    d = Z.tree_fan("rand4k_sbvh").d
    assert d["tri_indices"].size > d["indices"].size // 3, "a spatial-split tree references triangles more than once"
    d = Z.mesh_fan("single_tri_rootleaf").d
    assert d["indices"].size == 3 and np.asarray(d["nodes"]).reshape(-1, 12).shape[0] == 1, "the root is a leaf"
    d = Z.mesh_fan("bigleaf").d
    leaf = np.asarray(d["nodes"]).view(np.int32).reshape(-1, 12)
    assert d["tri_indices"].size >= 64 and leaf.shape[0] < d["tri_indices"].size // 8, "leaves of many triangles"


@pytest.mark.parametrize("label", Z.OUTSIDE)
def test_mesh_fans(label):
    f = Z.mesh_fan(label)
    assert f.n == (64 if label == "tiny_tris" else 256) and f.k == 64
    assert np.array_equal(f.rec["n"][:64], f.dirs) and np.all(np.isinf(f.rec["tmax"]))
    expand_equals_ref(f)
    _, traced, hit, stats = f.yard()
    print(f"{label}: {traced.mean():.3f} traced, {int(hit.sum())} bits set, {stats}")
    assert traced[np.arange(64), np.arange(64)].all(), "an origin's own direction is traced"
    assert hit.sum() >= 64, f"{label}: {int(hit.sum())} bits set"
    assert stats["stack_overflow"] == 0
