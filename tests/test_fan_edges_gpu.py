"""Occlusion fans on the GPU at the edges of the cull rule, of ray space and of mesh space (DESIGN.md 21,
"Tests at the edges"): the inputs of tests/fan_edge_common.py through fan_kernel's own cull rule, its
waves' choice of a traversal loop, its per-lane tmax and restart value, and its direction staging.
tests/test_fan_edges.py shows on the CPU that the inputs reach their edges.

The two yardsticks of tests/test_fan_gpu.py and nothing else: S_strict against the oracle on
fan_ref.c's traced rays, and all three arithmetics, with and without RT_FLAG_EXACT_DIV, against the
expanded query on the same context.  Everything is compared as words."""
import numpy as np
import pytest

import rtamd
import fan_common as F
import fan_edge_common as Z
from test_fan_gpu import ARITHMETICS, EXACT_DIV, GUARD, MESH_KEYS, STRICT, query_masks, same_masks, upload
from test_ray_query_edges_gpu import general  # noqa: F401  (the split-records context, a module fixture)

pytestmark = pytest.mark.gpu


def against_both(r, fan, label=None, exact_div=True):
    """A fan on context r in all three arithmetics (and with RT_FLAG_EXACT_DIV) against the expanded query
    on r, and S_strict against the oracle.  Returns the masks per arithmetic."""
    label = label or fan.label
    out = {}
    for mode, f in ARITHMETICS.items():
        for extra in ((0, EXACT_DIV) if exact_div else (0,)):
            got = r.trace_fan(fan.rec, fan.dirs, flags=f | extra)
            same_masks(got, query_masks(r, fan.rec, fan.dirs, f | extra), f"{label} {mode} extra={extra}: the expanded query")
            if mode == "strict":
                same_masks(got, fan.want, f"{label} extra={extra}: the oracle")
            if not extra:
                out[mode] = got
    return out


def bit(masks, i, j):
    return (int(masks[j >> 5, i]) >> (j & 31)) & 1


# ---- A: the cull rule's edge set ----

def test_cull_rule_edge_set(renderer):
    fan = Z.cull_edge()
    upload(renderer, fan.d)
    first = against_both(renderer, fan)
    rec, dirs = Z.with_reserved_and_w(fan)
    for mode, f in ARITHMETICS.items():
        for extra in (0, EXACT_DIV):
            same_masks(renderer.trace_fan(rec, dirs, flags=f | extra), first[mode], f"reserved = 0xFFFFFFFF and w set, {mode} extra={extra}")
    # the rule's consequences by name, each on a ray that hits (tests/test_fan_edges.py)
    plain = Z.plain_hits(fan)
    for mode, got in first.items():
        for name, rows, cols, traced in Z.cull_consequences(fan):
            want = 1 if traced and name != "the float above 0.001 is traced" else 0
            for i in rows:
                for j in cols[plain[cols]]:
                    assert bit(got, i, j) == want, f"{mode}: {name}: origin {i}, direction {j}"


# ---- B: origins at the edges of the quotient's domain ----

def test_origin_groups_inside_and_outside_the_domain(renderer):
    g = Z.origin_groups()
    upload(renderer, g.d)
    for mode, got in against_both(renderer, g).items():
        share = rtamd.fan_bits(got, g.k).reshape(11, 64, 64).mean(axis=(1, 2))
        assert np.all(share[Z.RUNS_SMALL] > 0.20) and not share[Z.RUNS_LARGE].any(), f"{mode}: {share}"


@pytest.mark.parametrize("value", list(Z.LANE_VALUES))
def test_one_lane_moves_its_wave_to_the_division_form(renderer, value):
    whole = Z.one_lane(0, value)[0]
    upload(renderer, whole.d)
    base = against_both(renderer, whole, exact_div=False)
    for lane in Z.LANES:
        _, f, at = Z.one_lane(lane, value)
        keep = np.setdiff1d(np.arange(f.n), at)
        for mode, got in against_both(renderer, f, exact_div=False).items():
            assert np.array_equal(got[:, keep], base[mode][:, keep]), f"{mode} lane {lane} at x = {value}: the other 63 lanes' words"


# ---- C: a direction table at the edges of direction space ----

@pytest.mark.parametrize("cull", [False, True], ids=["nocull", "cull"])
def test_edge_direction_table(renderer, general, cull):  # noqa: F811
    fan = Z.table_fan(cull)
    upload(renderer, fan.d)
    g = general(fan.d)
    got = against_both(renderer, fan)
    for mode, f in ARITHMETICS.items():
        same_masks(g.trace_fan(fan.rec, fan.dirs, flags=f), got[mode], f"{fan.label} {mode}: general vs fast")
        same_masks(g.trace_fan(fan.rec, fan.dirs, flags=f), query_masks(g, fan.rec, fan.dirs, f), f"{fan.label} {mode}: general fan vs general query")
        bits = rtamd.fan_bits(got[mode], fan.k)
        for j in range(fan.k):
            alone = rtamd.fan_bits(renderer.trace_fan(fan.rec, fan.dirs[j:j + 1], flags=f), 1)[:, 0]
            assert np.array_equal(bits[:, j], alone), f"{fan.label} {mode}: direction {j} ({Z.edge_table()[1][j]}) alone"
        assert cull or bits.mean() > 0.15


# ---- D: tmax per lane ----

def test_tmax_sweep_per_lane(renderer):
    fan, jstar, turn, (ids, _) = Z.tmax_sweep()
    upload(renderer, fan.d)
    got = against_both(renderer, fan)["strict"]
    own = np.array([bit(got, i, int(jstar[i])) for i in range(fan.n)])
    hits = ids >= 0
    assert not own[hits & (turn <= 2)].any(), "0.5 t*, the float below t* and t* itself: the lane's own hit is out of reach"
    assert own[hits & (turn >= 4)].all(), "2 t* and +inf: the lane's ray hits"
    above = hits & (turn == 3)
    assert np.array_equal(own[above], fan.yard()[2][np.arange(fan.n), jstar][above].astype(int)), "the float above t*: the oracle's any hit"


def test_restart_begins_from_the_lanes_own_tmax(renderer):
    d = upload(renderer, Z.comb_tmax("quarter").d)
    before = renderer.overflow_count()
    for setting in ("quarter", "turns", "default"):
        fan = Z.comb_tmax(setting)
        assert fan.d is d
        for mode, f in ARITHMETICS.items():
            got = renderer.trace_fan(fan.rec, fan.dirs, flags=f)
            assert renderer.last_deferred() > 0, "these rays outgrow the LDS stack and restart"
            same_masks(got, query_masks(renderer, fan.rec, fan.dirs, f), f"{fan.label} {mode}: the expanded query")
            if mode == "strict":
                same_masks(got, fan.want, f"{fan.label}: the oracle")
    assert renderer.overflow_count() == before


# ---- E: trees and meshes no fan has run on ----

@pytest.mark.parametrize("name", Z.TREES)
def test_trees(renderer, general, name):  # noqa: F811
    fan = Z.tree_fan(name)
    upload(renderer, fan.d)
    got = against_both(renderer, fan)
    g = general(fan.d)
    for mode, masks in against_both(g, fan, f"{name} general").items():
        same_masks(masks, got[mode], f"{name} {mode}: general vs fast")


def test_tree_built_on_the_gpu_then_copied_and_loaded(renderer):
    import torch
    fan = Z.tree_fan("rand2k_built")
    renderer.build_scene({key: fan.d[key] for key in MESH_KEYS}, max_leaf=2, keys="extent")
    got = against_both(renderer, fan, "the GPU's own tree")
    n = renderer.scene_image_size()
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    renderer.pack_scene(buf.data_ptr(), n)
    c = rtamd.Renderer(0)
    try:
        c.load_scene(buf.data_ptr(), n)
        for mode, masks in against_both(c, fan, "after scene_image_load", exact_div=False).items():
            same_masks(masks, got[mode], f"after scene_image_load {mode}: the source context's")
        upload(c, Z.cull_edge().d)
        c.copy_scene_from(renderer)
        for mode, masks in against_both(c, fan, "after scene_copy", exact_div=False).items():
            same_masks(masks, got[mode], f"after scene_copy {mode}: the source context's")
    finally:
        c.close()


@pytest.mark.parametrize("label", Z.OUTSIDE)
def test_meshes_at_the_edges_of_mesh_space(renderer, label):
    fan = Z.mesh_fan(label)
    upload(renderer, fan.d)
    got = against_both(renderer, fan)
    assert rtamd.fan_bits(got["strict"], fan.k).sum() >= 64, label


# ---- F: table size and origin order ----

def test_table_sizes_on_one_fresh_context():
    import torch
    x = F.inputs("rand2k")
    n = 65
    rec = rtamd.pack_fan_origins(x["origins"][:n], x["normals"][:n], x["quarter"])
    fresh = rtamd.Renderer(0)
    try:
        upload(fresh, x["d"])
        for k in (1, rtamd.RT_FAN_MAX_DIRS, 33):            # the staged table grows, then shrinks
            dirs = F.fibonacci(k)
            got = fresh.trace_fan(rec, dirs)
            same_masks(got, query_masks(fresh, rec, dirs, 0), f"host form k={k}")
            assert got.any()
        k = rtamd.RT_FAN_MAX_DIRS
        dirs, w = F.fibonacci(k), k // 32
        want = query_masks(fresh, rec, dirs, 0)
        d_org = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
        d_dirs = torch.from_numpy(rtamd.pack_fan_dirs(dirs).reshape(-1).copy()).cuda()
        d_masks = torch.full((w * n + 64,), GUARD, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        fresh.trace_fan_device(d_org.data_ptr(), n, d_dirs.data_ptr(), k, d_masks.data_ptr())
        torch.cuda.synchronize()
        out = d_masks.cpu().numpy().view(np.uint32)
        assert w == 128 and np.all(out[w * n:] == GUARD), "the kernel wrote past masks[128 * 65]"
        same_masks(out[:w * n].reshape(w, n), want, f"device form k={k}")
    finally:
        fresh.close()


def test_origin_order(renderer):
    x = F.inputs("rand2k")
    upload(renderer, x["d"])
    n, k = 300, 100
    pick = np.arange(n) % x["origins"].shape[0]
    rec = rtamd.pack_fan_origins(x["origins"][pick], x["normals"][pick], x["quarter"])
    dirs = F.fibonacci(k)
    perm = np.random.default_rng(21).permutation(n)
    assert not np.array_equal(perm, np.arange(n))
    for mode, f in ARITHMETICS.items():
        got = renderer.trace_fan(rec, dirs, flags=f)
        assert got.any()
        same_masks(renderer.trace_fan(np.ascontiguousarray(rec[perm]), dirs, flags=f), np.ascontiguousarray(got[:, perm]), f"permuted origins, {mode}")
    same_masks(renderer.trace_fan(rec, dirs, flags=STRICT), F.yardstick_for(x["d"], rec, dirs), "in order vs the oracle")
