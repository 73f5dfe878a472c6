"""The attribute ray query on the GPU at the edges of normal, ray and mesh space ("Tests
at the edges"): the inputs of tests/hit_attr_edge_common.py through query_attr_kernel, hit_attr,
ray_tri_uv, the read of the shading record and the LDS-staged stores.  tests/test_hit_attr_edges.py
shows on the CPU that the inputs reach their edges and pins the yardstick there.

Records are sixteen uint32 words, compared by hit_attr_edge_common.assert_same_records_nan: words,
except that where the yardstick's float word is a NaN the GPU's must be a NaN (x86 and gfx950 generate
different default NaNs); how many words took that exception is asserted per input (EXCUSED), and it is
zero for every input that is not NaN-making.  S_strict is exact against the yardstick on all three
code paths; S_ref and S_hw have no oracle: their id and t are rt_trace_rays' own, their three paths
agree word for word, and their float fields are held against S_strict's and against float64 by
gross-error bounds, 8 x the largest figure of the first GPU run (DESIGN.md 19 has the tables)."""
import ctypes as C

import numpy as np
import pytest

import rtamd
import hit_attr_edge_common as X
from hit_attr_common import FLOAT_FIELDS, ID, T, TMAX_WORD, U, V, miss_words, ray_words, ref_hit_attr, ref_next_rays
from refit_common import np_refit, scene_image, with_vertices
from test_hit_attr_gpu import MESH_KEYS, attr, plain
from test_ray_query_edges_gpu import HDR_FAST_DIV, general  # noqa: F401  (the split-records context, a module fixture)

pytestmark = pytest.mark.gpu

STRICT, HW, EXACT_DIV = rtamd.RT_FLAG_STRICT_MATH, rtamd.RT_FLAG_HW_MATH, rtamd.RT_FLAG_EXACT_DIV
GUARD = 0x5A5A5A5A
bits = X.bits

# Words that took the NaN exception, S_strict against the yardstick, (closest, any hit), the same on all
# three paths.  Measured on the first GPU run: none anywhere.  Of 6,303 / 6,846 (normals/nan_component,
# det/floor_y0), 690 / 852 (det/slant_through_origin), 2,964 / 2,973 (signed_zeros_grid16), 177 / 177
# (rand512*2^38) and 30 / 30 (rand512*2^40) NaN words every one has the yardstick's bits.  The NaNs of
# these inputs are an input's own NaN, which both sides pass on, or come from the quotient 0 / 0 in
# normal_at, for which the division's last step on gfx950 returns 0xFFC00000 as x86 does; the rule
# stays for the default NaN of an addition or a multiplication, 0x7FC00000 there and 0xFFC00000 here.
EXCUSED = {label: (0, 0) for label in X.NAN_MAKING if X.NAN_MAKING[label][0] == "nan"}
# ImageHeader::fast_div of the scaled meshes: which form of the slab test the fast kernel ran
FAST_DIV = {f"rand512*2^{k}": 1 for k in X.SCALES}

# test_ref_and_hw_against_strict: per group and field the largest difference of S_ref's and S_hw's
# records from S_strict's on the first GPU run (t and p relative to |o| + t, the others absolute);
# the bounds are 8 x these.  A gross-error check, not a precision claim.
DEVIATION_MEASURED = {
    "normal": {"t": 1.5433237390034455e-07, "u": 6.556510925292969e-07, "v": 5.513429641723633e-07, "p": 1.297025925580376e-07,
               "ndotd": 1.7881393432617188e-07, "ng": 1.1920928955078125e-07, "ns": 1.7481794357299805, "ns_conditioned": 1.8259510397911072e-05},
    "ray": {"t": 3.685412727529574e-07, "u": 5.5283308029174805e-05, "v": 6.209313869476318e-05, "p": 3.685412727529574e-07,
            "ndotd": 2.384185791015625e-07, "ng": 1.1920928955078125e-07, "ns": 2.0, "ns_conditioned": 1.1175870895385742e-05},
    "mesh": {"t": 4.802079956695851e-07, "u": 2.0489096641540527e-06, "v": 3.6209821701049805e-06, "p": 3.429135259520391e-07,
             "ndotd": 2.980232238769531e-07, "ng": 1.1920928955078125e-07, "ns": 1.55308598279953, "ns_conditioned": 0.00024750828742980957},
}
# test_ref_and_hw_against_float64: hit_attr_edge_common.float64_errors of S_ref's and S_hw's own records,
# the first GPU run's largest per group; the bounds are 8 x these.
FLOAT64_MEASURED = {
    "normal": {"bary": 1.4074561804979138e-07, "p": 5.346723197373739e-08, "ng": 8.434057374717696e-08, "ndotd": 1.4813722204465307e-07,
               "unit": 9.536743050819751e-08},
    "ray": {"bary": 6.313266144276297e-07, "p": 7.757745865840056e-08, "ng": 3.665029975064016e-07, "ndotd": 1.5829191524208142e-07,
            "unit": 1.0615533729829707e-07},
    "mesh": {"bary": 1.8744715409737202e-06, "p": 5.373196142913997e-08, "ng": 3.3475083455747345e-06, "ndotd": 1.2599363445886524e-06,
             "unit": 1.0402646033469409e-07},
}
# S_strict float words that are NaN where S_ref's or S_hw's is a number, per input, closest and any hit
# together: (S_ref, S_hw).  rand512*2^38 stands at the overflow threshold of normal_at: S_ref contracts
# each a*b - c*d and the sums of three into fused multiply-adds, so a product that rounds to infinity
# on its own in S_strict and S_hw (and makes inf - inf) never exists as a float there.
NAN_EXCEPTIONS = {"rand512*2^38": (72, 0)}
FIELDS = list(FLOAT_FIELDS) + ["ns_conditioned"]   # ns over hit_attr_edge_common.ns_well_conditioned's rays alone
LEFT_OUT_CAP = 0.01
INTERIOR = np.float32(2.0 ** -10)


def put(r, case):
    """The case's scene in the renderer (rand2k_built through build_scene on the GPU): its inputs."""
    inputs = X.inputs_of(case)
    d = inputs[0].d
    if case == "rand2k_built":
        r.build_scene({k: d[k] for k in MESH_KEYS}, max_leaf=2, keys="extent")
    else:
        r.upload(rtamd.Scene.from_arrays(d))
    return inputs


def three_paths(renderer, g):
    return [("fast", renderer, 0), ("EXACT_DIV", renderer, EXACT_DIV), ("general", g, 0)]


# ---- 1: S_strict against the yardstick ----

@pytest.mark.parametrize("case", X.CASES)
def test_strict_equals_the_yardstick(renderer, general, case):  # noqa: F811
    """Every input, closest and any hit (the any-hit id is the oracle's), on the fast kernel, with
    RT_FLAG_EXACT_DIV and on the general kernel of the split-records context."""
    inputs = put(renderer, case)
    g = general(inputs[0].d)
    if case in FAST_DIV:
        assert scene_image(renderer)[HDR_FAST_DIV] == FAST_DIV[case], "which slab test ran"
    for inp in inputs:
        for k, any_hit in enumerate((False, True)):
            want = inp.want(any_hit)[0]
            miss = want[:, ID].view(np.int32) < 0
            for path, r, extra in three_paths(renderer, g):
                what = f"{inp.label} any={any_hit} {path}"
                got = attr(r, inp.rays, STRICT | extra, any_hit)
                excused = X.assert_same_records_nan(got, want, what)
                assert np.array_equal(got[miss], miss_words(inp.rays)[miss]), what + ": a miss is -1, the tmax word, 14 zeros"
                if inp.label in EXCUSED:
                    print(f"{what}: {excused} of {int(X.nan_words(want).sum())} NaN words took the exception")
                    assert EXCUSED[inp.label] is None or excused == EXCUSED[inp.label][k], what
                else:
                    assert excused == 0, what


# ---- 2: id and t are rt_trace_rays' own ----

@pytest.mark.parametrize("case", X.CASES)
def test_id_and_t_are_the_plain_querys(renderer, case):
    for inp in put(renderer, case):
        for flags in (0, HW, STRICT):
            for extra in (0, EXACT_DIV):
                for any_hit in (False, True):
                    a = attr(renderer, inp.rays, flags | extra, any_hit)
                    ids, t = plain(renderer, inp.rays, flags | extra, any_hit)
                    what = f"{inp.label} flags={flags | extra} any={any_hit}"
                    assert np.array_equal(a[:, ID].view(np.int32), ids), what + ": ids"
                    assert np.array_equal(a[:, T], bits(t)), what + ": t"
                    assert not a[:, 11].any() and not a[:, 15].any(), what + ": the reserved words are 0"
                    assert np.array_equal(a[ids < 0], miss_words(inp.rays)[ids < 0]), what + ": the miss record"


# ---- 3: S_ref and S_hw, the three paths agree ----

@pytest.mark.parametrize("case", X.CASES)
def test_ref_and_hw_paths_agree(renderer, general, case):  # noqa: F811
    """Plain word equality, NaN bits included: the same arithmetic on one GPU."""
    inputs = put(renderer, case)
    g = general(inputs[0].d)
    for inp in inputs:
        for flags in (0, HW):
            for any_hit in (False, True):
                got = [(path, attr(r, inp.rays, flags | extra, any_hit)) for path, r, extra in three_paths(renderer, g)]
                for path, rec in got[1:]:
                    bad = np.flatnonzero(np.any(rec != got[0][1], axis=1))
                    assert bad.size == 0, f"{inp.label} flags={flags} any={any_hit}: {path} vs fast, {bad.size} records differ, first {bad[:5]}"


# ---- 4 and 5: S_ref and S_hw against S_strict and against float64 ----

def field_deviation(inp, s, a):
    """Per float field the largest difference of records `a` from S_strict's `s` over the rays whose ids
    agree and whose S_strict record holds no NaN (t and p relative to |o| + t), the number of rays
    with interior S_strict barycentrics, how many of those are left out for a differing id, and the
    number of S_strict NaN words that are numbers in `a`."""
    sid, aid = s[:, ID].view(np.int32), a[:, ID].view(np.int32)
    nan_s = X.nan_words(s)
    both = (sid >= 0) & (aid == sid) & ~nan_s.any(axis=1)
    f = lambda rec, cols: rec[both][:, cols].view(np.float32).astype(np.float64)
    worst = {k: 0.0 for k in FIELDS}
    cond = both & X.ns_well_conditioned(inp.d, inp.rays, s)
    if np.any(cond):
        ns = FLOAT_FIELDS["ns"]
        worst["ns_conditioned"] = float(np.abs(a[cond][:, ns].view(np.float32).astype(np.float64)
                                               - s[cond][:, ns].view(np.float32).astype(np.float64)).max())
    if np.any(both):
        r = ray_words(inp.rays)[both].astype(np.float64)
        scale = np.linalg.norm(r[:, 0:3], axis=1) + f(s, [T])[:, 0]
        for k, cols in FLOAT_FIELDS.items():
            diff = np.abs(f(a, cols) - f(s, cols)).max(axis=1)
            worst[k] = float(np.max(diff / scale if k in ("t", "p") else diff))
    with np.errstate(invalid="ignore"):
        u, v = s[:, U].view(np.float32), s[:, V].view(np.float32)
        interior = (sid >= 0) & (u >= INTERIOR) & (v >= INTERIOR) & (np.float32(1) - u - v >= INTERIOR)
    same = (sid >= 0) & (aid == sid)
    numbers = int(np.sum(nan_s[same] & ~X.nan_words(a)[same]))
    return worst, int(interior.sum()), int(np.sum(interior & (aid != sid))), numbers, int(cond.sum())


def measure_group(renderer, group):
    """S_ref's and S_hw's fast-path records of every input of a group, closest and any hit, against
    S_strict's and against float64: (deviation per field, float64 errors, rays with interior barycentrics
    and those of them left out per arithmetic, S_strict NaN words that are numbers per input)."""
    deviation = {k: 0.0 for k in FIELDS}
    f64 = dict(bary=0.0, p=0.0, ng=0.0, ndotd=0.0, unit=0.0)
    interior, left_out, numbers, conditioned = {0: 0, HW: 0}, {0: 0, HW: 0}, {}, 0
    for case in X.cases_of(group):
        for inp in put(renderer, case):
            for any_hit in (False, True):
                s = attr(renderer, inp.rays, STRICT, any_hit)
                for flags in (0, HW):
                    a = attr(renderer, inp.rays, flags, any_hit)
                    worst, n_in, n_out, n_num, n_cond = field_deviation(inp, s, a)
                    conditioned += n_cond
                    if worst["ns"] > 1e-3:
                        print(f"{inp.label} flags={flags} any={any_hit}: ns differs from S_strict's by {worst['ns']:.3g}, "
                              f"by {worst['ns_conditioned']:.3g} on its {n_cond} well-conditioned rays")
                    for k, v in worst.items():
                        assert np.isfinite(v), f"{inp.label} flags={flags}: {k}"
                        deviation[k] = max(deviation[k], v)
                    interior[flags] += n_in
                    left_out[flags] += n_out
                    if n_out:
                        print(f"{inp.label} flags={flags} any={any_hit}: {n_out} of {n_in} interior rays have another id than S_strict's")
                    if inp.nan_making or n_num:
                        numbers.setdefault(inp.label, {0: 0, HW: 0})[flags] += n_num
                    e = X.float64_errors(inp.d, inp.rays, a)
                    for k in f64:
                        f64[k] = max(f64[k], e[k])
    return deviation, f64, interior, left_out, numbers, conditioned


_MEASURED = {}


def measured(renderer, group):
    if group not in _MEASURED:
        _MEASURED[group] = measure_group(renderer, group)
    return _MEASURED[group]


@pytest.mark.parametrize("group", X.GROUPS)
def test_ref_and_hw_against_strict(renderer, group):
    deviation, _, interior, left_out, numbers, conditioned = measured(renderer, group)
    print(group, "largest |S_ref or S_hw - S_strict| per field:", deviation, "rays with a well-conditioned ns:", conditioned)
    assert conditioned >= 2000, "too few rays for the bound on ns_conditioned to mean anything"
    print(group, "interior rays:", interior, "left out for another id:", left_out, "S_strict NaN words that are numbers:", numbers)
    for flags in (0, HW):
        assert interior[flags] >= 1000
        assert left_out[flags] <= LEFT_OUT_CAP * interior[flags], f"{group} flags={flags}: {left_out[flags]} of {interior[flags]} interior rays left out"
    for label, n in numbers.items():
        assert (n[0], n[HW]) == NAN_EXCEPTIONS.get(label, (0, 0)), f"{label}: S_strict NaN words that are numbers in (S_ref, S_hw): {n}"
    for k, v in deviation.items():
        assert DEVIATION_MEASURED[group][k] is not None, f"no bound yet for {k}"
        bound = 8.0 * DEVIATION_MEASURED[group][k]
        assert v <= bound, f"{group}: {k} differs from S_strict's by {v} > {bound}"


@pytest.mark.parametrize("group", X.GROUPS)
def test_ref_and_hw_against_float64(renderer, group):
    f64 = measured(renderer, group)[1]
    print(group, "float64 errors of S_ref's and S_hw's own records:", f64)
    for k, v in f64.items():
        bound = 8.0 * FLOAT64_MEASURED[group][k]
        assert v <= bound, f"{group}: {k} is {v} > {bound} off float64"


# ---- 6: the frame continued from the GPU's records ----

@pytest.mark.parametrize("label", X.FRAME_LABELS)
def test_records_continue_the_gpu_frame(renderer, label):
    """Attributes from the GPU, ref_next_rays, rt_trace_rays: the bounce-1 ids and t and the bounce-0
    shadow ids of render(depth=2, STRICT, aux).  A pixel whose reflected ray is NaN (a NaN ns) shows in
    the aux planes as traced and missed, id -1 and t = 2^32: the very words a query gives that invalid
    ray, so the comparison needs no exception; its shadow ray starts from p and is an ordinary ray."""
    inp = put(renderer, label)[0]
    renderer.set_params(inp.params)
    g = renderer.render(X.W, X.H, depth=2, flags=STRICT, aux=True)
    ref = X.oracle_frame(label)
    assert np.array_equal(g["hits"], ref["hits"]) and np.array_equal(bits(g["t"]), bits(ref["t"])), "the frame is the oracle's"
    a = attr(renderer, inp.rays)
    traced, hit = g["hits"][:, 0, 0] != -2, g["hits"][:, 0, 0] >= 0
    assert np.array_equal(a[traced, ID].view(np.int32), g["hits"][traced, 0, 0]) and np.array_equal(a[hit, T], bits(g["t"][hit, 0]))
    only = a.copy()
    only[~hit] = miss_words(inp.rays)[~hit]
    refl, shadow = ref_next_rays(inp.rays, only, inp.params[16:19])
    nan_ray = np.isnan(refl).any(axis=1)
    assert not np.any(g["hits"][hit, 1, 0] == -2), "every pixel that hit traced its reflected ray"
    assert np.all(g["hits"][nan_ray, 1, 0] == -1) and np.all(bits(g["t"][nan_ray, 1]) == TMAX_WORD)
    if inp.nan_making:
        assert int(nan_ray.sum()) >= 64 and int(nan_ray.sum()) == X.ns_counts(inp.want()[0])[1]
    else:
        assert not nan_ray.any()
    ids1, t1 = plain(renderer, refl)
    assert np.array_equal(ids1[hit], g["hits"][hit, 1, 0]), f"{label}: bounce-1 ids"
    assert np.array_equal(bits(t1[hit]), bits(g["t"][hit, 1])), f"{label}: bounce-1 t"
    sid, _ = plain(renderer, shadow, any_hit=True)
    assert np.array_equal(sid[hit], g["hits"][hit, 0, 1]), f"{label}: bounce-0 shadow ids"


# ---- 7: group tails and staging with edge records ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_group_tails_with_nan_records(renderer, n):
    import torch
    inp = put(renderer, "normals/nan_component")[0]
    full = inp.want()[0]
    start = int(np.flatnonzero(X.nan_words(full).any(axis=1))[0])   # the first record is a NaN one
    rays = np.ascontiguousarray(inp.rays[start:start + n + 3])      # more rays in memory than asked for
    want = full[start:start + n]
    assert X.nan_words(want).any(axis=1).sum() >= max(1, n // 4), "NaN records among those staged"
    hits = np.full((n + 2, 16), GUARD, np.uint32)                   # two guard records after hits[n]
    rc = rtamd.lib().rt_trace_rays_attr(renderer._h, rays.ctypes.data_as(C.c_void_p), n, STRICT, hits.ctypes.data_as(C.c_void_p))
    assert rc == 0
    assert np.all(hits[n:] == GUARD), "the host form wrote past hits[n]"
    X.assert_same_records_nan(hits[:n], want, f"host form n={n}")
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_hits = torch.full(((n + 2) * 16,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    renderer.trace_rays_attr_device(d_rays.data_ptr(), n, d_hits.data_ptr(), flags=STRICT)
    torch.cuda.synchronize()
    got = d_hits.cpu().numpy().view(np.uint32).reshape(n + 2, 16)
    assert np.all(got[n:] == GUARD), "the kernel wrote past hits[n]"
    X.assert_same_records_nan(got[:n], want, f"device form n={n}")
    assert np.array_equal(got[:n], hits[:n]), "host and device form agree in NaN bits too"


def test_every_class_in_one_buffer(renderer):
    """All ray classes of rand2k in one buffer, in order and under a fixed permutation: each record is
    what it is alone (the yardstick's, and in S_ref and S_hw the class's own launch's)."""
    inputs = [inp for inp in put(renderer, "rand2k") if not inp.label.endswith("/tmax")]
    assert len(inputs) == 14
    rays = np.concatenate([inp.rays for inp in inputs])
    perm = np.random.default_rng(19).permutation(rays.shape[0])
    shuffled = np.ascontiguousarray(rays[perm])
    for any_hit in (False, True):
        want = np.concatenate([inp.want(any_hit)[0] for inp in inputs])
        assert X.assert_same_records_nan(attr(renderer, rays, STRICT, any_hit), want, f"in order any={any_hit}") == 0
        assert X.assert_same_records_nan(attr(renderer, shuffled, STRICT, any_hit), want[perm], f"permuted any={any_hit}") == 0
        for flags in (0, HW):
            alone = np.concatenate([attr(renderer, inp.rays, flags, any_hit) for inp in inputs])
            assert np.array_equal(attr(renderer, rays, flags, any_hit), alone), f"flags={flags} any={any_hit}: in order"
            assert np.array_equal(attr(renderer, shuffled, flags, any_hit), alone[perm]), f"flags={flags} any={any_hit}: permuted"


# ---- 8: edge normals and vertices through rt_update_vertices ----

def test_edge_normals_through_update_vertices(renderer):
    """The open stage with its tame normals, updated to normals/nan_component's, to normals/length_1e-25's
    and back: after each update the records are the yardstick's on those arrays, after the last the first."""
    tame = put(renderer, "det/base")[0]
    first = attr(renderer, tame.rays)
    assert X.assert_same_records_nan(first, tame.want()[0], "tame") == 0
    verts = tame.d["vertices"]
    for label in ("normals/nan_component", "normals/length_1e-25", "det/base"):
        inp = X.get(label)
        assert np.array_equal(inp.d["vertices"], verts) and np.array_equal(inp.rays, tame.rays)
        assert label == "det/base" or not np.array_equal(bits(inp.d["normals"]), bits(tame.d["normals"]))
        renderer.update_vertices(verts, inp.d["normals"])
        for any_hit in (False, True):
            X.assert_same_records_nan(attr(renderer, inp.rays, STRICT, any_hit), inp.want(any_hit)[0], f"updated to {label} any={any_hit}")
    assert np.array_equal(attr(renderer, tame.rays), first), "back to the tame normals: the first records"


def test_edge_vertices_through_update_vertices(renderer):
    """det/base's scene updated to det/floor_1e-6's vertices (the whole stage 4 + 1e-6 higher: the floor's
    Cramer determinant is small) and back, against the yardstick on the CPU-refit nodes."""
    from oracle import oracle
    base = put(renderer, "det/base")[0]
    first = attr(renderer, base.rays)
    edge = X.get("det/floor_1e-6")
    verts = edge.d["vertices"]
    assert verts.shape == base.d["vertices"].shape and not np.array_equal(verts, base.d["vertices"])
    assert all(np.array_equal(edge.d[k], base.d[k]) for k in ("indices", "normals", "normals_indices"))
    renderer.update_vertices(verts)
    e = with_vertices(base.d, verts, np_refit(base.d, verts)[0])
    for any_hit in (False, True):
        ids, t, _ = oracle.trace_rays(e, edge.rays, any_hit=any_hit)
        assert int((ids >= 0).sum()) >= 2000
        want = ref_hit_attr(e, edge.rays, ids, t)
        assert X.assert_same_records_nan(attr(renderer, edge.rays, STRICT, any_hit), want, f"floor_1e-6's vertices any={any_hit}") == 0
        if not any_hit:
            assert np.array_equal(want, edge.want()[0]), "the refit tree reports the hits of the case's own tree"
    renderer.update_vertices(base.d["vertices"])
    assert np.array_equal(attr(renderer, base.rays), first), "back to the base vertices: the first records"
