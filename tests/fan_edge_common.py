"""Shared by test_fan_edges.py (CPU) and test_fan_edges_gpu.py: the occlusion fans at the
edges of the cull rule, of ray space and of mesh space.

A Fan is a scene (arrays with a tree), packed rt_fan_origin records and a direction table, float32
(k, 3) or (k, 4); its yardstick, fan_common.yardstick_for with the traced flags, the oracle's hits and
its counters, is computed once (shared; do not modify).  Everything is seeded; no Fan has more than
704 origins, and but for the table-size case none has more than 96 directions.

 A  cull_edge        fan_common's edge records and edge directions on cornell12
 B  origin_groups    one run of 64 origins per value of ray_edge_common.ORIGIN_VALUES, rand2k
    one_lane         192 hit points of rand2k with one lane of every group at x = 2^-67 or 2^61
 C  edge_table       96 directions of five classes, interleaved; 192 hit points of rand2k
 D  tmax_sweep       per-lane tmax around the lane's own closest hit; rand2k
    comb_tmax        deep_comb40 with one tmax and with three by turns
 E  tree_fan         rand2k_built, rand3k_bigleaf, rand4k_sbvh by fan_common's recipe
    mesh_fan         single_tri_rootleaf, bigleaf and hit_attr_edge_common.MESH_LABELS from outside
 F  (rand2k's inputs as they are: built in the GPU test)"""
import numpy as np

import fan_common as F
import hit_attr_edge_common as X
import ray_edge_common as E
from ray_query_common import TMAX_DEFAULT, scene_arrays, scene_box

F32 = np.float32
ARITHMETICS = ["ref", "strict", "hw"]
N_ORIGINS = 192            # three groups of 64
LANES = (0, 31, 63)
LANE_VALUES = {"2^-67": E.p2(-67), "2^61": E.p2(61)}
TREES = ["rand2k_built", "rand3k_bigleaf", "rand4k_sbvh"]
OUTSIDE = ["single_tri_rootleaf", "bigleaf"] + X.MESH_LABELS
RESERVED = 0xFFFFFFFF
W_VALUES = [F32(np.nan), F32(np.inf), F32(-1e30), F32(1.0)]
# the runs of origin_groups by ORIGIN_VALUES' order: inside the quotient's domain, outside it; small, large
RUNS_INSIDE, RUNS_OUTSIDE = [0, 1, 4, 5, 7], [2, 3, 6, 8, 9, 10]
RUNS_SMALL, RUNS_LARGE = [0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 10]

_CACHE = {}


class Fan:
    def __init__(self, label, d, rec, dirs):
        import rtamd
        assert rec.dtype == rtamd.FAN_ORIGIN_DTYPE and rec.shape[0] <= 704
        self.label, self.d, self.rec, self.dirs = label, d, rec, np.ascontiguousarray(dirs, F32)
        self.n, self.k = rec.shape[0], self.dirs.shape[0]
        self._yard = None

    def yard(self):
        """(masks, traced (n, k), hit (n, k), the oracle's counters), computed once."""
        if self._yard is None:
            self._yard = F.yardstick_for(self.d, self.rec, self.dirs, want_stats=True)
        return self._yard

    @property
    def want(self):
        return self.yard()[0]


def _once(key, make):
    if key not in _CACHE:
        with np.errstate(all="ignore"):
            _CACHE[key] = make()
    return _CACHE[key]


def rand2k_records(n=N_ORIGINS, cull=False, tmax="quarter"):
    """The first n of fan_common.inputs("rand2k")'s origins as records."""
    import rtamd
    x = F.inputs("rand2k")
    return rtamd.pack_fan_origins(x["origins"][:n], x["normals"][:n] if cull else None, x["quarter"] if tmax == "quarter" else tmax)


# ---- A: the cull rule's edge set ----

def cull_edge_dirs():
    """fan_common.edge_dirs with (1e-20, 1e-20, 1e-20) replaced by 2^-85 (1, 2, 3): the squared length
    stays 2^8 clear of FLT_MIN, the margin ray_edge_common.normalize_branch asks for."""
    dirs = F.edge_dirs().copy()
    at = np.flatnonzero(np.all(dirs == F32(1e-20), axis=1))
    assert at.size == 1
    dirs[at[0]] = E.p2(-85) * np.array([1, 2, 3], F32)
    return dirs


def cull_edge():
    return _once("cull_edge", lambda: Fan("cull_edge", scene_arrays("cornell12"), F.edge_records(), cull_edge_dirs()))


def with_reserved_and_w(fan):
    """The same fan with every record's reserved word 0xFFFFFFFF and the table's w column NaN, +inf,
    -1e30 and 1 by turns: both are ignored, so the words are the first fan's."""
    rec = fan.rec.copy()
    rec["reserved"] = np.uint32(RESERVED)
    dirs = np.zeros((fan.k, 4), F32)
    dirs[:, :3] = fan.dirs[:, :3]
    dirs[:, 3] = np.array(W_VALUES, F32)[np.arange(fan.k) % len(W_VALUES)]
    return rec, dirs


def _normal_rows(rec, normal):
    return np.all(rec["n"].view(np.uint32) == np.array(normal, F32).view(np.uint32)[None, :], axis=1)


def _dir_col(dirs, direction):
    return int(np.flatnonzero(np.all(dirs[:, :3] == np.array(direction, F32)[None, :], axis=1))[0])


def cull_consequences(fan):
    """The consequences tests/test_fan.py spells out for rt_fan_expand, as rays of the cull-edge fan: a
    list of (name, origin rows, direction columns, traced).  Every record has the same origin, so what a
    ray would hit if traced is what the zero-normal record with the same tmax hits: `plain` below."""
    rec, dirs = fan.rec, fan.dirs
    tm = rec["tmax"]
    valid_o = np.all(np.isfinite(rec["o"]), axis=1)
    good = valid_o & (tm > F32(0.001)) & (tm != np.nextafter(F32(0.001), F32(1)))   # +inf and the default
    valid_d = np.flatnonzero(np.all(np.isfinite(dirs), axis=1) & np.any(dirs != 0, axis=1))
    nonfinite = ~np.all(np.isfinite(rec["n"]), axis=1)
    j_big, j_x = _dir_col(dirs, (1e30, 1e30, 1e30)), _dir_col(dirs, (1, 0, 0))
    above = tm == np.nextafter(F32(0.001), F32(1))
    zero = _normal_rows(rec, (0, 0, 0))
    return [
        ("-0 normals do not cull", np.flatnonzero(good & (_normal_rows(rec, (-0.0, -0.0, -0.0)) | _normal_rows(rec, (0.0, -0.0, 0.0)))), valid_d, True),
        ("a NaN or inf normal voids the origin", np.flatnonzero(good & nonfinite), valid_d, False),
        ("(1e30, -1e30, 0) . (1e30, 1e30, 1e30) is traced", np.flatnonzero(good & _normal_rows(rec, (1e30, -1e30, 0))), np.array([j_big]), True),
        ("(1e-45, 0, 0) . (1, 0, 0) is traced", np.flatnonzero(good & _normal_rows(rec, (1e-45, 0, 0))), np.array([j_x]), True),
        ("tmax = 0.001 is not traced", np.flatnonzero(valid_o & zero & (tm == F32(0.001))), valid_d, False),
        ("the float above 0.001 is traced", np.flatnonzero(valid_o & zero & above), valid_d, True),
    ]


def plain_hits(fan):
    """bool (k,): direction j hits cornell12 from the edge set's one origin within the default tmax, by the
    oracle: the zero-normal, default-tmax record's row of the yardstick."""
    row = np.flatnonzero(_normal_rows(fan.rec, (0, 0, 0)) & (fan.rec["tmax"] == TMAX_DEFAULT) & np.all(np.isfinite(fan.rec["o"]), axis=1))
    return fan.yard()[2][row[0]]


# ---- B: origins at the edges of the quotient's domain ----

def origin_groups():
    """One run of 64 origins per value of ORIGIN_VALUES on axis lane % 3, the other two coordinates
    uniform in rand2k's box shrunk to 80 %; no culling, a quarter of the diagonal, Fibonacci 64."""
    def make():
        import rtamd
        d = scene_arrays("rand2k")
        lo, hi = scene_box(d)
        mid, half = 0.5 * (lo.astype(np.float64) + hi), 0.4 * (hi.astype(np.float64) - lo)
        rng = np.random.default_rng(2101)
        o = []
        for val in E.ORIGIN_VALUES:
            k = np.arange(E.GROUP)
            oo = rng.uniform(mid - half, mid + half, (E.GROUP, 3)).astype(F32)
            oo[k, k % 3] = val
            o.append(oo)
        return Fan("origin_groups", d, rtamd.pack_fan_origins(np.concatenate(o), None, F.quarter_diagonal(d)), F.fibonacci())
    return _once("origin_groups", make)


def one_lane(lane, value):
    """(the whole fan, the fan with lane `lane` of every group moved to x = LANE_VALUES[value], the
    replaced rows)."""
    def make():
        d = scene_arrays("rand2k")
        whole = _once("one_lane_whole", lambda: Fan("one_lane/whole", d, rand2k_records(), F.fibonacci()))
        at = np.arange(lane, N_ORIGINS, 64)
        rec = whole.rec.copy()
        rec["o"][at, 0] = LANE_VALUES[value]
        return whole, Fan(f"one_lane/{lane}/{value}", d, rec, F.fibonacci()), at
    return _once(("one_lane", lane, value), make)


def domain_table(dirs, arithmetic):
    """bool (k,): E.axis_ok of the normalised table on every axis, for an origin inside the domain."""
    return np.all(E.axis_ok(np.ones((1, 3), F32), E.normalised(dirs), arithmetic), axis=1)


def rays_in_domain(fan, arithmetic):
    """bool (n, k): E.in_domain of every ray of a fan."""
    dn = E.normalised(fan.dirs)
    return np.all(E.axis_ok(fan.rec["o"][:, None, :], dn[None, :, :], arithmetic), axis=2)


# ---- C: a direction table at the edges of direction space ----

def _zero(j):
    return F32(-0.0) if j % 2 else F32(0.0)


def direction_classes():
    """The five classes of the 96-direction table, name -> float32 (m, 3); 20 + 18 + 24 + 28 + 6."""
    sign = lambda j, bit: -1.0 if (j >> bit) & 1 else 1.0
    octants = [(sign(j, 0) * m[0], sign(j, 1) * m[1], sign(j, 2) * m[2])
               for m, count in (((1, 2, 3), 8), ((3, 1, 2), 8), ((2, 3, 1), 4)) for j in range(count)]
    axis1 = []
    for j in range(18):   # axis, sign and magnitude by turns; the zeros of either sign
        v = [_zero(j), _zero(j // 2), _zero(j // 4)]
        v[j % 3] = (1.0 if (j // 3) % 2 == 0 else -1.0) * (1.0, 2.5, 0.375)[(j // 6) % 3]
        axis1.append(tuple(v))
    axis2 = []
    for j in range(24):   # the zero's axis and sign, the other two components' signs
        v = [sign(j, 2) * (1.0 + 0.25 * (j % 5)), sign(j, 3) * (0.5 + 0.125 * (j % 7)), sign(j, 4) * 2.0]
        v[j % 3] = _zero(j // 3)
        axis2.append(tuple(v))
    near = []
    for variant in range(4):   # per magnitude two with both small components and two with one of them zero
        for q, m in enumerate(E.NEAR_AXIS_MAGNITUDES):
            j = variant * 7 + q
            axis = j % 3
            v = [sign(j, 0) * m, sign(j, 1) * m, sign(j, 2) * m]
            if variant % 2:
                v[(axis + 1 + (j // 3) % 2) % 3] = _zero(j)
            v[axis] = sign(j, 3)
            near.append(tuple(v))
    scaled = [tuple(E.p2(e) * F32(c) for c in v) for e in (-85, 100) for v in ((1, 2, 3), (-3, 4, -0.5), (0, -1, 0))]
    return {"octant": np.array(octants, F32), "axis1": np.array(axis1, F32), "axis2": np.array(axis2, F32),
            "near_axis": np.array(near, F32), "scaled": np.array(scaled, F32)}


def edge_table():
    """(directions float32 (96, 3), class name per direction): the classes interleaved by their
    fractional position, so that each class is spread over the whole table."""
    def make():
        cls = direction_classes()
        rows = sorted(((i + 0.5) / v.shape[0], c, i) for c, (name, v) in enumerate(cls.items()) for i in range(v.shape[0]))
        names = list(cls)
        return np.stack([cls[names[c]][i] for _, c, i in rows]), [names[c] for _, c, _ in rows]
    return _once("edge_table", make)


def table_fan(cull):
    def make():
        return Fan(f"edge_table/{'cull' if cull else 'nocull'}", scene_arrays("rand2k"), rand2k_records(cull=cull), edge_table()[0])
    return _once(("table_fan", cull), make)


# ---- D: tmax per lane ----

def tmax_sweep():
    """(fan, j* per origin, turn per origin, the closest hit's (ids, t) of ray (i, j*)): rand2k's 192
    origins, no culling, Fibonacci 64; tmax_i by hit_attr_edge_common.sweep_tmax around t* of ray
    (i, j* = i % 64); an origin whose ray misses keeps the default."""
    def make():
        import rtamd
        from oracle import oracle
        x = F.inputs("rand2k")
        o, dirs = x["origins"][:N_ORIGINS], x["dirs"]
        jstar = np.arange(N_ORIGINS) % 64
        ids, t, _ = oracle.trace_rays(x["d"], rtamd.pack_rays(o, dirs[jstar]))
        tm, turn = X.sweep_tmax(ids, t, np.full(N_ORIGINS, TMAX_DEFAULT, F32))
        return Fan("tmax_sweep", x["d"], rtamd.pack_fan_origins(o, None, tm), dirs), jstar, turn, (ids, t)
    return _once("tmax_sweep", make)


def comb_tmax(setting):
    """deep_comb40 with test_fan_gpu.py's 128 origins and 48 directions; tmax a quarter of the diagonal
    ("quarter"), the default ("default") or by turns default, half and quarter of it ("turns")."""
    def make():
        import rtamd
        d = E.edge_scene("deep_comb40")
        o, dirs, _ = E.ray_class("deep_comb40", "incoherent")
        q = F.quarter_diagonal(d)
        tm = {"quarter": q, "default": None,
              "turns": np.array([TMAX_DEFAULT, F32(2) * q, q], F32)[np.arange(128) % 3]}[setting]
        return Fan(f"deep_comb40/{setting}", d, rtamd.pack_fan_origins(o[:128], None, tm), np.ascontiguousarray(dirs[:48]))
    return _once(("comb_tmax", setting), make)


# ---- E: trees and meshes no fan has run on ----

def tree_fan(name):
    """fan_common's recipe on one of TREES: the hit points of 512 incoherent rays, their normals,
    Fibonacci 64, a quarter of the diagonal."""
    def make():
        x = F.inputs(name)
        return Fan(name, x["d"], F.records(name, "quarter"), x["dirs"])
    return _once(("tree_fan", name), make)


def mesh_fan(label):
    """One of OUTSIDE seen from outside: the first 256 origins (64 for tiny_tris) of the input's own rays
    (hit_attr_edge_common's for a mesh label, the scene's incoherent rays otherwise), each with its ray's
    raw direction as the normal; the table is the first 64 of those directions; tmax = +inf."""
    def make():
        import rtamd
        if label in X.MESH_LABELS:
            inp = X.get(label)
            d, o, dirs = inp.d, inp.rays["o"], inp.rays["d"]
        else:
            d = E.edge_scene(label)
            o, dirs, _ = E.ray_class(label, "incoherent")
        n = 64 if label == "tiny_tris" else 256
        o, dirs = np.ascontiguousarray(o[:n], F32), np.ascontiguousarray(dirs[:n], F32)
        return Fan(label, d, rtamd.pack_fan_origins(o, dirs, F32(np.inf)), dirs[:64].copy())
    return _once(("mesh_fan", label), make)
