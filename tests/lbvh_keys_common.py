"""Shared by test_lbvh_keys.py (CPU) and test_lbvh_keys_gpu.py: a numpy restatement of the
extent-aware keys (plan, cell, key), lbvh_common's restatement and validity checker
run over those keys, the degenerate meshes, and the SAH cost of a node array by rt_scene_sah's
definition."""
import contextlib

import numpy as np

import lbvh_common
from conftest import load_golden
from lbvh_common import F, INDEX_BITS, _w1

EXTENT = 0x100             # RT_BUILD_EXTENT_KEYS
MORTON_BITS, AXIS_BITS_MAX = 39, 20


def np_c2(verts, idx):
    """c2 = lo + hi of every triangle, and its bounds (fminf / fmaxf: a NaN operand is ignored)."""
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    p = np.asarray(verts, F)[tri][:, :, :3]
    lo, hi = np.fmin(np.fmin(p[:, 0], p[:, 1]), p[:, 2]), np.fmax(np.fmax(p[:, 0], p[:, 1]), p[:, 2])
    with np.errstate(all="ignore"):
        c2 = (lo + hi).astype(F)
    return c2, np.fmin.reduce(c2, 0), np.fmax.reduce(c2, 0)


def np_plan(cmin, cmax):
    """(plan[39] axis numbers, bits[3]): every bit goes to the axis whose cells are the widest."""
    with np.errstate(all="ignore"):
        w = (np.asarray(cmax, F) - np.asarray(cmin, F)).astype(F)
    w = [x if np.isfinite(x) and x > 0 else F(0.0) for x in w]
    bits, plan = [0, 0, 0], []
    for _ in range(MORTON_BITS):
        best = -1
        for a in range(3):                                         # a tie goes to the lowest axis
            if bits[a] < AXIS_BITS_MAX and (best < 0 or w[a] > w[best]):
                best = a
        plan.append(best)
        bits[best] += 1
        w[best] = F(w[best] * F(0.5))
    return plan, bits


def np_cells(c2, cmin, cmax, bits):
    if cmax == cmin or bits == 0:
        return np.zeros(c2.shape[0], np.int64)
    top = (1 << bits) - 1
    with np.errstate(all="ignore"):
        scale = F(1 << bits) / F(cmax - cmin)
        f = ((c2 - cmin).astype(F) * scale).astype(F)
        high, low = f >= F(top), (f > 0) & ~(f >= F(top))          # (a NaN compares false both times: cell 0)
    cell = np.zeros(c2.shape[0], np.int64)
    cell[high] = top
    cell[low] = f[low].astype(np.int64)
    return cell


def np_keys_extent(verts, idx):
    """The 64-bit key of every triangle with the extent-aware plan (numpy uint64 [n])."""
    c2, cmin, cmax = np_c2(verts, idx)
    plan, bits = np_plan(cmin, cmax)
    cell = [np_cells(c2[:, a], cmin[a], cmax[a], bits[a]) for a in range(3)]
    left = list(bits)
    key = np.zeros(c2.shape[0], np.uint64)
    for k, a in enumerate(plan):                                   # Morton bit 38 - k: the next unused bit of cell[a]
        left[a] -= 1
        key |= ((cell[a] >> left[a]) & 1).astype(np.uint64) << np.uint64(INDEX_BITS + MORTON_BITS - 1 - k)
    return key | np.arange(c2.shape[0], dtype=np.uint64)


def plan_bits(verts, idx):
    _, cmin, cmax = np_c2(verts, idx)
    return np_plan(cmin, cmax)[1]


@contextlib.contextmanager
def _extent_keys():
    """lbvh_common's restatement and checker take their keys from its np_keys: give them these."""
    old = lbvh_common.np_keys
    lbvh_common.np_keys = np_keys_extent
    try:
        yield
    finally:
        lbvh_common.np_keys = old


def np_lbvh_extent(verts, idx, max_leaf):
    with _extent_keys():
        return lbvh_common.np_lbvh(verts, idx, max_leaf)


def check_valid_extent(verts, idx, nodes, refs, max_leaf):
    with _extent_keys():
        return lbvh_common.check_valid(verts, idx, nodes, refs, max_leaf)


def needle():
    """300 triangles whose x extent is 2^22 times the others: x would take 22 bits more than y and
    z, so the 20-bit cap binds (bits 20 / 10 / 9)."""
    rng = np.random.default_rng(22)
    c = rng.uniform(0.0, 1.0, (300, 3)).astype(F)
    c[0], c[1] = 0.0, 1.0                                          # the extent is exactly (2^22, 1, 1) * 2
    c[:, 0] *= F(2.0 ** 22)
    off = np.array([[-0.5, 0.0, 0.0625], [0.5, -0.0625, 0.0], [0.0, 0.0625, -0.0625]], F)
    return _w1((c[:, None, :] + off[None]).astype(F).reshape(-1, 3)), np.arange(900, dtype=np.int32)


def nonfinite():
    """The first 300 triangles of rand2k with one vertex at x = +inf: an axis whose extent is not finite."""
    d = load_golden("rand2k")
    i = d["indices"][:900]
    v = np.array(d["vertices"], F, copy=True)
    v[i[7], 0] = np.inf
    return v, i


_CACHE = {}
DEGENERATE = ["single_tri_rootleaf", "cornell12", "copies70", "grid16", "needle", "nonfinite"]
SMALL = DEGENERATE + ["rand2k", "cubes2_obj"]                      # the restatement runs on these
ALL = SMALL + ["hf40k", "hf320"]


def mesh(name):
    """(vertices, indices) of a named mesh (shared; do not modify)."""
    if name in ("needle", "nonfinite"):
        if name not in _CACHE:
            _CACHE[name] = {"needle": needle, "nonfinite": nonfinite}[name]()
        return _CACHE[name]
    return lbvh_common.mesh(name)


_TWIN = {}


def twin_extent(name, max_leaf):
    """rt_bvh_build_lbvh with RT_BUILD_EXTENT_KEYS over a named mesh (or (vertices, indices)), computed once."""
    import rtamd
    key = (name, max_leaf) if isinstance(name, str) else None
    if key is not None and key in _TWIN:
        return _TWIN[key]
    v, i = mesh(name) if isinstance(name, str) else name
    b = rtamd.Mesh.from_arrays(v, i).build_lbvh(max_leaf, keys="extent")
    out = (b.nodes, b.tri_indices)
    if key is not None:
        _TWIN[key] = out
    return out


def np_half_area(mn, mx):
    """hA(box) = (dx*dy + dy*dz) + dz*dx in float32, single operations."""
    with np.errstate(all="ignore"):
        d = (np.asarray(mx, F) - np.asarray(mn, F)).astype(F)
        return ((d[..., 0] * d[..., 1]).astype(F) + (d[..., 1] * d[..., 2]).astype(F)).astype(F) + (d[..., 2] * d[..., 0]).astype(F)


def np_scene_sah(nodes):
    """rt_scene_sah's definition over a host node array (nn, 12): (inner_area, leaf_area_tris,
    root_area) in float64.  Inner records are the reachable valid inner nodes, each once; every
    child slot counts: an inner child its area, a leaf its area times its count, a malformed node
    nothing."""
    nodes = np.asarray(nodes, F)
    ni = nodes.view(np.int32)
    nn = nodes.shape[0]
    area = np_half_area(nodes[:, 0:3], nodes[:, 4:7]).astype(np.float64)
    left, right = ni[:, 8], ni[:, 9]
    valid = (left >= 0) & (right >= 0) & (left < nn) & (right < nn)
    root_area = float(area[0])
    if left[0] < 0:
        return 0.0, root_area * max(int(ni[0, 11]), 0), root_area
    seen, stack = np.zeros(nn, bool), [0]
    while stack:
        n = stack.pop()
        if seen[n] or not valid[n]:
            continue
        seen[n] = True
        stack += [int(left[n]), int(right[n])]
    kids = np.concatenate([left[seen], right[seen]])               # per child slot: a two-parent node counts twice
    inner_kids = kids[valid[kids]]
    leaf_kids = kids[left[kids] < 0]
    inner = root_area + float(area[inner_kids].sum()) if seen[0] else 0.0
    leaf = float((area[leaf_kids] * np.maximum(ni[leaf_kids, 11], 0)).sum())
    return inner, leaf, root_area


def np_cost(nodes):
    """The normalised SAH cost (inner_area + leaf_area_tris) / root_area."""
    inner, leaf, root = np_scene_sah(nodes)
    return (inner + leaf) / root
