"""Shared by test_mesh_edges.py (CPU) and test_mesh_edges_gpu.py: the meshes at the edges of mesh
space -- long one-sided trees, depth and height lists of exactly 1,024 and 1,025
nodes, zeros of both signs, NaNs and infinities, subnormal and huge extents, points and segments,
triangle counts at the 256-thread block edge -- with the properties each one is made for, measured
on the CPU; restatements of the leaf and union rule that ignore a NaN as fminf / fmaxf do
(lbvh_common's and refit_common's take ndarray.min, which propagates it); and the zero rule, the
one freedom a comparison in the new tests grants."""
import contextlib

import numpy as np

import lbvh_common
import lbvh_keys_common
from conftest import load_golden
from lbvh_common import F, INDEX_BITS
from lbvh_keys_common import np_c2, np_cells, np_plan
from refit_common import leaf_vertices, reachable

U = np.uint32
SIGN = 0x80000000
BOX = [0, 1, 2, 4, 5, 6]
CELL_BITS = 13


# ---- the meshes -------------------------------------------------------------------------------

def lattice(p):
    """Triangle t = (p, p + (0.25, 0, 0), p + (0, 0.25, 0)), p an integer triple in float: c2 - cmin
    is 2 (p - p_min) exactly."""
    p = np.asarray(p, F).reshape(-1, 3)
    c = np.repeat(p, 3, 0)
    c[1::3, 0] += F(0.25)
    c[2::3, 1] += F(0.25)
    return np.concatenate([c, np.ones((c.shape[0], 1), F)], 1), np.arange(c.shape[0], dtype=np.int32)


def single_bit_cell(j):
    """The j-th single-bit cell: 2^(12 - j // 3) on axis j % 3, so Morton bit 38 - j alone."""
    p = [0.0, 0.0, 0.0]
    p[j % 3] = float(1 << (12 - j // 3))
    return p


def chain52():
    """2^12 + 40 triangles: a one-sided Morton chain of 39 levels into a one-sided index-bit chain of 13."""
    n = (1 << 12) + 40
    p = np.full((n, 3), 8192.0, F)
    origin = [0] + [1 << k for k in range(13)]
    p[origin] = 0.0
    free = np.setdiff1d(np.arange(n), origin)[:39]
    for j, t in enumerate(free):
        p[t] = single_bit_cell(j)
    return lattice(p)


def _grid(xs, ys, zs):
    return np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3).astype(F)


def lattice4096_points():
    g = 512.0 * np.arange(16)
    return _grid(g, g, g)


def lattice_chain():
    """A 16 x 16 x 8 sub-lattice in the upper half of x, the origin, 14 single-bit cells, the far corner."""
    sub = _grid(4096.0 + 256.0 * np.arange(16), 512.0 * np.arange(16), 1024.0 * np.arange(8))
    rest = [[0.0, 0.0, 0.0]] + [single_bit_cell(j) for j in range(1, 15)] + [[8192.0, 8192.0, 8192.0]]
    return lattice(np.concatenate([sub, np.array(rest, F)]))


def two_scale():
    """lattice4096, then 4,096 triangles in [0, 0.4)^3: all of them in cell 0, ordered by index bits."""
    small = np.random.default_rng(5).uniform(0.0, 0.4, (4096, 3)).astype(F)
    return lattice(np.concatenate([lattice4096_points(), small]))


def rand512():
    d = load_golden("rand2k")
    return np.array(d["vertices"], F, copy=True), d["indices"][:3 * 512]


def signed_zeros(v, seed):
    """A seeded half of all zero coordinates becomes -0.0; a seeded 10 % of the other x coordinates
    becomes +0.0 or -0.0."""
    rng = np.random.default_rng(seed)
    v = np.array(v, F, copy=True)
    xyz = v[:, :3]
    zero = xyz == 0
    other = np.flatnonzero(~zero[:, 0])
    pick = other[rng.random(other.size) < 0.1]
    xyz[pick, 0] = np.where(rng.random(pick.size) < 0.5, F(0.0), F(-0.0))
    flip = zero & (rng.random(xyz.shape) < 0.5)
    xyz[flip] = F(-0.0)
    return v


def nonfinite(kind):
    v, i = rand512()
    tri = i.reshape(-1, 3)
    if kind == "a":                                    # one coordinate
        v[tri[7, 1], 1] = np.nan
    elif kind == "b":                                  # a whole triangle
        v[tri[40], :3] = np.nan
    elif kind == "c":                                  # one axis, in every vertex
        v[:, 2] = np.nan
    elif kind == "d":
        v[tri[11, 0], 0] = -np.inf
    elif kind == "e":                                  # finite vertices whose lo + hi overflows
        v[tri[20], 1] = F(3e38)
        v[tri[21], 1] = F(-3e38)
        v[tri[22, 0], 1], v[tri[22, 1], 1] = F(3e38), F(-3e38)
    elif kind == "f":                                  # both infinities on one axis
        v[tri[30, 0], 2], v[tri[31, 0], 2] = np.inf, -np.inf
        v[tri[32, 0], 2], v[tri[32, 1], 2] = np.inf, -np.inf
    return v, i


TINY_SCALE = {"a": -136, "b": -121, "c": -131}


def tiny_points():
    return np.random.default_rng(64).integers(0, 64, (300, 3)).astype(F)


def tiny(kind):
    v, i = lattice(tiny_points())
    v[:, :3] = np.ldexp(v[:, :3], TINY_SCALE[kind]).astype(F)
    return v, i


def huge():
    v, i = rand512()
    v[:, :3] = np.ldexp(v[:, :3], 58).astype(F)
    return v, i


def degenerate():
    """A seeded third of the triangles is a point (i, i, i), a third a segment (i, i, j); 32 share vertex 0."""
    v, i = rand512()
    tri = np.array(i.reshape(-1, 3), np.int32, copy=True)
    kind = np.random.default_rng(33).integers(0, 3, tri.shape[0])
    tri[kind == 0, 1] = tri[kind == 0, 2] = tri[kind == 0, 0]
    tri[kind == 1, 1] = tri[kind == 1, 0]
    tri[np.flatnonzero(kind == 2)[:32], 0] = 0
    return v, tri.ravel()


LATTICE = ["chain52", "lattice4096", "lattice_chain", "two_scale"]
ZEROS = ["signed_zeros_grid16", "signed_zeros_rand512"]
NONFINITE = ["nonfinite_" + k for k in "abcdef"]
TINY = ["tiny_" + k for k in "abc"]
BLOCK_EDGES = [f"rand2k_first{k}" for k in (255, 256, 257, 511, 513)]
FINITE = ["chain52", "lattice_chain", "two_scale"] + ZEROS + ["degenerate"] + BLOCK_EDGES   # the ones that are rendered
ALL = LATTICE + ZEROS + NONFINITE + TINY + ["huge", "degenerate"] + BLOCK_EDGES

# kept nodes per depth at max_leaf 1 (per-axis keys), and how each list of heights begins: measured by the host twin
POW2 = [1 << k for k in range(12)]                     # 1 .. 2048
DEPTHS = {
    "chain52": [1, 2, 2, 3, 5, 9, 17, 25, 48, 65, 129, 255, 509, 1017, 2011] + [1] * 37,
    "lattice4096": POW2,
    "lattice_chain": [1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513, 1025, 2, 1, 1],
    "two_scale": POW2 + [1] + POW2,
}
HEIGHTS = {"chain52": [2039, 1023, 512], "lattice4096": [2048, 1024, 512], "lattice_chain": [1025, 513, 257],
           "two_scale": [4095, 2047, 1023]}            # how each list of heights begins

_MESH = {}


def mesh(name):
    """(vertices float32 (nv, 4), indices int32 (3n,)) of a named mesh (shared; do not modify)."""
    if name not in _MESH:
        if name.startswith("rand2k_first"):
            d = load_golden("rand2k")
            _MESH[name] = (d["vertices"], d["indices"][:3 * int(name[len("rand2k_first"):])])
        elif name == "signed_zeros_grid16":
            v, i = lbvh_common.mesh("grid16")
            _MESH[name] = (signed_zeros(v, 16), i)
        elif name == "signed_zeros_rand512":
            v, i = rand512()
            _MESH[name] = (signed_zeros(v, 512), i)
        elif name.startswith("nonfinite_"):
            _MESH[name] = nonfinite(name[-1])
        elif name.startswith("tiny_"):
            _MESH[name] = tiny(name[-1])
        elif name == "lattice4096":
            _MESH[name] = lattice(lattice4096_points())
        else:
            _MESH[name] = {"chain52": chain52, "lattice_chain": lattice_chain, "two_scale": two_scale, "huge": huge,
                           "degenerate": degenerate}[name]()
    return _MESH[name]


def base_vertices(name):
    """The tame vertices an edge mesh is a transform of (the same indices), or None."""
    if name in ("signed_zeros_rand512", "huge") or name.startswith("nonfinite_"):
        return rand512()[0]
    if name == "signed_zeros_grid16":
        return lbvh_common.mesh("grid16")[0]
    if name.startswith("tiny_"):
        return lattice(tiny_points())[0]
    return None


def moved_vertices(name):
    """refit_common.moved_vertices' seeded displacement, in the mesh's own unit."""
    v = np.array(mesh(name)[0], F, copy=True)
    unit = F(2.0 ** 58) if name == "huge" else F(2.0 ** TINY_SCALE[name[-1]]) if name.startswith("tiny_") else F(1.0)
    rng = np.random.default_rng(len(name) + v.shape[0])
    with np.errstate(all="ignore"):
        v[:, :3] += rng.uniform(-1.5, 1.5, (v.shape[0], 3)).astype(F) * unit
    return v


def arrays(name):
    """The mesh with normals and materials: test_scene_build_gpu.arrays' seeded recipe (the golden
    file's own for the meshes over rand2k's triangles)."""
    from test_scene_build_gpu import arrays as recipe, first
    v, i = mesh(name)
    if i.size <= 3 * 2000 and np.array_equal(i, load_golden("rand2k")["indices"][:i.size]):
        return dict(first(recipe("rand2k"), i.size // 3), vertices=v)
    lbvh_common._CACHE.setdefault(name, (v, i))        # the recipe takes the mesh from lbvh_common.mesh
    return recipe(name)


# ---- keys ---------------------------------------------------------------------------------------

def flush(x):
    """A subnormal becomes a zero of its sign: what a device that flushes would compute with."""
    x = np.asarray(x, F)
    return np.where(np.abs(x) < F(2.0 ** -126), np.copysign(F(0.0), x), x).astype(F)


def np_keys_edge(verts, idx, extent, ftz=False):
    """The 64-bit keys, per-axis or extent-aware, NaN-correct (lbvh_keys_common's c2, plan and cell);
    with ftz every operand and result of the device's float steps is flushed."""
    fl = flush if ftz else (lambda x: x)
    verts = np.array(verts, F, copy=True)
    verts[:, :3] = fl(verts[:, :3])
    c2, _, _ = np_c2(verts, idx)
    c2 = fl(c2)
    cmin, cmax = np.fmin.reduce(c2, 0), np.fmax.reduce(c2, 0)
    if extent:
        plan, bits = np_plan(cmin, cmax)
    else:
        plan, bits = [k % 3 for k in range(3 * CELL_BITS)], [CELL_BITS] * 3
    cell = []
    for a in range(3):
        if not ftz:
            cell.append(np_cells(c2[:, a], cmin[a], cmax[a], bits[a]))
            continue
        with np.errstate(all="ignore"):                  # np_cells, every step flushed
            if cmax[a] == cmin[a] or bits[a] == 0:
                cell.append(np.zeros(c2.shape[0], np.int64))
                continue
            top = (1 << bits[a]) - 1
            scale = fl(F(1 << bits[a]) / fl(F(cmax[a] - cmin[a])))
            f = fl(fl((c2[:, a] - cmin[a]).astype(F)) * scale)
            high, low = f >= F(top), (f > 0) & ~(f >= F(top))
            c = np.zeros(c2.shape[0], np.int64)
            c[high] = top
            c[low] = f[low].astype(np.int64)
            cell.append(c)
    left = list(bits)
    key = np.zeros(c2.shape[0], np.uint64)
    for k, a in enumerate(plan):
        left[a] -= 1
        key |= ((cell[a] >> left[a]) & 1).astype(np.uint64) << np.uint64(INDEX_BITS + len(plan) - 1 - k)
    return key | np.arange(c2.shape[0], dtype=np.uint64)


def np_cells_per_axis(verts, idx):
    """The per-axis cells (n, 3) of the 13-bit keys."""
    c2, cmin, cmax = np_c2(verts, idx)
    return np.stack([np_cells(c2[:, a], cmin[a], cmax[a], CELL_BITS) for a in range(3)], 1)


# ---- the leaf and union rule, NaN-correct -----------------------------------------------------------

def np_refit(d, verts):
    """refit_common.np_refit with the C code's rule: fminf / fmaxf over a leaf's vertices, seeded
    with the first (a NaN is ignored unless every operand is one).  Returns (nodes, reachable order)."""
    verts = np.asarray(verts, F)
    nodes = np.array(d["nodes"], F, copy=True)
    ni = nodes.view(np.int32)
    order = reachable(nodes)
    for n in reversed(order):
        if ni[n, 8] >= 0:
            l, r = ni[n, 8], ni[n, 9]
            nodes[n, 0:3] = np.fmin(nodes[l, 0:3], nodes[r, 0:3])
            nodes[n, 4:7] = np.fmax(nodes[l, 4:7], nodes[r, 4:7])
        elif ni[n, 11] > 0:
            p = verts[leaf_vertices(d, n), :3]
            nodes[n, 0:3] = np.fmin.reduce(p, 0)
            nodes[n, 4:7] = np.fmax.reduce(p, 0)
    return nodes, order


def zero_mask(d, verts):
    """(nn, 12) bool: the box words the zero rule may excuse -- the extreme is a zero and the
    vertices below the node hold zeros of both signs on that axis."""
    verts = np.asarray(verts, F)
    nodes, order = np_refit(d, verts)
    ni = nodes.view(np.int32)
    nn = nodes.shape[0]
    pos, neg = np.zeros((nn, 3), bool), np.zeros((nn, 3), bool)
    for n in reversed(order):
        if ni[n, 8] >= 0:
            l, r = ni[n, 8], ni[n, 9]
            pos[n], neg[n] = pos[l] | pos[r], neg[l] | neg[r]
        elif ni[n, 11] > 0:
            p = verts[leaf_vertices(d, n), :3]
            z, s = p == 0, np.signbit(p)
            pos[n], neg[n] = (z & ~s).any(0), (z & s).any(0)
    mask = np.zeros((nn, 12), bool)
    both = pos & neg
    mask[:, 0:3] = both & (nodes[:, 0:3] == 0)
    mask[:, 4:7] = both & (nodes[:, 4:7] == 0)
    return mask


def excused(got, want, mask, label):
    """The zero rule.  `got` and `want` as words; every differing word must be excusable (mask), a
    zero on both sides.  mask None: plain equality.  Returns the number of words excused."""
    got, want = np.asarray(got).view(U).ravel(), np.asarray(want).view(U).ravel()
    assert got.shape == want.shape, f"{label}: sizes {got.shape} vs {want.shape}"
    k = np.flatnonzero(got != want)
    if mask is None:
        assert k.size == 0, f"{label}: {k.size} words differ, first at {k[:8]}: {got[k[:8]]} vs {want[k[:8]]}"
        return 0
    m = np.asarray(mask, bool).ravel()
    bad = k[~m[k] | ((got[k] | want[k]) != SIGN) | ((got[k] & want[k]) != 0)]
    assert bad.size == 0, f"{label}: {bad.size} words differ beyond the zero rule, first at {bad[:8]}: " \
                          f"{got[bad[:8]]} vs {want[bad[:8]]}"
    return int(k.size)


def flipped(nodes, mask):
    """The nodes with the sign of every excusable word flipped: uploaded next to the nodes
    themselves, the words of the scene image that differ are the image's excusable words."""
    out = np.array(nodes, F, copy=True)
    out.view(U)[mask] ^= U(SIGN)
    return out


@contextlib.contextmanager
def _edge_rules(extent, zeros):
    """lbvh_common's restatement and checker with the NaN-correct keys and refit; on a mesh with
    zeros of both signs the checker's refit comparison follows the zero rule."""
    count = [0]

    def refit(d, verts):
        want, order = np_refit(d, verts)
        if zeros:
            count[0] += excused(d["nodes"], want, zero_mask(d, verts), "refit of the output")
            return np.array(d["nodes"], F, copy=True), order
        return want, order

    old = lbvh_common.np_keys, lbvh_common.np_refit
    lbvh_common.np_keys = lbvh_keys_common.np_keys_extent if extent else (lambda v, i: np_keys_edge(v, i, False))
    lbvh_common.np_refit = refit
    try:
        with np.errstate(all="ignore"):
            yield count
    finally:
        lbvh_common.np_keys, lbvh_common.np_refit = old


def np_lbvh(verts, idx, max_leaf, extent=False):
    """lbvh_common.np_lbvh's tree over the NaN-correct keys, its boxes by np_refit above."""
    with _edge_rules(extent, False):
        nodes, refs = lbvh_common.np_lbvh(verts, idx, max_leaf)
    nodes, _ = np_refit({"nodes": nodes, "tri_indices": refs, "indices": np.asarray(idx, np.int32)}, verts)
    return nodes, refs


def check_valid(verts, idx, nodes, refs, max_leaf, extent=False, zeros=False):
    """lbvh_common.check_valid's structural conditions; boxes compared as words with the NaN-correct
    refit.  Returns (K, depth, words excused)."""
    with _edge_rules(extent, zeros) as count:
        K, depth = lbvh_common.check_valid(verts, idx, nodes, refs, max_leaf)
    return K, depth, count[0]


_TWIN, _HANDLE = {}, {}


def twin(name, max_leaf, extent=False):
    """rt_bvh_build_lbvh over a named mesh: (nodes, tri_indices), computed once."""
    import rtamd
    key = (name, max_leaf, extent)
    if key not in _TWIN:
        if name not in _HANDLE:
            _HANDLE[name] = rtamd.Mesh.from_arrays(*mesh(name))
        b = _HANDLE[name].build_lbvh(max_leaf, keys="extent" if extent else "axis")
        _TWIN[key] = (b.nodes, b.tri_indices)
    return _TWIN[key]


def tree(name, nodes, refs):
    return {"nodes": nodes, "tri_indices": refs, "indices": mesh(name)[1]}


# ---- what a tree looks like to the launch schedules ---------------------------------------------------

def depth_counts(nodes):
    """(kept nodes per depth from the root, the depth of the deepest leaf)."""
    ni = np.asarray(nodes).view(np.int32)
    counts, level, depth = [], [0], 0
    while level:
        inner = [n for n in level if ni[n, 8] >= 0]
        if not inner:
            break
        counts.append(len(inner))
        level = [int(c) for n in inner for c in ni[n, 8:10]]
        depth += 1
    return counts, depth


def height_counts(nodes):
    """Kept nodes per height (a leaf 0, a kept node 1 + its higher child), height 1 first: the refit plan's lists."""
    ni = np.asarray(nodes).view(np.int32)
    h = np.zeros(ni.shape[0], np.int64)
    for n in reversed(reachable(nodes)):
        if ni[n, 8] >= 0:
            h[n] = 1 + max(h[ni[n, 8]], h[ni[n, 9]])
    return np.bincount(h[h > 0])[1:].tolist()
