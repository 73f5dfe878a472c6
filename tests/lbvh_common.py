"""Shared by test_lbvh.py (CPU) and test_lbvh_gpu.py: a numpy / plain-Python restatement of the
LBVH definition, recursive over the sorted keys; the seeded meshes; and the validity
checker every built tree must pass."""
import bisect

import numpy as np

from conftest import load_golden
from refit_common import np_refit

INDEX_BITS = 25
INDEX_MASK = (1 << INDEX_BITS) - 1
F = np.float32


def np_keys(verts, idx):
    """Steps 1-5: the 64-bit key of every triangle (numpy uint64 [n])."""
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    p = np.asarray(verts, F)[tri][:, :, :3]                       # (n, 3 corners, 3 axes)
    lo, hi = np.fmin(np.fmin(p[:, 0], p[:, 1]), p[:, 2]), np.fmax(np.fmax(p[:, 0], p[:, 1]), p[:, 2])
    c2 = (lo + hi).astype(F)
    cmin, cmax = c2.min(0), c2.max(0)
    key = np.zeros(tri.shape[0], np.uint64)
    for a in range(3):                                             # x in the most significant place of a triple
        if cmax[a] == cmin[a]:
            cell = np.zeros(tri.shape[0], np.int64)
        else:
            scale = F(8192.0) / F(cmax[a] - cmin[a])
            cell = np.minimum(8191, (((c2[:, a] - cmin[a]).astype(F)) * scale).astype(F).astype(np.int64))
        for bit in range(13):
            key |= ((cell >> bit) & 1).astype(np.uint64) << np.uint64(INDEX_BITS + 3 * bit + (2 - a))
    return key | np.arange(tri.shape[0], dtype=np.uint64)


def _clz64(x):
    return 64 - int(x).bit_length()


def np_lbvh(verts, idx, max_leaf):
    """Steps 6-10 over np_keys: (nodes float32 (nn, 12), tri_indices int32 (n,)).  For small meshes."""
    verts = np.asarray(verts, F)
    idx = np.asarray(idx, np.int32)
    keys = sorted(int(k) for k in np_keys(verts, idx))
    n = len(keys)
    refs = np.array([3 * (k & INDEX_MASK) for k in keys], np.int32)
    kept, leaves = {}, []                                          # Karras number -> (a, b, s); (first, count)

    def split(a, b):
        """The last s in [a, b) with clz(k[a] ^ k[s]) > clz(k[a] ^ k[b])."""
        m = 63 - _clz64(keys[a] ^ keys[b])                         # the highest bit in which k[a] and k[b] differ
        s = bisect.bisect_left(keys, ((keys[a] >> m) | 1) << m, a, b + 1) - 1
        assert a <= s < b and (keys[s] >> m) & 1 == 0 and (keys[s + 1] >> m) & 1 == 1
        return s

    def walk(number, a, b):
        if b - a + 1 <= max_leaf:
            leaves.append((a, b - a + 1))
            return
        s = split(a, b)
        kept[number] = (a, b, s)
        walk(s, a, s)
        walk(s + 1, s + 1, b)

    walk(0, 0, n - 1)
    order = sorted(kept)
    rank = {num: r for r, num in enumerate(order)}
    leaves.sort()
    leaf_id = {first: len(order) + r for r, (first, _) in enumerate(leaves)}
    nodes = np.zeros((len(order) + len(leaves), 12), F)
    ni = nodes.view(np.int32)
    nodes[:, 3] = nodes[:, 7] = 1.0
    for first, cnt in leaves:
        ni[leaf_id[first], 8:12] = (-1, -1, first, cnt)
    for num in order:
        a, b, s = kept[num]
        left = rank[s] if s - a + 1 > max_leaf else leaf_id[a]
        right = rank[s + 1] if b - s > max_leaf else leaf_id[s + 1]
        ni[rank[num], 8:12] = (left, right, -1, 0)

    def fit(i):
        if ni[i, 8] < 0:
            tri = refs[ni[i, 10]:ni[i, 10] + ni[i, 11]]
            p = verts[idx[(tri[:, None] + np.arange(3)[None, :]).ravel()], :3]
            nodes[i, 0:3], nodes[i, 4:7] = p.min(0), p.max(0)
        else:
            l, r = int(ni[i, 8]), int(ni[i, 9])
            fit(l)
            fit(r)
            nodes[i, 0:3] = np.fmin(nodes[l, 0:3], nodes[r, 0:3])
            nodes[i, 4:7] = np.fmax(nodes[l, 4:7], nodes[r, 4:7])

    fit(0)
    return nodes, refs


def check_valid(verts, idx, nodes, refs, max_leaf):
    """What every LBVH output must satisfy (the issue's list)."""
    verts, idx = np.asarray(verts, F), np.asarray(idx, np.int32)
    n = idx.size // 3
    ni = nodes.view(np.int32)
    nn = nodes.shape[0]
    inner = ni[:, 8] >= 0
    K = int(inner.sum())
    assert nn == 2 * K + 1
    assert inner[:K].all() and not inner[K:].any()                 # kept nodes first, then leaves
    assert (ni[inner, 10] == -1).all() and (ni[inner, 11] == 0).all()
    assert (ni[~inner, 8] == -1).all() and (ni[~inner, 9] == -1).all()
    assert (nodes[:, 3] == 1.0).all() and (nodes[:, 7] == 1.0).all()
    # root is node 0: every other node is the child of exactly one node, node 0 of none
    kids = np.concatenate([ni[inner, 8], ni[inner, 9]])
    assert kids.size == nn - 1 and np.array_equal(np.sort(kids), np.arange(1, nn))
    # every triangle in exactly one leaf position; leaves tile [0, n) in order, 1..max_leaf each
    assert refs.shape == (n,) and np.array_equal(np.sort(refs), 3 * np.arange(n))
    first, cnt = ni[~inner, 10], ni[~inner, 11]
    assert (cnt >= 1).all() and (cnt <= max_leaf).all()
    assert first[0] == 0 and np.array_equal(first[1:], (first + cnt)[:-1]) and first[-1] + cnt[-1] == n
    # positions in strictly ascending key order
    k = np_keys(verts, idx)[refs // 3]
    assert (k[1:] > k[:-1]).all()
    # depth <= 64, and each inner range is its children's ranges side by side
    depth = np.zeros(nn, np.int64)
    lo, hi = np.zeros(nn, np.int64), np.zeros(nn, np.int64)
    lo[~inner], hi[~inner] = first, first + cnt
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        if inner[i]:
            for c in (int(ni[i, 9]), int(ni[i, 8])):
                depth[c] = depth[i] + 1
                stack.append(c)
    assert len(order) == nn and depth.max() <= 64
    for i in reversed(order):
        if inner[i]:
            l, r = ni[i, 8], ni[i, 9]
            assert hi[l] == lo[r]
            lo[i], hi[i] = lo[l], hi[r]
            assert hi[i] - lo[i] > max_leaf                        # a kept node holds more than max_leaf positions
    assert lo[0] == 0 and hi[0] == n
    # every box is the refit of the same arrays
    d = {"nodes": nodes, "tri_indices": refs, "indices": idx}
    want, _ = np_refit(d, verts)
    assert np.array_equal(want.view(np.uint32), nodes.view(np.uint32))
    return K, int(depth.max())


def _w1(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.ones((xyz.shape[0], 1), F)], 1)


def copies70():
    """70 copies of one triangle: every cmax == cmin branch; order from the index bits alone."""
    v = _w1([[1.0, 2.0, 3.0], [4.0, 2.5, 3.0], [1.0, 6.0, 5.0]])
    return v, np.tile(np.arange(3, dtype=np.int32), 70)


def deep40():
    """40 triangles with centroids at (2^-k, 2^-k, 2^-k) * 100, k = 0..39: a one-sided tree."""
    k = np.arange(40)
    c = (F(100.0) * np.ldexp(F(1.0), -k).astype(F))[:, None, None] * np.ones((1, 1, 3), F)
    off = np.array([[-1.0, 0.0, 1.0], [1.0, -1.0, 0.0], [0.0, 1.0, -1.0]], F)[None] * np.ldexp(F(1.0), -k - 4).astype(F)[:, None, None]
    return _w1((c + off).astype(F).reshape(-1, 3)), np.arange(120, dtype=np.int32)


def grid16():
    """A flat 16 x 16 grid (512 triangles) in the plane y = 0: one axis with zero extent."""
    g = np.arange(17, dtype=F) * F(2.5) - F(20.0)
    x, z = np.meshgrid(g, g, indexing="ij")
    v = _w1(np.stack([x.ravel(), np.zeros(289, F), z.ravel()], 1))
    q = (np.arange(16)[:, None] * 17 + np.arange(16)[None, :]).ravel()
    tri = np.concatenate([np.stack([q, q + 1, q + 17], 1), np.stack([q + 1, q + 18, q + 17], 1)])
    return v, tri.astype(np.int32).ravel()


def cornell_first(k):
    d = load_golden("cornell12")
    return d["vertices"], d["indices"][:3 * k]


_CACHE = {}
SMALL = ["single_tri_rootleaf", "cornell12", "copies70", "deep40", "grid16", "rand2k"]   # the restatement runs on these
ALL = SMALL + ["hf40k", "hf320"]


def mesh(name):
    """(vertices float32 (nv, 4), indices int32 (3n,)) of a named mesh (shared; do not modify)."""
    if name not in _CACHE:
        if name in ("copies70", "deep40", "grid16"):
            _CACHE[name] = {"copies70": copies70, "deep40": deep40, "grid16": grid16}[name]()
        elif name == "hf320":
            import rtamd
            a = rtamd.Mesh.heightfield(320, 320).arrays()
            _CACHE[name] = (a["vertices"], a["indices"])
        else:
            d = load_golden(name)
            _CACHE[name] = (d["vertices"], d["indices"])
    return _CACHE[name]


_TWIN = {}


def twin(name, max_leaf):
    """rt_bvh_build_lbvh over the named mesh (or (vertices, indices)): (nodes, tri_indices), computed once."""
    import rtamd
    key = (name, max_leaf) if isinstance(name, str) else None
    if key is None or key not in _TWIN:
        v, i = mesh(name) if isinstance(name, str) else name
        b = rtamd.Mesh.from_arrays(v, i).build_lbvh(max_leaf)
        if key is None:
            return b.nodes, b.tri_indices
        _TWIN[key] = (b.nodes, b.tri_indices)
    return _TWIN[key]
