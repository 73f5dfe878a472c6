"""Shared by test_refit.py (CPU) and test_refit_gpu.py: the numpy restatement of the BVH refit
(DESIGN.md 14), the moved vertex sets and two synthetic trees no fixture has -- a comb of 60
inner nodes (a chain of heights without a shared node) and four leaves of 40, 3, 0 and 35
triangles (counts >= 31 take the escape table; the empty leaf keeps its box)."""
import numpy as np

from conftest import load_golden

FIXTURES = ["hf40k", "rand4k_sbvh", "cubes2_dae", "cornell12", "single_tri_rootleaf"]
SYNTHETIC = ["comb60", "bigleaf"]
BOX = [0, 1, 2, 4, 5, 6]          # min.xyz, max.xyz words of a node
KEPT = [3, 7, 8, 9, 10, 11]       # w components and the child / leaf words: never touched


def reachable(nodes):
    """Node indices from the root, every parent before its children."""
    ni = nodes.view(np.int32)
    order, stack = [], [0]
    while stack:
        n = stack.pop()
        order.append(n)
        if ni[n, 8] >= 0:
            stack += [int(ni[n, 9]), int(ni[n, 8])]
    return order


def leaf_vertices(d, n):
    """Vertex indices of every triangle in leaf n's range."""
    ni = d["nodes"].view(np.int32)
    tri = d["tri_indices"][ni[n, 10]:ni[n, 10] + ni[n, 11]]
    return d["indices"][(tri[:, None] + np.arange(3)[None, :]).ravel()]


def np_refit(d, verts):
    """The refit restated: leaf min / max over its triangles' vertices, unions upward; a leaf
    with num_tris <= 0 keeps its box.  Returns (nodes, reachable order)."""
    nodes = np.array(d["nodes"], np.float32, copy=True)
    ni = nodes.view(np.int32)
    order = reachable(nodes)
    for n in reversed(order):
        if ni[n, 8] >= 0:
            l, r = ni[n, 8], ni[n, 9]
            nodes[n, 0:3] = np.fmin(nodes[l, 0:3], nodes[r, 0:3])
            nodes[n, 4:7] = np.fmax(nodes[l, 4:7], nodes[r, 4:7])
        elif ni[n, 11] > 0:
            p = verts[leaf_vertices(d, n), :3]
            nodes[n, 0:3] = p.min(0)
            nodes[n, 4:7] = p.max(0)
    return nodes, order


def referenced_box(d, verts, order):
    """Min / max over every vertex a reachable leaf references (and the kept box of an empty
    leaf, which only the big-leaf tree has): what the root box must be."""
    ni = d["nodes"].view(np.int32)
    vi = np.concatenate([leaf_vertices(d, n) for n in order if ni[n, 8] < 0 and ni[n, 11] > 0])
    p = verts[vi, :3]
    kept = [n for n in order if ni[n, 8] < 0 and ni[n, 11] <= 0]
    lo = np.concatenate([p, d["nodes"][kept, 0:3]])
    hi = np.concatenate([p, d["nodes"][kept, 4:7]])
    return lo.min(0), hi.max(0)


def _finish(verts, nodes, refs):
    """Scene arrays around a hand-built tree: one normal per vertex, the Cornell materials."""
    nv, ntri = verts.shape[0], verts.shape[0] // 3
    mats = load_golden("cornell12")["materials"]
    normals = np.tile(np.array([0, 0, 1, 0], np.float32), (nv, 1))
    d = {"vertices": verts, "indices": np.arange(nv, dtype=np.int32), "nodes": nodes,
         "tri_indices": np.asarray(refs, np.int32), "normals": normals,
         "normals_indices": np.arange(nv, dtype=np.int32), "materials": mats,
         "tri_to_material": (np.arange(ntri, dtype=np.int32) % mats.shape[0]).astype(np.int32),
         "scene_min": verts[:, :3].min(0), "scene_max": verts[:, :3].max(0)}
    d["nodes"], _ = np_refit(d, verts)   # the boxes the tree starts with
    return d


def _node(nodes, n, left, right, off, cnt):
    nodes.view(np.int32)[n, 8:12] = (left, right, off, cnt)
    nodes[n, 3] = nodes[n, 7] = 1.0


def _triangles(rng, ntri, extent):
    c = rng.uniform(-extent, extent, (ntri, 1, 3)).astype(np.float32)
    v = (c + rng.uniform(-4, 4, (ntri, 3, 3)).astype(np.float32)).reshape(-1, 3)
    return np.concatenate([v, np.ones((v.shape[0], 1), np.float32)], 1)


def comb60():
    """Inner node i = node 2i: left = leaf 2i+1 (triangle i), right = inner i+1; the last one's
    right is leaf 120 (triangle 60).  Heights 1..60, one record each."""
    rng = np.random.default_rng(60)
    verts = _triangles(rng, 61, 60.0)
    nodes = np.zeros((121, 12), np.float32)
    for i in range(60):
        _node(nodes, 2 * i, 2 * i + 1, 2 * i + 2, -1, 0)
        _node(nodes, 2 * i + 1, -1, -1, i, 1)
    _node(nodes, 120, -1, -1, 60, 1)
    return _finish(verts, nodes, 3 * np.arange(61))


def bigleaf():
    """Root 0 -> inner 1 {leaf 3: 40 triangles, leaf 4: 3}, inner 2 {leaf 5: empty, leaf 6: 35}."""
    rng = np.random.default_rng(78)
    verts = _triangles(rng, 78, 50.0)
    nodes = np.zeros((7, 12), np.float32)
    _node(nodes, 0, 1, 2, -1, 0)
    _node(nodes, 1, 3, 4, -1, 0)
    _node(nodes, 2, 5, 6, -1, 0)
    _node(nodes, 3, -1, -1, 0, 40)
    _node(nodes, 4, -1, -1, 40, 3)
    _node(nodes, 5, -1, -1, -1, 0)
    _node(nodes, 6, -1, -1, 43, 35)
    nodes[5, 0:3] = (-70.0, -3.0, 2.0)     # the empty leaf's own box, outside the triangles'
    nodes[5, 4:7] = (-65.0, 0.0, 4.0)
    return _finish(verts, nodes, 3 * np.arange(78))


_CACHE = {}


def scene_arrays(name):
    """Fixture or synthetic scene as a dict of arrays (shared; do not modify)."""
    if name not in _CACHE:
        _CACHE[name] = {"comb60": comb60, "bigleaf": bigleaf}[name]() if name in SYNTHETIC else load_golden(name)
    return _CACHE[name]


def moved_vertices(name):
    """The test's new vertices: a seeded float32 displacement; cornell12 is scaled by 1.25 and the
    single triangle translated far enough that its frame changes."""
    v = np.array(scene_arrays(name)["vertices"], np.float32, copy=True)
    if name == "cornell12":
        v[:, :3] *= np.float32(1.25)
    elif name == "single_tri_rootleaf":
        v[:, :3] += np.array([6.0, -4.0, 3.0], np.float32)
    else:
        rng = np.random.default_rng(len(name) + v.shape[0])
        v[:, :3] += rng.uniform(-1.5, 1.5, (v.shape[0], 3)).astype(np.float32)
    return v


def scene_image(r):
    """The renderer's scene image, packed into a zeroed device buffer, as uint32 words."""
    import torch
    n = r.scene_image_size()
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    r.pack_scene(buf.data_ptr(), n)
    return buf.cpu().numpy().view(np.uint32)


def with_vertices(d, verts, nodes):
    """A copy of the scene dict with other vertices and nodes."""
    e = dict(d)
    e["vertices"], e["nodes"] = verts, nodes
    return e
