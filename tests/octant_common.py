"""Shared by the octant-loop tests: cameras whose primary rays all lie in one
direction octant, the host-side ray directions of a camera, and a hand-made scene with an
inverted child box."""
import dataclasses

import numpy as np

W = H = 64
F32 = np.float32


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def look_at_params(d, eye, half=0.25):
    """The fixture's params with the camera at `eye`, looking at the centre of the scene box through
    an image plane at distance 1 with half-width `half` (a / b span it, c is its corner)."""
    p = np.array(d["params"], np.float32, copy=True).reshape(8, 4)
    centre = 0.5 * (np.asarray(d["scene_min"], np.float64) + np.asarray(d["scene_max"], np.float64))
    eye = np.asarray(eye, np.float64)
    f = _unit(centre - eye)
    r = _unit(np.cross(f, [0.0, 1.0, 0.0] if abs(f[1]) < 0.9 else [1.0, 0.0, 0.0]))
    u = np.cross(r, f)
    p[0, :3] = 2 * half * r
    p[1, :3] = 2 * half * u
    p[2, :3] = eye + f - half * r - half * u
    p[3, :3] = eye
    p[6, :3] = d["scene_min"]
    p[7, :3] = d["scene_max"]
    return p.reshape(-1)


def _box(d):
    lo, hi = np.asarray(d["scene_min"], np.float64), np.asarray(d["scene_max"], np.float64)
    return 0.5 * (lo + hi), float(np.max(hi - lo))


def octant_params(d, k):
    """Every primary ray in octant k (bit i set: direction component i negative): the eye outside
    the box corner opposite to the direction (1, 1, 1) / sqrt(3) with those signs, looking at the
    centre.  With half-width 0.25 a ray's component deviates from the axis' 0.577 by at most
    0.25 * sqrt(2) * sqrt(1 - 1/3) = 0.29, so all three signs hold (ray_dirs checks it)."""
    centre, ext = _box(d)
    sgn = np.array([-1.0 if k >> i & 1 else 1.0 for i in range(3)])
    return look_at_params(d, centre - sgn * 1.2 * ext)


def straddle_params(d):
    """A frame whose rays' x components change sign in the middle."""
    centre, ext = _box(d)
    return look_at_params(d, centre + np.array([0.05, 1.0, 1.0]) * 1.2 * ext)


def axis_params(d, name):
    """An axis-aligned camera for a 65 x 65 frame: pixel 33's xf = yf = 32.5 / 65 = 0.5 exactly, so the
    middle column's rays have x == 0 and the middle row's y == 0 (every term below is a small integer,
    exact in float32).  For knot16k it is test_zero_direction_component_pixels' camera."""
    p = np.array(d["params"], np.float32, copy=True).reshape(8, 4)
    if name == "knot16k":
        half, eye, dist = 50.0, np.array([0.0, 0.0, 220.0]), 100.0
        p[4, :3] = [-23, 200, 3]
    else:
        centre, ext = _box(d)
        half = float(2 ** np.ceil(np.log2(ext / 4)))
        dist = 2 * half
        eye = np.round(centre) + np.array([0.0, 0.0, np.round(1.5 * ext)])
    p[0, :3] = [2 * half, 0, 0]
    p[1, :3] = [0, 2 * half, 0]
    p[2, :3] = [eye[0] - half, eye[1] - half, eye[2] - dist]
    p[3, :3] = eye
    p[6, :3] = d["scene_min"]
    p[7, :3] = d["scene_max"]
    return p.reshape(-1)


def ray_dirs(params, w, h):
    """(h, w, 3) float32: image_pos - campos of every pixel, by the kernel's own operations
    (primary_ray: xf = float((x - 0.5) / w), image_pos = (c + a * xf) + b * yf; the later normalize
    keeps every sign and every zero)."""
    p = np.asarray(params, np.float32).reshape(8, 4)
    a, b, c, eye = p[0, :3], p[1, :3], p[2, :3], p[3, :3]
    xf = ((np.arange(w, dtype=np.float64) - 0.5) / np.float64(F32(w))).astype(F32)
    yf = ((np.arange(h, dtype=np.float64) - 0.5) / np.float64(F32(h))).astype(F32)
    t1 = (a[None, None, :] * xf[None, :, None]).astype(F32) + c[None, None, :]
    t2 = (b[None, None, :] * yf[:, None, None]).astype(F32)
    return ((t1 + t2).astype(F32) - eye[None, None, :]).astype(F32)


def octant_of(dirs):
    """The octant shared by all rays of `dirs` (no zero component, signs uniform), else None."""
    if np.any(dirs == 0.0):
        return None
    neg = np.signbit(dirs).reshape(-1, 3)
    if np.any(neg != neg[0]):
        return None
    return int(neg[0, 0]) | int(neg[0, 1]) << 1 | int(neg[0, 2]) << 2


# ---- a hand-made two-leaf BVH whose right child box has min.x > max.x ----

TRI_VERTS = np.array([[-40, -10, 0, 1], [40, -10, 0, 1], [0, 50, 5, 1],
                      [-30, 0, -30, 1], [30, 0, -30, 1], [0, 0, 30, 1]], np.float32)


def two_leaf_nodes(inverted):
    """Root (inner) + one leaf per triangle of TRI_VERTS, boxes = the triangles' bounds; `inverted`
    swaps the right leaf's min.x and max.x (30 > -30).  (3, 12) float32 raw BVH_Node_ words."""
    nodes = np.zeros((3, 12), np.float32)
    words = nodes.view(np.int32)
    lo = [TRI_VERTS[3 * t:3 * t + 3, :3].min(axis=0) for t in range(2)]
    hi = [TRI_VERTS[3 * t:3 * t + 3, :3].max(axis=0) for t in range(2)]
    nodes[0, 0:3], nodes[0, 4:7] = np.minimum(lo[0], lo[1]), np.maximum(hi[0], hi[1])
    words[0, 8:12] = [1, 2, -1, 0]
    for t in range(2):
        nodes[1 + t, 0:3], nodes[1 + t, 4:7] = lo[t], hi[t]
        words[1 + t, 8:12] = [-1, -1, t, 1]
    if inverted:
        nodes[2, 0], nodes[2, 4] = nodes[2, 4], nodes[2, 0]
    return nodes


def two_leaf_scene(inverted):
    """(Scene, params) of the two triangles with the hand-made tree, 64 x 64 default camera."""
    import rtamd
    m = rtamd.Mesh.from_arrays(TRI_VERTS, np.arange(6, dtype=np.int32))
    s = rtamd.Scene.from_mesh(m, m.build_bvh())
    s = dataclasses.replace(s, nodes=two_leaf_nodes(inverted), tri_indices=np.array([0, 3], np.int32))
    return s, rtamd.params_to_array(m.camera_params(W, H))
