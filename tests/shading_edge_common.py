"""Shared by test_shading_edges.py (CPU) and test_shading_edges_gpu.py: shading inputs at their edges
 and a float64 restatement of one bounce of the shading.

Shading is everything from a closest hit to the packed pixel: normal_at, normalize,
cook_torrance_ggx, reflect, rgb_to_int (rt_device_math.h) and shade_hit, finish_color, park_next,
shadow_coef, scene_box_hit (rt_kernel_body.inc).  The committed fixtures share one light, unit normals
and albedo in [0, 1]; the cases here move each of those to where the code branches.

A stage is a small seeded scene (at most ~200 triangles, tree by Mesh.from_arrays(v, i).build_lbvh(2))
and a camera of its own: `room`, a closed box with objects whose reflected rays never leave, and `open`,
a floor with the same objects whose reflected rays mostly leave.  A Case is scene arrays, a Params
block, a depth and a label "class/name", plus what its predicate needs (per-triangle tags).  Each class
has a predicate on the oracle's aux output (hits, t, rgb) that at least MIN_PIXELS pixels must
satisfy; tests/test_shading_edges.py asserts it.  Everything is built once and shared: do not modify.

np_shade is written from volumeRender.cl:27-53 (Cramer barycentrics), :1306-1403 (the shading at a hit)
and :1732-1779 (Cook-Torrance GGX) as cited in rt_device_math.h, in plain float64 numpy; it shares no
code and no evaluation order with oracle/rt_oracle.c."""
import numpy as np

F32 = np.float32
W, H = 96, 64
MIN_PIXELS = 64
DEPTH = 3                       # the depth of a case that is not about depth
F0, ROUGHNESS = 40.0 / 255.0, 0.5
AMBIENT = F32(0.3)
DIFFUSE = slice(12, 15)         # Material::diffuse.xyz in a material's 44 words (Mesh.h:20-67)
DIFFUSE_W = 15
NO_SHADOW = 1                   # RT_FLAG_NO_SHADOW
CLASSES = ["light", "normals", "det", "albedo", "pack", "depth", "box"]
MESH_KEYS = ("vertices", "indices", "nodes", "tri_indices", "normals", "normals_indices", "materials",
             "tri_to_material")


# ---- stages ----

class _Geo:
    """Triangles with their own three vertices and three normals each, a material and a tag."""

    def __init__(self):
        self.v, self.n, self.mat, self.tag = [], [], [], []

    def tri(self, p, n, mat, tag):
        self.v += [np.asarray(q, np.float64) for q in p]
        self.n += [np.asarray(q, np.float64) for q in n]
        self.mat.append(mat)
        self.tag.append(tag)

    def quad(self, p, n, mat, tag):
        """Corners p[0..3] in order; n: one normal or one per corner."""
        n = [n] * 4 if np.ndim(n) == 1 else n
        self.tri([p[0], p[1], p[2]], [n[0], n[1], n[2]], mat, tag)
        self.tri([p[0], p[2], p[3]], [n[0], n[2], n[3]], mat, tag)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def _geometry(kind, fy, slant, tilt):
    g = _Geo()
    X = 10.0 if kind == "room" else 14.0
    # the floor: corner normals tilted a little, so that the interpolation shows on many pixels
    corners = [(-X, fy, -X), (-X, fy, X), (X, fy, X), (X, fy, -X)]
    g.quad(corners, [_unit((sx * tilt, 1.0, sz * tilt)) for sx, sz in ((-1, -1), (-1, 1), (1, 1), (1, -1))], 0, "floor")
    if kind == "room":
        top = fy + 16.0
        g.quad([(-X, top, -X), (X, top, -X), (X, top, X), (-X, top, X)], (0.0, -1.0, 0.0), 1, "wall")
        g.quad([(-X, fy, -X), (-X, top, -X), (-X, top, X), (-X, fy, X)], (1.0, 0.0, 0.0), 1, "wall")
        g.quad([(X, fy, -X), (X, fy, X), (X, top, X), (X, top, -X)], (-1.0, 0.0, 0.0), 1, "wall")
        g.quad([(-X, fy, -X), (X, fy, -X), (X, top, -X), (-X, top, -X)], (0.0, 0.0, 1.0), 1, "wall")
        g.quad([(-X, fy, X), (-X, top, X), (X, top, X), (X, fy, X)], (0.0, 0.0, -1.0), 1, "wall")
    # a cube with face normals, half a unit above the floor
    c, s = np.array([-4.0, fy + 2.5, -3.0]), 2.0
    for axis in range(3):
        for sign in (-1.0, 1.0):
            nrm = np.zeros(3)
            nrm[axis] = sign
            u, w = np.zeros(3), np.zeros(3)
            u[(axis + 1) % 3], w[(axis + 2) % 3] = s, s
            o = c + nrm * s
            g.quad([o - u - w, o + u - w, o + u + w, o - u + w], nrm, 2, "cube")
    # a patch of 3 x 3 cells facing the camera, its vertex normals up to ~25 degrees off the face normal
    rng = np.random.default_rng(7)
    U, V = np.array([2.0, 0.0, 0.0]), np.array([0.0, 1.6, -1.2])
    face = _unit(np.cross(U, V))
    o = np.array([1.5, fy + 1.0, -0.5])
    vn = [[_unit(face + 0.3 * rng.uniform(-1.0, 1.0, 3)) for _ in range(4)] for _ in range(4)]
    for i in range(3):
        for j in range(3):
            p = [o + i * U + j * V, o + (i + 1) * U + j * V, o + (i + 1) * U + (j + 1) * V, o + i * U + (j + 1) * V]
            g.quad(p, [vn[i][j], vn[i + 1][j], vn[i + 1][j + 1], vn[i][j + 1]], 3, "patch")
    if slant:   # a plane through the origin of the coordinates: y = x / 2
        g.quad([(-6.0, -3.0, -8.0), (-6.0, -3.0, 2.0), (6.0, 3.0, 2.0), (6.0, 3.0, -8.0)], _unit((-0.5, 1.0, 0.0)), 1, "slant")
    return g


def camera(eye, target, w=W, h=H, half_width=0.6):
    """The a, b, c, campos words of a Params block: the image plane one unit in front of the eye, pixel
    (x, y) at c + a x/w + b y/h, row 0 at the top (volumeRender.cl:1169-1190)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = _unit(target - eye)
    right = _unit(np.cross(f, (0.0, 1.0, 0.0)))
    up = np.cross(right, f)
    a = right * 2.0 * half_width
    b = -up * 2.0 * half_width * h / w
    return a, b, eye + f - 0.5 * a - 0.5 * b, eye


_BVH = {}


def _tree(v, idx):
    """The LBVH of the triangles (it depends on the vertices alone), built once per geometry."""
    key = v.tobytes()
    if key not in _BVH:
        import rtamd
        bvh = rtamd.Mesh.from_arrays(v, idx).build_lbvh(2)
        _BVH[key] = (bvh.nodes.copy(), bvh.tri_indices.copy())
    return _BVH[key]


DEFAULT_ALBEDO = [(0.7, 0.7, 0.6), (0.6, 0.65, 0.8), (0.9, 0.2, 0.1), (0.1, 0.8, 0.4)]


class Case:
    def __init__(self, cls, name, scene, params, depth, tags, regular=None, w=W, h=H):
        self.cls, self.name, self.label = cls, name, f"{cls}/{name}"
        self.scene, self.params, self.depth, self.tags = scene, params, depth, tags
        self.regular, self.w, self.h = regular, w, h
        self.predicate = None

    def tris(self, tag):
        """3 * triangle (the id a hit reports) of every triangle with this tag."""
        return 3 * np.flatnonzero(self.tags == tag)


def stage(kind, fy=-4.0, offset=(0.0, 0.0, 0.0), slant=False, light=None, eye=None, target=None, tilt=0.1):
    """(scene arrays, params, tags) of a stage; light, eye and target are given before the offset; tilt:
    how far the floor's corner normals lean outwards (0: all straight up)."""
    g = _geometry(kind, fy, slant, tilt)
    off = np.asarray(offset, np.float64)
    nt = len(g.mat)
    v = np.zeros((3 * nt, 4), F32)
    v[:, :3] = (np.array(g.v) + off).astype(F32)
    n = np.zeros((3 * nt, 4), F32)
    n[:, :3] = np.array(g.n).astype(F32)
    idx = np.arange(3 * nt, dtype=np.int32)
    nodes, refs = _tree(v, idx)
    mats = np.zeros((4, 44), F32)
    for m, alb in enumerate(DEFAULT_ALBEDO):
        mats[m, DIFFUSE] = alb
        mats[m, DIFFUSE_W] = 1.0
    lo, hi = v[:, :3].min(axis=0), v[:, :3].max(axis=0)
    scene = {"vertices": v, "indices": idx, "nodes": nodes, "tri_indices": refs, "normals": n,
             "normals_indices": idx.copy(), "materials": mats, "tri_to_material": np.array(g.mat, np.int32),
             "scene_min": lo.copy(), "scene_max": hi.copy()}
    if eye is None:
        eye = (0.0, fy + 7.0, 8.5) if kind == "room" else (0.0, fy + 8.0, 17.0)
    if target is None:
        target = (0.0, fy + 3.0, -3.0) if kind == "room" else (0.0, fy + 1.5, -1.0)
    if light is None:
        light = (3.0, fy + 12.0, 3.0) if kind == "room" else (-8.0, fy + 20.0, 9.0)
    a, b, c, campos = camera(np.asarray(eye) + off, np.asarray(target) + off)
    params = np.zeros(32, F32)
    params[0:3], params[4:7], params[8:11], params[12:15] = a, b, c, campos
    params[16:19] = (np.asarray(light, np.float64) + off).astype(F32)
    params[20:24] = 1.0
    params[24:27], params[28:31] = lo, hi
    return scene, params, np.array(g.tag)


def _with(scene, **changed):
    d = dict(scene)
    d.update(changed)
    return d


# ---- the float64 restatement ----

def primary_rays(params, w, h):
    """(origins, unit directions), float64 (w*h, 3): volumeRender.cl:1169-1190 and RayInit (:205-211)."""
    p = np.asarray(params, np.float64).reshape(8, 4)[:, :3]
    a, b, c, campos = p[0], p[1], p[2], p[3]
    y, x = np.divmod(np.arange(w * h), w)
    xf, yf = (x - 0.5) / w, (y - 0.5) / h
    pos = c[None, :] + a[None, :] * xf[:, None] + b[None, :] * yf[:, None]
    return pos, _unit(pos - campos[None, :])


def _det3(a, b, c):
    """The determinant of the matrix with columns a, b, c, expanded along the first row as
    get_normal_at_tri_point writes it (volumeRender.cl:35)."""
    return (a[:, 0] * (b[:, 1] * c[:, 2] - c[:, 1] * b[:, 2]) - b[:, 0] * (a[:, 1] * c[:, 2] - c[:, 1] * a[:, 2])
            + c[:, 0] * (a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2]))


def _normalize(v):
    """normalize in exact arithmetic: v / |v|, a zero vector unchanged."""
    n = np.sqrt(np.sum(v * v, axis=1, keepdims=True))
    return np.divide(v, n, out=np.zeros_like(v), where=n > 0)


def _ggx_partial_geometry(c, alpha):
    cs = np.clip(c * c, 0.0, 1.0)
    tan2 = (1.0 - cs) / cs
    return 2.0 / (1.0 + np.sqrt(1.0 + alpha * alpha * tan2))


def _ggx_distribution(c, alpha):
    a2 = alpha * alpha
    nh = np.clip(c * c, 0.0, 1.0)
    den = nh * a2 + (1.0 - nh)
    return a2 / (np.pi * den * den)


def np_shade(scene, params, w, h, hits, t):
    """One bounce of the shading in float64 for every pixel whose primary ray hit: `hits` int32 (w*h,)
    the hit ids (3 * triangle, < 0: no hit), `t` the hit distances.  Returns (rgb float64 (w*h, 3), NaN
    where nothing was hit: rez_color with the x3 factor and the ambient term, which a depth-1 frame
    without the shadow ray stores as it is; detail: dict of per-pixel NL, NV, HV, Det and the
    interpolated normal before normalize)."""
    dt = np.dtype(np.float64)
    hits = np.asarray(hits)
    k = np.flatnonzero(hits >= 0)
    hid = hits[k]
    ori, dirs = primary_rays(params, w, h)
    ori, dirs = ori[k], dirs[k]
    vert = np.asarray(scene["vertices"], dt)[:, :3]
    nrm = np.asarray(scene["normals"], dt)[:, :3]
    vi, ni = np.asarray(scene["indices"]), np.asarray(scene["normals_indices"])
    p0, p1, p2 = (vert[vi[hid + j]] for j in range(3))
    n0, n1, n2 = (nrm[ni[hid + j]] for j in range(3))
    mat = np.asarray(scene["materials"], dt)[np.asarray(scene["tri_to_material"])[hid // 3]]
    albedo = mat[:, DIFFUSE]
    light = np.asarray(params, dt)[16:19]
    # :1314, :27-53
    v_new = ori + dirs * (np.asarray(t, dt)[k] - 0.001)[:, None]
    det = _det3(p0, p1, p2)
    with np.errstate(all="ignore"):
        l0, l1, l2 = _det3(v_new, p1, p2) / det, _det3(p0, v_new, p2) / det, _det3(p0, p1, v_new) / det
        n_raw = l0[:, None] * n0 + l1[:, None] * n1 + l2[:, None] * n2
        n = _normalize(n_raw)
        # :1357-1360, :1754-1779
        lv = _normalize(light[None, :] - v_new)
        v = _normalize(ori - v_new)
        hv = _normalize(v + lv)
        NL, NV = np.sum(n * lv, axis=1), np.sum(n * v, axis=1)
        NH, HV = np.sum(n * hv, axis=1), np.sum(hv * v, axis=1)
        alpha = ROUGHNESS * ROUGHNESS
        G = _ggx_partial_geometry(NV, alpha) * _ggx_partial_geometry(NL, alpha)
        D = _ggx_distribution(NH, alpha)
        F = F0 + (1.0 - F0) * (1.0 - np.clip(HV, 0.0, 1.0)) ** 5
        spec = G * D * F * 0.25 / (NV + 0.001)
        diff = np.clip(1.0 - F, 0.0, 1.0)
        brdf = np.maximum(0.0, albedo * (diff * NL / np.pi)[:, None] + spec[:, None])
        brdf[(NL <= 0.0) | (NV <= 0.0)] = 0.0
        rez = brdf * 3.0 + 0.3 * albedo    # :1389, :1402-1403
    rgb = np.full((hits.shape[0], 3), np.nan)
    rgb[k] = rez
    detail = {}
    for name, val in (("NL", NL), ("NV", NV), ("HV", HV), ("Det", det)):
        detail[name] = np.full(hits.shape[0], np.nan)
        detail[name][k] = val
    detail["n_raw"] = np.full((hits.shape[0], 3), np.nan)
    detail["n_raw"][k] = n_raw
    detail["v_new"] = np.full((hits.shape[0], 3), np.nan)
    detail["v_new"][k] = v_new
    return rgb, detail


def det_f32(scene, tri_ids):
    """get_normal_at_tri_point's Det of the triangles with these hit ids, every operation rounded to
    float32 in source order (volumeRender.cl:35)."""
    vert = np.asarray(scene["vertices"], F32)[:, :3]
    vi = np.asarray(scene["indices"])
    a, b, c = (vert[vi[np.asarray(tri_ids) + j]] for j in range(3))
    return _det3(a, b, c)


# ---- the oracle's frames of a case, computed once ----

_FRAMES = {}


def frames(case):
    """The oracle's frames of a case (shared; do not modify): "d" at the case's depth, "d1" at depth 1,
    "d1ns" at depth 1 without the shadow ray; each oracle.render's dict (out, hits, t, rgb, stats)."""
    if case.label not in _FRAMES:
        from oracle import oracle
        r = lambda depth, flags: oracle.render(case.scene, case.params, case.w, case.h, depth=depth, flags=flags)
        _FRAMES[case.label] = {"d": r(case.depth, 0), "d1": r(1, 0), "d1ns": r(1, NO_SHADOW)}
    return _FRAMES[case.label]


_DETAIL = {}


def detail(case):
    """np_shade of the case's depth-1 frame: (rgb, detail)."""
    if case.label not in _DETAIL:
        f = frames(case)["d1ns"]
        _DETAIL[case.label] = np_shade(case.scene, case.params, case.w, case.h, f["hits"][:, 0, 0], f["t"][:, 0])
    return _DETAIL[case.label]


def ambient_of(case, hit_ids):
    """The ambient term 0.3f * albedo (float32) of the triangles with these hit ids, (n, 3)."""
    m = np.asarray(case.scene["tri_to_material"])[np.asarray(hit_ids) // 3]
    return (AMBIENT * np.asarray(case.scene["materials"], F32)[m][:, DIFFUSE]).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ray_depth(frame):
    """Per pixel, how many of its rays hit: raytracer_bvh's ray_depth at the end (volumeRender.cl:1519)."""
    return (frame["hits"][:, :, 0] >= 0).sum(axis=1)


# ---- predicates: (pixels that satisfy the class's condition, pixels needed) ----

def _on(case, tag):
    h0 = frames(case)["d1"]["hits"][:, 0, 0]
    return np.isin(h0, case.tris(tag))


def _is_ambient(case, frame, mask):
    """Of the pixels in mask: those whose rgb is the ambient term of their triangle, bit for bit."""
    idx = np.flatnonzero(mask)
    amb = ambient_of(case, frame["hits"][idx, 0, 0])
    ok = np.zeros(mask.shape[0], bool)
    ok[idx] = np.all(bits(frame["rgb"][idx]) == bits(amb), axis=1)
    return ok


def _lit(case, tag=None):
    """Hit pixels (of a tag) of the depth-1 frame without shadows whose colour is above the ambient term."""
    f = frames(case)["d1ns"]
    mask = f["hits"][:, 0, 0] >= 0 if tag is None else _on(case, tag)
    idx = np.flatnonzero(mask)
    ok = np.zeros(mask.shape[0], bool)
    ok[idx] = np.all(f["rgb"][idx] > ambient_of(case, f["hits"][idx, 0, 0]), axis=1)
    return ok


def _every(mask, among):
    """The number of pixels in `among` if all of them satisfy `mask`, else 0."""
    return int(among.sum()) if np.all(mask[among]) else 0


def _pred_floor_ambient(case):
    floor = _on(case, "floor")
    return _every(_is_ambient(case, frames(case)["d1"], floor), floor), MIN_PIXELS


def _pred_floor_ambient_ns(case):
    floor = _on(case, "floor")
    return _every(_is_ambient(case, frames(case)["d1ns"], floor), floor), MIN_PIXELS


def _pred_light_at_camera(case):
    d = detail(case)[1]
    return int(np.sum(d["HV"] > 1.0 - 1e-12)), MIN_PIXELS


def _pred_light_opposite(case):
    d = detail(case)[1]
    return int(np.sum(_on(case, "floor") & (d["HV"] > 0) & (d["HV"] < 0.05) & (d["NL"] > 0) & (d["NV"] > 0))), MIN_PIXELS


def _pred_light_skim(case):
    """Every floor hit's vNew is within 0.001 of the light's height: inside the 0.001 offsets."""
    d = detail(case)[1]
    near = np.abs(np.asarray(case.params, np.float64)[17] - d["v_new"][:, 1]) < 0.001
    return _every(near, _on(case, "floor")), MIN_PIXELS


def _pred_lit(case):
    return int(_lit(case).sum()), MIN_PIXELS


def _pred_light_overflows(case):
    """Every hit's light_pos - vNew has an infinite float32 dot with itself, and the pixels are lit."""
    d = detail(case)[1]
    lv = (np.asarray(case.params, F32)[16:19][None, :] - d["v_new"].astype(F32)).astype(np.float64)
    hit = frames(case)["d1"]["hits"][:, 0, 0] >= 0
    over = np.sum(lv * lv, axis=1) > float(np.finfo(F32).max)
    return min(_every(over, hit), int(_lit(case).sum())), MIN_PIXELS


def _pred_floor_lit(case):
    return int(_lit(case, "floor").sum()), MIN_PIXELS


def _pred_flipped(case):
    d = detail(case)[1]
    floor = _on(case, "floor")
    return _every((d["NL"] > 0) & (d["NV"] <= 0) & _is_ambient(case, frames(case)["d1ns"], floor), floor), MIN_PIXELS


def _pred_through_zero(case):
    ny = detail(case)[1]["n_raw"][:, 1]
    floor = _on(case, "floor")
    return min(int(np.sum(floor & (ny > 0))), int(np.sum(floor & (ny < 0)))), MIN_PIXELS


def _pred_det_zero(tag):
    def pred(case):
        return (int(_on(case, tag).sum()) if np.all(det_f32(case.scene, case.tris(tag)) == 0) else 0), MIN_PIXELS
    return pred


def _pred_det_small(case):
    det = np.abs(det_f32(case.scene, case.tris("floor")))
    return (int(_on(case, "floor").sum()) if np.all((det > 0) & (det < 1e-2)) else 0), MIN_PIXELS


def _pred_hits(case):
    return int(np.sum(frames(case)["d1"]["hits"][:, 0, 0] >= 0)), MIN_PIXELS


def _pred_channel(test):
    """Pixels of the case's own frame whose rgb satisfies `test` (an (n, 3) -> (n,) function)."""
    def pred(case):
        with np.errstate(invalid="ignore"):
            return int(np.sum(test(frames(case)["d"]["rgb"]))), MIN_PIXELS
    return pred


def _pred_signed_zeros(case):
    f = frames(case)["d1"]
    hit = f["hits"][:, 0, 0] >= 0
    same = np.zeros(hit.shape[0], bool)
    same[hit] = f["rgb"][hit, 0] == f["rgb"][hit, 1]
    return _every(same, hit), MIN_PIXELS


def _pred_materials(case):
    m = np.asarray(case.scene["tri_to_material"])
    h0 = frames(case)["d1"]["hits"][:, 0, 0]
    hit = h0 >= 0
    return min(int(np.sum(m[h0[hit] // 3] == k)) for k in range(case.scene["materials"].shape[0])), MIN_PIXELS


def _pred_over_one(case):
    rgb = frames(case)["d"]["rgb"]
    hit = frames(case)["d"]["hits"][:, 0, 0] >= 0
    return min(int(np.sum(np.any(rgb >= 1.0, axis=1))), int(np.sum(hit & np.all(rgb < 1.0, axis=1)))), MIN_PIXELS


def _pred_negative_packs_zero(case):
    f = frames(case)["d"]
    neg = f["rgb"][:, 0] < 0
    return _every((f["out"] & 0xFF) == 0, neg), MIN_PIXELS


def near_integer(frame):
    """Pixels with a channel whose color * 255 (float32, as rgb_to_int receives it) lies strictly inside
    (0, 255) and within 1e-3 of an integer."""
    x = (frame["rgb"] * F32(255.0)).astype(np.float64)
    return np.any((x > 0.5) & (x < 254.5) & (np.abs(x - np.rint(x)) < 1e-3), axis=1)


def _pred_gradient(case):
    f = frames(case)["d1ns"]
    x = (f["rgb"][near_integer(f)] * F32(255.0)).astype(np.float64)
    both = np.any(x < np.rint(x)) and np.any(x >= np.rint(x))   # both sides of the truncation boundary
    return (int(near_integer(f).sum()) if both else 0), MIN_PIXELS


def _pred_depth_full(case):
    n = case.w * case.h
    return int(np.sum(ray_depth(frames(case)["d"]) == case.depth)), n // 2 + 1


def _pred_depth_spread(case):
    rd = ray_depth(frames(case)["d"])
    return (MIN_PIXELS if all(np.any(rd == k) for k in range(4)) else 0), MIN_PIXELS


def _pred_box_both(case):
    h0 = frames(case)["d"]["hits"][:, 0, 0]
    black = (h0 == -2) & (frames(case)["d"]["out"] == 0)
    return min(int(black.sum()), int(np.sum(h0 >= 0))), MIN_PIXELS


def _pred_box_is_true(case):
    """RayBoxIntersection takes fmin and fmax of the two planes on every axis (volumeRender.cl:236-254),
    so it does not see which of the two words is the smaller: the inverted box's frame is the true box's,
    word for word, and nothing else.  (Not "every pixel black", as one might expect of min > max.)"""
    f, g = frames(case)["d"], frames(by_label("box/true"))["d"]
    same = np.array_equal(f["out"], g["out"]) and np.array_equal(f["hits"], g["hits"]) and \
        np.array_equal(bits(f["rgb"]), bits(g["rgb"]))
    return (int(np.sum(f["hits"][:, 0, 0] >= 0)) if same else 0), MIN_PIXELS


# ---- the cases ----

def _case(cls, name, scene, params, tags, predicate, depth=DEPTH, regular=None):
    c = Case(cls, name, scene, params, depth, tags, regular)
    c.predicate = predicate
    return c


def _light_cases():
    fy = -4.0
    out = []
    far = _unit((-0.4, 1.0, 0.45))

    def add(name, pred, **kw):
        s, p, tags = stage("open", **kw)
        out.append(_case("light", name, s, p, tags, pred, regular="light"))
    add("below_floor", _pred_floor_ambient, light=(-8.0, fy - 20.0, 9.0))
    add("in_floor_plane", _pred_light_skim, light=(-8.0, fy, 9.0))
    s, p, tags = stage("open")
    p = p.copy()
    p[16:19] = p[12:15]
    out.append(_case("light", "at_camera", s, p, tags, _pred_light_at_camera, regular="light"))
    # the eye low over a floor with straight normals, the light low and far away straight ahead: on the
    # middle columns near the horizon l is nearly -v
    add("opposite_grazing", _pred_light_opposite, eye=(0.0, fy + 0.15, 13.5), target=(0.0, fy + 0.12, 0.0),
        light=(0.0, fy + 0.5, -400.0), tilt=0.0)
    add("skims_floor", _pred_light_skim, light=(2.0, fy + 0.0005, 3.0))
    add("distance_1e6", _pred_lit, light=tuple(far * 1e6))
    add("distance_1e30", _pred_light_overflows, light=tuple(far * 1e30))
    return out


def _normal_cases():
    out = []
    s, p, tags = stage("open")
    floor = np.flatnonzero(np.repeat(tags == "floor", 3))   # the floor's normals (one per corner)

    def add(name, normals, pred, regular=None, params=p):
        out.append(_case("normals", name, _with(s, normals=normals), params, tags, pred, regular=regular))

    def floor_changed(f):
        n = s["normals"].copy()
        n[floor, :3] = f(n[floor, :3])
        return n
    add("zero", floor_changed(lambda n: n * F32(0.0)), _pred_floor_ambient_ns)
    for name, k, reg in (("length_1e-3", 1e-3, "normals"), ("length_1e3", 1e3, "normals"), ("length_1e-25", 1e-25, None),
                         ("length_1e25", 1e25, None)):
        n = s["normals"].copy()
        n[:, :3] = (n[:, :3] * F32(k)).astype(F32)
        add(name, n, _pred_lit, regular=reg)

    def put(n, col, val):
        n = n.copy()
        n[:, col] = val
        return n
    add("inf_component", floor_changed(lambda n: put(n, 1, np.inf)), _pred_floor_lit)

    def one_nan(n):
        n = n.copy()
        n[0::3, 0] = np.nan   # corner 0 of each floor triangle
        return n
    add("nan_component", floor_changed(one_nan), _pred_floor_ambient_ns)
    below = p.copy()
    below[17] = F32(-24.0)   # the light below the floor, on the side the flipped normals face
    add("flipped", floor_changed(lambda n: -n), _pred_flipped, params=below)

    def opposite(n):
        n = np.tile(np.array([0.0, 1.0, 0.0], F32), (n.shape[0], 1))
        n[1::3] = -n[1::3]   # corner 1 of each floor triangle: n1 = -n0
        return n
    add("n0_minus_n1", floor_changed(opposite), _pred_through_zero)
    return out


def _det_cases():
    out = []
    for name, pred, reg, kw in (("base", _pred_hits, "det", {}),
                                ("floor_y0", _pred_det_zero("floor"), None, {"fy": 0.0}),
                                ("slant_through_origin", _pred_det_zero("slant"), None, {"slant": True}),
                                ("floor_1e-6", _pred_det_small, None, {"fy": 1e-6}),
                                ("offset_1e4", _pred_hits, "det_1e4", {"offset": (1e4, 1e4, 1e4)})):
        s, p, tags = stage("open", **kw)
        out.append(_case("det", name, s, p, tags, pred, regular=reg))
    return out


NAN_WORDS = (0x7FC00000, 0xFFFFFFFF, 0x7F800001, 0xFFC00001)


def scrambled_materials(mats, seed=11):
    """The materials with every word other than .diffuse replaced by random bit patterns; the first
    words after the technique words get NaN patterns, the technique words random small integers
    (Mesh.h's technique enum among them)."""
    rng = np.random.default_rng(seed)
    m = np.array(mats, F32, copy=True)
    w = m.view(np.uint32)
    keep = w[:, 12:16].copy()
    w[:, :] = rng.integers(0, 2 ** 32, w.shape, dtype=np.uint64).astype(np.uint32)
    w[:, 0:4] = rng.integers(0, 4, (w.shape[0], 4)).astype(np.uint32)
    w[:, 4:8] = np.array(NAN_WORDS, np.uint32)
    w[:, 16:20] = np.array(NAN_WORDS, np.uint32)
    w[:, 12:16] = keep
    return m


def _albedo_cases():
    out = []
    s, p, tags = stage("open")

    def uniform(rgb):
        m = s["materials"].copy()
        m[:, DIFFUSE] = np.array(rgb, F32)
        return _with(s, materials=m)

    def add(name, scene, pred, regular=None):
        out.append(_case("albedo", name, scene, p, tags, pred, regular=regular))
    add("zero_and_minus_zero", uniform((0.0, -0.0, 0.5)), _pred_signed_zeros, regular="albedo")
    add("2_10_1e30", uniform((2.0, 10.0, 1e30)), _pred_channel(lambda c: c[:, 2] > 1e29))
    add("3e38", uniform((3e38, 1.0, 1.0)), _pred_channel(lambda c: np.isinf(c[:, 0])))
    add("minus_half", uniform((-0.5, 0.5, -0.5)), _pred_channel(lambda c: c[:, 0] < 0))
    add("nan", uniform((np.nan, 0.5, 0.25)), _pred_channel(lambda c: np.isnan(c[:, 0])))
    rs, rp, rtags = stage("room")   # the room shows all four materials
    m = rs["materials"].copy()
    m[3, DIFFUSE] = np.array((0.1, 0.8, 2.0), F32)
    multi = _with(rs, materials=m)
    out.append(_case("albedo", "several_materials", multi, rp, rtags, _pred_materials, regular="albedo"))
    out.append(_case("albedo", "several_materials_scrambled", _with(multi, materials=scrambled_materials(m)), rp, rtags,
                     _pred_materials))
    return out


GRADIENT_ALBEDO = 99.98265 / 76.5   # 0.3 * albedo * 255 just below 100: the faint light carries it across


def _pack_cases():
    out = []
    fy = -4.0
    s, p, tags = stage("open", light=(-3.0, fy + 6.0, 6.0))

    def uniform(scene, rgb):
        m = scene["materials"].copy()
        m[:, DIFFUSE] = np.array(rgb, F32)
        return _with(scene, materials=m)
    out.append(_case("pack", "past_one", uniform(s, (1.6, 1.0, 0.55)), p, tags, _pred_over_one))
    out.append(_case("pack", "negative", uniform(s, (-0.2, 0.5, -1.0)), p, tags, _pred_negative_packs_zero))
    # a light 0.003 above a floor with straight normals, behind the camera: NL falls from 8e-5 to 4e-5
    # across the floor, a gradient of a hundredth of one step of the packed value on top of the ambient
    # term, which crosses 100 some 40 units from the light
    s, p, tags = stage("open", light=(0.0, fy + 0.003, 45.0), tilt=0.0)
    out.append(_case("pack", "gradient", uniform(s, (GRADIENT_ALBEDO,) * 3), p, tags, _pred_gradient))
    return out


def _depth_cases():
    out = []
    s, p, tags = stage("room")
    out.append(_case("depth", "room_8", s, p, tags, _pred_depth_full, depth=8))
    out.append(_case("depth", "room_5", s, p, tags, _pred_depth_full, depth=5))
    s, p, tags = stage("open")
    out.append(_case("depth", "open_8", s, p, tags, _pred_depth_spread, depth=8))
    return out


def _box_cases():
    out = []
    s, p, tags = stage("open")

    def add(name, pred, lo=None, hi=None, scene=s, params=p, tg=tags):
        q = params.copy()
        if lo is not None:
            q[24:27] = np.array(lo, F32)
        if hi is not None:
            q[28:31] = np.array(hi, F32)
        out.append(_case("box", name, scene, q, tg, pred))
    lo, hi = p[24:27].copy(), p[28:31].copy()
    add("true", _pred_hits)
    add("half", _pred_box_both, hi=(-1.0, hi[1], hi[2]))
    rs, rp, rt = stage("room")
    add("camera_inside", _pred_hits, scene=rs, params=rp, tg=rt)
    add("flat", _pred_box_both, hi=(hi[0], lo[1], hi[2]))
    add("inverted", _pred_box_is_true, lo=hi, hi=lo)
    add("nan_word", _pred_box_both, hi=(hi[0], np.nan, hi[2]))
    return out


_CASES = []


def cases():
    """Every case, in class order (built once)."""
    if not _CASES:
        for make in (_light_cases, _normal_cases, _det_cases, _albedo_cases, _pack_cases, _depth_cases, _box_cases):
            _CASES.extend(make())
        assert len({c.label for c in _CASES}) == len(_CASES)
        assert all(c.scene["indices"].size // 3 <= 200 for c in _CASES)
    return _CASES


def labels():
    return [c.label for c in cases()]


def by_label(label):
    return next(c for c in cases() if c.label == label)


case = by_label


REGULAR_GROUPS = ["light", "normals", "albedo", "det", "det_1e4"]

# The labels of cases(), written out so that a test module can be parametrised without building a
# scene when it is collected (test_shading_edges.py asserts that the two lists are equal).
LABELS = [
    "light/below_floor", "light/in_floor_plane", "light/at_camera", "light/opposite_grazing", "light/skims_floor",
    "light/distance_1e6", "light/distance_1e30",
    "normals/zero", "normals/length_1e-3", "normals/length_1e3", "normals/length_1e-25", "normals/length_1e25",
    "normals/inf_component", "normals/nan_component", "normals/flipped", "normals/n0_minus_n1",
    "det/base", "det/floor_y0", "det/slant_through_origin", "det/floor_1e-6", "det/offset_1e4",
    "albedo/zero_and_minus_zero", "albedo/2_10_1e30", "albedo/3e38", "albedo/minus_half", "albedo/nan",
    "albedo/several_materials", "albedo/several_materials_scrambled",
    "pack/past_one", "pack/negative", "pack/gradient",
    "depth/room_8", "depth/room_5", "depth/open_8",
    "box/true", "box/half", "box/camera_inside", "box/flat", "box/inverted", "box/nan_word",
]
