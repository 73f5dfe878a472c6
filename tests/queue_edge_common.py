"""Shared by test_queue_edges.py (CPU), test_queue_edges_gpu.py and test_frame_scratch_gpu.py: frames
whose ray queues sit at the branch points of the wavefront path's machinery between bounces (DESIGN.md 6:
the segmented queues, their chunk and super-chunk sums, wf_compact_sort_kernel, the persistent bounce
kernel) and of the per-stream frame scratch around it.

The stage is a wall of panels.  The camera looks along -z, the image plane one unit in front of the eye
(volumeRender.cl:1169-1190, shading_edge_common.camera / primary_rays).  The FRONT wall lies in the
plane D = 10 in front of the eye, normal +z, and is made of rectangular panels given as pixel rectangles
[x0, x1) x [y0, y1): a panel covers exactly the primary rays of those pixels, so the caller chooses the
bounce-1 queue pixel by pixel.  The optional BACK wall, one quad of +-400 with normal -z one unit behind
the eye, sends the bounce-1 rays forward again; what returns to the front wall is spread 3.2 times as
wide, so the queue thins out bounce by bounce.  Two small anchor triangles far outside the view keep the
scene box large: every primary ray passes the box test even when no panel is in view.

Two pitfalls shape it:
 1. The stage stands off the origin (OFFSET).  get_normal_at_tri_point solves for the barycentrics by
    Cramer's rule on absolute positions (volumeRender.cl:35-43): a wall in a plane through the origin has
    a zero determinant, and every shading normal and reflected direction is NaN.  keys/nan_keys wants
    exactly that and no other case does.
 2. A ray that meets the shared diagonal of a panel's two triangles misses both.  Panel edges therefore
    lie BETWEEN ray positions and unequally far from them in x and y (pixel coordinates x0 - 0.7,
    x1 - 0.3, y0 - 0.6, y1 - 0.4), which keeps the diagonal of a square panel off the pixel centres.  A
    panel of odd width and odd height still has a pixel at its centre, where both diagonals pass, and gets
    x1 - 0.4; the back wall stands about the origin, not about the eye, for the same reason.  A huge quad
    can still lose a pixel, so every predicate is on what the oracle reports, not on what the geometry
    intended.

A Case is a scene, a Params block, a frame size, a depth and a predicate on the oracle's aux output;
tests/test_queue_edges.py asserts the predicates.  n_k is the number of rays traced at bounce k (pixels
whose hits[:, k, 0] != -2); n_{k+1} of them hit.  Everything is built once and shared: do not modify."""
import numpy as np

from shading_edge_common import DIFFUSE, DIFFUSE_W, F32, bits, camera, primary_rays   # noqa: F401

NO_SHADOW = 1
D_FRONT, D_BACK = 10.0, 1.0     # the front wall in front of the eye, the back wall behind it
OFFSET = (1.5, 2.5, -17.0)      # pitfall 1
HALF_WIDTH = 0.6
PITCH = 100.0                   # screens of one scene stand this far apart in x (a batch's frames)
LIGHT = (3.0, 4.0, -3.0)        # between the walls, relative to the first screen's eye
NOT_TRACED = -2                 # hits[:, k, 0] of a pixel with no ray at bounce k

# frame geometries: the smallest at which each structure has an edge (16 x 16 tiles, 4 segments of 64 slots
# each, chunks of 32 segments = 8 tiles, super-chunks of 1024 segments = 256 tiles)
G_SUPER = (256, 272)    # 16 x 17 tiles, 1088 segments, 34 chunks: super-chunk 0 full, super-chunk 1 two chunks
G_EXACT = (256, 256)    # exactly 1024 segments: the last chunk is chunk 31 of super-chunk 0, no super-chunk 1
G_RAGGED = (251, 259)   # G_SUPER's tile grid with partial tiles right and below: segments with lanes off the frame
G_CHUNK = (128, 16)     # 8 tiles, 32 segments: exactly one chunk
G_CHUNK_PLUS = (144, 16)   # 36 segments: one chunk and four segments
G_SMALL = (40, 24)      # 6 tiles, 24 segments: less than a chunk
G_ONE = (1, 1)
GEOMETRIES = {"super": G_SUPER, "exact": G_EXACT, "ragged": G_RAGGED, "chunk": G_CHUNK, "chunk+": G_CHUNK_PLUS,
              "small": G_SMALL, "one": G_ONE}
TILE, SEG_RAYS, CHUNK_SEGS, SUPER_SEGS = 16, 64, 32, 1024   # rt_render.hip: kBlockPx, kSegRays, kChunkSegs, kSuperSegs


# ---- segments (rt_render.hip: "Ray queues are SEGMENTED", first-bounce waves) ----

def tiles(w, h):
    return (w + TILE - 1) // TILE, (h + TILE - 1) // TILE


def num_segments(w, h, k=1):
    tx, ty = tiles(w, h)
    return 4 * tx * ty * k


def segment_of(x, y, w):
    """The bounce-1 segment of pixel (x, y): wave q of tile tb owns segment 4 tb + q."""
    tx = (w + TILE - 1) // TILE
    tb = (y // TILE) * tx + x // TILE
    q = ((y % TILE) // 8) * 2 + (x % TILE) // 8
    return 4 * tb + q


def segment_counts(mask, w, h):
    """Rays per bounce-1 segment of a (w*h,) hit mask."""
    y, x = np.divmod(np.arange(w * h), w)
    return np.bincount(segment_of(x, y, w)[np.asarray(mask, bool)], minlength=num_segments(w, h))


def segment_rect(seg, w, h):
    """The pixels of bounce-1 segment `seg`, clipped to the frame: (x0, y0, x1, y1)."""
    tx = (w + TILE - 1) // TILE
    tb, q = divmod(seg, 4)
    x0 = (tb % tx) * TILE + (q & 1) * 8
    y0 = (tb // tx) * TILE + (q >> 1) * 8
    return x0, y0, min(x0 + 8, w), min(y0 + 8, h)


def tile_rect(tb, w, h):
    tx = (w + TILE - 1) // TILE
    x0, y0 = (tb % tx) * TILE, (tb // tx) * TILE
    return x0, y0, min(x0 + TILE, w), min(y0 + TILE, h)


# ---- the stage ----

def _rows(w, h):
    """The whole view as one panel per tile row (no panel is square, none has a diagonal across the view)."""
    return [(0, y, w, min(y + TILE, h)) for y in range(0, h, TILE)]


def _wall_point(u, v, w, h, half_width, dist, shift=0.0):
    """Where the ray through pixel coordinate (u, v) meets the plane `dist` in front of the eye, relative
    to the eye (x right, y up); shift: how many pixels the camera's c is moved on (keys/key_clamp)."""
    u, v = u + shift, v + shift
    return (dist * half_width * (2.0 * (u - 0.5) / w - 1.0), -dist * half_width * (h / w) * (2.0 * (v - 0.5) / h - 1.0))


class _Geo:
    def __init__(self):
        self.v, self.n, self.mat = [], [], []

    def tri(self, p, n, mat):
        self.v += [np.asarray(q, np.float64) for q in p]
        self.n += [np.asarray(n, np.float64)] * 3
        self.mat.append(mat)

    def quad(self, p, n, mat):
        self.tri([p[0], p[1], p[2]], n, mat)
        self.tri([p[0], p[2], p[3]], n, mat)

    def front(self, x0, y0, x1, y1, z, ex=0.0):
        """A panel of the front wall (normal +z) over [x0, x1] x [y0, y1] around the eye at x = ex."""
        self.quad([(ex + x0, y0, z), (ex + x1, y0, z), (ex + x1, y1, z), (ex + x0, y1, z)], (0.0, 0.0, 1.0), 0)


_BVH = {}


def _tree(v, idx):
    key = v.tobytes()
    if key not in _BVH:
        import rtamd
        bvh = rtamd.Mesh.from_arrays(v, idx).build_lbvh(2)
        _BVH[key] = (bvh.nodes.copy(), bvh.tri_indices.copy())
    return _BVH[key]


def stage(screens, w, h, back=True, offset=OFFSET, half_width=HALF_WIDTH, front="panels", shift=0.0):
    """(scene arrays, [params of screen 0, 1, ...]).  screens: per screen its panels as pixel rectangles
    (x0, y0, x1, y1) of a w x h frame; screen i stands PITCH * i to the right and has its own camera, all
    cameras sharing the light and the scene box (what a batch launch demands).  w and h may be lists, one
    frame size per screen (frames of different sizes from one uploaded scene).  front "closed": the front
    wall is instead three quads that reach far beyond the view, laid out so that whatever a ray can reach
    in eight bounces lies inside ONE triangle (no diagonal crosses it)."""
    g = _Geo()
    z = -D_FRONT
    span = PITCH * (max(len(screens), 1) - 1)
    ws = list(w) if np.ndim(w) else [w] * max(len(screens), 1)
    hs = list(h) if np.ndim(h) else [h] * max(len(screens), 1)
    for i, panels in enumerate(screens):
        ex = PITCH * i
        w, h = ws[i], hs[i]
        for (x0, y0, x1, y1) in panels:
            assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h, (x0, y0, x1, y1)
            # a panel of odd width AND odd height has a pixel at its centre, where both diagonals pass:
            # its right edge lies at x1 - 0.4 instead, which moves the centre off the pixel
            right = 0.4 if (x1 - x0) % 2 and (y1 - y0) % 2 else 0.3
            wx0, wy0 = _wall_point(x0 - 0.7, y0 - 0.6, w, h, half_width, D_FRONT, shift)
            wx1, wy1 = _wall_point(x1 - right, y1 - 0.4, w, h, half_width, D_FRONT, shift)
            g.front(wx0, wy1, wx1, wy0, z, ex)   # wy1 < wy0: row 0 is at the top
    if front == "closed":
        assert len(screens) == 1 and not screens[0]
        # the main quad's diagonal runs from (-100, -700) to (700, 100), the line y = x - 600: the view and
        # all that the rays reach (within +-100 of the eye) lies in its upper-left triangle
        g.front(-100.0, -700.0, 700.0, 100.0, z)
        g.front(-700.0, -700.0, -100.0, 100.0, z)
        g.front(-700.0, 100.0, 700.0, 700.0, z)
    if back:
        # +-400 about the ORIGIN, not about the eye: its diagonal then passes one unit beside the camera's
        # axis, where no reflected ray of the pixel lattice meets it exactly (about the eye, 80 of G_SUPER's
        # 69,632 bounce-1 rays met it and missed both triangles)
        B = 400.0
        ox, oy = -np.asarray(offset, np.float64)[:2]
        R = B + span   # further screens: as much wider to the right
        g.quad([(ox - B, oy - B, D_BACK), (ox - B, oy + B, D_BACK), (ox + R, oy + B, D_BACK), (ox + R, oy - B, D_BACK)],
               (0.0, 0.0, -1.0), 1)
    for s in (-1.0, 1.0):   # the anchors
        p = np.array([450.0 * s + (span if s > 0 else 0.0), 450.0 * s, -40.0 if s < 0 else 8.0])
        g.tri([p, p + (1.0, 0.0, 0.0), p + (0.0, 1.0, 0.0)], (0.0, 0.0, 1.0), 0)
    off = np.asarray(offset, np.float64)
    nt = len(g.mat)
    v = np.zeros((3 * nt, 4), F32)
    v[:, :3] = (np.array(g.v) + off).astype(F32)
    n = np.zeros((3 * nt, 4), F32)
    n[:, :3] = np.array(g.n).astype(F32)
    idx = np.arange(3 * nt, dtype=np.int32)
    nodes, refs = _tree(v, idx)
    mats = np.zeros((2, 44), F32)
    mats[0, DIFFUSE], mats[1, DIFFUSE] = (0.7, 0.6, 0.5), (0.4, 0.6, 0.8)
    mats[:, DIFFUSE_W] = 1.0
    lo, hi = v[:, :3].min(axis=0), v[:, :3].max(axis=0)
    scene = {"vertices": v, "indices": idx, "nodes": nodes, "tri_indices": refs, "normals": n,
             "normals_indices": idx.copy(), "materials": mats, "tri_to_material": np.array(g.mat, np.int32),
             "scene_min": lo.copy(), "scene_max": hi.copy()}
    cams = []
    for i in range(max(len(screens), 1)):
        eye = off + (PITCH * i, 0.0, 0.0)
        a, b, c, campos = camera(eye, eye + (0.0, 0.0, -1.0), ws[i], hs[i], half_width)
        c = c + a * (shift / ws[i]) + b * (shift / hs[i])
        p = np.zeros(32, F32)
        p[0:3], p[4:7], p[8:11], p[12:15] = a, b, c, campos
        p[16:19] = (np.asarray(LIGHT) + off).astype(F32)
        p[20:24] = 1.0
        p[24:27], p[28:31] = lo, hi
        cams.append(p)
    return scene, cams


# ---- populations: (w, h) -> panels ----

def pop_empty(w, h):
    return []


def pop_full(w, h):
    return _rows(w, h)


def pop_one_first(w, h):
    return [(0, 0, 1, 1)]


def pop_one_last(w, h):
    return [(w - 1, h - 1, w, h)]


def pop_segments(segs):
    def pop(w, h):
        rects = [segment_rect(s, w, h) for s in segs if s < num_segments(w, h)]
        return [r for r in rects if r[0] < r[2] and r[1] < r[3]]   # a partial tile's segments may lie off the frame
    return pop


def pop_tiles(tbs):
    def pop(w, h):
        return [tile_rect(t, w, h) for t in tbs]
    return pop


def pop_chunks(chunks):
    """Whole chunks: chunk c is the tiles 8 c .. 8 c + 7, one panel per run of tiles in a tile row."""
    def pop(w, h):
        tx, ty = tiles(w, h)
        out = []
        for c in chunks:
            t = 8 * c
            while t < min(8 * c + 8, tx * ty):
                run = min(8 * c + 8, (t // tx + 1) * tx, tx * ty) - t
                x0, y0, _, y1 = tile_rect(t, w, h)
                out.append((x0, y0, min(x0 + run * TILE, w), y1))
                t += run
        return out
    return pop


def pop_lane_counts(w, h):
    """One rectangle a x b at the origin of every 8 x 8 quadrant, a = seg % 9, b = (seg // 9) % 9."""
    out = []
    for s in range(num_segments(w, h)):
        a, b = s % 9, (s // 9) % 9
        x0, y0, x1, y1 = segment_rect(s, w, h)
        if a and b and x0 < w and y0 < h:
            out.append((x0, y0, min(x0 + a, x1), min(y0 + b, y1)))
    return out


def pop_every_other_tile(w, h):
    tx, ty = tiles(w, h)
    return [tile_rect(t, w, h) for t in range(tx * ty) if (t % tx + t // tx) % 2 == 0]


def pop_centre_quadrant(w, h):
    return [(w // 2 - 4, h // 2 - 4, w // 2 + 4, h // 2 + 4)]


# ---- cases ----

class Case:
    def __init__(self, cls, name, geo, scene, params, depth, back, predicate, size=None):
        self.cls, self.name, self.geo = cls, name, geo
        self.label = f"{cls}/{name}@{geo}"
        self.w, self.h = GEOMETRIES[geo] if size is None else size   # size: a frame size that is no named geometry
        self.scene, self.params, self.depth, self.back, self.predicate = scene, params, depth, back, predicate


_FRAMES = {}


def render_oracle(scene, params, w, h, depth, flags=0):
    from oracle import oracle
    return oracle.render(scene, params, w, h, depth=depth, flags=flags)


def oracle_frame(case, depth=None, flags=0):
    """The oracle's frame of a case at a depth (None: the case's own), computed once (shared; do not modify)."""
    depth = case.depth if depth is None else depth
    key = (case.label, depth, flags)
    if key not in _FRAMES:
        _FRAMES[key] = render_oracle(case.scene, case.params, case.w, case.h, depth, flags)
    return _FRAMES[key]


def frames(case):
    """The oracle's frames of a case: "d" at the case's depth, "ns" the same without the shadow ray; each
    oracle.render's dict (out, hits, t, rgb, stats)."""
    return {"d": oracle_frame(case), "ns": oracle_frame(case, flags=NO_SHADOW)}


def n_traced(frame):
    """[n_0, n_1, ...]: rays traced at each bounce."""
    return [int(np.sum(frame["hits"][:, k, 0] != NOT_TRACED)) for k in range(frame["hits"].shape[1])]


def n_of(case):
    """n_0 .. n_depth: the rays traced at each bounce, then the rays that hit at the last one."""
    f = frames(case)["d"]
    return n_traced(f) + [int(np.sum(f["hits"][:, -1, 0] >= 0))]


def queue1(case):
    """The bounce-1 queue's per-segment counts."""
    f = frames(case)["d"]
    return segment_counts(f["hits"][:, 0, 0] >= 0, case.w, case.h)


def _chunk_counts(seg):
    pad = (-len(seg)) % CHUNK_SEGS
    return np.concatenate([seg, np.zeros(pad, seg.dtype)]).reshape(-1, CHUNK_SEGS).sum(axis=1)


def _ns(*want):
    """n_1, n_2, ... begin with `want`."""
    def pred(case):
        n = n_of(case)
        return n[0] == case.w * case.h and tuple(n[1:1 + len(want)]) == tuple(want)
    return pred


def _pred_empty(case):
    return _ns(0)(case) and all(v == 0 for v in n_of(case)[1:])


def _pred_one(pixel_of, back):
    def pred(case):
        f = frames(case)["d"]
        hit = np.flatnonzero(f["hits"][:, 0, 0] >= 0)
        return hit.tolist() == [pixel_of(case)] and (_ns(1, 1, 0) if back else _ns(1, 0))(case)
    return pred


def _pred_one_segment(seg):
    def pred(case):
        q = queue1(case)
        return q[seg] == 64 and q.sum() == 64 and _ns(64, 64, 0)(case)
    return pred


def _pred_chunks(full):
    """Exactly these chunks hold rays, and they are full (a partial tile's segments as full as the frame lets them be)."""
    def pred(case):
        q = queue1(case)
        whole = segment_counts(np.ones(case.w * case.h, bool), case.w, case.h)
        want = np.zeros_like(q)
        for c in full:
            want[CHUNK_SEGS * c:CHUNK_SEGS * (c + 1)] = whole[CHUNK_SEGS * c:CHUNK_SEGS * (c + 1)]
        return np.array_equal(q, want) and q.sum() > 0
    return pred


def _pred_last_super(case):
    q = queue1(case)
    return q[:SUPER_SEGS].sum() == 0 and np.all(q[SUPER_SEGS:] == 64) and len(q) > SUPER_SEGS


def _pred_super_ends(case):
    q = queue1(case)
    last = len(q) - 1
    return last == 1087 and q[0] > 0 and q[last] > 0 and q[1:last].sum() == 0


def _pred_segment_checker(case):
    q = queue1(case)
    return np.all(q[1::2] == 64) and np.all(q[0::2] == 0)


def _pred_lane_counts(case):
    q = queue1(case)
    vals = set(q.tolist())
    per_chunk = [len(set(q[i:i + CHUNK_SEGS].tolist())) for i in range(0, len(q), CHUNK_SEGS)]
    return len(vals) >= 24 and {0, 1, 64} <= vals and min(per_chunk) >= 3


def _pred_full(case):
    n = n_of(case)
    return n[0] == case.w * case.h and n[1] == case.w * case.h


def _pred_closed(case):
    n = n_of(case)
    return case.depth == 8 and all(v >= case.w * case.h - 4 for v in n[:8])


def _pred_thinning(case):
    n = n_of(case)
    return case.depth == 8 and n[1] > n[3] > n[5] > n[7] > 0 and any(v % 64 for v in n[3:8])


def _pred_dies_at(k):
    def pred(case):
        n = n_of(case)
        return case.depth == 8 and n[k] == 0 < n[k - 1] and all(v == 0 for v in n[k:])
    return pred


def _pred_below_one_wave(case):
    n = n_of(case)
    return case.depth == 8 and any(0 < n[k + 1] < 64 <= n[k] for k in range(1, 8))


# -- sort keys --

def thin_axis(params):
    """The sort key's axis as the host chooses it from the caller's params (rt_render.hip, render_frames:
    "the local sort's key axis: the scene box's thinnest", ties to y), in float32."""
    p = np.asarray(params, F32)
    ext = (p[28:31] - p[24:27]).astype(F32)
    return 1 if ext[1] <= ext[0] and ext[1] <= ext[2] else 2 if ext[2] < ext[0] else 0


def keys_of_queue1(case, scale):
    """The bucket of every bounce-1 ray as wf_compact_sort_kernel computes it, restated in float64 from the
    primary directions and the front wall's normal: r = d - 2 (d.n) n, floor((r_axis + 1) * scale) clamped
    to [0, 2 scale - 1].  (Also the unclamped value.)"""
    f = frames(case)["d"]
    hit = f["hits"][:, 0, 0] >= 0
    _, d = primary_rays(case.params, case.w, case.h)
    n = np.array([0.0, 0.0, 1.0])
    r = d[hit] - 2.0 * (d[hit] @ n)[:, None] * n[None, :]
    raw = np.floor((r[:, thin_axis(case.params)] + 1.0) * scale).astype(np.int64)
    return np.clip(raw, 0, 2 * scale - 1), raw


def _pred_axis(axis):
    def pred(case):
        return thin_axis(case.params) == axis and _pred_full(case)
    return pred


def _pred_axis_tie(case):
    p = np.asarray(case.params, F32)
    ext = (p[28:31] - p[24:27]).astype(F32)
    return ext[0] == ext[1] == ext[2] and thin_axis(case.params) == 1 and _pred_full(case)


def _pred_one_bucket(case):
    """One bucket of the 8; with the batch key's 16 buckets the queue cannot stay in one (the view's corner
    rays lean 41 degrees), so there it is the top two."""
    k4, _ = keys_of_queue1(case, 4)
    k8, _ = keys_of_queue1(case, 8)
    return len(set(k4.tolist())) == 1 and set(k8.tolist()) <= {14, 15} and _pred_full(case)


def _pred_all_buckets(case):
    k4, _ = keys_of_queue1(case, 4)
    k8, _ = keys_of_queue1(case, 8)
    return set(k4.tolist()) == set(range(8)) and set(k8.tolist()) == set(range(16)) and _pred_full(case)


def clamp_pixel(case):
    return (case.h // 2) * case.w + case.w // 2


def _pred_key_clamp(case):
    """The primary ray of the centre pixel is exactly (0, 0, -1) in float32 as in float64 (the camera's words
    are powers of two and c is shifted by half a pixel); the front wall's normals are exactly (0, 0, 1), so
    get_normal_at_tri_point's weighted sum has x = y = 0 exactly and normalize returns (0, 0, 1) (z / sqrt(z z)
    is 1 for a correctly rounded sqrt), and reflect gives d - 2 (d.n) n = (0, 0, 1) exactly: (1 + 1) * scale
    is 2 * scale, one past the last bucket.  The oracle's output shows the rest: the pixel hits the front wall
    and its bounce-1 ray goes straight back, meeting the back wall D_FRONT + D_BACK further on (less the two
    0.001 steps off the surfaces)."""
    f = frames(case)["d"]
    pix = clamp_pixel(case)
    p = np.asarray(case.params, F32)
    x, y = F32(case.w // 2), F32(case.h // 2)
    pos = p[8:11] + p[0:3] * ((x - F32(0.5)) / F32(case.w)) + p[4:7] * ((y - F32(0.5)) / F32(case.h))
    d32 = (pos - p[12:15]).astype(F32)
    _, d64 = primary_rays(case.params, case.w, case.h)
    _, raw = keys_of_queue1(case, 4)
    hit = np.flatnonzero(f["hits"][:, 0, 0] >= 0)
    at = int(np.searchsorted(hit, pix))
    front = np.all(case.scene["normals"][case.scene["normals_indices"][f["hits"][pix, 0, 0]:][:3], :3] == (0.0, 0.0, 1.0))
    return (d32.tolist() == [0.0, 0.0, -1.0] and d64[pix].tolist() == [0.0, 0.0, -1.0] and hit[at] == pix
            and raw[at] == 8 and raw.max() == 8 and front and f["hits"][pix, 1, 0] >= 0
            and abs(float(f["t"][pix, 1]) - (D_FRONT + D_BACK - 0.002)) < 1e-4 and _pred_full(case))


def _pred_nan_keys(case):
    f = frames(case)["d"]
    n = n_of(case)
    det = np.linalg.det(case.scene["vertices"][:3 * 2, :3].astype(np.float64).reshape(2, 3, 3))   # a panel's two triangles
    return n[1] > 0 and n[2] == 0 and bool(np.all(det == 0.0)) and f["hits"].shape[1] == 3


def _with_box(params, lo, hi):
    q = params.copy()
    q[24:27], q[28:31] = np.array(lo, F32), np.array(hi, F32)
    return q


STARRED = ("super", "exact", "ragged", "small")
CLASSES = ["pop", "depth", "keys"]


def _build():
    out = []

    def add(cls, name, geo, pop, pred, depth=3, back=True, **kw):
        w, h = GEOMETRIES[geo]
        scene, cams = stage([pop(w, h)], w, h, back=back, **kw)
        c = Case(cls, name, geo, scene, cams[0], depth, back, pred)
        out.append(c)
        return c
    for geo in STARRED + ("one",):
        add("pop", "empty", geo, pop_empty, _pred_empty)
    for geo in STARRED:
        add("pop", "one_first", geo, pop_one_first, _pred_one(lambda c: 0, False), back=False)
        add("pop", "one_last", geo, pop_one_last, _pred_one(lambda c: c.w * c.h - 1, True))
    add("pop", "one_segment", "super", pop_segments([403]), _pred_one_segment(403))
    add("pop", "one_chunk", "super", pop_chunks([5]), _pred_chunks([5]))
    add("pop", "one_chunk", "chunk", pop_chunks([0]), _pred_chunks([0]))
    add("pop", "one_chunk", "chunk+", pop_chunks([0]), _pred_chunks([0]))
    add("pop", "one_chunk_reverse", "chunk+", pop_chunks([1]), _pred_chunks([1]))
    add("pop", "last_super", "super", pop_chunks([32, 33]), _pred_last_super)
    add("pop", "super_ends", "super", pop_segments([0, 1087]), _pred_super_ends)
    add("pop", "chunk_checker", "super", pop_chunks(range(1, 34, 2)), _pred_chunks(range(1, 34, 2)))
    add("pop", "segment_checker", "super", pop_segments(range(1, 1088, 2)), _pred_segment_checker)
    add("pop", "lane_counts", "super", pop_lane_counts, _pred_lane_counts)
    for geo in STARRED + ("one",):
        add("pop", "full", geo, pop_full, _pred_full)
    add("depth", "closed", "super", pop_empty, _pred_closed, depth=8, front="closed")
    add("depth", "thinning", "super", pop_full, _pred_thinning, depth=8)
    add("depth", "dies_at_2", "super", pop_full, _pred_dies_at(2), depth=8, back=False)
    add("depth", "dies_at_3", "super", pop_chunks([32, 33]), _pred_dies_at(3), depth=8)
    add("depth", "below_one_wave", "super", pop_centre_quadrant, _pred_below_one_wave, depth=8)
    # sort keys: the full stage, the CALLER'S box enlarged (more rays pass the box test, none fewer)
    full = add("keys", "one_bucket", "super", pop_full, _pred_one_bucket)
    lo, hi = full.params[24:27].astype(np.float64), full.params[28:31].astype(np.float64)
    assert thin_axis(full.params) == 2
    for name, axis, blo, bhi in (("axis_x", 0, (lo[0], -3000.0, -3000.0), (hi[0], 3000.0, 3000.0)),
                                 ("axis_y", 1, (-3000.0, lo[1], -3000.0), (3000.0, hi[1], 3000.0)),
                                 ("axis_z", 2, (-3000.0, -3000.0, lo[2]), (3000.0, 3000.0, hi[2]))):
        out.append(Case("keys", name, "super", full.scene, _with_box(full.params, blo, bhi), 3, True, _pred_axis(axis)))
    out.append(Case("keys", "axis_tie", "super", full.scene, _with_box(full.params, (-1024.0,) * 3, (1024.0,) * 3), 3, True,
                    _pred_axis_tie))
    wide = add("keys", "all_buckets", "super", pop_full, _pred_all_buckets, half_width=4.0)
    wlo, whi = wide.params[24:27].astype(np.float64), wide.params[28:31].astype(np.float64)
    wide.params = _with_box(wide.params, (wlo[0], -3000.0, -3000.0), (whi[0], 3000.0, 3000.0))   # sorted along x
    add("keys", "key_clamp", "exact", pop_full, _pred_key_clamp, half_width=0.5, shift=0.5)   # c half a pixel on
    add("keys", "nan_keys", "super", pop_full, _pred_nan_keys, offset=(1.5, 2.5, D_FRONT))   # the front wall in z = 0
    assert len({c.label for c in out}) == len(out)
    return out


_CASES = []


def cases():
    if not _CASES:
        _CASES.extend(_build())
    return _CASES


def labels():
    return [c.label for c in cases()]


def case(label):
    return next(c for c in cases() if c.label == label)


# The labels of cases(), written out so that a test module can be parametrised without building a scene
# when it is collected (test_queue_edges.py asserts that the two lists are equal).
LABELS = [
    "pop/empty@super", "pop/empty@exact", "pop/empty@ragged", "pop/empty@small", "pop/empty@one",
    "pop/one_first@super", "pop/one_last@super", "pop/one_first@exact", "pop/one_last@exact",
    "pop/one_first@ragged", "pop/one_last@ragged", "pop/one_first@small", "pop/one_last@small",
    "pop/one_segment@super", "pop/one_chunk@super", "pop/one_chunk@chunk", "pop/one_chunk@chunk+",
    "pop/one_chunk_reverse@chunk+", "pop/last_super@super", "pop/super_ends@super", "pop/chunk_checker@super",
    "pop/segment_checker@super", "pop/lane_counts@super",
    "pop/full@super", "pop/full@exact", "pop/full@ragged", "pop/full@small", "pop/full@one",
    "depth/closed@super", "depth/thinning@super", "depth/dies_at_2@super", "depth/dies_at_3@super",
    "depth/below_one_wave@super",
    "keys/one_bucket@super", "keys/axis_x@super", "keys/axis_y@super", "keys/axis_z@super", "keys/axis_tie@super",
    "keys/all_buckets@super", "keys/key_clamp@exact", "keys/nan_keys@super",
]


# ---- a batch's frames: different populations under one camera set ----

BATCH_POPS = [("empty", pop_empty), ("full", pop_full), ("one_last", pop_one_last), ("lane_counts", pop_lane_counts),
              ("every_other_tile", pop_every_other_tile), ("one_first", pop_one_first), ("centre", pop_centre_quadrant),
              ("segment_checker", pop_segments(range(1, 1088, 2)))]
_BATCH = {}


def batch_stage(w, h, k):
    """One scene with k screens side by side, each its own population, and the k cameras (one light, one
    scene box): (scene, [params], [population names])."""
    if (w, h, k) not in _BATCH:
        pops = BATCH_POPS[:k]
        scene, cams = stage([p(w, h) for _, p in pops], w, h)
        _BATCH[(w, h, k)] = (scene, cams, [n for n, _ in pops])
    return _BATCH[(w, h, k)]


_BATCH_FRAMES = {}


def batch_frames(w, h, k, depth):
    """The oracle's frame of every camera of batch_stage(w, h, k) (shared; do not modify)."""
    key = (w, h, k, depth)
    if key not in _BATCH_FRAMES:
        scene, cams, _ = batch_stage(w, h, k)
        _BATCH_FRAMES[key] = [render_oracle(scene, p, w, h, depth) for p in cams]
    return _BATCH_FRAMES[key]


_EXTRA = {}


def extra_case(name, w, h, pop, depth=3, back=True, **kw):
    """A case outside the list (a frame-scratch test's own size), built once: its label is name@WxH."""
    key = f"{name}@{w}x{h}"
    if key not in _EXTRA:
        scene, cams = stage([pop(w, h)], w, h, back=back, **kw)
        c = Case("extra", name, f"{w}x{h}", scene, cams[0], depth, back, None, size=(w, h))
        _EXTRA[key] = c
    return _EXTRA[key]


def camera_params(base, w, h, dx=0.0, half_width=HALF_WIDTH):
    """`base` (a stage's params) with the camera of a w x h frame in its place, the eye moved dx to the right:
    any frame size of one scene (the panels stay where the stage's own size put them)."""
    p = np.array(base, F32, copy=True)
    eye = np.asarray(OFFSET, np.float64) + (dx, 0.0, 0.0)
    a, b, c, campos = camera(eye, eye + (0.0, 0.0, -1.0), w, h, half_width)
    p[0:3], p[4:7], p[8:11], p[12:15] = a, b, c, campos
    return p


# ---- on the GPU ----

SENTINEL = 0x12345678   # fills every output buffer before a frame: a finite float, no hit id, no pixel of these stages


def put(renderer, scene, params):
    import rtamd
    renderer.upload(rtamd.Scene.from_arrays(scene))
    renderer.set_params(params)


class Pending:
    """A frame enqueued by enqueue(): its sentinel-filled device buffers; get() waits and reads them back."""

    def __init__(self, stream, npx, depth, aux):
        import torch
        self.stream, self.npx, self.depth = stream, npx, depth
        d = max(depth, 1)
        with torch.cuda.stream(stream):
            def buf(n):
                return torch.full((max(n, 1),), SENTINEL, dtype=torch.int32, device="cuda")
            self.out = buf(npx)
            self.aux = (buf(npx * d * 2), buf(npx * d), buf(npx * 3)) if aux else None

    def get(self):
        self.stream.synchronize()
        res = {"out": self.out.cpu().numpy().view(np.uint32)[:self.npx]}
        if self.aux:
            d = max(self.depth, 1)
            res["hits"] = self.aux[0].cpu().numpy().reshape(self.npx, d, 2)[:, :self.depth]
            res["t"] = self.aux[1].cpu().numpy().view(F32).reshape(self.npx, d)[:, :self.depth]
            res["rgb"] = self.aux[2].cpu().numpy().view(F32).reshape(self.npx, 3)
        return res


def enqueue(renderer, w, h, depth, flags, stream, tiling=None, aux=True):
    """rt_render_device on the torch stream `stream` with the renderer's current params, into buffers filled
    with SENTINEL on that stream; returns at once (a Pending)."""
    import rtamd
    npx = w * h if tiling is None else rtamd.tiling_pixels(w, h, tiling.rank, tiling.nranks, tiling.band_rows)
    pend = Pending(stream, npx, depth, aux)
    renderer.render_device(w, h, depth, flags, pend.out.data_ptr(), tiling=tiling, stream=stream.cuda_stream,
                           aux_ptrs=None if not aux else tuple(t.data_ptr() for t in pend.aux))
    return pend


def render(renderer, w, h, depth, flags, stream, tiling=None, aux=True):
    return enqueue(renderer, w, h, depth, flags, stream, tiling, aux).get()


def band_pixels(w, h, tiling):
    """The frame's pixel indices of a rank's bands, in its buffer's order."""
    import rtamd
    rows = [np.arange(y0, y0 + n) for y0, n in rtamd.rank_bands(h, tiling.rank, tiling.nranks, tiling.band_rows)]
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return (rows[:, None] * w + np.arange(w)[None, :]).reshape(-1)


def rows_of(frame, idx):
    return {k: v[idx] for k, v in frame.items() if k in ("out", "hits", "t", "rgb")}


def same_rgb(got, want):
    """Bit for bit; where `want` is NaN, `got` is NaN (payload and sign not compared)."""
    nan = np.isnan(want)
    return np.where(nan, np.isnan(got), bits(got) == bits(want))


def same_frame(got, want, label):
    """Every word of hits, t, rgb (where both have them) and the packed pixels; no sentinel is left."""
    assert not np.any(got["out"] == SENTINEL), f"{label}: {int(np.sum(got['out'] == SENTINEL))} pixels never written"
    if "hits" in got and "hits" in want:
        assert got["hits"].shape == want["hits"].shape, f"{label}: {got['hits'].shape} vs {want['hits'].shape}"
        bad = np.argwhere(got["hits"] != want["hits"])
        assert bad.size == 0, (f"{label}: {len(bad)} hit ids differ ({int(np.sum(got['hits'] == SENTINEL))} never written), "
                               f"first at {bad[:3].tolist()}")
        bad = np.argwhere(bits(got["t"]) != bits(want["t"]))
        assert bad.size == 0, f"{label}: {len(bad)} t differ, first at {bad[:3].tolist()}"
        bad = np.argwhere(~same_rgb(got["rgb"], want["rgb"]))
        assert bad.size == 0, (f"{label}: {len(bad)} rgb words differ, first at {bad[:3].tolist()}: "
                               f"{got['rgb'][bad[0, 0]]} vs {want['rgb'][bad[0, 0]]}")
    bad = np.flatnonzero(got["out"] != want["out"])
    assert bad.size == 0, f"{label}: {bad.size} packed pixels differ, first {bad[:3]}: " \
                          f"{[hex(v) for v in got['out'][bad[:3]]]} vs {[hex(v) for v in want['out'][bad[:3]]]}"
