"""Ray queries: what rt_trace_rays_device costs against the frame kernel that traces
the same rays.

On one config's scene (default C3, the 1M-triangle heightfield, 1080p) on one GPU, alternating in
one session, medians of --reps after --warmup rounds, kernel times from HIP events:
  frame      the frame's primary rays alone: rt_render_device, depth 1, RT_FLAG_NO_SHADOW
             (rt_last_timing's kernel time) -- the yardstick
  closest    the same rays as an rt_ray buffer, closest hit (rt_last_query_timing), in the frame
             kernel's order (a 64-ray group = an 8 x 8 pixel tile) and in row-major pixel order
  any        the tile-ordered buffer with RT_FLAG_ANY_HIT
  incoherent as many rays with uniform origins in the scene box, aimed at uniform points in it
Each as ms and Mrays/s, the closest / frame ratio, and the time the query's own traffic (32 B in,
8 B out per ray) takes at the stream-copy rate measured here.  Writes one JSON file.
  attr_*     every buffer again through rt_trace_rays_attr_device, alternating with its
             plain query: ms, Mrays/s and attribute / plain; its extra traffic is 56 B more out per ray
             and 112 B more in per hit ray

    python scripts/ray_query_bench.py [--config c3] [--reps 20] [--warmup 5] [--flags 0] [--out profiles/ray_query/c3.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-opencl-raytracer_amd"))


def primary_rays(p, w, h):
    """The frame's primary rays (volumeRender.cl:1169-1190) in row-major pixel order, float64 then
    rounded: within an ulp of the kernel's own (this is a timing, not a parity check)."""
    a, b, c, campos = (p[k:k + 3].astype(np.float64) for k in (0, 4, 8, 12))
    xf = ((np.arange(w) - 0.5) / w).astype(np.float32).astype(np.float64)
    yf = ((np.arange(h) - 0.5) / h).astype(np.float32).astype(np.float64)
    ip = c[None, None, :] + a[None, None, :] * xf[None, :, None] + b[None, None, :] * yf[:, None, None]
    o = ip.astype(np.float32).reshape(-1, 3)
    return o, (o.astype(np.float64) - campos[None, :]).astype(np.float32)


def tile_order(w, h):
    """Pixel indices in the frame kernel's order: 8 x 8 tiles row by row, Morton order inside a tile."""
    k = np.arange(64)
    mx = (k & 1) | ((k >> 1) & 2) | ((k >> 2) & 4)
    my = ((k >> 1) & 1) | ((k >> 2) & 2) | ((k >> 3) & 4)
    ty, tx = np.meshgrid(np.arange(0, h, 8), np.arange(0, w, 8), indexing="ij")
    x = (tx.reshape(-1, 1) + mx[None, :]).reshape(-1)
    y = (ty.reshape(-1, 1) + my[None, :]).reshape(-1)
    keep = (x < w) & (y < h)
    return (y[keep] * w + x[keep]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--flags", type=int, default=0, help="math flags for the frame and the queries")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import rtamd
    from rtamd import configs
    cfg = configs.CONFIGS[a.config]
    w, h = cfg["w"], cfg["h"]
    mesh, bvh, build_s = configs.make_scene(cfg, via_dae=False)
    scene = rtamd.Scene.from_mesh(mesh, bvh)
    p = rtamd.params_to_array(mesh.camera_params(w, h))
    r = rtamd.Renderer(0)
    r.upload(scene)
    r.set_params(p)
    n = w * h
    o, d = primary_rays(p, w, h)
    order = tile_order(w, h)
    assert order.size == n and np.array_equal(np.sort(order), np.arange(n))
    lo, hi = p[24:27], p[28:31]
    rng = np.random.default_rng(18)
    io = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    idir = (rng.uniform(lo, hi, (n, 3)).astype(np.float32) - io).astype(np.float32)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def dev(rays):
        return torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()

    bufs = {"closest_tiled": (dev(rtamd.pack_rays(o[order], d[order])), False),
            "closest_rowmajor": (dev(rtamd.pack_rays(o, d)), False),
            "any_tiled": (dev(rtamd.pack_rays(o[order], d[order])), True),
            "incoherent": (dev(rtamd.pack_rays(io, idir)), False)}
    d_hits = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    d_attr = torch.zeros(16 * n, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_copy = torch.zeros(40 * n, dtype=torch.uint8, device="cuda")
    d_copy2 = torch.zeros(40 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = {k: [] for k in ["frame", "copy40"] + list(bufs) + ["attr_" + k for k in bufs]}
    hits = {}
    fflags = a.flags | rtamd.RT_FLAG_NO_SHADOW
    for it in range(a.warmup + a.reps):
        r.render_device(w, h, 1, fflags, d_out.data_ptr(), stream=s)
        ms["frame"].append(r.last_timing()[1])
        for k, (buf, any_hit) in bufs.items():
            r.trace_rays_device(buf.data_ptr(), n, d_hits.data_ptr(), any_hit=any_hit, flags=a.flags, stream=s)
            ms[k].append(r.last_query_ms())
            r.trace_rays_attr_device(buf.data_ptr(), n, d_attr.data_ptr(), any_hit=any_hit, flags=a.flags, stream=s)
            ms["attr_" + k].append(r.last_query_ms())
            if it == 0:
                hits[k] = int((d_hits[0::2] >= 0).sum().item())
                hits["attr_" + k] = int((d_attr[0::16] >= 0).sum().item())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):   # 40 B per ray read and written: twice the query's own traffic
            e0.record()
            d_copy2.copy_(d_copy)
            e1.record()
        stream.synchronize()
        ms["copy40"].append(e0.elapsed_time(e1))
    deferred = r.last_deferred()
    r.close()
    med = {k: statistics.median(v[a.warmup:]) for k, v in ms.items()}
    res = {"config": a.config, "flags": a.flags, "width": w, "height": h, "rays": n, "triangles": scene.num_triangles,
           "bvh": "SplitBVHBuilder (the config's)", "bvh_build_s": round(build_s, 2), "reps": a.reps, "warmup": a.warmup,
           "library": rtamd.library_digest(),
           "frame_primary_only_kernel_ms": round(med["frame"], 4),
           "frame_mrays_per_s": round(n / med["frame"] / 1e3, 1),
           "query_traffic_ms_at_copy_rate": round(med["copy40"] / 2.0, 4),
           "copy_gbs": round(2 * 40 * n / med["copy40"] / 1e6, 1),
           "closest_over_frame": round(med["closest_tiled"] / med["frame"], 3),
           "closest_over_frame_plus_traffic": round(med["closest_tiled"] / (med["frame"] + med["copy40"] / 2.0), 3),
           "last_deferred": deferred}
    for k in bufs:
        res[k] = {"ms": round(med[k], 4), "mrays_per_s": round(n / med[k] / 1e3, 1), "hits": hits[k],
                  "min_ms": round(min(ms[k][a.warmup:]), 4), "max_ms": round(max(ms[k][a.warmup:]), 4)}
    for k in bufs:
        ka = "attr_" + k
        res[ka] = {"ms": round(med[ka], 4), "mrays_per_s": round(n / med[ka] / 1e3, 1), "hits": hits[ka],
                   "min_ms": round(min(ms[ka][a.warmup:]), 4), "max_ms": round(max(ms[ka][a.warmup:]), 4),
                   "over_plain": round(med[ka] / med[k], 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
