"""Closest-point queries: what rt_closest_points_device costs, beside rt_trace_rays_device
(closest hit) on the frame's rays in the matching order as the scale a reader already knows.

On one config's scene (default C3, the 1M-triangle heightfield, 1080p, SBVH) on one GPU.  Point sets of
w * h points: (1) the frame's hit points from rt_trace_rays_attr lifted by 0.5 along ng (a ray that
missed keeps its origin), in the frame kernel's tile order; (2) the same in row-major order; (3) the
same under a fixed shuffle; (4) uniform in the scene box, r = +inf; (5) uniform in the scene box, r = 1 %
of the diagonal.  One session, alternating, medians of --reps after --warmup rounds, kernel ms from HIP
events (rt_last_query_timing).  Beside each: the host twin's mean inner visits and triangle tests per
point over every --sample-th point, so that a reader can see whether time follows visits.  Writes one
JSON file.

    python scripts/closest_bench.py [--config c3] [--reps 20] [--warmup 5] [--sample 16] [--out profiles/closest/c3.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-opencl-raytracer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ray_query_bench import primary_rays, tile_order   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16)
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
    o, d = primary_rays(p, w, h)
    n = w * h
    attr = r.trace_rays_attr(o, d)
    hit = attr["id"] >= 0
    lifted = np.where(hit[:, None], attr["p"] + np.float32(0.5) * attr["ng"], o).astype(np.float32)
    v = scene.vertices[:, :3]
    lo, hi = v.min(0), v.max(0)
    diag = float(np.sqrt(np.sum((hi.astype(np.float64) - lo) ** 2)))
    uniform = np.random.default_rng(22).uniform(lo, hi, (n, 3)).astype(np.float32)
    tile, rowmajor, shuffle = tile_order(w, h), np.arange(n), np.random.default_rng(21).permutation(n)
    inf = np.float32(np.inf)
    sets = [("hit_points_tile", lifted[tile], inf, tile), ("hit_points_rowmajor", lifted, inf, rowmajor),
            ("hit_points_shuffle", lifted[shuffle], inf, shuffle), ("uniform_r_inf", uniform, inf, shuffle),
            ("uniform_r_1pct", uniform, np.float32(0.01 * diag), shuffle)]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()

    d_out = torch.zeros(8 * n, dtype=torch.int32, device="cuda")
    d_hits = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    bufs = {}
    for name, q, rad, order in sets:
        bufs[name] = (dev(rtamd.pack_points(q, rad)), dev(rtamd.pack_rays(o[order], d[order])))
    torch.cuda.synchronize()
    ms = {(name, form): [] for name, _, _, _ in sets for form in ("closest", "rays")}
    for _ in range(a.warmup + a.reps):
        for name, _, _, _ in sets:
            d_pts, d_rays = bufs[name]
            r.closest_points_device(d_pts.data_ptr(), n, d_out.data_ptr(), stream=s)
            ms[(name, "closest")].append(r.last_query_ms())
            r.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=s)
            ms[(name, "rays")].append(r.last_query_ms())
    rows = []
    for name, q, rad, _ in sets:
        d_pts, _ = bufs[name]
        r.closest_points_device(d_pts.data_ptr(), n, d_out.data_ptr(), stream=s)
        stream.synchronize()
        found = float((d_out[0::8] >= 0).float().mean().item())
        sub = np.ascontiguousarray(q[::a.sample])
        _, st = rtamd.closest_points_host(scene, rtamd.pack_points(sub, rad), stats=True)
        c, t = (ms[(name, form)][a.warmup:] for form in ("closest", "rays"))
        mc, mt = statistics.median(c), statistics.median(t)
        rows.append({"set": name, "points": n, "found_share": round(found, 4),
                     "closest_ms": round(mc, 4), "closest_mpoints_per_s": round(n / mc / 1e3, 1),
                     "closest_min_ms": round(min(c), 4), "closest_max_ms": round(max(c), 4),
                     "rays_ms": round(mt, 4), "rays_mrays_per_s": round(n / mt / 1e3, 1),
                     "rays_min_ms": round(min(t), 4), "rays_max_ms": round(max(t), 4),
                     "closest_over_rays": round(mc / mt, 2),
                     "twin_sample_points": int(sub.shape[0]),
                     "twin_inner_visits_per_point": round(st["inner_visits"] / sub.shape[0], 2),
                     "twin_tri_tests_per_point": round(st["tri_tests"] / sub.shape[0], 2),
                     "twin_overflows": st["overflows"],
                     "ns_per_step": round(mc * 1e6 / (n * (st["inner_visits"] + st["tri_tests"]) / sub.shape[0]), 4)})
        print(json.dumps(rows[-1]), flush=True)
    overflow = r.overflow_count()
    r.close()
    res = {"config": a.config, "width": w, "height": h, "triangles": scene.num_triangles, "bvh": "SplitBVHBuilder (the config's)",
           "bvh_build_s": round(build_s, 2), "reps": a.reps, "warmup": a.warmup, "library": rtamd.library_digest(),
           "frame_hit_share": round(float(hit.mean()), 4), "scene_diagonal": round(diag, 3), "overflow_count": overflow,
           "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
