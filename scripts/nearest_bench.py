"""k-nearest-triangle queries: what rt_nearest_k_device costs for k in {1, 2, 4, 8}, beside
rt_closest_points_device on the same points in the same session as the scale a reader already knows.

On one config's scene (default C3, the 1M-triangle heightfield, 1080p, SBVH) on one GPU.  Point sets of
w * h points, closest_bench.py's (1), (3) and (4): the frame's hit points from rt_trace_rays_attr lifted by
0.5 along ng (a ray that missed keeps its origin) in the frame kernel's tile order; the same under a fixed
shuffle; uniform in the scene box.  r = +inf throughout.  One session, alternating, medians of --reps
after --warmup rounds, kernel ms from HIP events (rt_last_query_timing).  Beside each: the host twin's
mean inner visits and triangle tests per point over every --sample-th point.  Writes one JSON file.

    python scripts/nearest_bench.py [--config c3] [--reps 20] [--warmup 5] [--sample 16] [--out profiles/nearest/c3.json]
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

KS = (1, 2, 4, 8)


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
    uniform = np.random.default_rng(22).uniform(lo, hi, (n, 3)).astype(np.float32)
    tile, shuffle = tile_order(w, h), np.random.default_rng(21).permutation(n)
    sets = [("hit_points_tile", lifted[tile]), ("hit_points_shuffle", lifted[shuffle]), ("uniform_r_inf", uniform)]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    d_out = torch.zeros(max(KS) * 8 * n, dtype=torch.int32, device="cuda")
    bufs = {name: torch.from_numpy(np.ascontiguousarray(rtamd.pack_points(q, None)).view(np.uint8).reshape(-1)).cuda()
            for name, q in sets}
    torch.cuda.synchronize()
    ms = {(name, k): [] for name, _ in sets for k in (0,) + KS}   # k = 0: rt_closest_points
    for _ in range(a.warmup + a.reps):
        for name, _ in sets:
            d_pts = bufs[name]
            for k in KS:
                r.closest_points_device(d_pts.data_ptr(), n, d_out.data_ptr(), stream=s)
                ms[(name, 0)].append(r.last_query_ms())
                r.nearest_k_device(d_pts.data_ptr(), n, k, d_out.data_ptr(), stream=s)
                ms[(name, k)].append(r.last_query_ms())
    rows = []
    for name, q in sets:
        sub = np.ascontiguousarray(q[::a.sample])
        c = ms[(name, 0)][len(KS) * a.warmup:]
        mc = statistics.median(c)
        _, st = rtamd.closest_points_host(scene, rtamd.pack_points(sub, None), stats=True)
        row = {"set": name, "points": n, "closest_ms": round(mc, 4), "closest_min_ms": round(min(c), 4),
               "closest_max_ms": round(max(c), 4), "closest_runs": len(c), "twin_sample_points": int(sub.shape[0]),
               "closest_twin_inner_visits_per_point": round(st["inner_visits"] / sub.shape[0], 2),
               "closest_twin_tri_tests_per_point": round(st["tri_tests"] / sub.shape[0], 2), "k": {}}
        for k in KS:
            t = ms[(name, k)][a.warmup:]
            mt = statistics.median(t)
            _, st = rtamd.nearest_k_host(scene, rtamd.pack_points(sub, None), k, stats=True)
            row["k"][str(k)] = {"ms": round(mt, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                                "mpoints_per_s": round(n / mt / 1e3, 1), "over_closest": round(mt / mc, 3),
                                "within_closest_spread": bool(min(c) <= mt <= max(c)),
                                "twin_inner_visits_per_point": round(st["inner_visits"] / sub.shape[0], 2),
                                "twin_tri_tests_per_point": round(st["tri_tests"] / sub.shape[0], 2),
                                "twin_overflows": st["overflows"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    overflow = r.overflow_count()
    r.close()
    res = {"config": a.config, "width": w, "height": h, "triangles": scene.num_triangles, "bvh": "SplitBVHBuilder (the config's)",
           "bvh_build_s": round(build_s, 2), "reps": a.reps, "warmup": a.warmup, "library": rtamd.library_digest(),
           "frame_hit_share": round(float(hit.mean()), 4), "overflow_count": overflow, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
