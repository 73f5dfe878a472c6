"""First-k-hits ray queries: what rt_trace_rays_k_device costs for k in {1, 2, 4, 8}, beside
rt_trace_rays_device's closest hit on the same rays in the same session as the scale a reader already knows.

On one config's scene (default C3, the 1M-triangle heightfield, 1080p, SBVH) on one GPU, in S_ref (flags 0).
The frame's w * h primary rays in the frame kernel's tile order, and the same under a fixed shuffle.  One
session, alternating, medians of --reps after --warmup rounds, kernel ms from HIP events
(rt_last_query_timing).  Beside each: the host twin's (S_strict) mean inner visits and triangle tests per
ray over every --sample-th ray.  Writes one JSON file.

    python scripts/multihit_bench.py [--config c3] [--reps 20] [--warmup 5] [--sample 16] [--out profiles/multihit/c3.json]
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
    tile, shuffle = tile_order(w, h), np.random.default_rng(21).permutation(n)
    sets = [("primary_tile", tile), ("primary_shuffle", shuffle)]
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    d_out = torch.zeros(max(KS) * 4 * n, dtype=torch.int32, device="cuda")
    packed = {name: np.ascontiguousarray(rtamd.pack_rays(o[order], d[order], None)) for name, order in sets}
    bufs = {name: torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda() for name, rec in packed.items()}
    torch.cuda.synchronize()
    ms = {(name, k): [] for name, _ in sets for k in (0,) + KS}   # k = 0: rt_trace_rays_device, closest hit
    for _ in range(a.warmup + a.reps):
        for name, _ in sets:
            d_rays = bufs[name]
            for k in KS:
                r.trace_rays_device(d_rays.data_ptr(), n, d_out.data_ptr(), stream=s)
                ms[(name, 0)].append(r.last_query_ms())
                r.trace_rays_k_device(d_rays.data_ptr(), n, k, d_out.data_ptr(), stream=s)
                ms[(name, k)].append(r.last_query_ms())
    hits = None
    rows = []
    for name, _ in sets:
        sub = np.ascontiguousarray(packed[name][::a.sample])
        c = ms[(name, 0)][len(KS) * a.warmup:]
        mc = statistics.median(c)
        row = {"set": name, "rays": n, "closest_ms": round(mc, 4), "closest_min_ms": round(min(c), 4),
               "closest_max_ms": round(max(c), 4), "closest_runs": len(c), "twin_sample_rays": int(sub.shape[0]), "k": {}}
        for k in KS:
            t = ms[(name, k)][a.warmup:]
            mt = statistics.median(t)
            got, st = rtamd.trace_rays_k_host(scene, sub, None, k, stats=True)
            if k == max(KS):
                hits = round(float((got["id"] >= 0).sum() / sub.shape[0]), 3)
            row["k"][str(k)] = {"ms": round(mt, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                                "mrays_per_s": round(n / mt / 1e3, 1), "over_closest": round(mt / mc, 3),
                                "twin_inner_visits_per_ray": round(st["inner_visits"] / sub.shape[0], 2),
                                "twin_tri_tests_per_ray": round(st["tri_tests"] / sub.shape[0], 2),
                                "twin_overflows": st["overflows"]}
        row["twin_hits_of_8_per_ray"] = hits
        rows.append(row)
        print(json.dumps(row), flush=True)
    overflow = r.overflow_count()
    r.close()
    res = {"config": a.config, "width": w, "height": h, "triangles": scene.num_triangles, "bvh": "SplitBVHBuilder (the config's)",
           "bvh_build_s": round(build_s, 2), "reps": a.reps, "warmup": a.warmup, "flags": 0, "library": rtamd.library_digest(),
           "overflow_count": overflow, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
