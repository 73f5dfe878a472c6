"""Occlusion fans: what rt_trace_fan_device costs against rt_trace_rays_device
(RT_FLAG_ANY_HIT) on the same rays, expanded.

On one config's scene (default C3, the 1M-triangle heightfield, 1080p) on one GPU.  The origins are the
hit points and shading normals of the frame's primary rays (rt_trace_rays_attr), the first --origins of
those that hit, in three orders: the frame kernel's tile order, row-major pixel order, and a fixed
shuffle.  The directions are the k-point Fibonacci sphere, k = 64 and 256; culling is on.  Per order, k
and arithmetic the fan alternates with the any-hit query of rt_fan_expand's traced rays in one session;
medians of --reps after --warmup rounds: kernel ms from HIP events (rt_last_query_timing), Mrays/s over
the traced rays, wall ms from the enqueue to the end of the kernel, and the bytes each form moves.
Writes one JSON file.

    python scripts/fan_bench.py [--config c3] [--origins 262144] [--reps 20] [--warmup 5] [--out profiles/fan/c3.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-opencl-raytracer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ray_query_bench import primary_rays, tile_order   # noqa: E402


def fibonacci(k):
    i = np.arange(k, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / k
    r = np.sqrt(1.0 - z * z)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--origins", type=int, default=262144)
    ap.add_argument("--ks", default="64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
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
    attr = r.trace_rays_attr(o, d)
    orders = {"tile": tile_order(w, h), "rowmajor": np.arange(w * h), "shuffle": np.random.default_rng(21).permutation(w * h)}
    arith = {"ref": 0, "hw": rtamd.RT_FLAG_HW_MATH, "strict": rtamd.RT_FLAG_STRICT_MATH}
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()

    rows = []
    for oname, order in orders.items():
        hit = order[attr["id"][order] >= 0][:a.origins]
        rec = rtamd.pack_fan_origins(attr["p"][hit], attr["ns"][hit])
        n = rec.shape[0]
        d_org = dev(rec)
        for k in (int(x) for x in a.ks.split(",")):
            dirs = fibonacci(k)
            rays, traced = rtamd.fan_expand(rec, dirs)
            sel = np.ascontiguousarray(rays[traced])
            del rays
            m = sel.shape[0]
            d_rays = dev(sel)
            del sel
            d_dirs = dev(rtamd.pack_fan_dirs(dirs))
            words = ((k + 31) // 32) * n
            d_masks = torch.zeros(words, dtype=torch.int32, device="cuda")
            d_hits = torch.zeros(2 * m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ms = {(mode, form): [] for mode in arith for form in ("fan", "query")}
            wall = {key: [] for key in ms}
            for _ in range(a.warmup + a.reps):
                for mode, f in arith.items():
                    t0 = time.perf_counter()
                    r.trace_fan_device(d_org.data_ptr(), n, d_dirs.data_ptr(), k, d_masks.data_ptr(), flags=f, stream=s)
                    ms[(mode, "fan")].append(r.last_query_ms())
                    wall[(mode, "fan")].append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    r.trace_rays_device(d_rays.data_ptr(), m, d_hits.data_ptr(), any_hit=True, flags=f, stream=s)
                    ms[(mode, "query")].append(r.last_query_ms())
                    wall[(mode, "query")].append((time.perf_counter() - t0) * 1e3)
            occluded = float((d_hits[0::2] >= 0).float().mean().item())
            for mode in arith:
                fan, qry = (statistics.median(ms[(mode, form)][a.warmup:]) for form in ("fan", "query"))
                rows.append({"order": oname, "k": k, "arithmetic": mode, "origins": n, "traced_rays": m,
                             "traced_share": round(m / (n * k), 4), "occluded_share_strict": round(occluded, 4),
                             "fan_ms": round(fan, 4), "query_ms": round(qry, 4), "fan_over_query": round(fan / qry, 3),
                             "fan_mrays_per_s": round(m / fan / 1e3, 1), "query_mrays_per_s": round(m / qry / 1e3, 1),
                             "fan_wall_ms": round(statistics.median(wall[(mode, "fan")][a.warmup:]), 4),
                             "query_wall_ms": round(statistics.median(wall[(mode, "query")][a.warmup:]), 4),
                             "fan_min_ms": round(min(ms[(mode, "fan")][a.warmup:]), 4),
                             "fan_max_ms": round(max(ms[(mode, "fan")][a.warmup:]), 4),
                             "query_min_ms": round(min(ms[(mode, "query")][a.warmup:]), 4),
                             "query_max_ms": round(max(ms[(mode, "query")][a.warmup:]), 4),
                             "fan_bytes": 32 * n + 16 * k + 4 * words, "query_bytes": 40 * m})
                print(json.dumps(rows[-1]), flush=True)
            del d_rays, d_hits, d_masks
            torch.cuda.empty_cache()
    deferred = r.last_deferred()
    r.close()
    res = {"config": a.config, "width": w, "height": h, "triangles": scene.num_triangles, "bvh": "SplitBVHBuilder (the config's)",
           "bvh_build_s": round(build_s, 2), "reps": a.reps, "warmup": a.warmup, "library": rtamd.library_digest(),
           "last_deferred": deferred, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
