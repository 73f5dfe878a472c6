"""Animated geometry: what a vertex update costs against the only path there was
before it -- refit the nodes on the host and rt_upload_scene everything again.

On one config's scene (default C3, the 1M-triangle heightfield) on one GPU:
  update    rt_update_vertices_device from a device vertex buffer: kernel time
            (rt_last_update_timing) and wall clock of the synchronous call, median of --updates
  reupload  rt_upload_scene of host arrays that are ALREADY refit (the host refit is not
            counted), wall clock, median of --uploads
Prints one JSON line with both, their ratio, the update's launch count and the number of inner
records per height.

    python scripts/refit_bench.py [--config c3] [--updates 20] [--uploads 5]
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

TOP_MAX = 1024   # rt_refit.hip kTopMax: heights with at most this many records share the last launch


def heights(nodes):
    """Inner nodes per height (longest path down to a leaf), height 1 first.  The builders emit
    children after their parent, so one backward pass over the array does."""
    ni = nodes.view(np.int32)
    left, right = ni[:, 8].tolist(), ni[:, 9].tolist()
    h = [0] * len(left)
    for n in range(len(left) - 1, -1, -1):
        if left[n] >= 0:
            assert left[n] > n and right[n] > n
            h[n] = 1 + max(h[left[n]], h[right[n]])
    return np.bincount(np.asarray(h))[1:].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--uploads", type=int, default=5)
    a = ap.parse_args()
    import torch
    import rtamd
    from rtamd import configs
    cfg = configs.CONFIGS[a.config]
    mesh, bvh, build_s = configs.make_scene(cfg, via_dae=False)
    scene = rtamd.Scene.from_mesh(mesh, bvh)
    per_height = heights(scene.nodes)
    r = rtamd.Renderer(0)
    r.upload(scene)
    base = torch.from_numpy(scene.vertices).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    kernel_ms, wall_ms = [], []
    for k in range(a.updates + 2):           # two untimed
        s = 1.0 + 0.015625 * (k % 8)
        dv = base * torch.tensor([s, s, s, 1.0], device="cuda:0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.update_vertices((dv.data_ptr(), stream))
        wall_ms.append(1e3 * (time.perf_counter() - t0))
        kernel_ms.append(r.last_update_ms())
    last = dv.cpu().numpy()
    nodes2 = rtamd.refit_nodes(scene, last)  # the host refit: outside the timing
    mn, mx = r.scene_bounds()
    assert np.array_equal(mn, nodes2[0, 0:3]) and np.array_equal(mx, nodes2[0, 4:7]), "update and host refit disagree"
    scene2 = rtamd.Scene.from_arrays(dict(scene.arrays(), vertices=last, nodes=nodes2))
    up_ms = []
    for _ in range(a.uploads + 1):           # one untimed
        t0 = time.perf_counter()
        r.upload(scene2)
        up_ms.append(1e3 * (time.perf_counter() - t0))
    r.close()
    upd_k, upd_w = statistics.median(kernel_ms[2:]), statistics.median(wall_ms[2:])
    up = statistics.median(up_ms[1:])
    print(json.dumps({
        "config": a.config, "triangles": scene.num_triangles, "bvh_nodes": int(scene.nodes.shape[0]),
        "references": int(scene.tri_indices.size), "bvh_build_s": round(build_s, 2),
        "update_kernel_ms": round(upd_k, 4), "update_wall_ms": round(upd_w, 4), "reupload_wall_ms": round(up, 3),
        "reupload_over_update_wall": round(up / upd_w, 2), "heights": len(per_height),
        "launches": 2 + sum(1 for c in per_height if c > TOP_MAX), "inner_records_per_height": per_height}))


if __name__ == "__main__":
    main()
