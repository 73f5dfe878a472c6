"""On-GPU scene build: what mesh-to-renderable costs through rt_build_scene_device
against the path it replaces, measured in one session.

On one config's mesh (default C3, the 1M-triangle heightfield) on one GPU, per max_leaf 1, 2, 4, 8,
medians of --runs after one untimed call of each (scratch allocation):
  scene_kernel_ms   rt_last_scene_build_timing of rt_build_scene_device (first to last kernel)
  scene_wall_ms     wall clock of the synchronous rt_build_scene_device call, device arrays in
  parent_wall_ms    rt_build_bvh_device + download of nodes / references + rt_upload_scene, wall clock
  scene_rest_ms     scene_wall_ms - scene_kernel_ms: everything of the call that is no kernel -- the
                    hipMalloc of the new scene's arrays, the index copies, the wait for frames in
                    flight, the hipFree of the old scene -- so an upper bound of the allocation cost
The two paths alternate run by run, so that a drift of the machine meets both.  The last scene of
each max_leaf is checked against the parent path's scene image.  Prints one JSON line.

    python scripts/scene_build_bench.py [--config c3] [--runs 9]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-opencl-raytracer_amd"))

med = statistics.median


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--runs", type=int, default=9)
    a = ap.parse_args()
    import torch
    import rtamd
    from rtamd import configs
    cfg = configs.CONFIGS[a.config]
    mesh = configs.make_mesh(cfg, via_dae=False)
    m = mesh.arrays()
    v, idx = m["vertices"], m["indices"]
    n = idx.size // 3
    out = {"config": a.config, "triangles": n, "runs": a.runs, "max_leaf": {}}

    ra, rb = rtamd.Renderer(0), rtamd.Renderer(0)      # A: the new call; B: the parent path
    lib = rtamd.lib()
    dev = {k: torch.from_numpy(np.ascontiguousarray(m[k])).to("cuda:0")
           for k in ("vertices", "indices", "normals", "normals_indices", "tri_to_material")}
    mats = np.ascontiguousarray(m["materials"], np.float32)
    d_nodes = torch.zeros((2 * n - 1, 12), dtype=torch.float32, device="cuda:0")
    d_refs = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    nn = C.c_int32()
    p = lambda t: C.c_void_p(t.data_ptr())

    def scene(max_leaf):
        rc = lib.rt_build_scene_device(ra._h, p(dev["vertices"]), v.shape[0], p(dev["indices"]), idx.size, max_leaf,
                                       p(dev["normals"]), m["normals"].shape[0], p(dev["normals_indices"]),
                                       mats.ctypes.data_as(C.c_void_p), mats.shape[0], p(dev["tri_to_material"]),
                                       C.c_void_p(stream or None))
        assert rc == 0, lib.rt_last_error(ra._h)

    def parent(max_leaf):
        rc = lib.rt_build_bvh_device(rb._h, p(dev["vertices"]), v.shape[0], p(dev["indices"]), idx.size, max_leaf,
                                     p(d_nodes), 2 * n - 1, p(d_refs), n, C.byref(nn), C.c_void_p(stream or None))
        assert rc == 0, lib.rt_last_error(rb._h)
        nodes = d_nodes[:nn.value].cpu().numpy()
        refs = d_refs.cpu().numpy()
        rb.upload(rtamd.Scene(v, idx, nodes, refs, m["normals"], m["normals_indices"], m["materials"],
                              m["tri_to_material"], m["scene_min"], m["scene_max"]))

    def image(r):
        size = r.scene_image_size()
        buf = torch.zeros(size, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        r.pack_scene(buf.data_ptr(), size)
        return buf

    for max_leaf in (1, 2, 4, 8):
        scene(max_leaf)                                   # untimed: scratch allocation
        parent(max_leaf)
        kernel, wall, old = [], [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            scene(max_leaf)
            wall.append(1e3 * (time.perf_counter() - t0))
            kernel.append(ra.last_scene_build_ms())
            t0 = time.perf_counter()
            parent(max_leaf)
            old.append(1e3 * (time.perf_counter() - t0))
        same = bool(torch.equal(image(ra), image(rb)))
        out["max_leaf"][str(max_leaf)] = {
            "scene_kernel_ms": round(med(kernel), 4), "scene_wall_ms": round(med(wall), 4),
            "scene_rest_ms": round(med(w - k for w, k in zip(wall, kernel)), 4),
            "scene_wall_min_ms": round(min(wall), 4), "scene_wall_max_ms": round(max(wall), 4),
            "parent_wall_ms": round(med(old), 3), "parent_wall_min_ms": round(min(old), 3),
            "parent_wall_max_ms": round(max(old), 3), "speedup": round(med(old) / med(wall), 2),
            "inner_records": int((nn.value - 1) // 2), "heights": int(ra.refit_level_counts().size),
            "images_equal": same}
        assert same, f"max_leaf {max_leaf}: rt_build_scene and the parent path disagree"
    ra.close()
    rb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
