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
each max_leaf is checked against the parent path's scene image.

--keys names the Morton keys of the builds: axis, extent (RT_BUILD_EXTENT_KEYS,
DESIGN.md 17) or axis,extent -- both, alternating call by call; the entries of the extent-aware keys
carry the suffix _extent.  Every built scene also reports
  sah               its SAH cost (rt_scene_sah), and sah_ms, the wall clock of that call
  render_ms         the config's frame on it, kernel ms per frame (rt_last_timing), median of
                    --frames after --warmup
and with --sbvh the same three for an upload of the host's SBVH.  Prints one JSON line.

    python scripts/scene_build_bench.py [--config c3] [--runs 9] [--keys axis] [--sbvh]
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
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--keys", default="axis", help="axis, extent or axis,extent (alternating)")
    ap.add_argument("--sbvh", action="store_true", help="also rate and render the host's SBVH scene")
    a = ap.parse_args()
    kinds = a.keys.split(",")
    assert kinds and all(k in ("axis", "extent") for k in kinds), "--keys: axis, extent or axis,extent"
    import torch
    import rtamd
    from rtamd import configs
    cfg = configs.CONFIGS[a.config]
    mesh = configs.make_mesh(cfg, via_dae=False)
    m = mesh.arrays()
    v, idx = m["vertices"], m["indices"]
    n = idx.size // 3
    w, h, depth, flags = cfg["w"], cfg["h"], cfg["depth"], cfg["flags"]
    params = mesh.camera_params(w, h)
    out = {"config": a.config, "triangles": n, "runs": a.runs, "keys": kinds, "max_leaf": {}}

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

    def arg(max_leaf, kind):
        return max_leaf | (rtamd.RT_BUILD_EXTENT_KEYS if kind == "extent" else 0)

    def scene(max_leaf, kind):
        rc = lib.rt_build_scene_device(ra._h, p(dev["vertices"]), v.shape[0], p(dev["indices"]), idx.size, arg(max_leaf, kind),
                                       p(dev["normals"]), m["normals"].shape[0], p(dev["normals_indices"]),
                                       mats.ctypes.data_as(C.c_void_p), mats.shape[0], p(dev["tri_to_material"]),
                                       C.c_void_p(stream or None))
        assert rc == 0, lib.rt_last_error(ra._h)

    def parent(max_leaf, kind):
        rc = lib.rt_build_bvh_device(rb._h, p(dev["vertices"]), v.shape[0], p(dev["indices"]), idx.size, arg(max_leaf, kind),
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

    def rate(r):
        """The scene of r: its SAH cost, the wall clock of the query, the config's frame on it."""
        cost = r.scene_sah().cost
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r.scene_sah()
            ts.append(1e3 * (time.perf_counter() - t0))
        r.set_params(params)
        ms = []
        for f in range(a.warmup + a.frames):
            r.render(w, h, depth=depth, flags=flags)
            if f >= a.warmup:
                ms.append(r.last_kernel_ms())
        return {"sah": round(cost, 3), "sah_ms": round(med(ts), 4), "render_ms": round(med(ms), 4)}

    for max_leaf in (1, 2, 4, 8):
        for kind in kinds:
            scene(max_leaf, kind)                         # untimed: scratch allocation
            parent(max_leaf, kind)
        kernel, wall, old = ({k: [] for k in kinds} for _ in range(3))
        for _ in range(a.runs):
            for kind in kinds:                            # alternating call by call
                t0 = time.perf_counter()
                scene(max_leaf, kind)
                wall[kind].append(1e3 * (time.perf_counter() - t0))
                kernel[kind].append(ra.last_scene_build_ms())
                t0 = time.perf_counter()
                parent(max_leaf, kind)
                old[kind].append(1e3 * (time.perf_counter() - t0))
        for kind in kinds:
            scene(max_leaf, kind)
            parent(max_leaf, kind)
            same = bool(torch.equal(image(ra), image(rb)))
            k, wl, o = kernel[kind], wall[kind], old[kind]
            out["max_leaf"][str(max_leaf) + ("_extent" if kind == "extent" else "")] = dict({
                "scene_kernel_ms": round(med(k), 4), "scene_kernel_min_ms": round(min(k), 4),
                "scene_kernel_max_ms": round(max(k), 4), "scene_wall_ms": round(med(wl), 4),
                "scene_rest_ms": round(med(x - y for x, y in zip(wl, k)), 4),
                "scene_wall_min_ms": round(min(wl), 4), "scene_wall_max_ms": round(max(wl), 4),
                "parent_wall_ms": round(med(o), 3), "parent_wall_min_ms": round(min(o), 3),
                "parent_wall_max_ms": round(max(o), 3), "speedup": round(med(o) / med(wl), 2),
                "inner_records": int((nn.value - 1) // 2), "heights": int(ra.refit_level_counts().size),
                "images_equal": same}, **rate(ra))
            assert same, f"max_leaf {max_leaf}, {kind} keys: rt_build_scene and the parent path disagree"
    if a.sbvh:
        rb.upload(rtamd.Scene.from_mesh(mesh, mesh.build_sbvh(16)))
        out["sbvh"] = rate(rb)
    ra.close()
    rb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
