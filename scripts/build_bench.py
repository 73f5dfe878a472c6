"""On-GPU LBVH build: what a BVH build costs on the GPU against the host builders,
what the whole mesh-to-renderable path costs, and what the simpler tree costs per frame.

On one config's mesh (default C3, the 1M-triangle heightfield) on one GPU, medians of --runs:
  build      rt_build_bvh_device from device arrays into device arrays, per max_leaf 1, 2, 4, 8:
             kernel time (rt_last_build_timing) and wall clock of the synchronous call
  host       rt_bvh_build_sbvh, rt_bvh_build (max_leaf 8) and the host twin rt_bvh_build_lbvh,
             --threads threads (default 16), wall clock, median of --host-runs
  renderable build + download of nodes / references + rt_upload_scene, wall clock, per part
  render     the config's frame (C3: depth 1), kernel ms per frame (rt_last_timing), median of
             --frames after --warmup frames, on the LBVH at max_leaf 1, 2, 4, 8 and on the SBVH
--keys names the Morton keys of the GPU builds: axis, extent (RT_BUILD_EXTENT_KEYS,
DESIGN.md 17) or axis,extent -- both, alternating call by call so that a drift of the machine meets
both; the entries of the extent-aware keys carry the suffix _extent.  Every rendered scene also
reports its SAH cost (rt_scene_sah).  Prints one JSON line.

    python scripts/build_bench.py [--config c3] [--runs 9] [--host-runs 3] [--frames 40] [--keys axis]
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
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--keys", default="axis", help="axis, extent or axis,extent (alternating)")
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
    out = {"config": a.config, "triangles": n, "runs": a.runs, "host_runs": a.host_runs, "threads": a.threads,
           "frames": a.frames, "keys": kinds}

    def timed(fn, k):
        ts, res = [], None
        for _ in range(k):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        return med(ts), res

    # host builders
    sbvh_s, sbvh = timed(lambda: mesh.build_sbvh(a.threads), a.host_runs)
    sah_s, _ = timed(lambda: mesh.build_bvh(8, a.threads), a.host_runs)
    twin_s, twin = timed(lambda: mesh.build_lbvh(4), a.host_runs)
    out["host"] = {"sbvh_s": round(sbvh_s, 3), "binned_sah_s": round(sah_s, 3), "lbvh_twin_s": round(twin_s, 3)}

    r = rtamd.Renderer(0)
    lib = rtamd.lib()
    d_v = torch.from_numpy(v).to("cuda:0")
    d_i = torch.from_numpy(idx).to("cuda:0")
    d_nodes = torch.zeros((2 * n - 1, 12), dtype=torch.float32, device="cuda:0")
    d_refs = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    nn = C.c_int32()

    def build(max_leaf, kind):
        arg = max_leaf | (rtamd.RT_BUILD_EXTENT_KEYS if kind == "extent" else 0)
        rc = lib.rt_build_bvh_device(r._h, C.c_void_p(d_v.data_ptr()), v.shape[0], C.c_void_p(d_i.data_ptr()), idx.size,
                                     arg, C.c_void_p(d_nodes.data_ptr()), 2 * n - 1, C.c_void_p(d_refs.data_ptr()), n,
                                     C.byref(nn), C.c_void_p(stream or None))
        assert rc == 0, lib.rt_last_error(r._h)
        return nn.value

    def render_ms(scene):
        r.upload(scene)
        r.set_params(params)
        ms = []
        for f in range(a.warmup + a.frames):
            r.render(w, h, depth=depth, flags=flags)
            if f >= a.warmup:
                ms.append(r.last_kernel_ms())
        return med(ms)

    out["build"], out["renderable"], out["render_ms"], out["sah"] = {}, {}, {}, {}
    for max_leaf in (1, 2, 4, 8):
        for kind in kinds:
            build(max_leaf, kind)                         # untimed: scratch allocation
        kernel, wall, num = {k: [] for k in kinds}, {k: [] for k in kinds}, {}
        for _ in range(a.runs):
            for kind in kinds:                            # alternating call by call
                t0 = time.perf_counter()
                num[kind] = build(max_leaf, kind)
                wall[kind].append(1e3 * (time.perf_counter() - t0))
                kernel[kind].append(r.last_build_ms())
        for kind in kinds:
            tag = str(max_leaf) + ("_extent" if kind == "extent" else "")
            out["build"][tag] = {"kernel_ms": round(med(kernel[kind]), 4), "kernel_min_ms": round(min(kernel[kind]), 4),
                                 "kernel_max_ms": round(max(kernel[kind]), 4), "wall_ms": round(med(wall[kind]), 4),
                                 "nodes": num[kind]}
            # mesh to renderable: build + download + upload
            parts = []
            for _ in range(3):
                t0 = time.perf_counter()
                n_nodes = build(max_leaf, kind)
                t1 = time.perf_counter()
                nodes = d_nodes[:n_nodes].cpu().numpy()
                refs = d_refs.cpu().numpy()
                t2 = time.perf_counter()
                scene = rtamd.Scene(v, idx, nodes, refs, m["normals"], m["normals_indices"], m["materials"],
                                    m["tri_to_material"], m["scene_min"], m["scene_max"])
                r.upload(scene)
                t3 = time.perf_counter()
                parts.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0))
            b, dl, up, tot = (1e3 * med(p[k] for p in parts) for k in range(4))
            out["renderable"][tag] = {"build_ms": round(b, 3), "download_ms": round(dl, 3), "upload_ms": round(up, 3),
                                      "total_ms": round(tot, 3)}
            if max_leaf == 4 and kind == "axis":
                assert np.array_equal(nodes.view(np.uint32), twin.nodes.view(np.uint32)), "device build and host twin disagree"
            out["render_ms"]["lbvh_" + tag] = round(render_ms(scene), 4)
            out["sah"]["lbvh_" + tag] = round(r.scene_sah().cost, 3)
    out["render_ms"]["sbvh"] = round(render_ms(rtamd.Scene.from_mesh(mesh, sbvh)), 4)
    out["sah"]["sbvh"] = round(r.scene_sah().cost, 3)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
