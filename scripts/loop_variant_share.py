#!/usr/bin/env python3
"""Which copy of the fast traversal's loop a config's wave traversals take (rt_loop_variant_counts,
DESIGN.md 7.2): the config's scene and frame with its default camera, one JSON line with the 18
counters and the share of closest-hit / any-hit / all wave traversals that run an octant loop.
Usage: python3 scripts/loop_variant_share.py [CONFIG=c3]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-opencl-raytracer_amd"))

import rtamd  # noqa: E402
from rtamd.configs import CONFIGS, make_scene  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "c3"
    cfg = CONFIGS[name]
    mesh, bvh, _ = make_scene(cfg, via_dae=False)
    w, h = cfg["w"], cfg["h"]
    r = rtamd.Renderer(0)
    r.upload(rtamd.Scene.from_mesh(mesh, bvh))
    r.set_params(rtamd.params_to_array(mesh.camera_params(w, h)))
    c = r.loop_variant_counts(w, h, cfg["depth"], cfg["flags"])
    r.close()
    share = lambda v: round(sum(v[1:]) / max(1, sum(v)), 4)
    print(json.dumps({"config": name, "closest": c["closest"], "any": c["any"], "octant_share_closest": share(c["closest"]),
                      "octant_share_any": share(c["any"]),
                      "octant_share": round((sum(c["closest"][1:]) + sum(c["any"][1:])) / max(1, sum(c["closest"]) + sum(c["any"])), 4)}))


if __name__ == "__main__":
    main()
