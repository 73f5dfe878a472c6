#!/usr/bin/env python3
"""What the calls that install a scene cost in wall time (each derives the walk references):
rt_upload_scene, rt_scene_copy and rt_build_scene of the 40 k-triangle fixture hf40k, (median, min) of 30
calls in ms.  Run once per library, alternating (RTAMD_LIB=... selects it; LABEL names it in the output).
Prints one JSON line (profiles/r16/install_cost.jsonl)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "real-time-opencl-raytracer_amd", "."):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402

import rtamd  # noqa: E402
from conftest import load_golden  # noqa: E402

d = load_golden("hf40k")
sc = rtamd.Scene.from_arrays(d)
a, b = rtamd.Renderer(0), rtamd.Renderer(0)
a.upload(sc)


def med(f, n=30):
    f()
    f()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4), round(min(t), 4)


print(json.dumps({"lib": os.environ.get("LABEL", "main"), "upload_ms": med(lambda: b.upload(sc)),
                  "copy_ms": med(lambda: b.copy_scene_from(a)), "build_scene_ms": med(lambda: b.build_scene(d))}))
