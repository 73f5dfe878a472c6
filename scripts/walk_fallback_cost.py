#!/usr/bin/env python3
"""What the host's fallback costs a scene without walk references: depth-1 S_ref frames of
escape40 (tests/refit_common.py's tree with leaves of 40 and 35 references) at 1024 x 1024, five times 200
frames, ms per frame.  Run once per library (RTAMD_LIB=... selects it; LABEL names it in the output):

    LABEL=parent RTAMD_LIB=$PWD/real-time-opencl-raytracer_amd/lib/ab/parent/librtamd.so python3 scripts/walk_fallback_cost.py
    LABEL=main python3 scripts/walk_fallback_cost.py
Prints one JSON line (profiles/r16/escape40_cost.jsonl)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "real-time-opencl-raytracer_amd", "."):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtamd  # noqa: E402
from refit_common import scene_arrays  # noqa: E402

d = dict(scene_arrays("bigleaf"))
W = H = 1024
m = rtamd.Mesh.from_arrays(d["vertices"], d["indices"])
p = rtamd.params_to_array(m.camera_params(W, H, radius=90.0))
r = rtamd.Renderer(0)
r.upload(rtamd.Scene.from_arrays(d))
r.set_params(p)
out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
res = []
for rep in range(5):
    for _ in range(20):
        r.render_device(W, H, 1, 0, out.data_ptr())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        r.render_device(W, H, 1, 0, out.data_ptr())
    torch.cuda.synchronize()
    res.append((time.perf_counter() - t0) / 200 * 1e3)
print(json.dumps({"lib": os.environ.get("LABEL", "main"), "ms_per_frame": res,
                  "checksum": int(out.cpu().numpy().view(np.uint32).astype(np.uint64).sum())}))
