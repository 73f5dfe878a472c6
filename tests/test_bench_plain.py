"""bench.py's plain run and its --dump-outputs: a run without --full sets up, warms up, times
--steps frames and prints the result line, with none of the figures that take runs of their own;
--dump-outputs writes the last timed frame, whose camera follows from --warmup and --steps alone
(not from how many frames the time-based warm-up ran), so two runs dump the same frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("batch_check", "one_frame_per_launch", "frame_latency", "host_boundary", "frame_check",
             "gathered_frame_equals_single_rank_render")


def test_dump_outputs_whole_frame_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    w, h = 16, 9
    packed = np.random.default_rng(1).integers(-2**31, 2**31, w * h, dtype=np.int64).astype(np.int32)
    by = packed.view(np.uint8).reshape(-1, 4).astype(np.float32)
    bench.dump_outputs(str(tmp_path), packed, w, h)
    f = np.load(tmp_path / "frame.npy")
    assert f.dtype == np.float32 and f.shape == (h, w, 4) and np.array_equal(f.reshape(-1, 4), by)
    assert not (tmp_path / "frame_pixels.npy").exists()
    bench.dump_outputs(str(tmp_path), packed[:40], w, h)   # a shard's bands: rows of pixels
    assert np.array_equal(np.load(tmp_path / "frame.npy"), by[:40])
    # over the cap: the same sample of pixels every time, with their indices
    monkeypatch.setattr(bench, "DUMP_FULL_PIXELS", 100)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_PIXELS", 37)
    bench.dump_outputs(str(tmp_path), packed, w, h)
    idx = np.load(tmp_path / "frame_pixels.npy")
    assert idx.dtype == np.float64 and idx.shape == (37,) and len(set(idx.tolist())) == 37
    assert np.array_equal(np.load(tmp_path / "frame.npy"), by[idx.astype(np.int64)])
    bench.dump_outputs(str(tmp_path / "again"), packed, w, h)
    assert np.array_equal(np.load(tmp_path / "again" / "frame_pixels.npy"), idx)
    bench.dump_outputs(str(tmp_path), packed[:100], w, h)   # whole again: no stale index file
    assert not (tmp_path / "frame_pixels.npy").exists()


def test_frame_check_options_need_full():
    for extra in (["--frame-check", "every"], ["--inject-fault", "wrong-bands"]):
        p = subprocess.run([sys.executable, BENCH] + extra, capture_output=True, text=True, timeout=60, cwd=ROOT)
        assert p.returncode == 2 and "--full" in p.stderr, p.stderr[-1000:]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_timed_frame(tmp_path):
    import bench
    import rtamd
    from rtamd import configs
    steps, warmup = 6, 3   # depth 1: launches of 4 frames, so one full launch and a part-filled one
    cmd = [sys.executable, BENCH, "--gpus", "1", "--config", "c1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(tmp_path / "dump")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, lines   # the result is the one line on stdout
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["warmup"] == warmup and res["n_gpus"] == 1
    assert res["value"] > 0 and res["unit"] == "Mrays/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["ms_per_step"] > 0 and res["metric"] == bench.METRIC
    assert res["roofline"] is None and res["cpu_baseline"] is None and "parity_vs_oracle" not in res
    assert not [k for k in FULL_ONLY if k in res["config"]]
    # the dumped frame: camera (warmup + steps - 1) % 32 of the jittered default camera, single render
    cfg = configs.CONFIGS["c1"]
    w, h = cfg["w"], cfg["h"]
    mesh, bvh, _ = configs.make_scene(cfg)
    cams = bench.jittered_cameras(rtamd.params_to_array(mesh.camera_params(w, h)), w, h, 32)
    r = rtamd.Renderer(0)
    try:
        r.upload(rtamd.Scene.from_mesh(mesh, bvh))
        r.set_params(cams[(warmup + steps - 1) % 32])
        want = r.render(w, h, depth=cfg["depth"], flags=cfg["flags"])
    finally:
        r.close()
    got = np.load(tmp_path / "dump" / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (h, w, 4)
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(h, w, 4).astype(np.float32))
