"""The four query families -- ray queries (rt_hit and rt_hit_attr records), occlusion fans, closest
points and k nearest triangles -- through the host code they share: the context's
staging buffers as one family after another grows and reuses them, caller memory the device reaches
by itself, and every refusal with its code and its rt_last_error text.  Everything is exact: the
host forms are compared word for word with the device forms on the same context."""
import ctypes as C
import math

import numpy as np
import pytest

import rtamd
from conftest import load_golden

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
STRICT, HW = rtamd.RT_FLAG_STRICT_MATH, rtamd.RT_FLAG_HW_MATH
RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE = -1, -3
GUARD = 0x5A5A5A5A


def cvp(addr):
    return C.c_void_p(addr or None)


def words(a):
    return np.ascontiguousarray(a).view(U32).reshape(-1)


def box(d):
    v = np.asarray(d["vertices"], F32).reshape(-1, 4)[:, :3]
    return v.min(axis=0), v.max(axis=0)


def some_points(d, n, seed):
    lo, hi = box(d)
    return (lo + np.random.default_rng(seed).random((n, 3)) * (hi - lo)).astype(F32)


def some_dirs(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 3)).astype(F32)


def on_device(r, inputs, out_words, launch):
    """`launch(addresses of the inputs..., address of the output)` on torch buffers -> the output's
    words; four guard words after the output stay as they are."""
    import torch
    bufs = [torch.from_numpy(words(a).view(np.int32).copy()).cuda() for a in inputs]
    out = torch.full((out_words + 4,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    launch(*[b.data_ptr() for b in bufs], out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(U32)
    assert np.all(got[out_words:] == GUARD), "the kernel wrote past its output"
    return got[:out_words]


# ---- the host forms, one family after another on one context ----

def step_closest(r, d, n, seed):
    rec = rtamd.pack_points(some_points(d, n, seed), None)
    host = lambda: words(r.closest_points(rec))
    dev = lambda: on_device(r, [rec], 8 * n, lambda p, o: r.closest_points_device(p, n, o))
    return host, dev


def step_nearest(r, d, n, k, seed):
    rec = rtamd.pack_points(some_points(d, n, seed), None)
    host = lambda: words(r.nearest_k(rec, k))
    dev = lambda: on_device(r, [rec], 8 * k * n, lambda p, o: r.nearest_k_device(p, n, k, o))
    return host, dev


def step_rays(r, d, n, seed):
    o, dirs = some_points(d, n, seed), some_dirs(n, seed + 1)
    rays = rtamd.pack_rays(o, dirs)

    def host():
        ids, t = r.trace_rays(o, dirs, flags=STRICT)
        return np.stack([ids.view(U32), t.view(U32)], axis=1).reshape(-1)
    dev = lambda: on_device(r, [rays], 2 * n, lambda p, h: r.trace_rays_device(p, n, h, flags=STRICT))
    return host, dev


def step_attr(r, d, n, seed):
    o, dirs = some_points(d, n, seed), some_dirs(n, seed + 1)
    rays = rtamd.pack_rays(o, dirs)
    host = lambda: words(r.trace_rays_attr(o, dirs, flags=STRICT))
    dev = lambda: on_device(r, [rays], 16 * n, lambda p, h: r.trace_rays_attr_device(p, n, h, flags=STRICT))
    return host, dev


def step_fan(r, d, n, k, seed):
    rec = rtamd.pack_fan_origins(some_points(d, n, seed))
    dirs = rtamd.pack_fan_dirs(some_dirs(k, seed + 1))
    w = (k + 31) // 32
    host = lambda: words(r.trace_fan(rec, dirs, flags=STRICT))
    dev = lambda: on_device(r, [rec, dirs], w * n,
                            lambda po, pd, pm: r.trace_fan_device(po, n, pd, k, pm, flags=STRICT))
    return host, dev


def test_interleaved_staging():
    """n = 65: one full group of 64 and one lane; k = 33: one full chunk of 32 bits and one bit.  The
    staging in grows at the first ray query (twice the points' bytes) and at n = 130, the staging out
    at the attribute records and at the eight planes; every other call reuses what another family left."""
    d = load_golden("cornell12")
    r = rtamd.Renderer(0)
    try:
        r.upload(rtamd.Scene.from_arrays(d))
        steps = [("closest_points n=65", step_closest(r, d, 65, 1)),
                 ("trace_rays n=65", step_rays(r, d, 65, 2)),
                 ("trace_rays_attr n=65", step_attr(r, d, 65, 4)),
                 ("trace_fan n=65 k=33", step_fan(r, d, 65, 33, 6)),
                 ("nearest_k k=8 n=65", step_nearest(r, d, 65, 8, 8)),
                 ("trace_rays n=130", step_rays(r, d, 130, 9)),
                 ("closest_points n=1", step_closest(r, d, 1, 11))]
        for label, (host, dev) in steps:
            got = host()
            ms, deferred = r.last_query_ms(), r.last_deferred()
            assert math.isfinite(ms) and ms >= 0.0, f"{label}: last_query_ms {ms}"
            want = dev()
            assert r.last_deferred() == deferred, f"{label}: last_deferred, host form {deferred}"
            assert got.shape == want.shape and np.array_equal(got, want), \
                f"{label}: {int((got != want).sum())} words of the host form differ from the device form"
            assert np.any(got != got[0]), f"{label}: the inputs reach the scene"
    finally:
        r.close()


def test_pinned_memory_nearest_k(renderer):
    """Input and output in pinned tensors, which the device reaches without staging."""
    import torch
    d = load_golden("cornell12")
    renderer.upload(rtamd.Scene.from_arrays(d))
    n, k = 65, 2
    rec = rtamd.pack_points(some_points(d, n, 21), None)
    want = words(renderer.nearest_k(rec, k))
    assert np.any(want != want[0])
    pts = torch.from_numpy(words(rec).view(np.int32).copy()).pin_memory()
    out = torch.full((8 * k * n + 4,), GUARD, dtype=torch.int32).pin_memory()
    assert pts.is_pinned() and out.is_pinned() and pts.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = rtamd.lib().rt_nearest_k(renderer._h, cvp(pts.data_ptr()), n, k, 0, cvp(out.data_ptr()))
    assert rc == 0, rtamd.lib().rt_last_error(renderer._h)
    got = out.numpy().view(U32)
    assert np.all(got[8 * k * n:] == GUARD)
    assert np.array_equal(got[:8 * k * n], want), "pinned and pageable memory give different records"
    assert renderer.last_query_ms() >= 0.0 and renderer.last_deferred() == 0


# ---- refusals: code and text ----

RAY, FAN, CLOSEST, NEAREST = "ray", "fan", "closest", "nearest"
ENTRIES = [("rt_trace_rays", RAY, False), ("rt_trace_rays_device", RAY, True),
           ("rt_trace_rays_attr", RAY, False), ("rt_trace_rays_attr_device", RAY, True),
           ("rt_trace_fan", FAN, False), ("rt_trace_fan_device", FAN, True),
           ("rt_closest_points", CLOSEST, False), ("rt_closest_points_device", CLOSEST, True),
           ("rt_nearest_k", NEAREST, False), ("rt_nearest_k_device", NEAREST, True)]
N_RANGE = {RAY: ": n must be 0..2^30", FAN: ": n must be 0..2^26", CLOSEST: ": n must be 0..2^30", NEAREST: ": n must be 0..2^30"}
N_OVER = {RAY: (1 << 30) + 1, FAN: (1 << 26) + 1, CLOSEST: (1 << 30) + 1, NEAREST: (1 << 30) + 1}
NULLS = {RAY: ": rays or hits is NULL", FAN: ": origins, dirs or masks is NULL", CLOSEST: ": pts or out is NULL",
         NEAREST: ": pts or out is NULL"}
BAD_FLAG = {RAY: (rtamd.RT_FLAG_WAVEFRONT, ": a flag that is not a ray query's"),
            FAN: (rtamd.RT_FLAG_ANY_HIT, ": a flag that is not a fan's"),
            CLOSEST: (STRICT, ": flags must be 0"), NEAREST: (STRICT, ": flags must be 0")}
BOTH_MATHS = {RAY: ": RT_FLAG_STRICT_MATH and RT_FLAG_HW_MATH exclude each other",
              FAN: ": RT_FLAG_STRICT_MATH and RT_FLAG_HW_MATH exclude each other",
              CLOSEST: ": flags must be 0", NEAREST: ": flags must be 0"}
OK_FLAGS = {RAY: STRICT, FAN: STRICT, CLOSEST: 0, NEAREST: 0}
MISALIGNED = {"rt_trace_rays_device": "rt_trace_rays_device: d_rays must be 16-byte aligned and d_hits 8-byte aligned",
              "rt_trace_rays_attr_device": "rt_trace_rays_attr_device: d_rays and d_hits must be 16-byte aligned",
              "rt_trace_fan_device": "rt_trace_fan_device: d_origins and d_dirs must be 16-byte aligned and d_masks 4-byte aligned",
              "rt_closest_points_device": "rt_closest_points_device: d_pts and d_out must be 16-byte aligned",
              "rt_nearest_k_device": "rt_nearest_k_device: d_pts and d_out must be 16-byte aligned"}
NO_SCENE = ": no scene uploaded"
FAN_K = ": k must be 1..RT_FAN_MAX_DIRS"
NEAREST_K = ": k must be 1..8"
NEAREST_NK = ": n * k must be at most 2^30"
CTX_NULL = ": ctx is NULL"


def invoke(name, family, device, h, inp, n, flags, out, k=2, dirs=None):
    fn = getattr(rtamd.lib(), name)
    if family == FAN:
        args = [h, cvp(inp), n, cvp(dirs), k, flags, cvp(out)]
    elif family == NEAREST:
        args = [h, cvp(inp), n, k, flags, cvp(out)]
    else:
        args = [h, cvp(inp), n, flags, cvp(out)]
    return fn(*(args + [None] if device else args))


def refusal_table(fresh, ctx, host, dev):
    """(label, ctx the text is read from, code, text, the call) for every refused call; host and dev are
    (input, directions, output) addresses of valid buffers for n = 4."""
    rows = []
    for name, family, device in ENTRIES:
        inp, dirs, out = dev if device else host
        ok = OK_FLAGS[family]

        def add(label, text, code=RT_ERR_INVALID_ARG, h=ctx, **kw):
            a = dict(name=name, family=family, device=device, h=h, inp=inp, n=4, flags=ok, out=out, dirs=dirs)
            a.update(kw)
            rows.append((f"{name}, {label}", h, code, text if text.startswith(name) else name + text,
                         lambda a=a: invoke(**a)))

        add("ctx NULL", CTX_NULL, h=None)
        add("n = -1", N_RANGE[family], n=-1)
        add("n above the maximum", N_RANGE[family], n=N_OVER[family])
        add("NULL input", NULLS[family], inp=0)
        add("NULL output", NULLS[family], out=0)
        add("a flag outside the mask", BAD_FLAG[family][1], flags=BAD_FLAG[family][0])
        add("HW | STRICT", BOTH_MATHS[family], flags=HW | STRICT)
        add("no scene", NO_SCENE, code=RT_ERR_NO_SCENE, h=fresh)
        if device:
            step = 2 if family == FAN else 4
            add("misaligned input", MISALIGNED[name], inp=inp + 4)
            add("misaligned output", MISALIGNED[name], out=out + step)
        if family == FAN:
            add("k = 0", FAN_K, k=0)
            add("k above RT_FAN_MAX_DIRS", FAN_K, k=rtamd.RT_FAN_MAX_DIRS + 1)
            add("NULL directions", NULLS[family], dirs=0)
            if device:
                add("misaligned directions", MISALIGNED[name], dirs=dirs + 4)
            # the order: n, then k, then NULL pointers, then flags, then no scene
            add("n = -1 and k = 0", N_RANGE[family], n=-1, k=0)
            add("k = 0 and a NULL input", FAN_K, k=0, inp=0)
            add("a NULL input and a flag outside the mask", NULLS[family], inp=0, flags=BAD_FLAG[family][0])
            add("a flag outside the mask and no scene", BAD_FLAG[family][1], flags=BAD_FLAG[family][0], h=fresh)
        if family == NEAREST:
            add("k = 0", NEAREST_K, k=0)
            add("k = 9", NEAREST_K, k=9)
            add("k = 9 with n = 0", NEAREST_K, k=9, n=0)
            add("n * k above 2^30", NEAREST_NK, n=(1 << 27) + 1, k=8)
            # the order: everything closest points refuse, no scene included, before k
            add("no scene and k = 9", NO_SCENE, code=RT_ERR_NO_SCENE, h=fresh, k=9)
            add("a flag and k = 9", BAD_FLAG[family][1], flags=BAD_FLAG[family][0], k=9)
            add("n above the maximum and k = 9", N_RANGE[family], n=N_OVER[family], k=9)
    return rows


def test_refusal_codes_and_texts(renderer):
    import torch
    L = rtamd.lib()
    renderer.upload(rtamd.Scene.from_arrays(load_golden("cornell12")))
    h_in = np.zeros(64, U32)
    h_dirs = np.zeros(16, U32)
    h_out = np.full(512, GUARD, U32)
    d_in = torch.zeros(64, dtype=torch.int32, device="cuda")
    d_dirs = torch.zeros(16, dtype=torch.int32, device="cuda")
    d_out = torch.full((512,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    host = (h_in.ctypes.data, h_dirs.ctypes.data, h_out.ctypes.data)
    dev = (d_in.data_ptr(), d_dirs.data_ptr(), d_out.data_ptr())
    assert all(a % 16 == 0 for a in dev)
    fresh = rtamd.Renderer(0)
    try:
        rows = refusal_table(fresh._h, renderer._h, host, dev)
        assert len(rows) >= 10 * 8
        for label, h, code, text, call in rows:
            rc = call()
            got = L.rt_last_error(h)
            assert rc == code, f"{label}: code {rc}, expected {code}"
            assert got is not None and got.decode() == text, f"{label}: {got!r}, expected {text!r}"
        # n == 0 is RT_OK before any alignment test, whatever the pointers are
        for name, family, device in ENTRIES:
            if device:
                inp, dirs, out = dev
                assert invoke(name, family, device, renderer._h, inp + 4, 0, OK_FLAGS[family], out + 2, dirs=dirs + 4) == 0, name
            assert invoke(name, family, device, renderer._h, 0, 0, OK_FLAGS[family], 0, dirs=0) == 0, name
    finally:
        fresh.close()
    torch.cuda.synchronize()
    assert np.all(h_out == GUARD) and np.all(d_out.cpu().numpy().view(U32) == GUARD), "a refused call wrote to its output"
    assert np.all(h_in == 0) and np.all(d_in.cpu().numpy() == 0)
