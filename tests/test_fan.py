"""Occlusion fans without a GPU: the inputs of the GPU tests have the properties those
tests rely on; rt_fan_expand, the definition in host code, equals the plain-C restatement of
tests/fan_ref.c in every ray word and every traced flag, on the inputs and at the edges of the rule;
the flag agrees with the float64 sign of dot(n, d) wherever that is not marginal; the mask layout
packs and unpacks; the refusals that need no GPU; and rt_fan_expand alone under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/fan_expand_sanitize_main.cpp, a program of its own)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtamd
import fan_common as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-opencl-raytracer_amd")
INVALID = -1


def ray_words(rays):
    return np.ascontiguousarray(rays).view(np.uint8).reshape(-1).view(np.uint32).reshape(-1, 8)


def assert_expand_equals_ref(rec, dirs, label):
    rays, traced = rtamd.fan_expand(rec, dirs)
    want_rays, want_traced = F.ref_expand(rec, dirs)
    bad = np.flatnonzero(np.any(ray_words(rays) != want_rays, axis=1))
    assert bad.size == 0, f"{label}: {bad.size} rays differ in a word, first {bad[:5]}"
    bad = np.flatnonzero(traced != want_traced)
    assert bad.size == 0, f"{label}: {bad.size} traced flags differ, first {bad[:5]}"
    return want_rays, want_traced


@pytest.mark.parametrize("name", F.SCENES)
def test_inputs_have_the_properties_the_gpu_tests_rely_on(name):
    """Per scene, with the oracle alone: at least 10 % of the traced bits are set and at least 10 % are
    clear under both tmax settings; at least 40 % of the rays are culled; no stack overflows; and any hit
    agrees with closest hit on hit or miss for every traced ray."""
    from oracle import oracle
    x = F.inputs(name)
    assert x["origins"].shape[0] >= 100
    for setting in ("default", "quarter"):
        masks, traced, hit, stats = F.yardstick(name, setting)
        share = hit[traced].mean()
        print(f"{name} {setting}: {x['origins'].shape[0]} origins, traced {traced.mean():.3f}, set {share:.3f}")
        assert 0.10 <= share <= 0.90
        assert 1.0 - traced.mean() >= 0.40
        assert stats["stack_overflow"] == 0
        rays, flat = F.ref_expand(F.records(name, setting), x["dirs"])
        ids, _, _ = oracle.trace_rays(x["d"], rays[flat], any_hit=False)
        assert np.array_equal(ids >= 0, hit[traced]), "any hit and closest hit disagree on hit or miss"
    _, traced, _, _ = F.yardstick(name, "nocull")
    assert traced.all()


@pytest.mark.parametrize("name", F.SCENES)
def test_expand_equals_the_c_restatement_on_the_inputs(name):
    x = F.inputs(name)
    for setting in F.SETTINGS:
        assert_expand_equals_ref(F.records(name, setting), x["dirs"], f"{name} {setting}")


def test_expand_equals_the_c_restatement_at_the_edges():
    """The edge set: every class of normal, tmax and direction meets every other.  Beyond equality with
    fan_ref.c, the rule's own consequences are spelled out for a few of them."""
    rec, dirs = F.edge_records(), F.edge_dirs()
    rays, traced = assert_expand_equals_ref(rec, dirs, "edge set")
    n, k = rec.shape[0], dirs.shape[0]
    traced = traced.reshape(n, k)
    assert traced.any() and not traced.all()
    tm, nr = rec["tmax"], rec["n"]
    assert not traced[np.isnan(tm) | (tm <= np.float32(0.001))].any(), "tmax 0.001, NaN, 0 and -1 trace nothing"
    assert not traced[~np.all(np.isfinite(nr), axis=1)].any(), "a non-finite normal traces nothing"
    assert not traced[~np.all(np.isfinite(rec["o"]), axis=1)].any()
    bad_dir = ~np.all(np.isfinite(dirs), axis=1) | np.all(dirs == 0, axis=1)
    assert not traced[:, bad_dir].any(), "zero, NaN and inf directions trace nothing"
    good = (tm > np.float32(0.001)) & np.all(np.isfinite(rec["o"]), axis=1)
    zero_n = np.all(nr == 0, axis=1)   # either sign of zero
    assert traced[np.ix_(good & zero_n, ~bad_dir)].all(), "a zero normal of either sign culls nothing"
    big = np.all(nr == np.float32(1e30), axis=1) & good
    j_big = int(np.flatnonzero(np.all(dirs == np.float32(1e30), axis=1))[0])
    j_neg = int(np.flatnonzero(np.all(dirs == np.float32(-1e30), axis=1))[0])
    assert big.any() and traced[big, j_big].all() and not traced[big, j_neg].any(), "the dot overflows to +-inf"
    mixed = (nr[:, 0] == np.float32(1e30)) & (nr[:, 1] == np.float32(-1e30)) & good
    # nx dx rounds to +inf; the fmas' own products are exact and finite, so no inf - inf arises: +inf stays
    assert mixed.any() and traced[mixed, j_big].all() and not traced[mixed, j_neg].any(), "the first product's inf decides"
    sub = (nr[:, 0] == np.float32(1e-45)) & good
    j_x = int(np.flatnonzero(np.all(dirs == np.array([1, 0, 0], np.float32), axis=1))[0])
    assert traced[sub, j_x].all(), "a subnormal normal is not flushed"
    # the ray words: the origin record's first four words and the direction's three, reserved 0
    w = rays.reshape(n, k, 8)
    assert np.array_equal(w[:, :, :4], np.broadcast_to(F.origin_words(rec)[:, None, :4], (n, k, 4)))
    assert np.array_equal(w[:, :, 4:7], np.broadcast_to(F.dir_words(dirs)[None, :, :3], (n, k, 3)))
    assert not w[:, :, 7].any()


@pytest.mark.parametrize("name", F.SCENES)
def test_flag_agrees_with_the_float64_sign(name):
    x = F.inputs(name)
    _, traced = F.ref_expand(F.records(name, "default"), x["dirs"])
    n64, d64 = x["normals"].astype(np.float64), x["dirs"].astype(np.float64)
    dot = n64 @ d64.T
    clear = np.abs(dot) > 1e-3 * np.linalg.norm(n64, axis=1)[:, None] * np.linalg.norm(d64, axis=1)[None, :]
    assert clear.mean() > 0.9   # (the comparison below is not vacuous; cubes2_obj's axis normals meet direction 0's zero y)
    assert np.array_equal(traced.reshape(dot.shape)[clear], (dot > 0)[clear])


@pytest.mark.parametrize("k", [1, 31, 32, 33, 64, 65])
def test_pack_and_unpack_round_trip(k):
    rng = np.random.default_rng(k)
    n = 37
    bits = rng.integers(0, 2, (n, k)).astype(bool)
    bits[:, k - 1] = True
    masks = rtamd.fan_pack(bits)
    assert masks.shape == ((k + 31) // 32, n) and masks.dtype == np.uint32
    assert np.array_equal(masks, F.pack_bits(bits))
    assert np.array_equal(rtamd.fan_bits(masks, k), bits)
    if k % 32:
        assert not np.any(masks[-1] >> np.uint32(k % 32)), "the bits j >= k of the last word are 0"
    i, j = 5, k - 1
    assert (int(masks[j >> 5, i]) >> (j & 31)) & 1 == 1


def test_refusals_that_need_no_gpu():
    L = rtamd.lib()
    rec = rtamd.pack_fan_origins(np.zeros((2, 3), np.float32))
    dirs = rtamd.pack_fan_dirs(np.ones((3, 3), np.float32))
    masks = np.zeros(2, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rt_trace_fan(None, vp(rec), 2, vp(dirs), 3, 0, vp(masks)) == INVALID
    assert L.rt_trace_fan_device(None, vp(rec), 2, vp(dirs), 3, 0, vp(masks), None) == INVALID
    rays = np.zeros(6, rtamd.RAY_DTYPE)
    traced = np.full(6, 7, np.uint8)
    for n in (-1, (1 << 26) + 1, 1 << 62):
        assert L.rt_fan_expand(vp(rec), n, vp(dirs), 3, vp(rays), vp(traced)) == INVALID
    for k in (0, -1, rtamd.RT_FAN_MAX_DIRS + 1, -(1 << 31)):
        assert L.rt_fan_expand(vp(rec), 2, vp(dirs), k, vp(rays), vp(traced)) == INVALID
    assert L.rt_fan_expand(None, 2, vp(dirs), 3, vp(rays), vp(traced)) == INVALID
    assert L.rt_fan_expand(vp(rec), 2, None, 3, vp(rays), vp(traced)) == INVALID
    assert L.rt_fan_expand(vp(rec), 2, vp(dirs), 3, None, vp(traced)) == INVALID
    assert L.rt_fan_expand(vp(rec), 2, vp(dirs), 3, vp(rays), None) == INVALID
    assert np.all(traced == 7) and not rays.view(np.uint32).any(), "a refused call writes nothing"
    assert L.rt_fan_expand(None, 0, None, 0, None, None) == 0, "n == 0 is RT_OK"
    assert L.rt_fan_expand(vp(rec), 2, vp(dirs), 3, vp(rays), vp(traced)) == 0
    assert np.all(traced == 1)   # zero normals, default tmax, direction (1, 1, 1)
    assert rtamd.lib().rt_abi_version() == 3


def test_fan_expand_is_clean_under_asan_ubsan(tmp_path):
    """csrc/host/fan_expand.cpp and tests/fan_expand_sanitize_main.cpp, compiled together with every
    sanitizer report fatal and run as a program of their own: the edge set, buffers of exactly n * k
    records, and hostile sizes, which must be refused before a byte is touched."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "fan_expand_sanitize_main")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(PKG, "csrc", "host", "fan_expand.cpp"), os.path.join(ROOT, "tests", "fan_expand_sanitize_main.cpp"),
                    "-lm"], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "ALL OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
