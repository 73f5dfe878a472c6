"""The extent-aware Morton keys on the CPU: rt_bvh_build_lbvh with
RT_BUILD_EXTENT_KEYS byte for byte against a numpy restatement of the plan, the cells and the key
(lbvh_keys_common); the validity of its output; nothing changed without the flag; the SAH cost the
definition must reach on the flat heightfield; the refused values; and lbvh_builder.cpp with the
flag alone under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtamd
from conftest import ROOT
from lbvh_common import mesh as base_mesh, np_lbvh, twin
from lbvh_keys_common import (ALL, EXTENT, SMALL, check_valid_extent, mesh, np_cost, np_keys_extent, np_lbvh_extent,
                              plan_bits, twin_extent)

PKG = os.path.join(ROOT, "real-time-opencl-raytracer_amd")
RT_ERR_INVALID_ARG = -1


def _same(got, want, label):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, label
    assert np.array_equal(got[1], want[1]), f"{label}: references"
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{label}: nodes"


@pytest.mark.parametrize("max_leaf", [1, 4])
@pytest.mark.parametrize("name", SMALL)
def test_twin_with_the_flag_equals_the_numpy_restatement(name, max_leaf):
    """All 48 bytes of every node, and every reference.  copies70: no extent at all, the cap alone
    decides the plan; grid16: y gets no bit; needle: the 20-bit cap binds; nonfinite: an infinite
    extent counts as none; cubes2_obj: three different bit counts."""
    v, i = mesh(name)
    _same(twin_extent(name, max_leaf), np_lbvh_extent(v, i, max_leaf), f"{name} max_leaf {max_leaf}")


def test_the_plans_of_the_degenerate_meshes():
    assert plan_bits(*mesh("copies70")) == [20, 19, 0]
    assert plan_bits(*mesh("grid16")) == [20, 0, 19]
    assert plan_bits(*mesh("needle")) == [20, 10, 9]
    assert plan_bits(*mesh("nonfinite"))[0] == 0
    assert plan_bits(*mesh("cubes2_obj")) == [15, 10, 14]
    assert plan_bits(*mesh("deep40")) == [13, 13, 13]


@pytest.mark.parametrize("name", ALL)
def test_twin_output_with_the_flag_is_valid(name):
    """lbvh_common.check_valid with the key order taken from the new keys."""
    v, i = mesh(name)
    n = i.size // 3
    for max_leaf in ((1, 4, 8) if n <= 4096 else (4,)):
        nodes, refs = twin_extent(name, max_leaf)
        K, depth = check_valid_extent(v, i, nodes, refs, max_leaf)
        assert K == (nodes.shape[0] - 1) // 2 and depth <= 64
    assert np.unique(np_keys_extent(v, i)).size == n                # keys stay unique


# sha256 over nodes then tri_indices of rt_bvh_build_lbvh WITHOUT the flag at max_leaf 4, recorded
# from the library before this option existed
PARENT_DIGESTS = {
    "cornell12": "80b45b1465b0a9fb68ba4f2cf99a116e883a2ad959ca84b8eb553c8221f70294",
    "grid16": "a9c74ed1907e982033ae938455bbe27b9d696dc0630fcb0bb5e4c4a020adf54b",
    "rand2k": "c8425cebe043e1f299c046b1676f5a66275bfc4c67d703a76ef498f7029dfdee",
    "hf40k": "382dbd3b80bc2db51eeffa5d06a5cb93f7a8ff480fe63309f9c2b4b590e63074",
    "cubes2_obj": "2ede036931de007f744ae4b78dbb4372647911835565254313565077cc4e47f3",
}


def _digest(tree):
    return hashlib.sha256(np.ascontiguousarray(tree[0]).tobytes() + np.ascontiguousarray(tree[1]).tobytes()).hexdigest()


@pytest.mark.parametrize("name", sorted(PARENT_DIGESTS))
def test_without_the_flag_the_twin_is_unchanged(name):
    """The bytes recorded before the option existed; and, on meshes with unequal extents, not the
    bytes of the extent-aware keys (the flag does something)."""
    assert _digest(twin(name, 4)) == PARENT_DIGESTS[name]
    if name in ("hf40k", "cubes2_obj"):   # (grid16's x and z extents are equal: finer cells, the same order)
        assert _digest(twin_extent(name, 4)) != PARENT_DIGESTS[name]
    v, i = base_mesh(name)
    if i.size // 3 <= 4096:
        _same(twin(name, 4), np_lbvh(v, i, 4), f"{name}: the per-axis restatement")


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
def test_equal_extents_give_the_per_axis_keys(max_leaf):
    _same(twin_extent("deep40", max_leaf), twin("deep40", max_leaf), f"deep40 max_leaf {max_leaf}")


@pytest.mark.parametrize("max_leaf", [1, 4])
def test_sah_cost_on_the_flat_heightfield(max_leaf):
    """A condition on the definition: with the flag the normalised SAH cost of the twin's tree over
    hf40k (extent 396 x 32 x 398) is at most 0.75 of the cost without it (the restatement gives
    0.61 at max_leaf 1 and 0.60 at 4)."""
    axis, extent = np_cost(twin("hf40k", max_leaf)[0]), np_cost(twin_extent("hf40k", max_leaf)[0])
    print(f"hf40k max_leaf {max_leaf}: per-axis {axis:.2f}, extent-aware {extent:.2f}, ratio {extent / axis:.3f}")
    assert extent <= 0.75 * axis


def test_refused_values():
    m = rtamd.Mesh.cornell()
    for bad in (EXTENT | 0, EXTENT | 9, 0x200 | 4, 0x10000 | EXTENT | 4, -1):
        with pytest.raises(rtamd.RtError) as e:
            m.build_lbvh(bad)
        assert e.value.code == RT_ERR_INVALID_ARG, hex(bad)
    with pytest.raises(ValueError):
        m.build_lbvh(4, keys="morton")
    h = C.c_void_p()
    assert rtamd.lib().rt_bvh_build_lbvh(m._h, EXTENT | 4, C.byref(h)) == 0
    rtamd.lib().rt_bvh_destroy(h)
    assert rtamd.RT_BUILD_EXTENT_KEYS == EXTENT and rtamd.lib().rt_abi_version() == 3
    dbl = C.c_double()
    assert rtamd.lib().rt_scene_sah(None, C.byref(dbl), C.byref(dbl), C.byref(dbl)) == RT_ERR_INVALID_ARG


def test_lbvh_builder_cpp_with_the_flag_alone_under_asan_ubsan(tmp_path):
    """csrc/host/lbvh_builder.cpp + tests/lbvh_keys_sanitize_main.cpp, every sanitizer report fatal."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "lbvh_keys_sanitize")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(PKG, "csrc", "host"), os.path.join(PKG, "csrc", "host", "lbvh_builder.cpp"),
                    os.path.join(ROOT, "tests", "lbvh_keys_sanitize_main.cpp"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ALL OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    for what in ("plans: ok", "single (max_leaf 1): ok", "coincident (max_leaf 4): ok", "flat (max_leaf 1): ok",
                 "needle (max_leaf 1): ok", "one infinite vertex (max_leaf 4): ok", "non-finite: ok", "refusals: ok"):
        assert what in p.stdout, what
