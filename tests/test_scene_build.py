"""rt_build_scene without a GPU: the header declares the four entry points, the
library exports them, the ABI version stays 3, and each refuses a NULL context before any device
call."""
import ctypes as C
import os
import re
import subprocess

import rtamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["rt_build_scene", "rt_build_scene_device", "rt_last_scene_build_timing", "rt_refit_level_counts"]
RT_ERR_INVALID_ARG = -1


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", rtamd.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", out))
    for name in ENTRY_POINTS:
        assert re.search(r"^int\s+%s\s*\(" % name, txt, flags=re.M), name
        assert name in exported and hasattr(rtamd.lib(), name), name
        assert name in rtamd.ABI_SYMBOLS
    assert rtamd.lib().rt_abi_version() == 3   # additive: no version bump


def test_a_null_context_is_an_invalid_argument():
    lib = rtamd.lib()
    buf = (C.c_uint32 * 64)()
    p = C.cast(buf, C.c_void_p)                # never dereferenced: the context is checked first
    assert lib.rt_build_scene(None, p, 3, p, 3, 2, p, 3, p, p, 1, p) == RT_ERR_INVALID_ARG
    assert b"NULL" in lib.rt_last_error(None)
    assert lib.rt_build_scene_device(None, p, 3, p, 3, 2, p, 3, p, p, 1, p, None) == RT_ERR_INVALID_ARG
    ms, h = C.c_float(), C.c_int32()
    assert lib.rt_last_scene_build_timing(None, C.byref(ms)) == RT_ERR_INVALID_ARG
    assert lib.rt_refit_level_counts(None, buf, 64, C.byref(h)) == RT_ERR_INVALID_ARG


def test_renderer_has_the_python_side():
    for name in ("build_scene", "last_scene_build_ms", "refit_level_counts"):
        assert callable(getattr(rtamd.Renderer, name)), name
