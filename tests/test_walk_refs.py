"""The walk references' host twin (rtamd::derive_walk in csrc/host/scene_encode.cpp, rtrec::walk_ref in
csrc/rt_records.h) alone under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "real-time-opencl-raytracer_amd")


def test_walk_refs_host_twin_under_asan_ubsan(tmp_path):
    """csrc/host/scene_encode.cpp + tests/walk_refs_sanitize_main.cpp, every sanitizer report fatal:
    leaves of 1, 2, 15, 16 and 17 references, an empty leaf, escape leaves of 40 and 35, root leaves,
    kRefError; every walk reference decodes back to the present reference's (offset, count), and a
    scene has none exactly for the 17-reference, escape and error cases."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "walk_refs_sanitize")
    host = os.path.join(PKG, "csrc", "host")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(ROOT, "include"), "-I", host,
                    "-I", os.path.join(PKG, "csrc"), os.path.join(host, "scene_encode.cpp"),
                    os.path.join(ROOT, "tests", "walk_refs_sanitize_main.cpp"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ALL OK" in p.stdout and "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    for what in ("leaves of 1 2 15 16: walk", "a leaf of 17: no walk", "17 last: no walk", "an empty leaf: walk",
                 "no references: walk", "escape leaves 40 and 35: no walk", "root leaf of 1: walk", "root leaf of 16: walk",
                 "root leaf of 17: no walk", "root escape leaf of 31: no walk", "kRefError child: no walk",
                 "kRefError root: no walk", "hostile references: ok"):
        assert what in p.stdout, what
