"""The builders and the refit at the edges of mesh space, on the CPU: every
mesh of mesh_edge_common.py has the property it is made for (the depth and height lists that decide
the GPU passes' launch schedule, operands with zeros of both signs, distinct cells under subnormal
extents); the host twin rt_bvh_build_lbvh equals the NaN-correct restatement on each, per-axis and
extent-aware keys, and its output is valid and a fixed point of rt_refit_nodes; and the two
stand-alone sanitizer programs run their new meshes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lbvh_common
import lbvh_keys_common
import rtamd
from conftest import ROOT, load_golden
from mesh_edge_common import (ALL, DEPTHS, F, HEIGHTS, LATTICE, NONFINITE, TINY, POW2, ZEROS, check_valid, depth_counts, excused,
                              height_counts, mesh, np_cells_per_axis, np_keys_edge, np_lbvh, tiny_points, tree, twin, zero_mask)
from lbvh_keys_common import np_c2

PKG = os.path.join(ROOT, "real-time-opencl-raytracer_amd")

@pytest.mark.parametrize("name", LATTICE)
def test_lattice_meshes_give_the_launch_schedules_they_are_made_for(name):
    """Kept nodes per depth and per height of the twin's tree at max_leaf 1.  chain52: depth 52,
    K = 4,135; lattice4096: a depth of exactly 1,024; lattice_chain: a depth and a height of exactly
    1,025; two_scale: from the deepest a level launch, a top run, a level launch, a top run."""
    nodes, _ = twin(name, 1)
    counts, depth = depth_counts(nodes)
    heights = height_counts(nodes)
    print(f"{name}: K {(nodes.shape[0] - 1) // 2}, depth {depth}, per depth {counts}, per height {heights}")
    assert counts == DEPTHS[name]
    assert heights[:3] == HEIGHTS[name] and sum(heights) == sum(counts) == (nodes.shape[0] - 1) // 2
    if name == "chain52":
        assert depth == 52 and len(heights) == 52 and sum(counts) == 4135
    if name == "two_scale":                            # > 1,024 twice, with short depths between and above
        long = [c > 1024 for c in counts]
        assert long == [False] * 11 + [True] + [False] * 12 + [True]
    if name == "lattice4096":                          # at max_leaf 2 no list is above 1,024: one-workgroup kernels alone
        n2, _ = twin(name, 2)
        assert (n2.shape[0] - 1) // 2 == 2047
        assert depth_counts(n2)[0] == POW2[:11] and height_counts(n2) == POW2[:11][::-1]


@pytest.mark.parametrize("name", ZEROS)
def test_signed_zero_meshes_have_extremes_with_operands_of_both_signs(name):
    v, i = mesh(name)
    assert np.signbit(v[:, :3][v[:, :3] == 0]).any() and not np.signbit(v[:, :3][v[:, :3] == 0]).all()
    nodes, refs = twin(name, 1)
    hit = zero_mask(tree(name, nodes, refs), v).any(1)
    print(f"{name}: {int(hit.sum())} of {nodes.shape[0]} nodes have a zero extreme over zeros of both signs")
    assert hit.sum() >= 64


@pytest.mark.parametrize("name", TINY)
def test_tiny_meshes_keep_distinct_cells_that_a_flush_would_merge(name):
    """tiny_a (2^-136): every coordinate subnormal, the scale infinite -- cells 0 and top; tiny_b
    (2^-121): the smallest scale at which 2^13 / extent is still finite -- the whole lattice of cells,
    and no subnormal anywhere (2 (p - p_min) 2^-121 >= 2^-120), so a flush changes nothing there;
    tiny_c (2^-131): a normal extent with c2 - cmin subnormal for p - p_min < 16."""
    v, i = mesh(name)
    cells = [int(np.unique(c).size) for c in np_cells_per_axis(v, i).T]
    changed = [int((np_keys_edge(v, i, e) != np_keys_edge(v, i, e, ftz=True)).sum()) for e in (False, True)]
    print(f"{name}: distinct cells per axis {cells}, keys a flush changes (per-axis, extent) {changed}")
    assert min(cells) >= (3 if name == "tiny_b" else 2)
    if name == "tiny_b":
        assert np.abs(v[:, :3][v[:, :3] != 0]).min() >= F(2.0 ** -126) and changed == [0, 0]
    else:
        assert min(changed) >= 1
    c2, cmin, cmax = np_c2(v, i)
    ext = (cmax - cmin).astype(F)
    tiny = F(2.0 ** -126)
    assert (ext < tiny).all() if name == "tiny_a" else (ext >= tiny).all()
    if name == "tiny_c":
        assert ((c2 - cmin)[(c2 - cmin) > 0] < tiny).any()
    assert np.unique(tiny_points(), axis=0).shape[0] > 250


def test_nonfinite_huge_and_degenerate_meshes_are_what_they_say():
    with np.errstate(all="ignore"):
        c2 = {k: np_c2(*mesh("nonfinite_" + k)) for k in "abcdef"}
    assert np.isnan(mesh("nonfinite_a")[0][:, :3]).sum() == 1
    assert np.isnan(c2["b"][0]).all(1).sum() == 1                      # one triangle without a finite c2
    assert np.isnan(c2["c"][0][:, 2]).all() and np.isnan(c2["c"][1][2])   # an axis without a finite bound
    assert c2["d"][1][0] == -np.inf
    assert np.isfinite(mesh("nonfinite_e")[0]).all() and c2["e"][1][1] == -np.inf and c2["e"][2][1] == np.inf
    assert c2["f"][1][2] == -np.inf and c2["f"][2][2] == np.inf and np.isnan(c2["f"][0][:, 2]).sum() == 1
    v, _ = mesh("huge")
    assert np.abs(v[:, :3]).max() > F(2.0 ** 60) and np.abs(v[:, :3]).min() < F(2.0 ** 60)
    v, i = mesh("degenerate")
    t = i.reshape(-1, 3)
    points = (t[:, 0] == t[:, 1]) & (t[:, 1] == t[:, 2])
    segments = (t[:, 0] == t[:, 1]) & ~points
    assert points.sum() >= 128 and segments.sum() >= 128 and (t[:, 0] == 0).sum() == 32


@pytest.mark.parametrize("name", ALL)
def test_edge_keys_restate_the_shared_ones(name):
    """np_keys_edge is lbvh_keys_common's extent-aware restatement, and lbvh_common's per-axis one
    where that one is defined (a finite scale)."""
    v, i = mesh(name)
    assert np.array_equal(np_keys_edge(v, i, True), lbvh_keys_common.np_keys_extent(v, i))
    if name not in NONFINITE + ["tiny_a", "tiny_c"]:
        assert np.array_equal(np_keys_edge(v, i, False), lbvh_common.np_keys(v, i))


@pytest.mark.parametrize("extent", [False, True], ids=["axis", "extent"])
@pytest.mark.parametrize("max_leaf", [1, 4, 8])
@pytest.mark.parametrize("name", ALL)
def test_twin_equals_the_restatement_is_valid_and_a_fixed_point_of_the_refit(name, max_leaf, extent):
    """All 48 bytes of every node and every reference; on the meshes with zeros of both signs under
    the zero rule.  check_valid's structural conditions, boxes compared as words.  rt_refit_nodes
    with the same vertices changes nothing, under the same equality."""
    v, i = mesh(name)
    zeros = name in ZEROS
    nodes, refs = twin(name, max_leaf, extent)
    want_nodes, want_refs = np_lbvh(v, i, max_leaf, extent)
    assert np.array_equal(refs, want_refs)
    mask = zero_mask(tree(name, want_nodes, want_refs), v) if zeros else None
    n1 = excused(nodes, want_nodes, mask, f"{name}: twin against the restatement")
    K, depth, n2 = check_valid(v, i, nodes, refs, max_leaf, extent, zeros)
    assert K == (nodes.shape[0] - 1) // 2 and depth == depth_counts(nodes)[1]
    d = dict(load_golden("cornell12"), vertices=v, indices=i, nodes=nodes, tri_indices=refs)
    again = rtamd.refit_nodes(rtamd.Scene.from_arrays(d), v)
    n3 = excused(again, nodes, mask, f"{name}: rt_refit_nodes of the twin's output")
    print(f"{name} max_leaf {max_leaf} {'extent' if extent else 'axis'}: K {K}, depth {depth}, words excused by the "
          f"zero rule: restatement {n1}, check_valid {n2}, refit {n3}")


def _sanitized(tmp_path, source, main):
    exe = str(tmp_path / main[:-4])
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(PKG, "csrc", "host"), os.path.join(PKG, "csrc", "host", source),
                    os.path.join(ROOT, "tests", main), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ALL OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    return p.stdout


@pytest.mark.parametrize("source,main,lines", [
    ("lbvh_builder.cpp", "lbvh_sanitize_main.cpp",
     ["chain52 (max_leaf 1): ok, 8271 nodes, depth 52", "chain52 extent keys (max_leaf 1): ok", "nan coordinate (max_leaf 1): ok",
      "nan axis (max_leaf 4): ok", "overflowing c2 (max_leaf 1): ok"]),
    ("refit.cpp", "refit_sanitize_main.cpp",
     ["chain52: ok, 52 heights", "nan coordinate: ok, 52 heights", "nan axis: ok, 52 heights",
      "overflowing c2: ok, 52 heights"])])
def test_sanitizer_programs_run_the_edge_meshes(tmp_path, source, main, lines):
    """The two stand-alone AddressSanitizer + UndefinedBehaviorSanitizer programs, as test_lbvh.py
    and test_refit.py build them, with chain52 and nonfinite (a), (c) and (e)."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = _sanitized(tmp_path, source, main)
    for what in lines:
        assert what in out, (what, out[-2000:])
