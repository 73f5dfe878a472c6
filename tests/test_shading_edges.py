"""Shading at its edges on the CPU: the classes of tests/shading_edge_common.py reach
their edges by the oracle's own output, and the oracle's shading equals a float64 restatement written
from volumeRender.cl on every hit pixel of the regular cases.  tests/test_shading_edges_gpu.py then holds
the kernels to the oracle on the same cases.  Run with -s for the per-class pixel counts and the
measured differences."""
import numpy as np
import pytest

import shading_edge_common as S

RGB_TOL = 1e-4   # the project's bar for float RGB (tests/test_fullsize_gpu.py)

# np_shade against oracle.render(depth=1, RT_FLAG_NO_SHADOW): the largest absolute rgb difference over
# every hit pixel of a group's cases, measured on an x86-64 host, and the bound, twice that value.
#   group      measured    bound     cases
#   light      9.79e-06    1.96e-05  the seven light positions (1e30 too: float64 does not overflow there)
#   normals    3.51e-06    7.02e-06  lengths 1e-3 and 1e3
#   albedo     5.11e-06    1.02e-05  0 / -0.0 / 0.5, and four materials up to 2.0
#   det        2.35e-06    4.70e-06  the open stage where it is built, floor at y = -4
#   det_1e4    5.14e-01    1.03      the same stage translated by (1e4, 1e4, 1e4)
# The first four are float32's rounding of colours up to 2.8 and stay well below RGB_TOL.  det_1e4 is
# no rounding noise: get_normal_at_tri_point solves for the barycentrics by Cramer's rule on ABSOLUTE
# positions (volumeRender.cl:35-43), so at 1e4 its determinants are sums of terms near 1e12 that cancel
# to about 1e5, and float32 keeps one or two digits of the numerators.  On the patch, whose vertex
# normals differ, the interpolated normal is then off by tens of degrees (319 of its 563 pixels differ
# by more than 1e-3); the floor and the cube, whose normals hardly vary, stay within 2.6e-4.  That is
# the reference's own arithmetic, which the oracle restates (test_shading_edges_gpu.py holds S_ref to
# the reference kernel run live on this very case); float64 does not cancel, hence the difference.
# The bound says only that nothing worse happens there.
NP_SHADE_MEASURED = {"light": 9.79e-06, "normals": 3.51e-06, "albedo": 5.11e-06, "det": 2.35e-06, "det_1e4": 5.14e-01}
NP_SHADE_BOUND = {g: 2.0 * v for g, v in NP_SHADE_MEASURED.items()}


def test_the_case_list_is_the_static_one():
    """The labels the tests are parametrised with (no scene is built at collection) are the generators'."""
    assert S.LABELS == S.labels()
    assert sorted({c.cls for c in S.cases()}) == sorted(S.CLASSES)


@pytest.mark.parametrize("cls", S.CLASSES)
def test_every_class_reaches_its_edge(cls):
    """Each case's predicate on the oracle's aux output holds on at least MIN_PIXELS pixels (the depth
    cases: on more than half the frame)."""
    for c in S.cases():
        if c.cls != cls:
            continue
        n, need = c.predicate(c)
        f = S.frames(c)["d"]
        print(f"{c.label}: {n} pixels satisfy the predicate (need {need}); {int((f['hits'][:, 0, 0] >= 0).sum())} of "
              f"{c.w * c.h} primary rays hit, ray_depth counts {np.bincount(S.ray_depth(f), minlength=c.depth + 1).tolist()}")
        assert need >= S.MIN_PIXELS and n >= need, c.label
        assert f["stats"]["stack_overflow"] == 0, c.label


@pytest.mark.parametrize("group", S.REGULAR_GROUPS)
def test_oracle_shading_equals_the_float64_restatement(group):
    """oracle.render(depth=1, RT_FLAG_NO_SHADOW) against np_shade on every hit pixel of every regular
    case of the group: no pixel is left out, a pixel the restatement has no finite colour for fails."""
    worst = 0.0
    some = False
    for c in S.cases():
        if c.regular != group:
            continue
        some = True
        f = S.frames(c)["d1ns"]
        want, _ = S.detail(c)
        hit = f["hits"][:, 0, 0] >= 0
        assert int(hit.sum()) >= S.MIN_PIXELS
        assert np.all(np.isfinite(want[hit])) and np.all(np.isfinite(f["rgb"][hit])), c.label
        assert np.all(f["rgb"][~hit] == 0)
        diff = float(np.max(np.abs(f["rgb"][hit].astype(np.float64) - want[hit])))
        print(f"{c.label}: {int(hit.sum())} hit pixels, largest |oracle - np_shade| = {diff:.3e} "
              f"(largest colour {float(want[hit].max()):.3g})")
        worst = max(worst, diff)
    assert some
    print(f"group {group}: measured {worst:.3e}, recorded {NP_SHADE_MEASURED[group]:.3e}, bound {NP_SHADE_BOUND[group]:.3e}")
    assert worst <= NP_SHADE_BOUND[group]
    if group != "det_1e4":
        assert NP_SHADE_BOUND[group] <= RGB_TOL


def test_regular_cases_are_the_ones_named():
    """The regular cases: the finite light positions, normals of length 1e-3 to 1e3, albedo in [0, 2],
    det where the stage is built and at the 1e4 offset."""
    reg = {c.label: c.regular for c in S.cases() if c.regular}
    assert {k for k, g in reg.items() if g == "light"} == {c.label for c in S.cases() if c.cls == "light"}
    assert {k for k, g in reg.items() if g == "normals"} == {"normals/length_1e-3", "normals/length_1e3"}
    assert {k for k, g in reg.items() if g == "det"} == {"det/base"}
    assert {k for k, g in reg.items() if g == "det_1e4"} == {"det/offset_1e4"}
    for k, g in reg.items():
        if g == "albedo":
            a = S.case(k).scene["materials"][:, S.DIFFUSE]
            assert np.all((a >= 0) & (a <= 2))
    assert np.all(np.isfinite(np.concatenate([S.case(k).params[16:19] for k in reg])))


def test_material_words_other_than_diffuse_change_nothing():
    """The second copy, with every material word other than .diffuse filled with random bit patterns (NaN
    patterns and the technique words included), renders the first copy's frame in every word."""
    a, b = S.case("albedo/several_materials"), S.case("albedo/several_materials_scrambled")
    wa, wb = a.scene["materials"].view(np.uint32), b.scene["materials"].view(np.uint32)
    assert np.array_equal(wa[:, 12:16], wb[:, 12:16])
    other = np.delete(np.arange(44), np.arange(12, 16))
    assert np.all(np.any(wa[:, other] != wb[:, other], axis=1))
    assert np.any(np.isnan(b.scene["materials"][:, other])) and np.any(wb[:, :4] != 0)
    for k in a.scene:
        assert k == "materials" or a.scene[k].tobytes() == b.scene[k].tobytes()
    for which in ("d", "d1", "d1ns"):
        fa, fb = S.frames(a)[which], S.frames(b)[which]
        assert np.array_equal(fa["out"], fb["out"]) and np.array_equal(fa["hits"], fb["hits"])
        assert np.array_equal(S.bits(fa["t"]), S.bits(fb["t"])) and np.array_equal(S.bits(fa["rgb"]), S.bits(fb["rgb"]))


def test_the_truncation_boundary_is_sampled():
    """pack/gradient: color * 255 falls within 1e-3 of an integer on at least MIN_PIXELS pixels, on both
    sides of it, and the packed byte is the truncation (volumeRender.cl:186-195) on every pixel."""
    c = S.case("pack/gradient")
    f = S.frames(c)["d1ns"]
    near = S.near_integer(f)
    print(f"pack/gradient: {int(near.sum())} pixels within 1e-3 of a packed step")
    assert int(near.sum()) >= S.MIN_PIXELS
    x = f["rgb"] * np.float32(255.0)
    want = np.clip(x, 0, 255).astype(np.uint32)   # finite colours here: truncation toward zero
    got = np.stack([f["out"] & 0xFF, (f["out"] >> 8) & 0xFF, (f["out"] >> 16) & 0xFF], axis=1)
    assert np.array_equal(got, want)
    below, above = near & np.any(x < np.rint(x), axis=1), near & np.any(x >= np.rint(x), axis=1)
    assert below.any() and above.any()
    assert len(np.unique(got[near])) >= 2, "both sides of the step reach the packed pixels"


def test_non_finite_colours_pack_as_the_reference_clamp_does():
    """rgbToInt's clamp (volumeRender.cl:186-195) in the oracle's arithmetic, fmin(fmax(x, 0), 255): a
    NaN channel packs 0, +inf 255, a negative one 0, on the cases that produce them."""
    for label, ch, test, byte in (("albedo/nan", 0, np.isnan, 0), ("albedo/3e38", 0, np.isposinf, 255),
                                  ("albedo/minus_half", 0, lambda v: v < 0, 0)):
        f = S.frames(S.case(label))["d"]
        with np.errstate(invalid="ignore"):
            m = test(f["rgb"][:, ch])
        assert int(m.sum()) >= S.MIN_PIXELS, label
        assert np.all(((f["out"][m] >> (8 * ch)) & 0xFF) == byte), label
