"""The yardstick of the attribute ray query, pinned to the oracle on the CPU.

tests/hit_attr_ref.c's records are right if a path continued from them is the oracle's own path:
fed the oracle's bounce-0 ids and t of a frame, its records alone (with the primary rays and the
light) must rebuild the frame's reflection and shadow rays so exactly that the oracle's ray query
returns the frame's own bounce-1 ids, every bit of its bounce-1 t, and its bounce-0 shadow ids.
That covers p and ns; u and v come from the same lines as Moller-Trumbore's t, which is compared
with the traversal's; ng and ndotd are checked against the winding in float64."""
import ctypes as C

import numpy as np
import pytest

import rtamd
from hit_attr_common import (ID, NDOTD, NG, P, T, TMAX_WORD, U, V, miss_words, oracle_frame, ray_words, ref_hit_attr,
                             ref_next_rays, ref_normalize, words)
from ray_query_common import oracle_normalize, oracle_ray_tri

SCENES = ["cornell12", "rand2k", "hf40k", "knot16k", "cubes2_obj"]
RT_ERR_INVALID_ARG = -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", SCENES)
def test_records_continue_the_oracles_frame(name):
    from oracle import oracle
    f = oracle_frame(name)
    d, p, rays, ref = f["d"], f["params"], f["rays"], f["ref"]
    ids0 = ref["hits"][:, 0, 0].copy()
    t0 = ref["t"][:, 0].copy()
    hit = ids0 >= 0
    ids0[~hit] = -1                                           # untraced pixels (-2) count as misses
    attrs, t_mt = ref_hit_attr(d, rays, ids0, t0, want_t=True)
    assert np.array_equal(attrs[~hit], miss_words(rays)[~hit])
    assert np.array_equal(attrs[hit, ID].view(np.int32), ids0[hit]) and np.array_equal(attrs[hit, T], bits(t0[hit]))
    # Moller-Trumbore's t by the helper's lines is the traversal's, in every bit
    assert np.array_equal(bits(t_mt[hit]), bits(t0[hit])), f"{name}: the recomputed t differs from the traversal's"
    refl, shadow = ref_next_rays(rays, attrs, p[16:19])
    # bounce 1: closest hit of the reflection rays
    ids1, t1, _ = oracle.trace_rays(d, refl)
    want1, want_t1 = ref["hits"][hit, 1, 0], ref["t"][hit, 1]
    assert int((want1 >= 0).sum()) >= 100, f"{name}: only {int((want1 >= 0).sum())} bounce-1 hits"
    assert np.array_equal(ids1[hit], want1), f"{name}: {int((ids1[hit] != want1).sum())} bounce-1 ids differ"
    assert np.array_equal(bits(t1[hit]), bits(want_t1)), f"{name}: bounce-1 t differs"
    assert np.all(ids1[~hit] == -1)
    # bounce 0's shadow rays: any hit
    sid, _, _ = oracle.trace_rays(d, shadow, any_hit=True)
    want_s = ref["hits"][hit, 0, 1]
    if name != "hf40k":
        assert int((want_s >= 0).sum()) >= 100, f"{name}: only {int((want_s >= 0).sum())} shadowed pixels"
    assert np.array_equal(sid[hit], want_s), f"{name}: {int((sid[hit] != want_s).sum())} shadow ids differ"
    # both faces are hit where the scene has them
    nd = attrs[hit, NDOTD].view(np.float32)
    if name in ("cornell12", "rand2k"):
        assert int((nd < 0).sum()) >= 500 and int((nd > 0).sum()) >= 500, (name, int((nd < 0).sum()), int((nd > 0).sum()))


@pytest.mark.parametrize("name", SCENES)
def test_uv_and_geometric_normal_against_float64(name):
    """A gross-error check (a swapped u and v, a flipped or unnormalised ng), not a precision claim: u, v
    and ng lose digits on grazing rays and sliver triangles, so the bounds are on the median (u, v: a swap
    would move most points by a good part of their triangle) and on the 99th percentile (ng, ndotd)."""
    f = oracle_frame(name)
    d, rays, ref = f["d"], f["rays"], f["ref"]
    ids0, t0 = ref["hits"][:, 0, 0], ref["t"][:, 0]
    hit = np.flatnonzero(ids0 >= 0)
    a = ref_hit_attr(d, rays, np.where(ids0 >= 0, ids0, -1), t0)[hit]
    r = ray_words(rays)[hit]
    v = d["vertices"][:, :3].astype(np.float64)
    tri = d["indices"][ids0[hit][:, None] + np.arange(3)[None, :]]
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    u, vv = a[:, U].view(np.float32).astype(np.float64), a[:, V].view(np.float32).astype(np.float64)
    assert np.all(u >= 0) and np.all(vv >= 0) and np.all(u + vv <= 1.0), "an accepted hit passed ray_tri's tests"
    dn = r[:, 4:7].astype(np.float64)
    dn /= np.linalg.norm(dn, axis=1)[:, None]
    surface = r[:, 0:3].astype(np.float64) + dn * t0[hit].astype(np.float64)[:, None]
    bary = (1.0 - u - vv)[:, None] * p0 + u[:, None] * p1 + vv[:, None] * p2
    scale = np.abs(v).max() + np.abs(r[:, 0:3]).max() + t0[hit].max()
    assert np.median(np.abs(bary - surface).max(axis=1)) <= 1e-5 * scale, "u, v do not give the hit point"
    pp = a[:, P:P + 3].view(np.float32).astype(np.float64)
    assert np.max(np.abs(pp - (surface - 0.001 * dn))) <= 1e-5 * scale, "p is not 0.001 short of the surface"
    g = np.cross(p1 - p0, p2 - p0)
    g /= np.linalg.norm(g, axis=1)[:, None]
    ng = a[:, NG:NG + 3].view(np.float32).astype(np.float64)
    assert np.percentile(np.abs(ng - g).max(axis=1), 99) <= 1e-4, "ng is not the winding's unit normal"
    assert np.percentile(np.abs(a[:, NDOTD].view(np.float32) - np.sum(g * dn, axis=1)), 99) <= 1e-4


def test_helper_normalize_and_t_are_the_oracles():
    f = oracle_frame("rand2k")
    d, rays, ref = f["d"], f["rays"], f["ref"]
    ids0, t0 = ref["hits"][:, 0, 0], ref["t"][:, 0]
    r = ray_words(rays)
    rng = np.random.default_rng(19)
    vecs = [r[k, 4:7] for k in rng.integers(0, r.shape[0], 64)]
    vecs += [np.array(v, np.float32) for v in ([0, 0, 0], [1e-30, 0, 1e-30], [3e38, -3e38, 1e38], [np.inf, 1, -np.inf], [0, -2.5, 0])]
    for v in vecs:
        assert np.array_equal(bits(ref_normalize(v)), bits(oracle_normalize(v))), v
    hit = np.flatnonzero(ids0 >= 0)[::7][:200]
    _, t_mt = ref_hit_attr(d, rays[hit], ids0[hit], t0[hit], want_t=True)
    for j, k in enumerate(hit):
        want = oracle_ray_tri(d, r[k, 0:3], oracle_normalize(r[k, 4:7]), int(ids0[k]))
        assert bits(t_mt[j])[0] == bits(want)[0], (k, t_mt[j], want)


def test_the_record_is_64_bytes_and_misses_are_what_the_abi_says():
    assert rtamd.HIT_ATTR_DTYPE.itemsize == 64 and C.sizeof(rtamd.rt_hit_attr) == 64
    names = [n for n, _ in rtamd.rt_hit_attr._fields_]
    assert names == ["id", "t", "u", "v", "px", "py", "pz", "ndotd", "ngx", "ngy", "ngz", "reserved0", "nsx", "nsy", "nsz",
                     "reserved1"]
    offs = {k: rtamd.HIT_ATTR_DTYPE.fields[k][1] for k in rtamd.HIT_ATTR_DTYPE.names}
    assert offs == {"id": 0, "t": 4, "u": 8, "v": 12, "p": 16, "ndotd": 28, "ng": 32, "reserved0": 44, "ns": 48, "reserved1": 60}
    for k in rtamd.HIT_ATTR_DTYPE.names:                      # the ctypes record and the dtype agree
        first = {"p": "px", "ng": "ngx", "ns": "nsx"}.get(k, k)
        assert getattr(rtamd.rt_hit_attr, first).offset == offs[k]
    rays = rtamd.pack_rays(np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32), tmax=np.array([1, 2, np.inf], np.float32))
    m = miss_words(rays)
    assert np.all(m[:, ID] == 0xFFFFFFFF) and np.array_equal(m[:, T], bits(rays["tmax"])) and not m[:, 2:].any()
    assert miss_words(rtamd.pack_rays(np.zeros((1, 3)), np.ones((1, 3))))[0, T] == TMAX_WORD
    assert words(np.zeros(2, rtamd.HIT_ATTR_DTYPE)).shape == (2, 16)


def test_a_null_context_is_refused_without_a_gpu():
    L = rtamd.lib()
    rays = rtamd.pack_rays(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    hits = np.zeros(4, rtamd.HIT_ATTR_DTYPE)
    pr, ph = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    assert L.rt_trace_rays_attr(None, pr, 4, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_attr_device(None, pr, 4, 0, ph, None) == RT_ERR_INVALID_ARG
    assert not words(hits).any()
    assert "rt_trace_rays_attr" in rtamd.ABI_SYMBOLS and "rt_trace_rays_attr_device" in rtamd.ABI_SYMBOLS
