"""Ray queries, the part that needs no GPU: the two records' sizes, the exported
symbols, the refusals made before any GPU work, and the self-checks of the yardsticks the GPU
tests are measured with (tests/ray_query_common.py)."""
import ctypes as C

import numpy as np
import pytest

import rtamd
from ray_query_common import (TMAX_DEFAULT, brute_force_closest, incoherent_rays, oracle_closest, quantised_frame,
                              scene_arrays)

RT_ERR_INVALID_ARG = -1


def test_record_sizes_and_constants():
    assert C.sizeof(rtamd.rt_ray) == 32 and C.sizeof(rtamd.rt_hit) == 8
    assert rtamd.RAY_DTYPE.itemsize == 32 and rtamd.HIT_DTYPE.itemsize == 8
    assert [rtamd.RAY_DTYPE.fields[k][1] for k in ("o", "tmax", "d", "reserved")] == [0, 12, 16, 28]
    assert [getattr(rtamd.rt_ray, k).offset for k in ("ox", "tmax", "dx", "reserved")] == [0, 12, 16, 28]
    assert rtamd.rt_hit.id.offset == 0 and rtamd.rt_hit.t.offset == 4
    assert rtamd.RT_FLAG_ANY_HIT == 128
    assert np.float32(rtamd.RT_RAY_TMAX_DEFAULT) == TMAX_DEFAULT == np.float32(np.uint32(0xFFFFFFFF))


def test_symbols_exported():
    L = rtamd.lib()
    for name in ("rt_trace_rays", "rt_trace_rays_device", "rt_last_query_timing"):
        assert name in rtamd.ABI_SYMBOLS
        assert hasattr(L, name), name
    assert L.rt_abi_version() == 3


def test_refusals_without_a_context():
    L = rtamd.lib()
    rays = np.zeros(4, rtamd.RAY_DTYPE)
    hits = np.zeros(4, rtamd.HIT_DTYPE)
    pr, ph = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    assert L.rt_trace_rays(None, pr, 4, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays(None, pr, 0, 0, ph) == RT_ERR_INVALID_ARG
    assert L.rt_trace_rays_device(None, pr, 4, 0, ph, None) == RT_ERR_INVALID_ARG
    ms = C.c_float()
    assert L.rt_last_query_timing(None, C.byref(ms)) == RT_ERR_INVALID_ARG
    assert not np.any(hits.view(np.uint32)), "a refused call wrote hits"


def test_pack_rays_keeps_the_tmax_bits():
    o = np.arange(9, dtype=np.float32).reshape(3, 3)
    d = -o
    nan = np.array([0x7FC12345, 0xFFA00001, 0x7F800000], np.uint32).view(np.float32)
    r = rtamd.pack_rays(o, d, nan)
    assert np.array_equal(r["tmax"].view(np.uint32), nan.view(np.uint32))
    assert np.array_equal(r["o"], o) and np.array_equal(r["d"], d) and not np.any(r["reserved"])
    assert np.all(rtamd.pack_rays(o, d)["tmax"] == TMAX_DEFAULT)
    assert np.all(rtamd.pack_rays(o, d, 2.5)["tmax"] == np.float32(2.5))
    with pytest.raises(ValueError):
        rtamd.pack_rays(o, d[:2])


def test_yardstick_1_equals_a_brute_force_minimum():
    """One ray through the oracle's 1 x 1 frame is the closest hit of exactly that ray: id and every
    bit of t equal a minimum over ALL triangles of the oracle's own ray-triangle test."""
    d = scene_arrays("rand2k")
    o, dirs, campos = incoherent_rays(d, n=50)
    ids, t = oracle_closest(d, o, campos)
    assert 10 < int((ids >= 0).sum()) < 50, "the rays should both hit and miss"
    assert np.all(t[ids < 0] == TMAX_DEFAULT)
    for k in range(50):
        bid, bt = brute_force_closest(d, o[k], dirs[k])
        assert np.float32(bt).view(np.uint32) == t[k].view(np.uint32), (k, bt, t[k])
        assert (bid >= 0) == (ids[k] >= 0), (k, bid, ids[k])
        if bid != ids[k]:   # two triangles at the same distance: the traversal may meet the other first
            from ray_query_common import oracle_normalize, oracle_ray_tri
            assert oracle_ray_tri(d, o[k], oracle_normalize(dirs[k]), int(ids[k])) == bt, (k, bid, ids[k])


def test_yardstick_2_rays_are_exact_and_are_the_frame_s():
    """The quantised frame's rays are exact in float32 (asserted inside the helper), and tracing them
    one by one through yardstick 1 gives the oracle's own frame at those pixels."""
    from oracle import oracle
    d = scene_arrays("rand2k")
    w, h = 64, 32
    p, o, dirs = quantised_frame(d, w, h)
    assert o.shape == (w * h, 3) and np.all(np.any(dirs != 0.0, axis=1))
    frame = oracle.render(d, p, w, h, depth=1, flags=1)
    traced = frame["hits"][:, 0, 0] != -2
    assert int((frame["hits"][:, 0, 0] >= 0).sum()) > 50, "the quantised camera sees too little"
    pix = np.arange(0, w * h, 13)
    campos = np.broadcast_to(p[12:15], (pix.size, 3))
    # yardstick 1 rebuilds the direction as fl(o - campos): the frame's own subtraction
    ids, t = oracle_closest(d, o[pix], campos)
    for j, k in enumerate(pix):
        if traced[k]:
            assert ids[j] == frame["hits"][k, 0, 0], (k, ids[j], frame["hits"][k, 0, 0])
            assert t[j].view(np.uint32) == frame["t"][k, 0].view(np.uint32), k
        else:   # outside the golden's scene box the frame traces nothing; such a ray can hit nothing
            assert ids[j] == -1, k
