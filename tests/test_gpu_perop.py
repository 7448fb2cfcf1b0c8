"""The per-op executor (generic.hip launch_op, api.cpp run_generic) in both of
its instantiations: every case of tests/perop_cases.py on forced path 1, float
plans against the reference's float class and the double class
(aFpPack=FPCLASS_DOUBLE) against its own double class (variant 4). The whole
frame and two row bands cut at an odd row give the reference's bytes: the bar
is array_equal. The op kinds each shape is there for are asserted by
tests/test_perop_table.py."""
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import helpers as H
from tests import perop_cases as PC
from tests import refbind as rb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    lib = abi.load()
    assert lib.avirhip_device_count() >= 1, "no gfx950 device"
    abi.check(lib.avirhip_init(0), "init")


_IMAGES = {}


def _image(sw, sh, ch, t):
    """One source per (size, channels, type), shared and never written."""
    key = (sw, sh, ch, np.dtype(t).name)
    if key not in _IMAGES:
        if np.dtype(t).kind == "u":
            a = rb.lcg_u8((sh, sw, ch), seed=sw + ch)
        else:
            a = rb.lcg_f32((sh, sw, ch), seed=7 * sw + ch)
            if t == np.float64:
                # (mantissa bits a float does not hold)
                b = rb.lcg_f32((sh, sw, ch), seed=sh)
                a = a.astype(np.float64) + b.astype(np.float64) * 2.0 ** -25
        a.setflags(write=False)
        _IMAGES[key] = a
    return _IMAGES[key]


@pytest.mark.parametrize("case", PC.CASES, ids=[PC.case_id(c)
                                                for c in PC.CASES])
def test_per_op_executor_gives_the_reference_bytes(case):
    name, ch, fp, tin, tout = case
    _, (sw, sh, nw, nh), mode, bits, _, _ = PC.row(name)
    lib = abi.load()
    src = _image(sw, sh, ch, tin)

    if fp == PC.DBL:
        assert H.need_ref("the double class")
        want = rb.ref_avir(src, nw, nh, out_dtype=tout, resbits=bits,
                           build_mode=mode, variant=4)
        r = avir_amd.CImageResizer(bits, aFpPack=abi.FPCLASS_DOUBLE)
    else:
        want = H.checker_avir(src, nw, nh, out_dtype=tout, resbits=bits,
                              build_mode=mode)
        r = avir_amd.CImageResizer(bits)

    v = avir_amd.CImageResizerVars()
    v.BuildMode = mode
    p = r.plan(sw, sh, nw, nh, ch, 0.0, v, avir_amd._NP2T[np.dtype(tin)],
               avir_amd._NP2T[np.dtype(tout)])
    abi.check(lib.avirhip_plan_set_path(p, abi.PATH_GENERIC), "set_path")

    got = r.resize(src, nw, nh, 0.0, tout, v)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), \
        "whole frame: %d of %d elements differ" % (
            int((got != want).sum()), got.size)

    cut = (nh // 2) | 1
    assert 0 < cut < nh
    out = np.zeros((nh, nw, ch), tout)
    for a, b in ((0, cut), (cut, nh)):
        abi.check(lib.avirhip_resize_band(
            p, src.ctypes.data, abi.MEM_HOST, out[a:b].ctypes.data,
            abi.MEM_HOST, a, b, None), "band")
    assert np.array_equal(out.view(np.uint8), want.view(np.uint8)), \
        "bands cut at row %d: %d of %d elements differ" % (
            cut, int((out != want).sum()), out.size)
