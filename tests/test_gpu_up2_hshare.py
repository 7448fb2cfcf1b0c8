"""The 2x marching kernel's horizontal interpolation with shared tap products
(k_up2< true, ... >, up2.hip: a thread streams over a row's C half pixels and
owns one half pixel of four source pixels U2_HS apart inside a group of
4 * U2_HS pixels of a 32-pixel strip), against the reference bit for bit.

Shapes are chosen for that ownership: source widths that cut a group of 8 and
of 16 pixels and the strip of 32 at every kind of place, and one wide frame
whose last strip is partial. Every case forces path 4 and asserts it
(avirhip_plan_get_path), so none silently tests another kernel. Build mode 1
keeps the plan in the kernel's shape (FIR7, zero-stuffed 2x, 12-tap bank) for
tiny images too."""
import ctypes as C
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 7, 8, 9, 15, 17, 31, 33, 63, 65]
WIDE = (141, 45)  # 4 strips of 32 + 13 pixels: a group of 8 and of 16 cut too
SHAPES = [(w, 19 + w % 7) for w in WIDTHS] + [WIDE]


@pytest.fixture(scope="module", autouse=True)
def _device():
    lib = abi.load()
    assert lib.avirhip_device_count() >= 1, "no gfx950 device"
    abi.check(lib.avirhip_init(0), "init")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, what
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: "
                             "got %r want %r" % (what, len(bad), g.size, i,
                                                 got[i], want[i]))


def _image(sw, sh, ch, dt, seed):
    if np.dtype(dt) == np.uint8:
        return rb.lcg_u8((sh, sw, ch), seed=seed)
    return rb.lcg_f32((sh, sw, ch), seed=seed)


def _plan_up2(src, bits, variant=0):
    """(resizer, vars, plan) of the exact 2x plan of `src`, forced onto path 4
    and checked to be there."""
    lib = abi.load()
    sh, sw, ch = src.shape
    r = avir_amd.CImageResizer(bits)
    v = avir_amd.CImageResizerVars()
    v.BuildMode = 1
    p = r.plan(sw, sh, 2 * sw, 2 * sh, ch, 0.0, v, rb._DT[src.dtype],
               rb._DT[src.dtype])
    abi.check(lib.avirhip_plan_set_path(p, abi.PATH_UP2), "set_path 4")
    abi.check(lib.avirhip_plan_set_variant(p, variant), "set_variant")
    assert lib.avirhip_plan_get_path(p) == abi.PATH_UP2
    return r, v, p


def _check(sw, sh, ch, dt, bits, variant=0):
    src = _image(sw, sh, ch, dt, 811 + 13 * sw + ch)
    want = H.checker_avir(src, 2 * sw, 2 * sh, resbits=bits, build_mode=1)
    r, v, p = _plan_up2(src, bits, variant)
    got = r.resize(src, 2 * sw, 2 * sh, aVars=v)
    assert abi.load().avirhip_plan_get_path(p) == abi.PATH_UP2
    _assert_same(got, want, "up2 %dx%d ch %d %s variant %d" % (
        sw, sh, ch, np.dtype(dt).name, variant))
    return src, want, r, v, p


@pytest.mark.parametrize("sw,sh", SHAPES)
def test_float_rgba(sw, sh):
    """k_up2< true, 0, 0 >: float RGBA in, float RGBA out."""
    _check(sw, sh, 4, np.float32, 16)


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("sw,sh", SHAPES)
def test_uint8_as_it_lies(sw, sh, ch):
    """k_up2< true, 4, 13 / 14 >: the caller's uint8 RGB / RGBA image read by
    the tile loader and stored by the vertical phase."""
    _check(sw, sh, ch, np.uint8, 8)


@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("sw,sh", SHAPES)
def test_float_few_channels(sw, sh, ch):
    """k_up2< true, 3 >: float pixels of 1-3 channels stored by the vertical
    phase."""
    _check(sw, sh, ch, np.float32, 16)


@pytest.mark.parametrize("sw,sh", [(9, 21), WIDE])
def test_plain_form(sw, sh):
    """k_up2< false > (AVIRHIP_VARIANT_UP2_PLAIN_V) keeps the 13-pixel window."""
    _check(sw, sh, 4, np.float32, 16, abi.VARIANT_UP2_PLAIN_V)


@pytest.mark.parametrize("sw,sh", [(33, 24), WIDE])
def test_band_and_compact_source_window(sw, sh):
    """Row bands of the float RGBA result, from the whole frame and from the
    compact device window that holds only the band's source rows."""
    import torch
    lib = abi.load()
    src, want, r, v, p = _check(sw, sh, 4, np.float32, 16)
    nw, nh = 2 * sw, 2 * sh
    for r0, r1 in [(0, nh // 3), (nh // 3, nh // 3 + 5), (nh // 3 + 5, nh)]:
        band = np.empty((r1 - r0, nw, 4), np.float32)
        abi.check(lib.avirhip_resize_band(
            p, src.ctypes.data, abi.MEM_HOST, band.ctypes.data, abi.MEM_HOST,
            r0, r1, None), "band")
        _assert_same(band, want[r0:r1], "band [%d,%d)" % (r0, r1))
        a, b = C.c_int(), C.c_int()
        abi.check(lib.avirhip_band_source_rows(p, r0, r1, C.byref(a),
                                               C.byref(b)), "band_source_rows")
        rows = torch.from_numpy(np.ascontiguousarray(
            src[a.value:b.value + 1])).to("cuda:0")
        d = torch.full(((r1 - r0) * nw * 4,), float("nan"),
                       dtype=torch.float32, device="cuda:0")
        abi.check(lib.avirhip_resize_window(
            p, rows.data_ptr(), abi.MEM_DEVICE, a.value,
            b.value - a.value + 1, d.data_ptr(), abi.MEM_DEVICE, r0, r1, None),
            "window")
        torch.cuda.synchronize()
        assert lib.avirhip_plan_get_path(p) == abi.PATH_UP2
        _assert_same(d.cpu().numpy().reshape(r1 - r0, nw, 4), want[r0:r1],
                     "window rows [%d,%d] band [%d,%d)" % (a.value, b.value,
                                                           r0, r1))
