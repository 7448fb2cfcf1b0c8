"""The 2x marching kernel's chunk split (avir_amd/csrc/up2_chunks.h: the first
nlong chunks of a strip are one marching step taller than the rest), against
the reference bit for bit.

A row's sums never depend on where a chunk starts, so every split must give the
same bits: whole frames under the default choice and under a forced chunk count
(AVIRHIP_UP2_NCHUNKS: nlong = 0, 1 and n - 1, one chunk only), every output row
as a band boundary (each band height chooses a split of its own, so this walks
every seam of whatever rule is in force without knowing it), compact device
windows around seams, and the uniform height AVIRHIP_UP2_CQ still forces.

The balanced split never clips a whole frame's last chunk by more than 7 rows
(the rows its chunks hold exceed the frame's by less than one marching step),
so the last chunk of ONE row is made with the uniform height: 5 x 62 + 1 rows.

Every case forces path 4 and asserts it. The forced splits are read back from
the library's AVIRHIP_VERBOSE line, so a knob that did nothing fails."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H

pytestmark = pytest.mark.gpu

W = 40  # source width: two strips, the second one partial


@pytest.fixture(scope="module", autouse=True)
def _device():
    lib = abi.load()
    assert lib.avirhip_device_count() >= 1, "no gfx950 device"
    abi.check(lib.avirhip_init(0), "init")


@pytest.fixture()
def knob():
    """sets AVIRHIP_UP2_* for one test (up2_run reads them per call)"""
    names = ("AVIRHIP_UP2_CQ", "AVIRHIP_UP2_NCHUNKS", "AVIRHIP_VERBOSE")
    saved = {n: os.environ.pop(n, None) for n in names}

    def put(**kw):
        for n in names:
            os.environ.pop(n, None)
        for k, v in kw.items():
            os.environ["AVIRHIP_" + k] = str(v)
    yield put
    for n, v in saved.items():
        os.environ.pop(n, None)
        if v is not None:
            os.environ[n] = v


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, what
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d raw words differ; first at %s: "
                             "got %#x want %#x" % (what, len(bad), g.size, i,
                                                   g[i], w[i]))


def _image(sw, sh, ch, dt, seed):
    if np.dtype(dt) == np.uint8:
        return rb.lcg_u8((sh, sw, ch), seed=seed)
    return rb.lcg_f32((sh, sw, ch), seed=seed)


def _plan_up2(src, bits, variant=0):
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


FORMATS = {"f32x4": (4, np.float32, 16, 0),
           "u8x3": (3, np.uint8, 8, 0),
           "plain": (4, np.float32, 16, abi.VARIANT_UP2_PLAIN_V)}


def _check(sh, fmt, what=""):
    ch, dt, bits, variant = FORMATS[fmt]
    src = _image(W, sh, ch, dt, 4111 + 7 * sh + ch)
    want = H.checker_avir(src, 2 * W, 2 * sh, resbits=bits, build_mode=1)
    r, v, p = _plan_up2(src, bits, variant)
    got = r.resize(src, 2 * W, 2 * sh, aVars=v)
    assert abi.load().avirhip_plan_get_path(p) == abi.PATH_UP2
    _assert_same(got, want, "up2 %dx%d %s %s" % (W, sh, fmt, what))
    return src, want, r, v, p


# one chunk only (shorter and taller than the shortest chunk), a few chunks,
# and the headline's height and its neighbours
HEIGHTS = [5, 50, 100, 300, 314, 700, 2159, 2160, 2161]


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("sh", HEIGHTS)
def test_whole_frame_default_split(sh, fmt, knob):
    knob()
    _check(sh, fmt)


# (rows, forced chunk count) -> (cq, nlong): S = ceil((rows + 18 n) / 8)
# marching steps dealt over n chunks, cq = 8 * (S // n) - 18, nlong = S % n
FORCED = [(300, 3, 102, 0),   # 45 steps: 15 15 15
          (314, 4, 78, 1),    # 49 steps: 13 12 12 12
          (300, 4, 70, 3),    # 47 steps: 12 12 12 11
          (2160, 17, 126, 3),  # the headline's strip: 3 x 19 + 14 x 18 steps
          (100, 1, 102, 0)]   # one chunk


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("sh,n,cq,nlong", FORCED)
def test_whole_frame_forced_chunk_count(sh, n, cq, nlong, fmt, knob, capfd):
    S = (sh + 18 * n + 7) // 8
    assert (cq, nlong) == (8 * (S // n) - 18, S % n if n > 1 else 0)
    knob(UP2_NCHUNKS=n, VERBOSE=1)
    capfd.readouterr()
    _check(sh, fmt, "n %d" % n)
    err = capfd.readouterr().err
    m = re.findall(r"k_up2: (\d+) items \(strips (\d+), cq (\d+), nlong (\d+)",
                   err)
    assert m, err
    assert all(x == (str(2 * n), "2", str(cq), str(nlong)) for x in m), m


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("sh,cq", [(311, 62), (300, 62), (314, 78),
                                   (2160, 134), (50, 62)])
def test_whole_frame_forced_uniform_height(sh, cq, fmt, knob, capfd):
    """AVIRHIP_UP2_CQ: one height, nlong = 0, the last chunk gets what is left
    (311 = 5 x 62 + 1: a last chunk of one row)."""
    knob(UP2_CQ=cq, VERBOSE=1)
    capfd.readouterr()
    _check(sh, fmt, "cq %d" % cq)
    m = re.findall(r"k_up2: (\d+) items \(strips (\d+), cq (\d+), nlong (\d+)",
                   capfd.readouterr().err)
    assert m and all(x == (str(2 * ((sh + cq - 1) // cq)), "2", str(cq), "0")
                     for x in m), m


def test_every_row_as_a_band_boundary(knob):
    """80 x 1400 float RGBA: for every output row r the bands [0, r) and
    [r, 1400) equal those rows of the whole-frame result (itself checked
    against the reference)."""
    import torch
    knob()
    lib = abi.load()
    sh = 700
    src, want, r, v, p = _check(sh, "f32x4")
    nw, nh = 2 * W, 2 * sh
    dsrc = torch.from_numpy(src).to("cuda:0")
    dwant = torch.from_numpy(_bits(want).view(np.int32)).to("cuda:0")
    dst = torch.empty((nh, nw, 4), dtype=torch.float32, device="cuda:0")
    bad = []
    for row in range(1, nh):
        dst.fill_(float("nan"))
        for r0, r1 in ((0, row), (row, nh)):
            abi.check(lib.avirhip_resize_band(
                p, dsrc.data_ptr(), abi.MEM_DEVICE,
                dst[r0:].data_ptr(), abi.MEM_DEVICE, r0, r1, None), "band")
        torch.cuda.synchronize()
        if not torch.equal(dst.view(torch.int32), dwant):
            bad.append(row)
    assert lib.avirhip_plan_get_path(p) == abi.PATH_UP2
    assert not bad, "bands cut at output rows %s differ" % bad[:20]


@pytest.mark.parametrize("r0,r1", [(119, 131), (615, 627), (1359, 1371),
                                   (100, 900)])
def test_compact_device_windows_around_seams(r0, r1, knob):
    """A band's split comes from its own height but lies on the frame's grid:
    a band of a few rows is one chunk of the shortest height, 62 source rows,
    so its grid has seams at the output rows 124 j. Windows around j = 1, 5
    and 11 hold only the source rows avirhip_band_source_rows names; the tall
    one crosses several chunks of a split with long ones."""
    import torch
    knob()
    lib = abi.load()
    sh = 700
    src, want, r, v, p = _check(sh, "f32x4")
    nw = 2 * W
    a, b = C.c_int(), C.c_int()
    abi.check(lib.avirhip_band_source_rows(p, r0, r1, C.byref(a), C.byref(b)),
              "band_source_rows")
    rows = torch.from_numpy(np.ascontiguousarray(
        src[a.value:b.value + 1])).to("cuda:0")
    d = torch.full(((r1 - r0) * nw * 4,), float("nan"), dtype=torch.float32,
                   device="cuda:0")
    abi.check(lib.avirhip_resize_window(
        p, rows.data_ptr(), abi.MEM_DEVICE, a.value, b.value - a.value + 1,
        d.data_ptr(), abi.MEM_DEVICE, r0, r1, None), "window")
    torch.cuda.synchronize()
    assert lib.avirhip_plan_get_path(p) == abi.PATH_UP2
    _assert_same(d.cpu().numpy().reshape(r1 - r0, nw, 4), want[r0:r1],
                 "window rows [%d,%d] band [%d,%d)" % (a.value, b.value, r0,
                                                       r1))
