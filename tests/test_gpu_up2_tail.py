"""The 2x marching kernel's tail body (k_up2< true, ... >, up2.hip, U2_TAIL):
the last marching step of a chunk of four steps or more updates only the
vertical sums that belong to the chunk's own rows and weaves no H1 into them,
one code variant per ring phase (last step 0, 1 or 2 modulo 3). Against the
reference bit for bit: raw words, no tolerance.

A chunk of h source rows marches h + 18 rows in steps of 8, so with ONE chunk
(AVIRHIP_UP2_NCHUNKS=1) the heights 7 ... 30 give 25 ... 48 rows: the last
step lies in ring phase 0 (7-14 rows), 1 (15-22) and 2 (23-30), cut by the
frame's end by 7 ... 0 rows each. 6 rows and fewer are three steps, which never
take the tail body. Taller frames are cut into chunks by forced counts whose
last steps lie in all three phases (the split is read back from the library's
AVIRHIP_VERBOSE line and the phases are asserted), and output rows around
seams serve as band boundaries and as the end of a compact device window.

Every case forces path 4 and asserts it."""
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

F16, F32, U8 = np.float16, np.float32, np.uint8
_T = {np.dtype(F16): abi.F16, np.dtype(F32): abi.F32, np.dtype(U8): abi.U8}
RB = 8  # source rows per marching step


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


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _assert_same(got, want, what):
    g, w = _words(got), _words(want)
    assert g.shape == w.shape, what
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d raw words differ; first at %s: "
                             "got %#x want %#x; rows %s" % (
                                 what, len(bad), g.size, i, g[i], w[i],
                                 sorted(set(bad[:, 0].tolist()))[:16]))


# form -> (channels, element type, result bits, variant)
FORMS = {"f32x4": (4, F32, 16, 0),
         "u8x3": (3, U8, 8, 0),
         "f16x4": (4, F16, 16, 0),
         "plain": (4, F32, 16, abi.VARIANT_UP2_PLAIN_V)}


def _image(sw, sh, form, seed):
    ch, dt = FORMS[form][:2]
    if dt == U8:
        return rb.lcg_u8((sh, sw, ch), seed=seed)
    a = rb.lcg_f32((sh, sw, ch), seed=seed)
    return a.astype(F16) if dt == F16 else a


_WANT = {}


def _case(sw, sh, form):
    """(source, expected result) of the exact 2x resize, computed once per
    shape and form and shared by the tests."""
    key = (sw, sh, form if form != "plain" else "f32x4")
    if key not in _WANT:
        ch, dt, bits, _ = FORMS[form]
        src = _image(sw, sh, key[2], 5003 + 11 * sh + sw)
        if dt == F16:
            # (a half call is the float call on the widened source, its
            # result narrowed nearest-even: include/avirhip.h, AVIRHIP_F16)
            want = H.checker_avir(src.astype(F32), 2 * sw, 2 * sh,
                                  out_dtype=F32, resbits=bits, build_mode=1)
            with np.errstate(over="ignore", invalid="ignore"):
                want = want.astype(F16)
        else:
            want = H.checker_avir(src, 2 * sw, 2 * sh, resbits=bits,
                                  build_mode=1)
        src.setflags(write=False)
        want.setflags(write=False)
        _WANT[key] = (src, want)
    return _WANT[key]


def _plan_up2(src, form):
    lib = abi.load()
    sh, sw, ch = src.shape
    _, dt, bits, variant = FORMS[form]
    r = avir_amd.CImageResizer(bits)
    v = avir_amd.CImageResizerVars()
    v.BuildMode = 1
    p = r.plan(sw, sh, 2 * sw, 2 * sh, ch, 0.0, v, _T[np.dtype(dt)],
               _T[np.dtype(dt)])
    abi.check(lib.avirhip_plan_set_path(p, abi.PATH_UP2), "set_path 4")
    abi.check(lib.avirhip_plan_set_variant(p, variant), "set_variant")
    assert lib.avirhip_plan_get_path(p) == abi.PATH_UP2
    return r, v, p


def _check(sw, sh, form, what=""):
    src, want = _case(sw, sh, form)
    r, v, p = _plan_up2(src, form)
    got = r.resize(src, 2 * sw, 2 * sh, aVars=v)
    assert abi.load().avirhip_plan_get_path(p) == abi.PATH_UP2
    _assert_same(got, want, "up2 %dx%d %s %s" % (sw, sh, form, what))
    return src, want, r, v, p


def _split(err, nstrips):
    """[(items, cq, nlong)] of the launches a call made (AVIRHIP_VERBOSE)."""
    m = re.findall(r"k_up2: (\d+) items \(strips (\d+), cq (\d+), nlong (\d+)",
                   err)
    assert m and all(int(x[1]) == nstrips for x in m), err
    return [(int(x[0]), int(x[2]), int(x[3])) for x in m]


def _chunks(sh, n, cq, nlong):
    """[(first source row, marching rows, tail ring phase or None)] of a
    strip's chunks (avir_amd/csrc/up2_chunks.h; the frame's end clips the
    last one; a chunk of three steps has no tail body)."""
    out = []
    for c in range(n):
        first = c * cq + RB * min(c, nlong)
        rows = min(first + (cq + RB if c < nlong else cq), sh) - first
        nsteps = rows + 18
        last = (nsteps - 1) // RB
        out.append((first, nsteps, last % 3 if nsteps > 3 * RB else None))
    return out


# ---- one chunk: every tail ring phase with every clip ----------------------

W1 = 40  # source width: one full strip of 32 and one partial


def test_single_chunk_heights_cover_phases_and_clips():
    """The arithmetic of the module's docstring, from the chunk rule."""
    seen = set()
    for sh in range(7, 31):
        S = (sh + 18 + RB - 1) // RB
        (first, nsteps, ph), = _chunks(sh, 1, RB * max(S, 4) - 18, 0)
        assert (first, nsteps) == (0, sh + 18) and ph is not None
        seen.add((ph, -nsteps % RB))
    assert seen == {(ph, clip) for ph in range(3) for clip in range(RB)}
    assert _chunks(6, 1, 14, 0)[0][2] is None


@pytest.mark.parametrize("form", ["f32x4", "u8x3", "f16x4"])
@pytest.mark.parametrize("sh", range(7, 31))
def test_single_chunk(sh, form, knob, capfd):
    """float RGBA (k_up2< true, 0, 0 >), uint8 RGB as it lies (< true, 4, 13 >),
    half RGBA in and out (< true, 6, 124 >)."""
    knob(UP2_NCHUNKS=1, VERBOSE=1)
    capfd.readouterr()
    _check(W1, sh, form, "one chunk")
    k = max((sh + 18 + RB - 1) // RB, 4)
    assert set(_split(capfd.readouterr().err, 2)) == {(2, RB * k - 18, 0)}


# ---- seams -----------------------------------------------------------------

W2, H2 = 48, 300  # one full strip and half a strip
COUNTS = (4, 5)   # 12 12 12 11 steps (phases 2, 1) and 10 10 10 10 9 (0, 2)


def _forced(n, form, knob, capfd):
    knob(UP2_NCHUNKS=n, VERBOSE=1)
    capfd.readouterr()
    res = _check(W2, H2, form, "n %d" % n)
    (items, cq, nlong), = set(_split(capfd.readouterr().err, 2))
    assert items == 2 * n
    return res, _chunks(H2, n, cq, nlong)


@pytest.mark.parametrize("form", ["f32x4", "u8x3", "f16x4"])
def test_whole_frame_seams_in_every_phase(form, knob, capfd):
    phases = set()
    for n in COUNTS:
        _, ck = _forced(n, form, knob, capfd)
        assert len(ck) == n and all(c[2] is not None for c in ck)
        phases |= {c[2] for c in ck}
    assert phases == {0, 1, 2}


@pytest.mark.parametrize("n", COUNTS)
def test_rows_around_seams_as_band_boundaries(n, knob, capfd):
    """For every output row within 3 of two seams of the whole frame's split,
    the bands [0, row) and [row, end) equal those rows of the frame."""
    import torch
    lib = abi.load()
    (src, want, r, v, p), ck = _forced(n, "f32x4", knob, capfd)
    nw, nh = 2 * W2, 2 * H2
    dsrc = torch.from_numpy(src).to("cuda:0")
    dwant = torch.from_numpy(_words(want).view(np.int32)).to("cuda:0")
    dst = torch.empty((nh, nw, 4), dtype=torch.float32, device="cuda:0")
    bad = []
    for seam in (2 * ck[1][0], 2 * ck[n - 1][0]):
        for row in range(seam - 3, seam + 4):
            dst.fill_(float("nan"))
            for r0, r1 in ((0, row), (row, nh)):
                abi.check(lib.avirhip_resize_band(
                    p, dsrc.data_ptr(), abi.MEM_DEVICE, dst[r0:].data_ptr(),
                    abi.MEM_DEVICE, r0, r1, None), "band")
            torch.cuda.synchronize()
            if not torch.equal(dst.view(torch.int32), dwant):
                bad.append(row)
    assert lib.avirhip_plan_get_path(p) == abi.PATH_UP2
    assert not bad, "bands cut at output rows %s differ" % bad


def test_compact_device_window_that_ends_on_a_seam(knob, capfd):
    """The 29 output rows up to a seam, from a device window that holds only
    the source rows avirhip_band_source_rows names."""
    import torch
    lib = abi.load()
    (src, want, r, v, p), ck = _forced(5, "f32x4", knob, capfd)
    nw = 2 * W2
    r1 = 2 * ck[2][0]
    r0 = r1 - 29
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


# ---- the plain form has no tail body ----------------------------------------

@pytest.mark.parametrize("sw,sh,n", [(W1, 19, 1), (W2, H2, 5)])
def test_plain_form_unchanged(sw, sh, n, knob):
    """k_up2< false > (AVIRHIP_VARIANT_UP2_PLAIN_V)."""
    knob(UP2_NCHUNKS=n)
    _check(sw, sh, "plain", "n %d" % n)
