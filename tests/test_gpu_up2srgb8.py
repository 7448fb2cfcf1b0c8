"""Exact-2x upsizing of 8-bit images with sRGB gamma: k_up2's SRC 313 / 314
and IO 8 / 9 kinds (up2.hip), one launch that linearises the caller's uint8
RGB / RGBA source where it lies and de-linearises and stores the uint8 result
itself.

Expected bits and inputs: tests/up2srgb8_cases.py (the reference with
UseSRGBGamma on the caller's own source; word for word). The calls are made
on device-resident torch tensors through avirhip_resize_band; the road a call
took is read from the launchers' AVIRHIP_VERBOSE lines."""
import re
import threading
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import up2srgb8_cases as U
from tests.gpass_route_cases import environment

pytestmark = pytest.mark.gpu

T = U.T
GUARD = 0x5a
TAG = re.compile(r"^(k_\w+|pack pass|output stage):", re.M)
SPLIT = re.compile(r"k_up2: (\d+) items \(strips (\d+), cq (\d+), nlong (\d+)")
PARENT = U.PARENT
# the issue's shape and the smallest of the case module at which the plan runs
# the transposed form, i.e. the kernel's gamma kinds (U.transposed)
BOTH4 = [U.SMALL[0], U.RGBA_BIG]
BOTH3 = [U.SMALL[0], U.RGB_BIG]


@pytest.fixture(autouse=True)
def _kinds_at_every_size():
    """The kernel's gamma kinds whatever the frame size (U.WIDE)."""
    with environment(dict(U.WIDE)):
        yield


def _both(ch):
    return BOTH4 if ch == 4 else BOTH3


def _gid(g):
    return "%dx%d" % g[:2]


def _lib():
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    return lib


def _plan(geom, tin, tout, ch, alpha, path, variant=0, pitch=0, gamma=True):
    """(resizer, plan) of the call on `path` (0: automatic), ResBitDepth 8."""
    lib = abi.load()
    sw, sh, nw, nh = geom
    r = avir_amd.CImageResizer(8)
    p = r.plan(sw, sh, nw, nh, ch, 0.0, U.gvars(alpha) if gamma else None,
               T[tin][0], T[tout][0], pitch)
    rc = lib.avirhip_plan_set_path(p, path)
    assert rc == 0, (rc, lib.avirhip_last_error())
    abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
    return r, p


def _dev(a, off=0, tail=0):
    """The array's bytes on the device, `off` bytes into an allocation."""
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros(off + b.size + tail, dtype=torch.uint8, device="cuda:0")
    t[off:off + b.size] = torch.from_numpy(b.copy()).to("cuda:0")
    return t


def _call(lib, p, sp, dp, r0, r1, stream=None, what="band"):
    rc = lib.avirhip_resize_band(p, sp, abi.MEM_DEVICE, dp, abi.MEM_DEVICE,
                                 r0, r1, stream)
    assert rc == 0, "%s: rc %d (%s)" % (
        what, rc, (lib.avirhip_last_error() or b"?").decode())


def _host(t, dtype, shape):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype).reshape(shape)


def _guarded(lib, p, sptr, want, what, off=0):
    """The whole frame into guard bytes, 64 + `off` in front of it and a row
    behind it: the reference's bits, the guards untouched."""
    import torch
    front = 64 + off
    rowb = want.shape[1] * want.shape[2] * want.dtype.itemsize
    d = torch.full((front + want.nbytes + rowb,), GUARD, dtype=torch.uint8,
                   device="cuda:0")
    _call(lib, p, sptr, d.data_ptr() + front, 0, want.shape[0], what=what)
    g = _host(d, np.uint8, (-1,))
    got = g[front:front + want.nbytes].copy().view(want.dtype)
    U.same(got, want, what + " frame")
    assert (g[:front] == GUARD).all(), what + ": stored in front of the image"
    assert (g[front + want.nbytes:] == GUARD).all(), \
        what + ": stored behind the image"
    return got


def _frame_and_bands(lib, p, dsrc, want, what):
    """Whole frame (guarded); the bands into one image; the odd band alone."""
    import torch
    nh = want.shape[0]
    rowb = want.shape[1] * want.shape[2] * want.dtype.itemsize
    _guarded(lib, p, dsrc.data_ptr(), want, what)
    bands, odd = U.bands(nh)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    for a, b in bands:
        _call(lib, p, dsrc.data_ptr(), d.data_ptr() + a * rowb, a, b,
              what=what)
    U.same(_host(d, want.dtype, want.shape), want, what + " bands")
    a, b = odd
    d = torch.zeros((b - a) * rowb, dtype=torch.uint8, device="cuda:0")
    _call(lib, p, dsrc.data_ptr(), d.data_ptr(), a, b, what=what)
    U.same(_host(d, want.dtype, want[a:b].shape), want[a:b],
           what + " odd band")


def _tags(capfd):
    return TAG.findall(capfd.readouterr().err)


def _tagged(lib, p, sptr, want, what, capfd, off=0, env=None):
    """(_guarded's result, the call's tags)"""
    e = {"AVIRHIP_VERBOSE": "1"}
    e.update(env or {})
    with environment(e):
        capfd.readouterr()
        got = _guarded(lib, p, sptr, want, what, off=off)
        err = capfd.readouterr().err
    return got, TAG.findall(err), err


# ---- 1. every pair and every shape -------------------------------------------------

@pytest.mark.parametrize("path", [0, 4], ids=["auto", "path4"])
@pytest.mark.parametrize("tin,tout,ch,alpha", U.CASES,
                         ids=["%s-%s-%dch-alpha%d" % c for c in U.CASES])
def test_every_pair(tin, tout, ch, alpha, path):
    lib = _lib()
    for geom in U.shapes(ch):
        src, want = U.case(geom, tin, tout, ch, alpha)
        r, p = _plan(geom, tin, tout, ch, alpha, path)
        what = "%s->%s %d ch alpha %d %r path %d" % (tin, tout, ch, alpha,
                                                      geom, path)
        _frame_and_bands(lib, p, _dev(src), want, what)
        assert lib.avirhip_plan_get_path(p) == abi.PATH_UP2, what


# ---- 2. the road -------------------------------------------------------------------

def _float_plan_bytes(lib, geom):
    """Device bytes of the float32 -> float32 RGBA plan of the geometry (no
    gamma) after a call."""
    import torch
    sw, sh, nw, nh = geom
    r0, p0 = _plan(geom, "f32", "f32", 4, -1, 4, gamma=False)
    s = torch.zeros(sh * sw * 16, dtype=torch.uint8, device="cuda:0")
    d = torch.zeros(nh * nw * 16, dtype=torch.uint8, device="cuda:0")
    _call(lib, p0, s.data_ptr(), d.data_ptr(), 0, nh, what="float")
    torch.cuda.synchronize()
    return int(lib.avirhip_plan_device_bytes(p0))


@pytest.mark.parametrize("path", [0, 4], ids=["auto", "path4"])
@pytest.mark.parametrize("ch", [4, 3])
def test_one_launch_no_float_copies(ch, path, capfd):
    """uint8 -> uint8, RGBA and RGB: k_up2 alone, and the plan holds neither
    float copy (2.2 MB and 8.7 MB at this size). Before these kinds: the pack
    pass, k_up2, the output stage, and both copies."""
    lib = _lib()
    geom = U.shapes(ch)[-1]
    alpha = 3 if ch == 4 else -1
    src, want = U.case(geom, "u8", "u8", ch, alpha)
    r, p = _plan(geom, "u8", "u8", ch, alpha, path)
    dsrc = _dev(src)
    got, tags, err = _tagged(lib, p, dsrc.data_ptr(), want, "u8->u8", capfd)
    print(tags)
    assert tags == ["k_up2"], tags
    over = int(lib.avirhip_plan_device_bytes(p)) - _float_plan_bytes(lib, geom)
    print("%d bytes over the float plan" % over)
    assert over <= 64 * 1024, over


def test_bounds_from_both_sides(capfd):
    """The roads are offered by frame size, in source pixels: uint8 -> uint8
    inside [RAW_MINPIX, RAW_MAXPIX], the store side alone up to STORE_MAXPIX;
    outside, the road from before these kinds. Each bound from both sides, at
    322x420 = 135,240 source pixels; and the defaults (1,700,000 to 2,700,000;
    none), under which a frame of this size keeps the three launches."""
    import os
    lib = _lib()
    geom = U.RGBA_BIG
    px = geom[0] * geom[1]
    src, want = U.case(geom, "u8", "u8", 4, 3)
    fsrc, fwant = U.case(geom, "f32", "u8", 4, 3)
    dsrc, dfsrc = _dev(src), _dev(fsrc)

    def tags(tin, env):
        r, p = _plan(geom, tin, "u8", 4, 3, 4)
        e = dict(U.WIDE)
        e.update(env)
        got, t, err = _tagged(lib, p, (dsrc if tin == "u8" else dfsrc).data_ptr(),
                              want if tin == "u8" else fwant, repr(env), capfd,
                              env=e)
        print(tin, env, t)
        return t

    none = {U.STORE_MAX: "0"}
    assert tags("u8", dict(none, **{U.RAW_MIN: str(px), U.RAW_MAX: str(px)})) \
        == ["k_up2"]
    assert tags("u8", dict(none, **{U.RAW_MIN: str(px + 1)})) == PARENT
    assert tags("u8", dict(none, **{U.RAW_MAX: str(px - 1)})) == PARENT
    assert tags("f32", {U.STORE_MAX: str(px)}) == ["pack pass", "k_up2"]
    assert tags("f32", {U.STORE_MAX: str(px - 1)}) == PARENT
    # a uint8 call beyond the raw window, inside the store bound
    assert tags("u8", {U.RAW_MAX: str(px - 1)}) == ["pack pass", "k_up2"]
    keep = {k: os.environ.pop(k) for k in U.WIDE}
    try:
        r, p = _plan(geom, "u8", "u8", 4, 3, 4)
        got, t, err = _tagged(lib, p, dsrc.data_ptr(), want, "defaults", capfd)
        r2, p2 = _plan(geom, "f32", "u8", 4, 3, 4)
        got, t2, err = _tagged(lib, p2, dfsrc.data_ptr(), fwant, "defaults",
                               capfd)
    finally:
        os.environ.update(keep)
    assert t == PARENT and t2 == PARENT, (t, t2)


@pytest.mark.parametrize("geom,ch", [(U.SHORT, 4), (U.STRIP16, 4),
                                     (U.STRIP16, 3)],
                         ids=["short", "strip16-rgba", "strip16-rgb"])
def test_short_frame_and_16_column_strip(geom, ch, capfd):
    """The kernel's gamma kinds on a frame under the smallest chunk (46 source
    rows: 6 in the last marching step) and on a 16-column last strip: one
    launch, the reference's bits into guard bytes, the bands."""
    lib = _lib()
    alpha = 3 if ch == 4 else -1
    src, want = U.case(geom, "u8", "u8", ch, alpha)
    r, p = _plan(geom, "u8", "u8", ch, alpha, 4)
    dsrc = _dev(src)
    got, tags, err = _tagged(lib, p, dsrc.data_ptr(), want, repr(geom), capfd)
    assert tags == ["k_up2"], tags
    _frame_and_bands(lib, p, dsrc, want, repr(geom))
    fsrc, fwant = U.case(geom, "f32", "u8", ch, alpha)
    r2, p2 = _plan(geom, "f32", "u8", ch, alpha, 4)
    dfsrc = _dev(fsrc)
    got, tags, err = _tagged(lib, p2, dfsrc.data_ptr(), fwant,
                             "f32 %r" % (geom,), capfd)
    assert tags == ["pack pass", "k_up2"], tags


@pytest.mark.parametrize("ch", [4, 3, 1])
def test_store_side_alone_has_no_output_stage(ch, capfd):
    """float32 -> uint8: the kernel's store behind the pack pass's linear
    copy (within the store bound: test_bounds_from_both_sides)."""
    lib = _lib()
    geom = U.shapes(ch)[-1]
    alpha = 3 if ch == 4 else -1
    src, want = U.case(geom, "f32", "u8", ch, alpha)
    r, p = _plan(geom, "f32", "u8", ch, alpha, 4)
    dsrc = _dev(src)
    got, tags, err = _tagged(lib, p, dsrc.data_ptr(), want, "f32->u8", capfd)
    assert tags == ["pack pass", "k_up2"], tags


# ---- 3. the roads agree ------------------------------------------------------------

@pytest.mark.parametrize("tin,tout,ch,alpha", U.PAIRS,
                         ids=["%s-%s-%dch-alpha%d" % c for c in U.PAIRS])
def test_roads_agree(tin, tout, ch, alpha, capfd):
    """AVIRHIP_VARIANT_UP2_UNFUSED_IO: pack pass, float k_up2, output stage
    -- the same bytes."""
    lib = _lib()
    for geom in (U.shapes(ch)[0], U.shapes(ch)[-1]):
        src, want = U.case(geom, tin, tout, ch, alpha)
        dsrc = _dev(src)
        r, p = _plan(geom, tin, tout, ch, alpha, 4)
        got, ftags, err = _tagged(lib, p, dsrc.data_ptr(), want,
                                  "fused %r" % (geom,), capfd)
        r2, p2 = _plan(geom, tin, tout, ch, alpha, 4,
                       abi.VARIANT_UP2_UNFUSED_IO)
        got2, tags, err = _tagged(lib, p2, dsrc.data_ptr(), want,
                                  "unfused %r" % (geom,), capfd)
        print(geom, ftags, tags)
        assert got.tobytes() == got2.tobytes(), geom
        assert ftags == U.road(geom, ch, tin == "u8" and ch >= 3), ftags
        assert tags == PARENT, tags


def test_each_side_has_its_switch(capfd):
    """AVIRHIP_UP2_NO_RAW: the pack pass in front of the kernel's store."""
    lib = _lib()
    geom = U.RGBA_BIG
    src, want = U.case(geom, "u8", "u8", 4, 3)
    r, p = _plan(geom, "u8", "u8", 4, 3, 4)
    dsrc = _dev(src)
    got, tags, err = _tagged(lib, p, dsrc.data_ptr(), want, "no raw", capfd,
                             env={"AVIRHIP_UP2_NO_RAW": "1"})
    assert tags == ["pack pass", "k_up2"], tags


# ---- 4. chunks and seams -----------------------------------------------------------

# (knob, value) -> (chunks, cq, nlong) of 80 and of 420 source rows
SPLITS = {80: [("AVIRHIP_UP2_CQ", 6, 14, 6, 0), ("AVIRHIP_UP2_CQ", 14, 6, 14, 0),
               ("AVIRHIP_UP2_CQ", 62, 2, 62, 0),
               ("AVIRHIP_UP2_NCHUNKS", 1, 1, 86, 0),
               ("AVIRHIP_UP2_NCHUNKS", 3, 3, 22, 2)],
          420: [("AVIRHIP_UP2_CQ", 6, 70, 6, 0),
                ("AVIRHIP_UP2_CQ", 14, 30, 14, 0),
                ("AVIRHIP_UP2_CQ", 62, 7, 62, 0),
                ("AVIRHIP_UP2_NCHUNKS", 1, 1, 422, 0),
                ("AVIRHIP_UP2_NCHUNKS", 3, 3, 142, 0)]}


@pytest.mark.parametrize("big", [0, 1], ids=["97x80", "big"])
@pytest.mark.parametrize("ch", [4, 3])
def test_forced_chunks(ch, big, capfd):
    """Chunks of 6, 14 and 62 source rows, and 1 and 3 chunks of equal work
    (80 rows: 13 and 6 + 6 + 5 marching steps; 420 rows: 55 and 3 x 20);
    the split read back from the launcher's line."""
    lib = _lib()
    geom = _both(ch)[big]
    strips = (geom[2] + 63) // 64
    alpha = 3 if ch == 4 else -1
    src, want = U.case(geom, "u8", "u8", ch, alpha)
    dsrc = _dev(src)
    for knob, val, n, cq, nlong in SPLITS[geom[1]]:
        S = (geom[1] + 18 * n + 7) // 8
        if knob.endswith("NCHUNKS"):
            assert (cq, nlong) == (8 * (S // n) - 18, S % n if n > 1 else 0)
        r, p = _plan(geom, "u8", "u8", ch, alpha, 4)
        got, tags, err = _tagged(lib, p, dsrc.data_ptr(), want,
                                 "%s %d" % (knob, val), capfd,
                                 env={knob: str(val)})
        assert tags == U.road(geom, ch, True), tags
        m = SPLIT.findall(err)
        assert m == [(str(strips * n), str(strips), str(cq), str(nlong))], m


@pytest.mark.parametrize("geom", BOTH4, ids=_gid)
def test_every_row_as_a_band_boundary(geom):
    """Chunks of 6 source rows: for every output row r the bands [0, r) and
    [r, nh) are the reference's rows."""
    import torch
    lib = _lib()
    nw, nh = geom[2:]
    src, want = U.case(geom, "u8", "u8", 4, 3)
    r, p = _plan(geom, "u8", "u8", 4, 3, 4)
    dsrc = _dev(src)
    dwant = torch.from_numpy(want.reshape(-1).copy()).to("cuda:0")
    dst = torch.empty(want.nbytes, dtype=torch.uint8, device="cuda:0")
    bad = []
    with environment({"AVIRHIP_UP2_CQ": "6"}):
        for row in range(1, nh):
            dst.fill_(GUARD)
            for r0, r1 in ((0, row), (row, nh)):
                _call(lib, p, dsrc.data_ptr(), dst.data_ptr() + r0 * nw * 4,
                      r0, r1)
            torch.cuda.synchronize()
            if not torch.equal(dst, dwant):
                bad.append(row)
    assert not bad, "bands cut at output rows %s differ" % bad[:20]


# ---- 5. placement ------------------------------------------------------------------

@pytest.mark.parametrize("big", [0, 1], ids=["97x80", "big"])
@pytest.mark.parametrize("ch", [4, 3])
def test_any_source_base_and_pitch_is_read_raw(ch, big, capfd):
    """uint8 asks nothing of a base or a pitch: source base + 1, + 2, + 3 and
    rows sw * ch + 1 ... 3 bytes apart are still one launch."""
    lib = _lib()
    geom = _both(ch)[big]
    sw, sh, nw, nh = geom
    alpha = 3 if ch == 4 else -1
    src, want = U.case(geom, "u8", "u8", ch, alpha)
    r, p = _plan(geom, "u8", "u8", ch, alpha, 4)
    for off in (1, 2, 3):
        t = _dev(src, off=off, tail=8)
        got, tags, err = _tagged(lib, p, t.data_ptr() + off, want,
                                 "source base + %d" % off, capfd)
        assert tags == U.road(geom, ch, True), (off, tags)
    for extra in (1, 2, 3):
        pitch = sw * ch + extra
        flat = np.full((sh, pitch), 0xff, np.uint8)
        flat[:, :sw * ch] = src.reshape(sh, sw * ch)
        r2, p2 = _plan(geom, "u8", "u8", ch, alpha, 4, pitch=pitch)
        t = _dev(flat)
        got, tags, err = _tagged(lib, p2, t.data_ptr(), want,
                                 "pitch + %d" % extra, capfd)
        assert tags == U.road(geom, ch, True), (extra, tags)


@pytest.mark.parametrize("big", [0, 1], ids=["97x80", "big"])
@pytest.mark.parametrize("ch", [4, 3])
def test_any_destination_base_is_stored_by_the_kernel(ch, big, capfd):
    """Destination base + 1: single-byte stores ask nothing of it."""
    lib = _lib()
    geom = _both(ch)[big]
    alpha = 3 if ch == 4 else -1
    src, want = U.case(geom, "u8", "u8", ch, alpha)
    r, p = _plan(geom, "u8", "u8", ch, alpha, 4)
    dsrc = _dev(src)
    got, tags, err = _tagged(lib, p, dsrc.data_ptr(), want,
                             "destination base + 1", capfd, off=1)
    assert tags == U.road(geom, ch, True), tags


def test_source_window_takes_the_staged_road():
    """A source-window call of the uint8 plan, the window between poisoned
    rows: the reference's bits."""
    import torch
    lib = _lib()
    geom = U.RGBA_BIG
    sw, sh, nw, nh = geom
    src, want = U.case(geom, "u8", "u8", 4, 3)
    r, p = _plan(geom, "u8", "u8", 4, 3, 0)
    w0, w1 = nh // 3, nh - 5
    a, b = r.band_source_rows(sw, sh, nw, nh, 4, w0, w1, 0.0, U.gvars(3),
                              abi.U8, abi.U8)
    G = 16
    big = np.full((b - a + 1 + 2 * G, sw * 4), 0xee, np.uint8)
    big[G:G + b - a + 1] = src.reshape(sh, sw * 4)[a:b + 1]
    dbig = _dev(big)
    d = torch.full(((w1 - w0) * nw * 4,), GUARD, dtype=torch.uint8,
                   device="cuda:0")
    rc = lib.avirhip_resize_window(
        p, dbig.data_ptr() + G * sw * 4, abi.MEM_DEVICE, a, b - a + 1,
        d.data_ptr(), abi.MEM_DEVICE, w0, w1, None)
    assert rc == 0, (rc, lib.avirhip_last_error())
    U.same(_host(d, np.uint8, want[w0:w1].shape), want[w0:w1], "window")


# ---- 6. every threshold ------------------------------------------------------------

@pytest.mark.parametrize("geom", [U.RAMP, U.RAMP_BIG], ids=_gid)
def test_every_threshold(geom, capfd):
    lib = _lib()
    src, want = U.ramp_case(geom)
    r, p = _plan(geom, "u8", "u8", 4, 3, 4)
    dsrc = _dev(src)
    got, tags, err = _tagged(lib, p, dsrc.data_ptr(), want, "ramp", capfd)
    assert tags == U.road(geom, 4, True), tags
    n = np.bincount(got.reshape(-1), minlength=256)
    assert (n > 0).all()


# ---- 7. special values -------------------------------------------------------------

@pytest.mark.parametrize("geom", [U.SPECIAL, U.SPECIAL_BIG], ids=_gid)
def test_special_values_take_the_direct_branch(geom, capfd):
    """float32 pixels whose linear results lie outside |v| <= 16, overflow or
    are not numbers: the store's direct expression (IO 8), the x86 build's
    out-of-range bytes included."""
    lib = _lib()
    src, want = U.special_case("u8", geom)
    r, p = _plan(geom, "f32", "u8", 4, 3, 4)
    dsrc = _dev(src)
    got, tags, err = _tagged(lib, p, dsrc.data_ptr(), want, "special values",
                             capfd)
    assert tags == U.road(geom, 4, False), tags


# ---- 8. threads --------------------------------------------------------------------

def test_four_threads_one_plan():
    """Four threads run whole-frame and band calls of ONE uint8 -> uint8 plan
    at once, each on its own stream into its own images."""
    import torch
    lib = _lib()
    geom = U.RGBA_BIG
    sw, sh, nw, nh = geom
    src, want = U.case(geom, "u8", "u8", 4, 3)
    r, p = _plan(geom, "u8", "u8", 4, 3, 0)
    dsrc = _dev(src)
    rowb = nw * 4
    bands, odd = U.bands(nh)
    out = [[torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
            for _ in range(2)] for _ in range(4)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    errs = []

    def work(i):
        try:
            st = streams[i].cuda_stream
            for _ in range(3):
                _call(lib, p, dsrc.data_ptr(), out[i][0].data_ptr(), 0, nh, st)
                for r0, r1 in bands:
                    _call(lib, p, dsrc.data_ptr(),
                          out[i][1].data_ptr() + r0 * rowb, r0, r1, st)
            streams[i].synchronize()
        except BaseException as e:  # (reported by the main thread)
            errs.append((i, e))

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for i in range(4):
        U.same(_host(out[i][0], np.uint8, want.shape), want,
               "thread %d frame" % i)
        U.same(_host(out[i][1], np.uint8, want.shape), want,
               "thread %d bands" % i)
