"""Whole-ratio (2x, 3x) downsizing of 8-bit images with sRGB gamma: k_dnfh's
DH_S8 kinds (dnf.hip), one launch that linearises the caller's uint8 RGBA
source where it lies and de-linearises and stores the uint8 result itself.

Expected bits and inputs: tests/dnsrgb8_cases.py (the reference with
UseSRGBGamma on the caller's own source; word for word). The calls are made
on device-resident torch tensors through avirhip_resize_band; the road a call
took is read from the launchers' AVIRHIP_VERBOSE lines."""
import re
import threading
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import dnsrgb8_cases as D
from tests.gpass_route_cases import environment

pytestmark = pytest.mark.gpu

T = D.T
GUARD = 0x5a
TAG = re.compile(r"^(k_\w+|pack pass|output stage):", re.M)


def _lib():
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    return lib


def _plan(geom, tin, tout, ch, alpha, path, variant=0, pitch=0, gamma=True):
    """(resizer, plan) of the call on `path` (0: automatic), ResBitDepth 8."""
    lib = abi.load()
    sw, sh, nw, nh = geom
    r = avir_amd.CImageResizer(8)
    p = r.plan(sw, sh, nw, nh, ch, 0.0, D.gvars(alpha) if gamma else None,
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
    D.same(got, want, what + " frame")
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
    bands, odd = D.bands(nh)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    for a, b in bands:
        _call(lib, p, dsrc.data_ptr(), d.data_ptr() + a * rowb, a, b,
              what=what)
    D.same(_host(d, want.dtype, want.shape), want, what + " bands")
    a, b = odd
    d = torch.zeros((b - a) * rowb, dtype=torch.uint8, device="cuda:0")
    _call(lib, p, dsrc.data_ptr(), d.data_ptr(), a, b, what=what)
    D.same(_host(d, want.dtype, want[a:b].shape), want[a:b],
           what + " odd band")


def _tags(capfd):
    return TAG.findall(capfd.readouterr().err)


# ---- 1. every pair and every shape -------------------------------------------------

_CASES = [(tin, tout, ch, al) for tin, tout, ch in D.PAIRS
          for al in D.alphas(ch)]


@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
@pytest.mark.parametrize("tin,tout,ch,alpha", _CASES,
                         ids=["%s-%s-%dch-alpha%d" % c for c in _CASES])
def test_every_pair(tin, tout, ch, alpha, path):
    lib = _lib()
    for geom in D.SHAPES + D.EXTRA_SHAPES:
        src, want = D.case(geom, tin, tout, ch, alpha)
        r, p = _plan(geom, tin, tout, ch, alpha, path)
        what = "%s->%s %d ch alpha %d %r path %d" % (tin, tout, ch, alpha,
                                                      geom, path)
        _frame_and_bands(lib, p, _dev(src), want, what)


# ---- 2. the road -------------------------------------------------------------------

def _float_plan_bytes(lib, geom):
    """Device bytes of the float32 -> float32 RGBA plan of the geometry (no
    gamma) after a call."""
    import torch
    sw, sh, nw, nh = geom
    r0, p0 = _plan(geom, "f32", "f32", 4, -1, 2, gamma=False)
    s = torch.zeros(sh * sw * 16, dtype=torch.uint8, device="cuda:0")
    d = torch.zeros(nh * nw * 16, dtype=torch.uint8, device="cuda:0")
    _call(lib, p0, s.data_ptr(), d.data_ptr(), 0, nh, what="float")
    torch.cuda.synchronize()
    return int(lib.avirhip_plan_device_bytes(p0))


@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
def test_one_launch_no_float_copies(path, capfd):
    """uint8 RGBA -> uint8 RGBA: k_dnfh alone, and the plan holds neither
    float copy (3.8 MB and 0.96 MB at this size)."""
    lib = _lib()
    geom = D.K2
    src, want = D.case(geom, "u8", "u8", 4, 3)
    r, p = _plan(geom, "u8", "u8", 4, 3, path)
    dsrc = _dev(src)
    with environment({"AVIRHIP_VERBOSE": "1"}):
        capfd.readouterr()
        _guarded(lib, p, dsrc.data_ptr(), want, "u8->u8")
        tags = _tags(capfd)
    print(tags)
    assert "k_dnfh" in tags, tags
    assert "pack pass" not in tags and "output stage" not in tags, tags
    over = int(lib.avirhip_plan_device_bytes(p)) - _float_plan_bytes(lib, geom)
    print("%d bytes over the float plan" % over)
    assert over <= 64 * 1024, over


# ---- 3. the roads agree ------------------------------------------------------------

@pytest.mark.parametrize("tin,tout,ch", D.PAIRS,
                         ids=["%s-%s-%dch" % c for c in D.PAIRS])
def test_roads_agree(tin, tout, ch, capfd):
    """AVIRHIP_VARIANT_DN_UNFUSED_IO: pack pass, k_dnf, output stage -- the
    same bytes."""
    lib = _lib()
    alpha = 3 if ch == 4 else -1
    for geom in (D.K2, D.K3):
        src, want = D.case(geom, tin, tout, ch, alpha)
        dsrc = _dev(src)
        r, p = _plan(geom, tin, tout, ch, alpha, 2)
        with environment({"AVIRHIP_VERBOSE": "1"}):
            capfd.readouterr()
            got = _guarded(lib, p, dsrc.data_ptr(), want,
                           "fused %r" % (geom,))
            ftags = _tags(capfd)
        r2, p2 = _plan(geom, tin, tout, ch, alpha, 2,
                       abi.VARIANT_DN_UNFUSED_IO)
        with environment({"AVIRHIP_VERBOSE": "1"}):
            capfd.readouterr()
            got2 = _guarded(lib, p2, dsrc.data_ptr(), want,
                            "unfused %r" % (geom,))
            tags = _tags(capfd)
        print(geom, ftags, tags)
        assert got.tobytes() == got2.tobytes(), geom
        # (RGBA pixels: these shapes are the kernel's plans, tests/
        # test_dnsrgb8_table.py; the planner's cost model sees the channel
        # count, a grey image may get the tiles' plan on both roads)
        assert "k_dnfh" in ftags or ch != 4, ftags
        assert ("k_dnfh" in ftags) == ("k_dnf" in tags), (ftags, tags)
        assert "output stage" not in ftags or tout != "u8" or \
            "k_dnfh" not in ftags, ftags
        assert "pack pass" in tags and "k_dnfh" not in tags, tags
        assert ("output stage" in tags) == (tout == "u8"), tags


# ---- 4. refused images -------------------------------------------------------------

@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
def test_refused_sources_go_through_the_pack_pass(path, capfd):
    """A source base 1, 2 or 3 bytes off and a pitch of 4 * sw + 2 bytes: the
    pack pass's linear copy, and still the kernel's store."""
    lib = _lib()
    for geom in (D.K2, D.K3):
        sw, sh, nw, nh = geom
        src, want = D.case(geom, "u8", "u8", 4, 3)
        r, p = _plan(geom, "u8", "u8", 4, 3, path)
        for off in (1, 2, 3):
            t = _dev(src, off=off, tail=8)
            with environment({"AVIRHIP_VERBOSE": "1"}):
                capfd.readouterr()
                _guarded(lib, p, t.data_ptr() + off, want,
                         "source base + %d" % off)
                tags = _tags(capfd)
            assert "pack pass" in tags and "k_dnfh" in tags, (off, tags)
            assert "output stage" not in tags, (off, tags)
        pitch = 4 * sw + 2
        flat = np.full((sh, pitch), 0xff, np.uint8)
        flat[:, :sw * 4] = src.reshape(sh, sw * 4)
        r2, p2 = _plan(geom, "u8", "u8", 4, 3, path, pitch=pitch)
        t = _dev(flat)
        with environment({"AVIRHIP_VERBOSE": "1"}):
            capfd.readouterr()
            _guarded(lib, p2, t.data_ptr(), want, "pitch 4 * sw + 2")
            tags = _tags(capfd)
        assert "pack pass" in tags and "k_dnfh" in tags, tags
        assert "output stage" not in tags, tags


@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
def test_any_destination_base_is_stored_by_the_kernel(path, capfd):
    """Destination base + 1: single-byte stores ask nothing of it."""
    lib = _lib()
    for geom in (D.K2, D.K3):
        src, want = D.case(geom, "u8", "u8", 4, 3)
        r, p = _plan(geom, "u8", "u8", 4, 3, path)
        dsrc = _dev(src)
        with environment({"AVIRHIP_VERBOSE": "1"}):
            capfd.readouterr()
            _guarded(lib, p, dsrc.data_ptr(), want, "destination base + 1",
                     off=1)
            tags = _tags(capfd)
        assert "k_dnfh" in tags, tags
        assert "pack pass" not in tags and "output stage" not in tags, tags


def test_store_side_alone_keeps_the_output_stage_on_large_frames(capfd):
    """RGB uint8 -> uint8: the kernel's store behind the pack pass up to
    dnsrgb_store_maxpix source pixels (api.cpp; AVIRHIP_DNSRGB_STORE_MAXPIX,
    read per call), k_dnf and the output stage beyond; the same bytes."""
    lib = _lib()
    geom = D.K3
    src, want = D.case(geom, "f32", "u8", 3, -1)
    dsrc = _dev(src)
    seen = []
    for maxpix in (geom[0] * geom[1], geom[0] * geom[1] - 1):
        r, p = _plan(geom, "f32", "u8", 3, -1, 2)
        with environment({"AVIRHIP_VERBOSE": "1",
                          "AVIRHIP_DNSRGB_STORE_MAXPIX": str(maxpix)}):
            capfd.readouterr()
            _guarded(lib, p, dsrc.data_ptr(), want, "maxpix %d" % maxpix)
            seen.append(_tags(capfd))
    print(seen)
    assert seen[0] == ["pack pass", "k_dnfh"], seen
    assert seen[1] == ["pack pass", "k_dnf", "output stage"], seen


# ---- 5. every threshold ------------------------------------------------------------

def test_every_threshold(capfd):
    lib = _lib()
    src, want = D.ramp_case()
    r, p = _plan(D.RAMP, "u8", "u8", 4, 3, 2)
    dsrc = _dev(src)
    with environment({"AVIRHIP_VERBOSE": "1"}):
        capfd.readouterr()
        got = _guarded(lib, p, dsrc.data_ptr(), want, "ramp")
        tags = _tags(capfd)
    assert tags == ["k_dnfh"], tags
    n = np.bincount(got.reshape(-1), minlength=256)
    assert (n > 0).all()


# ---- 6. special values -------------------------------------------------------------

def test_special_values_take_the_direct_branch(capfd):
    """float32 pixels whose linear results lie outside |v| <= 16, overflow or
    are not numbers: the store's direct expression, the x86 build's
    out-of-range bytes included."""
    lib = _lib()
    for geom in (D.SPECIAL, D.SPECIAL_BIG):
        src, want = D.special_case(geom, "u8")
        r, p = _plan(geom, "f32", "u8", 4, 3, 2)
        dsrc = _dev(src)
        with environment({"AVIRHIP_VERBOSE": "1"}):
            capfd.readouterr()
            _guarded(lib, p, dsrc.data_ptr(), want,
                     "special values %r" % (geom,))
            tags = _tags(capfd)
        assert "k_dnfh" in tags and "output stage" not in tags, tags


# ---- 7. threads --------------------------------------------------------------------

def test_four_threads_one_plan():
    """Four threads run whole-frame and band calls of ONE uint8 -> uint8 plan
    at once, each on its own stream into its own images; and source-window
    calls of ONE float32 -> uint8 plan whose window lies between NaN rows."""
    import torch
    lib = _lib()
    geom = D.K3
    sw, sh, nw, nh = geom
    src, want = D.case(geom, "u8", "u8", 4, 3)
    r, p = _plan(geom, "u8", "u8", 4, 3, 0)
    dsrc = _dev(src)
    rowb = nw * 4
    bands, odd = D.bands(nh)
    fsrc, fwant = D.case(geom, "f32", "u8", 4, 3)
    rf, pf = _plan(geom, "f32", "u8", 4, 3, 0)
    w0, w1 = nh // 3, nh - 5
    a, b = rf.band_source_rows(sw, sh, nw, nh, 4, w0, w1, 0.0, D.gvars(3),
                               abi.F32, abi.U8)
    G = 16
    big = np.full((b - a + 1 + 2 * G, sw * 4), np.nan, np.float32)
    big[G:G + b - a + 1] = fsrc.reshape(sh, sw * 4)[a:b + 1]
    dbig = _dev(big)
    wptr = dbig.data_ptr() + G * sw * 16
    out = [[torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
            for _ in range(3)] for _ in range(4)]
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
                rc = lib.avirhip_resize_window(
                    pf, wptr, abi.MEM_DEVICE, a, b - a + 1,
                    out[i][2].data_ptr() + w0 * rowb, abi.MEM_DEVICE, w0, w1,
                    st)
                assert rc == 0, (rc, lib.avirhip_last_error())
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
        D.same(_host(out[i][0], np.uint8, want.shape), want,
               "thread %d frame" % i)
        D.same(_host(out[i][1], np.uint8, want.shape), want,
               "thread %d bands" % i)
        D.same(_host(out[i][2], np.uint8, want.shape)[w0:w1], fwant[w0:w1],
               "thread %d window" % i)
