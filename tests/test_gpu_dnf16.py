"""Whole-ratio (2x, 3x) downsizing with half / bfloat16 RGBA images: k_dnfh
(dnf.hip), one launch over the caller's own images on path 2.

Expected bits and inputs: tests/dnf16_cases.py (the reference on the exactly
widened float32 source, its float32 result narrowed by numpy / by the
contract's integer formula; word for word, NaN equal to NaN). The calls are
made on device-resident torch tensors through avirhip_resize_band."""
import threading
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import dnf16_cases as D

pytestmark = pytest.mark.gpu

T = D.T


def _lib():
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    return lib


def _plan(geom, tin, tout, path, variant=0, pitch=0, ch=4):
    """(resizer, plan) of the call on `path` (0: automatic); plan None when the
    forced path cannot run the geometry (AVIRHIP_EUNSUPPORTED)."""
    lib = abi.load()
    sw, sh, nw, nh = geom
    r = avir_amd.CImageResizer(8 if tout == "u8" else 16)
    p = r.plan(sw, sh, nw, nh, ch, 0.0, None, T[tin][0], T[tout][0], pitch)
    rc = lib.avirhip_plan_set_path(p, path)
    if rc != 0:
        assert rc == abi.EUNSUPPORTED, rc
        return r, None
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


def _host(t, tout, shape):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(T[tout][1]).reshape(shape)


def _frame(lib, p, dsrc_ptr, want, tout, what):
    import torch
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    _call(lib, p, dsrc_ptr, d.data_ptr(), 0, want.shape[0], what=what)
    got = _host(d, tout, want.shape)
    D.same(got, want, tout, what)
    return got


def _frame_and_bands(lib, p, dsrc, want, tout, what):
    """Whole frame; the bands into one image; the odd band on its own."""
    import torch
    nh, nw = want.shape[:2]
    rb_ = nw * 4 * want.dtype.itemsize
    _frame(lib, p, dsrc.data_ptr(), want, tout, what + " frame")
    bands, odd = D.bands(nh)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    for a, b in bands:
        _call(lib, p, dsrc.data_ptr(), d.data_ptr() + a * rb_, a, b, what=what)
    D.same(_host(d, tout, want.shape), want, tout, what + " bands")
    if odd is not None:
        a, b = odd
        d = torch.zeros((b - a) * rb_, dtype=torch.uint8, device="cuda:0")
        _call(lib, p, dsrc.data_ptr(), d.data_ptr(), a, b, what=what)
        D.same(_host(d, tout, want[a:b].shape), want[a:b], tout,
               what + " odd band")


def _held_over_float(lib, geom, p, path):
    """Device bytes the plan holds, less those of the float32 -> float32 plan
    of the same geometry and path after the same call."""
    import torch
    sw, sh, nw, nh = geom
    src, want = D.case(geom, "f32", "f32")
    r0, p0 = _plan(geom, "f32", "f32", path)
    assert p0 is not None
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    dsrc = _dev(src)
    _call(lib, p0, dsrc.data_ptr(), d.data_ptr(), 0, nh, what="float")
    torch.cuda.synchronize()
    return (int(lib.avirhip_plan_device_bytes(p)) -
            int(lib.avirhip_plan_device_bytes(p0)))


_ids = ["%s-%s" % pr for pr in D.PAIRS]


# ---- 1. every pair ------------------------------------------------------------

@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_ids)
def test_every_pair(tin, tout, path):
    lib = _lib()
    ran = 0
    for geom in D.SHAPES + D.EXTRA_SHAPES:
        r, p = _plan(geom, tin, tout, path)
        if p is None:
            continue  # (a forced path that refuses a tiny shape)
        ran += (geom in D.SHAPES)
        src, want = D.case(geom, tin, tout)
        what = "%s->%s %r path %d" % (tin, tout, geom, path)
        _frame_and_bands(lib, p, _dev(src), want, tout, what)
        if path == 2 and geom in D.DNF_SHAPES and tout not in ("u8", "u16"):
            # (k_dnfh ran: neither float copy on the plan; DNF_SHAPES is
            # about float-type results, the planner gives small frames with
            # integer results other plans)
            over = _held_over_float(lib, geom, p, path)
            assert over < geom[2] * geom[3] * 16, (what, over)
    assert ran >= 5, "path %d took %d of the shapes" % (path, ran)


# ---- 2. held memory -------------------------------------------------------------

@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
@pytest.mark.parametrize("tin,tout", D.PAIRS, ids=_ids)
def test_no_float_copies_on_the_plan(tin, tout, path):
    """The plan of a call k_dnfh ran holds neither the float copy of the
    source (sw * sh * 16 bytes) nor the float result (nw * nh * 16, the smaller
    of the two); with AVIRHIP_VARIANT_DN_UNFUSED_IO it holds at least the
    latter."""
    lib = _lib()
    for geom in (D.K2, D.K3):
        sw, sh, nw, nh = geom
        src, want = D.case(geom, tin, tout)
        dsrc = _dev(src)
        what = "%s->%s %r path %d" % (tin, tout, geom, path)
        r, p = _plan(geom, tin, tout, path)
        _frame(lib, p, dsrc.data_ptr(), want, tout, what)
        over = _held_over_float(lib, geom, p, path)
        print("%s: %d bytes over the float plan (bound %d)" % (
            what, over, nw * nh * 16))
        assert over < nw * nh * 16, what
        r2, p2 = _plan(geom, tin, tout, path, abi.VARIANT_DN_UNFUSED_IO)
        _frame(lib, p2, dsrc.data_ptr(), want, tout, what + " unfused")
        over2 = _held_over_float(lib, geom, p2, path)
        print("%s unfused: %d bytes over the float plan" % (what, over2))
        assert over2 >= nw * nh * 16, what


def test_variant_128_is_accepted():
    lib = _lib()
    r, p = _plan(D.K2, "f16", "f16", 2)
    assert lib.avirhip_plan_set_variant(p, abi.VARIANT_DN_UNFUSED_IO) == 0
    assert lib.avirhip_plan_set_variant(p, 255) == 0
    assert lib.avirhip_plan_set_variant(p, 256) != 0
    assert lib.avirhip_plan_set_variant(p, 0) == 0


# ---- 3. the roads agree -----------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_roads_agree(t):
    """k_dnfh; pack pass, k_dnf and output stage (AVIRHIP_VARIANT_DN_UNFUSED_IO);
    the two pass kernels (AVIRHIP_VARIANT_DN_TWO_PASS); the generic kernels
    (forced path 1): the same bytes."""
    lib = _lib()
    for geom in (D.K2, D.K3):
        src, want = D.case(geom, t, t)
        dsrc = _dev(src)
        got = []
        for path, variant in [(2, 0), (2, abi.VARIANT_DN_UNFUSED_IO),
                              (2, abi.VARIANT_DN_TWO_PASS), (1, 0)]:
            r, p = _plan(geom, t, t, path, variant)
            assert p is not None, (geom, path)
            got.append(_frame(lib, p, dsrc.data_ptr(), want, t, "%r path %d "
                              "variant %d" % (geom, path, variant)))
        for g in got[1:]:
            assert g.tobytes() == got[0].tobytes(), geom


# ---- 4. refusals ------------------------------------------------------------------

@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_refused_sources_take_the_general_road(t, path):
    """A source base 2 bytes off and a row pitch that is no multiple of 4
    elements (padding NaN) go through the pack pass's float copy: the same
    bits, rc == 0. A pitch of whole pixels is admitted: no float copies."""
    lib = _lib()
    pad = (np.array([D.NAN], np.uint16)[0] if t == "bf16"
           else np.float16(np.nan))
    for geom in (D.K2, D.K3):
        sw, sh, nw, nh = geom
        src, want = D.case(geom, t, t)
        r, p = _plan(geom, t, t, path)
        off = _dev(src, off=2, tail=6)
        _frame(lib, p, off.data_ptr() + 2, want, t, "source base 2 bytes off")
        # (refused, not read in place: the plan holds the float source copy)
        over = _held_over_float(lib, geom, p, path)
        assert sw * sh * 16 <= over < sw * sh * 16 + nw * nh * 16, (geom, over)
        for extra in (1, 8):
            pitch = sw * 4 + extra
            flat = np.full((sh, pitch), pad, T[t][1])
            flat[:, :sw * 4] = src.reshape(sh, sw * 4)
            r2, p2 = _plan(geom, t, t, path, pitch=pitch)
            dflat = _dev(flat)
            _frame(lib, p2, dflat.data_ptr(), want, t, "pitch + %d" % extra)
            over = _held_over_float(lib, geom, p2, path)
            if extra == 8:
                assert over < nw * nh * 16, (geom, over)
            else:
                assert over >= sw * sh * 16, (geom, over)


@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
@pytest.mark.parametrize("tout", ["f16", "bf16"])
def test_uint8_source_behind_the_pack_pass(tout, path):
    """uint8 RGBA -> half / bfloat16: the kernel narrows and stores behind the
    pack pass; the plan holds the float copy of the source, no float result."""
    lib = _lib()
    for geom in (D.K2, D.K3):
        sw, sh, nw, nh = geom
        src, want = D.case(geom, "u8", tout)
        r, p = _plan(geom, "u8", tout, path)
        _frame_and_bands(lib, p, _dev(src), want, tout,
                         "u8->%s %r path %d" % (tout, geom, path))
        over = _held_over_float(lib, geom, p, path)
        print("u8->%s %r: %d bytes over the float plan" % (tout, geom, over))
        assert sw * sh * 16 <= over < sw * sh * 16 + nw * nh * 16


@pytest.mark.parametrize("path", [0, 2], ids=["auto", "path2"])
@pytest.mark.parametrize("tin,tout", [("f32", "f16"), ("f32", "bf16"),
                                      ("f16", "bf16"), ("u8", "f16")],
                         ids=["f32-f16", "f32-bf16", "f16-bf16", "u8-f16"])
def test_rgb_result_stored_by_the_kernel(tin, tout, path):
    """RGB pixels (3 elements) -> half / bfloat16 RGB: the source goes through
    the pack pass's float RGBA copy, a column wave's lane stores its channel at
    ( x * 3 + c ) * 2 and the padding lanes store nothing; the plan holds the
    source copy but no float result. Whole frame (zeroed destination with a
    guard row behind it) and bands."""
    import torch
    lib = _lib()
    for geom in (D.K2, D.K3):
        sw, sh, nw, nh = geom
        src, want = D.case(geom, tin, tout, ch=3)
        assert want.shape == (nh, nw, 3)
        dsrc = _dev(src)
        what = "RGB %s->%s %r path %d" % (tin, tout, geom, path)
        r, p = _plan(geom, tin, tout, path, ch=3)
        assert p is not None
        rb_ = nw * 3 * 2
        d = torch.full((want.nbytes + rb_,), 0x5a, dtype=torch.uint8,
                       device="cuda:0")
        _call(lib, p, dsrc.data_ptr(), d.data_ptr(), 0, nh, what=what)
        g = _host(d, "u8", (want.nbytes + rb_,))
        D.same(g[:want.nbytes].view(T[tout][1]), want, tout, what + " frame")
        assert (g[want.nbytes:] == 0x5a).all(), "stored behind the last row"
        bands, odd = D.bands(nh)
        d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
        for a, b in bands:
            _call(lib, p, dsrc.data_ptr(), d.data_ptr() + a * rb_, a, b,
                  what=what)
        D.same(_host(d, tout, want.shape), want, tout, what + " bands")
        over = _held_over_float(lib, geom, p, path)
        print("%s: %d bytes over the float RGBA plan" % (what, over))
        assert sw * sh * 16 <= over < sw * sh * 16 + nw * nh * 16, what


# ---- 5. special values ----------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_special_values(t):
    """Half: +-0, denormals, +-65504, +-Inf, NaN and a 64000 block whose
    overshoot crosses 65504, read and stored by k_dnfh< F16, F16 >. bfloat16:
    k_dnfh< F32, BF16 >'s store keeps float32 denormals, NaN and +-Inf."""
    lib = _lib()
    tin = "f16" if t == "f16" else "f32"
    for size, out in ([(D.SPECIAL_SRC, o) for o in D.SPECIAL_OUT] +
                      [(D.SPECIAL_BIG_SRC, o) for o in D.SPECIAL_BIG_OUT]):
        sw, sh = size
        src, ref, want = D.special_case(t, out, size)
        c = D.special_classes(t, ref, want)
        print(out, c)
        assert c["pos_inf"] > 0 and c["neg_inf"] > 0 and c["denormal"] > 0
        assert 0 < c["nan"] < c["size"] // 10
        if t == "f16":
            assert c["fin_to_inf"] > 0
        geom = (sw, sh, out[0], out[1])
        r, p = _plan(geom, tin, t, 2)
        assert p is not None
        dsrc = _dev(src)
        got = _frame(lib, p, dsrc.data_ptr(), want, t,
                     "special values %s %r" % (t, out))
        gf, wf = D.as_f32(got, t), D.as_f32(want, t)
        assert np.array_equal(np.isinf(gf), np.isinf(wf))
        assert np.array_equal(np.isnan(gf), np.isnan(wf))
        if size == D.SPECIAL_BIG_SRC or out == (64, 48):
            # (k_dnfh's plans, tests/dnf16_cases.py: the kernel ran)
            assert _held_over_float(lib, geom, p, 2) < out[0] * out[1] * 16


# ---- 6. the byte-offset guard -----------------------------------------------------

@pytest.mark.parametrize("side", ["under", "over"])
def test_byte_offset_guard(side):
    """A half source whose pitch puts sh * pitch_bytes just under 0x7fffffff
    (k_dnfh reads it: 32-bit byte offsets), and just over (the call runs by
    the pack pass, 64-bit addresses). Only the rows themselves are written."""
    import torch
    lib = _lib()
    geom = D.K2
    sw, sh, nw, nh = geom
    src, want = D.case(geom, "f16", "f16")
    pb = ((0x7fffffff - 1) // sh) & ~15
    if side == "over":
        pb += 16
    assert (sh * pb < 0x7fffffff) == (side == "under") and pb % 16 == 0
    pitch = pb // 2
    try:
        big = torch.empty((sh - 1) * pitch + sw * 4, dtype=torch.float16,
                          device="cuda:0")
    except RuntimeError as e:  # (out of memory)
        pytest.skip("cannot allocate %.1f GiB: %s" % (
            sh * pb / 2.0 ** 30, str(e).split("\n")[0]))
    view = big.as_strided((sh, sw * 4), (pitch, 1))
    view.copy_(torch.from_numpy(src.reshape(sh, sw * 4).copy()))
    r0, p0 = _plan(geom, "f16", "f16", 2)
    dsrc = _dev(src)
    packed = _frame(lib, p0, dsrc.data_ptr(), want, "f16", "packed frame")
    r, p = _plan(geom, "f16", "f16", 2, pitch=pitch)
    got = _frame(lib, p, big.data_ptr(), want, "f16", "far rows, " + side)
    assert got.tobytes() == packed.tobytes()
    over = _held_over_float(lib, geom, p, 2)
    assert (over < nw * nh * 16) == (side == "under"), over


# ---- 7. threads -------------------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_four_threads_one_plan(t):
    """Four threads run whole-frame and band calls of ONE plan at once, each
    on its own stream into its own images."""
    import torch
    lib = _lib()
    geom = D.K3
    sw, sh, nw, nh = geom
    src, want = D.case(geom, t, t)
    r, p = _plan(geom, t, t, 0)
    dsrc = _dev(src)
    rb_ = nw * 4 * 2
    bands, odd = D.bands(nh)
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
                for a, b in bands:
                    _call(lib, p, dsrc.data_ptr(),
                          out[i][1].data_ptr() + a * rb_, a, b, st)
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
        D.same(_host(out[i][0], t, want.shape), want, t, "thread %d frame" % i)
        D.same(_host(out[i][1], t, want.shape), want, t, "thread %d bands" % i)
