"""General-ratio resizing (path 5) with half / bfloat16 images: k_gh's typed
loader reads a 16-bit source where it lies, and the last pass (k_gv, k_gf,
k_sacc*) narrows and stores a 16-bit result itself (gp_store_int_row).

Expected bits and inputs: tests/gp16_cases.py (the reference on the exactly
widened float32 source, its float32 result narrowed by numpy / by the header's
integer formula; word for word, NaN equal to NaN). The calls are made on
device-resident torch tensors through avirhip_resize_band."""
import ctypes as C
import threading
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import gp16_cases as G
from tests.gpass_route_cases import environment

pytestmark = pytest.mark.gpu

T = G.T
P5 = G.P5
NO_IO16 = {"AVIRHIP_GP_NO_IO16": "1"}


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


def _frame(lib, p, sptr, want, tout, what, off=0):
    """The whole frame into a zeroed image `off` bytes into its allocation,
    with a guard row behind it."""
    import torch
    rb_ = want.shape[1] * want.shape[2] * want.dtype.itemsize
    d = torch.full((off + want.nbytes + rb_,), 0x5a, dtype=torch.uint8,
                   device="cuda:0")
    _call(lib, p, sptr, d.data_ptr() + off, 0, want.shape[0], what=what)
    g = _host(d, "u8", (off + want.nbytes + rb_,))
    assert (g[:off] == 0x5a).all() and (g[off + want.nbytes:] == 0x5a).all(), \
        what + ": stored outside the image"
    got = g[off:off + want.nbytes].copy().view(T[tout][1]).reshape(want.shape)
    G.same(got, want, tout, what)
    return got


def _frame_and_bands(lib, p, dsrc, want, tout, what, whole=True):
    """Whole frame; the bands into one image; the odd band on its own."""
    import torch
    nh, nw, ch = want.shape
    rb_ = nw * ch * want.dtype.itemsize
    if whole:
        _frame(lib, p, dsrc.data_ptr(), want, tout, what + " frame")
    bands, odd = G.bands(nh)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    for a, b in bands:
        _call(lib, p, dsrc.data_ptr(), d.data_ptr() + a * rb_, a, b, what=what)
    G.same(_host(d, tout, want.shape), want, tout, what + " bands")
    if odd is not None:
        a, b = odd
        d = torch.zeros((b - a) * rb_, dtype=torch.uint8, device="cuda:0")
        _call(lib, p, dsrc.data_ptr(), d.data_ptr(), a, b, what=what)
        G.same(_host(d, tout, want[a:b].shape), want[a:b], tout,
               what + " odd band")


_FLOAT_BYTES = {}


def _held_over_float(lib, geom, p, path, variant):
    """Device bytes the plan holds, less those of the float32 -> float32 RGBA
    plan of the same geometry, path and variant after the same call (float
    RGBA is the kernels' own format: that plan holds no copy of either image,
    whereas one of 1-3 channels holds both)."""
    import torch
    ch = 4
    key = (geom, path, variant)
    if key not in _FLOAT_BYTES:
        src, want = G.case(geom, "f32", "f32", ch)
        r0, p0 = _plan(geom, "f32", "f32", path, variant, ch=ch)
        assert p0 is not None
        d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
        dsrc = _dev(src)
        _call(lib, p0, dsrc.data_ptr(), d.data_ptr(), 0, geom[3], what="float")
        torch.cuda.synchronize()
        _FLOAT_BYTES[key] = int(lib.avirhip_plan_device_bytes(p0))
    torch.cuda.synchronize()
    return int(lib.avirhip_plan_device_bytes(p)) - _FLOAT_BYTES[key]


_ids = ["%s-%s" % pr for pr in G.PAIRS]
_routes = sorted(G.ROUTES)


# ---- 1. every pair ------------------------------------------------------------

@pytest.mark.parametrize("path", [0, P5], ids=["auto", "path5"])
@pytest.mark.parametrize("tin,tout", G.PAIRS, ids=_ids)
def test_every_pair(tin, tout, path):
    lib = _lib()
    for name in _routes:
        geom, variant = G.geom(name), G.variant(name)
        for ch in (G.CHANNELS[name] if (tin, tout) in G.SAME else [4]):
            r, p = _plan(geom, tin, tout, path, variant, ch=ch)
            assert p is not None, (name, path)
            src, want = G.case(geom, tin, tout, ch)
            what = "%s %s->%s x%d path %d" % (name, tin, tout, ch, path)
            _frame_and_bands(lib, p, _dev(src), want, tout, what)


# ---- 2. chunk seams of the row-ahead load -----------------------------------------

@pytest.mark.parametrize("chunk", G.GH_CHUNKS)
@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_chunk_seams_of_the_typed_loader(t, chunk):
    lib = _lib()
    for name in ("up_two_pass", "between"):
        geom, variant = G.geom(name), G.variant(name)
        for ch in (3, 4):
            r, p = _plan(geom, t, t, P5, variant, ch=ch)
            assert p is not None
            src, want = G.case(geom, t, t, ch)
            with environment({"AVIRHIP_GH_CHUNK": str(chunk)}):
                _frame_and_bands(lib, p, _dev(src), want, t,
                                 "%s %s x%d chunk %d" % (name, t, ch, chunk))


# ---- 3. held memory -------------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_no_float_copies_on_the_plan(t):
    """Both sides fused: the plan holds neither the float copy of the source
    (sw * sh * 16 bytes) nor the float result (nw * nh * 16). The store alone
    (accumulation kernels, k_gf): the source copy, no float result. Under
    AVIRHIP_GP_NO_IO16 a fresh plan holds both."""
    lib = _lib()
    for name in G.BOTH_FUSED + G.STORE_ONLY:
        geom, variant = G.geom(name), G.variant(name)
        sw, sh, nw, nh = geom
        src, want = G.case(geom, t, t)
        dsrc = _dev(src)
        what = "%s %s" % (name, t)
        r, p = _plan(geom, t, t, P5, variant)
        assert p is not None
        _frame(lib, p, dsrc.data_ptr(), want, t, what)
        over = _held_over_float(lib, geom, p, P5, variant)
        print("%s: %d bytes over the float plan (source copy %d, result %d)" %
              (what, over, sw * sh * 16, nw * nh * 16))
        if name in G.BOTH_FUSED:
            assert over < min(sw * sh, nw * nh) * 16, what
        else:
            assert sw * sh * 16 <= over < sw * sh * 16 + nw * nh * 16, what
        with environment(NO_IO16):
            r2, p2 = _plan(geom, t, t, P5, variant)
            _frame(lib, p2, dsrc.data_ptr(), want, t, what + " no io16")
            over2 = _held_over_float(lib, geom, p2, P5, variant)
        print("%s under AVIRHIP_GP_NO_IO16: %d bytes over" % (what, over2))
        assert over2 >= sw * sh * 16 + nw * nh * 16, what


# ---- 4. the roads agree -----------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_roads_agree(t):
    """The fused call; pack pass and output stage (AVIRHIP_GP_NO_IO16); the
    tiles; the generic kernels (forced path 1): the same bytes."""
    lib = _lib()
    for name in ("up_two_pass", "between", "mixed", "acc"):
        geom, variant = G.geom(name), G.variant(name)
        for ch in (4, 3):
            src, want = G.case(geom, t, t, ch)
            dsrc = _dev(src)
            what = "%s %s x%d" % (name, t, ch)
            r, p = _plan(geom, t, t, P5, variant, ch=ch)
            assert p is not None
            got = _frame(lib, p, dsrc.data_ptr(), want, t, what)
            with environment(NO_IO16):
                g = _frame(lib, p, dsrc.data_ptr(), want, t, what + " no io16")
            assert g.tobytes() == got.tobytes(), what
            tiles = 0
            for path in (2, 3, 1):
                r2, p2 = _plan(geom, t, t, path, ch=ch)
                if p2 is None:
                    assert path != 1
                    continue
                tiles += (path != 1)
                g = _frame(lib, p2, dsrc.data_ptr(), want, t,
                           "%s path %d" % (what, path))
                assert g.tobytes() == got.tobytes(), (what, path)
            assert tiles >= 1, what


# ---- 5. refusals ------------------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_refused_images_take_the_pack_road(t):
    """A source base 1 byte off: the pack pass's float copy. A destination 1
    byte off: the float result and the output stage. rc == 0 and the same bits
    both times. A base 2 or 6 bytes into its allocation and a row pitch of
    sw * ch + 1 / + 5 elements (NaN padding) are read where they lie."""
    lib = _lib()
    for name, ch in (("up_two_pass", 4), ("between", 4), ("up_two_pass", 3)):
        geom, variant = G.geom(name), G.variant(name)
        sw, sh, nw, nh = geom
        src, want = G.case(geom, t, t, ch)
        what = "%s %s x%d" % (name, t, ch)
        both = (sw * sh + nw * nh) * 16

        r, p = _plan(geom, t, t, P5, variant, ch=ch)
        off = _dev(src, off=1, tail=7)
        _frame(lib, p, off.data_ptr() + 1, want, t, what + " source 1 byte off")
        over = _held_over_float(lib, geom, p, P5, variant)
        assert sw * sh * 16 <= over < both, (what, over)

        r, p = _plan(geom, t, t, P5, variant, ch=ch)
        dsrc = _dev(src)
        _frame(lib, p, dsrc.data_ptr(), want, t, what + " result 1 byte off",
               off=1)
        over = _held_over_float(lib, geom, p, P5, variant)
        assert nw * nh * 16 <= over < both, (what, over)

        for o in (2, 6):
            r, p = _plan(geom, t, t, P5, variant, ch=ch)
            off = _dev(src, off=o, tail=8 - o)
            _frame(lib, p, off.data_ptr() + o, want, t,
                   "%s both %d bytes in" % (what, o), off=o)
            over = _held_over_float(lib, geom, p, P5, variant)
            assert over < min(sw * sh, nw * nh) * 16, (what, o, over)

        for extra in (1, 5):
            pitch = sw * ch + extra
            r, p = _plan(geom, t, t, P5, variant, pitch=pitch, ch=ch)
            dflat = _dev(G.padded(src, pitch, t))
            _frame_and_bands(lib, p, dflat, want, t,
                             "%s pitch + %d" % (what, extra))
            over = _held_over_float(lib, geom, p, P5, variant)
            assert over < min(sw * sh, nw * nh) * 16, (what, extra, over)


@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_images_under_four_elements(t):
    """Fewer than four elements up to the end of a band's last source row: the
    loader's 8-byte load does not fit, so `raw16` (api.cpp, avir_road) is false. The
    planner gives sources this small another chain than the pass kernels'
    (tests/test_gp16_table.py), so forced path 5 refuses their plans at
    avirhip_plan_set_path and the automatic path runs them: rc == 0, the
    reference's bits, nothing stored outside the image."""
    lib = _lib()
    for sw, sh, nw, nh, ch in G.TINY:
        geom = (sw, sh, nw, nh)
        src, want = G.case(geom, t, t, ch)
        dsrc = _dev(src)  # (an allocation of exactly the image's bytes)
        r5, p5 = _plan(geom, t, t, P5, ch=ch)
        assert p5 is None, geom
        r, p = _plan(geom, t, t, 0, ch=ch)
        what = "%r x%d %s" % (geom, ch, t)
        _frame(lib, p, dsrc.data_ptr(), want, t, what, off=2)
        for a in range(nh):
            d = _dev(np.zeros(nw * ch, T[t][1]))
            _call(lib, p, dsrc.data_ptr(), d.data_ptr(), a, a + 1, what=what)
            G.same(_host(d, t, want[a:a + 1].shape), want[a:a + 1], t,
                   "%s row %d" % (what, a))


@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_rows_of_three_elements(t):
    """The narrowest sources forced path 5 takes: rows of three elements, read
    where they lie (no float copy on the plan) -- every 8-byte load of the
    image's last row starts early and is shifted. The source is an allocation
    of exactly the image's bytes."""
    lib = _lib()
    for sw, sh, nw, nh, ch in G.THIN:
        geom = (sw, sh, nw, nh)
        src, want = G.case(geom, t, t, ch)
        dsrc = _dev(src)
        r, p = _plan(geom, t, t, P5, G.V_UPG2, ch=ch)
        assert p is not None, geom
        what = "%r x%d %s path 5" % (geom, ch, t)
        _frame_and_bands(lib, p, dsrc, want, t, what)
        over = _held_over_float(lib, geom, p, P5, G.V_UPG2)
        assert over < min(sw * sh, nw * nh) * 16, (what, over)
        # the band of the last rows alone, and the first row alone
        for a, b_ in ((nh - 1, nh), (0, 1)):
            d = _dev(np.zeros((b_ - a) * nw * ch, T[t][1]))
            _call(lib, p, dsrc.data_ptr(), d.data_ptr(), a, b_, what=what)
            G.same(_host(d, t, want[a:b_].shape), want[a:b_], t,
                   "%s rows %d..%d" % (what, a, b_))


# ---- 6. special values ----------------------------------------------------------

def _special(lib, tin, tout, which, src, ref, want):
    size, out, variant = which
    c = G.special_classes(tout, ref, want)
    print(tin, tout, which, c)
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0 and c["denormal"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    if tout == "f16":
        assert c["fin_to_inf"] > 0
    geom = size + out
    r, p = _plan(geom, tin, tout, P5, variant)
    assert p is not None
    dsrc = _dev(src)
    got = _frame(lib, p, dsrc.data_ptr(), want, tout,
                 "special values %s->%s %r" % (tin, tout, geom))
    gf, wf = G.as_f32(got, tout), G.as_f32(want, tout)
    assert np.array_equal(np.isinf(gf), np.isinf(wf))
    assert np.array_equal(np.isnan(gf), np.isnan(wf))
    return got


@pytest.mark.parametrize("which", [G.SPECIAL_UP, G.SPECIAL_DN],
                         ids=["up", "down"])
def test_special_values_half(which):
    """+-0, denormals, +-65504, +-Inf, NaN and a 64000 block whose overshoot
    crosses 65504 through the typed loader and the narrowing store; the block
    of source denormals reaches the result (it is not the flushed frame's)."""
    lib = _lib()
    src, ref, want = G.special_case("f16", which)
    got = _special(lib, "f16", "f16", which, src, ref, want)
    fsrc, fref, fwant = G.special_case("f16", which, flushed=True)
    assert int((G.words(got) != G.words(fwant)).sum()) > 0


@pytest.mark.parametrize("tin", ["f32", "bf16"])
@pytest.mark.parametrize("which", [G.SPECIAL_UP, G.SPECIAL_DN],
                         ids=["up", "down"])
def test_special_values_bfloat16(which, tin):
    """float32 denormals, NaN, +-Inf and a block near 1e38 into a bfloat16
    result, from the float32 frame and from its bfloat16 narrowing."""
    lib = _lib()
    if tin == "f32":
        src, ref, want = G.special_case("bf16", which)
    else:
        src, ref, want = G.special_bf16_case(which)
    _special(lib, tin, "bf16", which, src, ref, want)


# ---- 7. a source window -----------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_window_of_16_bit_rows_between_nans(t):
    """avirhip_resize_window from a device window whose surroundings are NaN:
    staged into the plan's frame-sized buffer, read raw from there."""
    import torch
    lib = _lib()
    for name in ("up_two_pass", "between"):
        geom, variant = G.geom(name), G.variant(name)
        sw, sh, nw, nh = geom
        src, want = G.case(geom, t, t)
        r, p = _plan(geom, t, t, P5, variant)
        assert p is not None
        r0, r1 = nh // 3, nh // 3 + 23
        a, b = C.c_int(), C.c_int()
        abi.check(lib.avirhip_band_source_rows(p, r0, r1, C.byref(a),
                                               C.byref(b)), "rows")
        n = b.value - a.value + 1
        guard = 8
        pad = (np.array([G.NAN], np.uint16)[0] if t == "bf16"
               else np.float16(np.nan))
        big = np.full((n + 2 * guard, sw, 4), pad, T[t][1])
        big[guard:guard + n] = src[a.value:b.value + 1]
        dbig = _dev(big)
        dst = torch.zeros((r1 - r0) * nw * 4 * 2, dtype=torch.uint8,
                          device="cuda:0")
        abi.check(lib.avirhip_resize_window(
            p, dbig.data_ptr() + guard * sw * 4 * 2, abi.MEM_DEVICE, a.value,
            n, dst.data_ptr(), abi.MEM_DEVICE, r0, r1, None), "window")
        G.same(_host(dst, t, want[r0:r1].shape), want[r0:r1], t,
               "%s %s window band" % (name, t))


# ---- 8. threads -------------------------------------------------------------------

def test_four_threads_one_plan():
    """Four threads run whole-frame and band calls of ONE plan at once, each
    on its own stream into its own images."""
    import torch
    lib = _lib()
    t = "f16"
    geom, variant = G.geom("up_two_pass"), G.variant("up_two_pass")
    sw, sh, nw, nh = geom
    src, want = G.case(geom, t, t)
    r, p = _plan(geom, t, t, P5, variant)
    dsrc = _dev(src)
    rb_ = nw * 4 * 2
    bands, odd = G.bands(nh)
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
        G.same(_host(out[i][0], t, want.shape), want, t, "thread %d frame" % i)
        G.same(_host(out[i][1], t, want.shape), want, t, "thread %d bands" % i)
