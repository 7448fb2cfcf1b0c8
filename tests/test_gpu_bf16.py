"""bfloat16 images on the GPU. The rule (include/avirhip.h, AVIRHIP_BF16): a
call with bfloat16 elements is the same call with float32 buffers -- the
source widened exactly (bits << 16), the float32 result narrowed
round-to-nearest-even by the integer formula

    (u + 0x7fff + ((u >> 16) & 1)) >> 16        (u: the float's bits, not NaN)

The expected bits of every call here are therefore

    reference(widen(src)) -> float32 result -> the formula

compared word for word, except that elements that are NaN on both sides count
as equal. The reference is the one every GPU test uses (tests/helpers.py).
bfloat16 host images are np.uint16 bit arrays; the calls go through the
pointer-level ABI with the type codes (numpy has no bfloat16)."""
import ctypes as C
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H

pytestmark = pytest.mark.gpu

# element types by name: (type code, numpy type of the host array)
_T = {"bf16": (abi.BF16, np.uint16), "f16": (abi.F16, np.float16),
      "f32": (abi.F32, np.float32), "u8": (abi.U8, np.uint8)}
NAN = 0x7fc0  # a bfloat16 NaN


def widen(b):
    """bfloat16 bits -> float32, exact for every bit pattern."""
    return (np.ascontiguousarray(b).astype(np.uint32) << 16).view(np.float32)


def narrow(f):
    """float32 -> bfloat16 bits: the contract's integer formula; NaN -> a NaN."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(f)] = NAN
    return r


def _isnan(a, t):
    return np.isnan(widen(a)) if t == "bf16" else (
        np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool))


def _src(shape, t, seed):
    if t == "u8":
        return rb.lcg_u8(shape, seed=seed)
    a = rb.lcg_f32(shape, seed=seed)
    return narrow(a) if t == "bf16" else a.astype(_T[t][1])


def _as_f32(src, t):
    return widen(src) if t == "bf16" else (
        src.astype(np.float32) if t == "f16" else src)


def _from_f32(res, t):
    if t == "bf16":
        return narrow(res)
    if t == "f16":
        with np.errstate(over="ignore", invalid="ignore"):
            return res.astype(np.float16)
    return res


def _want_avir(src, tin, nw, nh, tout, bits=8, **kw):
    rt = np.float32 if tout in ("bf16", "f16") else _T[tout][1]
    return _from_f32(H.checker_avir(_as_f32(src, tin), nw, nh, out_dtype=rt,
                                    resbits=bits, **kw), tout)


def _want_lancir(src, tin, nw, nh, tout, **kw):
    rt = np.float32 if tout in ("bf16", "f16") else _T[tout][1]
    return _from_f32(H.checker_lancir(_as_f32(src, tin), nw, nh, out_dtype=rt,
                                      **kw), tout)


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, tout, what):
    """Word for word; NaN == NaN whatever the payload."""
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype, what
    bad = _words(got) != _words(want)
    bad &= ~(_isnan(got, tout) & _isnan(want, tout))
    n = int(bad.sum())
    print("%s: %d of %d elements differ" % (what, n, want.size))
    assert n == 0, "%s: %d of %d elements differ, first at %r" % (
        what, n, want.size, tuple(np.argwhere(bad)[0]))


def _plan(r, sw, sh, nw, nh, ch, tin, tout, path, variant=0, pitch=0):
    """The plan on a forced path (None: the automatic one); None when the
    path cannot run the plan (AVIRHIP_EUNSUPPORTED -- anything else fails)."""
    lib = abi.load()
    p = r.plan(sw, sh, nw, nh, ch, 0.0, None, _T[tin][0], _T[tout][0], pitch)
    if path is None:
        return p
    rc = lib.avirhip_plan_set_path(p, path)
    if rc != 0:
        assert rc == abi.EUNSUPPORTED, rc
        return None
    abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
    return p


def _resize(r, src, tin, nw, nh, tout, aVars=None):
    """CImageResizer::resizeImage by type code, host buffers; None when the
    forced path refused the call."""
    sh, sw, ch = src.shape
    dst = np.zeros((nh, nw, ch), _T[tout][1])
    rc = abi.load().avirhip_resizer_resize(
        r._h, src.ctypes.data, abi.MEM_HOST, sw, sh, 0, dst.ctypes.data,
        abi.MEM_HOST, nw, nh, ch, 0.0,
        C.byref(aVars) if aVars is not None else None, _T[tin][0],
        _T[tout][0], None)
    if rc == abi.EUNSUPPORTED:
        return None
    abi.check(rc, "avirhip_resizer_resize")
    return dst


def _dev_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)
                            ).to("cuda:0")


# ---- the marching kernel -------------------------------------------------

@pytest.mark.parametrize("tin", ["bf16", "f32"])
def test_marching_kernel_bf16_rgba(tin, monkeypatch):
    """k_up2< true, 7, 224 > / k_up2< true, 7 >: bfloat16 RGBA pixels read
    where they lie and stored by the vertical phase, forced path 4: whole
    frames, bands, device images the fused forms must refuse (base 2 bytes off
    a dword, odd row pitch), and the same calls through the pack pass and the
    output stage (AVIRHIP_UP2_NO_RAW, AVIRHIP_VARIANT_UP2_UNFUSED_IO)."""
    import torch
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    ran = 0
    for (sw, sh) in [(97, 61), (333, 40), (1001, 9), (50, 50), (642, 361)]:
        src = _src((sh, sw, 4), tin, seed=sw + 4)
        nw, nh = sw * 2, sh * 2
        ref = H.checker_avir(_as_f32(src, tin), nw, nh, out_dtype=np.float32,
                             resbits=16)
        want = narrow(ref)
        if (sw, sh) == (642, 361):
            # ties on which round-half-up and nearest-even differ
            u = ref.view(np.uint32)
            ties = int((((u & 0xffff) == 0x8000) & (((u >> 16) & 1) == 0)
                        ).sum())
            print("ties to even, downwards, in the %s frame: %d" % (tin, ties))
            assert ties >= 10, ties
        r = avir_amd.CImageResizer(16)
        p = _plan(r, sw, sh, nw, nh, 4, tin, "bf16", abi.PATH_UP2)
        if p is None:
            continue
        ran += 1
        got = _resize(r, src, tin, nw, nh, "bf16")
        _same(got, want, "bf16", "frame %r" % ((sw, sh),))
        out = np.zeros((nh, nw, 4), np.uint16)
        for a_, b_ in [(0, nh // 3), (nh // 3, nh - 5), (nh - 5, nh)]:
            abi.check(lib.avirhip_resize_band(
                p, src.ctypes.data, abi.MEM_HOST, out[a_:b_].ctypes.data,
                abi.MEM_HOST, a_, b_, None), "band")
        _same(out, want, "bf16", "bands %r" % ((sw, sh),))
        # the same bytes without the raw source, and without any fused I/O
        monkeypatch.setenv("AVIRHIP_UP2_NO_RAW", "1")
        g2 = _resize(r, src, tin, nw, nh, "bf16")
        monkeypatch.delenv("AVIRHIP_UP2_NO_RAW")
        assert g2.tobytes() == got.tobytes(), ("pack pass", sw, sh)
        abi.check(lib.avirhip_plan_set_variant(
            p, abi.VARIANT_UP2_UNFUSED_IO), "variant")
        g3 = _resize(r, src, tin, nw, nh, "bf16")
        abi.check(lib.avirhip_plan_set_variant(p, 0), "variant")
        assert g3.tobytes() == got.tobytes(), ("unfused", sw, sh)
        # device images: a destination 2 bytes off dword alignment (the fused
        # store refuses it), a bfloat16 source likewise (the raw road refuses)
        dsrc = _dev_bytes(src)
        dst = torch.zeros(want.nbytes + 8, dtype=torch.uint8, device="cuda:0")
        calls = [(dsrc.data_ptr(), 2)]
        if tin == "bf16":
            buf = torch.zeros(src.nbytes + 8, dtype=torch.uint8,
                              device="cuda:0")
            buf[2:2 + src.nbytes] = dsrc
            calls.append((buf.data_ptr() + 2, 0))
        for sp, do in calls:
            abi.check(lib.avirhip_resize_band(
                p, sp, abi.MEM_DEVICE, dst.data_ptr() + do, abi.MEM_DEVICE, 0,
                nh, None), "device")
            torch.cuda.synchronize()
            g4 = dst.cpu().numpy()[do:do + want.nbytes].view(np.uint16)
            _same(g4, want, "bf16", "unaligned %s %r" % (
                "destination" if do else "source", (sw, sh)))
        if tin != "bf16":
            continue
        # an odd row pitch in elements: rows alternate in dword alignment; the
        # padding element is a NaN
        pitch = sw * 4 + 1
        p2 = _plan(r, sw, sh, nw, nh, 4, "bf16", "bf16", abi.PATH_UP2,
                   pitch=pitch)
        assert p2 is not None
        flat = np.full(sh * pitch, NAN, np.uint16)
        flat.reshape(sh, pitch)[:, :sw * 4] = src.reshape(sh, sw * 4)
        dflat = _dev_bytes(flat)
        abi.check(lib.avirhip_resize_band(
            p2, dflat.data_ptr(), abi.MEM_DEVICE, dst.data_ptr(),
            abi.MEM_DEVICE, 0, nh, None), "odd pitch")
        torch.cuda.synchronize()
        _same(dst.cpu().numpy()[:want.nbytes].view(np.uint16), want, "bf16",
              "odd pitch %r" % ((sw, sh),))
    assert ran >= 3, "path 4 took %d of the shapes" % ran


# ---- every family through the general road ---------------------------------

V = abi
# (sw, sh, nw, nh), [(path, variant)]: tests/param_cases.py and
# tests/gpass_route_cases.py sizes
FAMILIES = [
    # exact 2x: generic, tiles, marching kernel (both forms), pass kernels
    ((96, 70, 192, 140), [(0, 0), (1, 0), (2, 0), (4, 0),
                          (4, V.VARIANT_UP2_PLAIN_V), (5, 0)]),
    # upsizing: tiles, fused tile, pass kernels two-pass and fused (k_gf)
    ((300, 200, 460, 307), [(0, 0), (1, 0), (2, 0), (3, 0),
                            (5, V.VARIANT_UPG_TWO_PASS),
                            (5, V.VARIANT_UPG_FUSED)]),
    # 1 < k < 2 down
    ((600, 400, 400, 267), [(0, 0), (5, 0)]),
    # whole ratios 2 and 3: k_dnf, and its two passes
    ((600, 400, 300, 200), [(0, 0), (2, 0), (2, V.VARIANT_DN_TWO_PASS),
                            (3, 0)]),
    ((600, 402, 200, 134), [(0, 0), (2, 0), (2, V.VARIANT_DN_TWO_PASS)]),
    # 2.7x down: the accumulation kernels, both forms
    ((600, 405, 222, 150), [(0, 0), (1, 0), (5, 0),
                            (5, V.VARIANT_SACC_LADDER),
                            (5, V.VARIANT_SACC_OPTIMISTIC)]),
]

PAIRS = [("bf16", "bf16"), ("bf16", "u8"), ("u8", "bf16"), ("bf16", "f32"),
         ("bf16", "f16")]


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("tin,tout", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_every_family_converts_bf16_pixels(ch, tin, tout):
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    bits = 8 if tout == "u8" else 16
    ran = 0
    for (sw, sh, nw, nh), runs in FAMILIES:
        src = _src((sh, sw, ch), tin, seed=sw + ch)
        want = _want_avir(src, tin, nw, nh, tout, bits)
        for path, variant in runs:
            r = avir_amd.CImageResizer(bits)
            if _plan(r, sw, sh, nw, nh, ch, tin, tout, path, variant) is None:
                continue
            got = _resize(r, src, tin, nw, nh, tout)
            if got is None:
                continue
            ran += 1
            _same(got, want, tout, "%r path %d variant %d" % (
                (sw, sh, nw, nh), path, variant))
    # (26 runs in the table; narrow plans of small frames may refuse a path)
    assert ran >= 13, ran


# ---- CLancIR --------------------------------------------------------------

def _lancir(l, src, tin, nw, nh, tout, P=None, pitch=0, fill=0):
    """CLancIR::resizeImage by type code; None when the forced path refused
    the call. `pitch`: destination row pitch in elements (0: packed)."""
    sh, sw, ch = src.shape
    dst = np.full((nh, pitch or nw * ch), fill, _T[tout][1])
    rc = abi.load().avirhip_lancir_resize(
        l._h, src.ctypes.data, abi.MEM_HOST, sw, sh, dst.ctypes.data,
        abi.MEM_HOST, nw, nh, ch, C.byref(P) if P is not None else None,
        _T[tin][0], _T[tout][0], None)
    if rc == abi.EUNSUPPORTED:
        return None
    assert abi.check(rc, "avirhip_lancir_resize") == nh
    return dst


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("tin,tout", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_lancir_bf16_pixels(ch, tin, tout):
    """(160, 120) -> (320, 240) is the exact-2x geometry: k_lanc2 behind the
    pack pass and the output stage on its path."""
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    for (sw, sh, nw, nh) in [(160, 120, 320, 240), (192, 108, 250, 140),
                             (300, 240, 100, 80)]:
        src = _src((sh, sw, ch), tin, seed=sw + ch)
        want = _want_lancir(src, tin, nw, nh, tout)
        ran = 0
        for path, variant in [(0, 0), (1, 0), (4, 0), (5, 0),
                              (5, abi.VARIANT_UPG_FUSED)]:
            l = avir_amd.CLancIR()
            p = l.plan(sw, sh, nw, nh, ch, None, _T[tin][0], _T[tout][0])
            rc = lib.avirhip_plan_set_path(p, path)
            if rc != 0:
                assert rc == abi.EUNSUPPORTED
                continue
            abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
            got = _lancir(l, src, tin, nw, nh, tout)
            if got is None:
                continue
            ran += 1
            _same(got, want, tout, "lancir %r path %d variant %d" % (
                (sw, sh, nw, nh), path, variant))
        assert ran >= 2, ran  # (the automatic and the generic path at least)
        # a non-default `la`
        P = avir_amd.CLancIRParams()
        P.la = 4.0
        _same(_lancir(avir_amd.CLancIR(), src, tin, nw, nh, tout, P),
              _want_lancir(src, tin, nw, nh, tout, la=4.0), tout,
              "lancir %r la 4" % ((sw, sh, nw, nh),))
        # NewSSize larger than the row: the padding survives the call
        npad = 6
        wantp = _want_lancir(src, tin, nw, nh, tout, npad=npad)
        P = avir_amd.CLancIRParams(aNewSSize=nw * ch + npad)
        dst = _lancir(avir_amd.CLancIR(), src, tin, nw, nh, tout, P,
                      pitch=nw * ch + npad, fill=5)
        _same(dst[:, :nw * ch].reshape(nh, nw, ch), wantp, tout, "NewSSize")
        assert (dst[:, nw * ch:] == 5).all()


# ---- gamma ----------------------------------------------------------------

@pytest.mark.parametrize("tout", ["bf16", "u8"])
@pytest.mark.parametrize("geom", [(96, 70, 192, 140), (300, 200, 460, 307),
                                  (600, 402, 200, 134)])
def test_gamma_bf16_source(tout, geom):
    """UseSRGBGamma: the bfloat16 source is linearised as the float source is;
    the bfloat16 result is the narrowed LINEAR float result (a float-type
    result is not de-linearised, avir.h:4956-4979), the uint8 result is
    de-linearised."""
    sw, sh, nw, nh = geom
    src = _src((sh, sw, 4), "bf16", seed=sw)
    bits = 8 if tout == "u8" else 16
    want = _want_avir(src, "bf16", nw, nh, tout, bits, gamma=True, alpha=3)
    v = avir_amd.CImageResizerVars()
    v.UseSRGBGamma, v.AlphaIndex = 1, 3
    got = _resize(avir_amd.CImageResizer(bits), src, "bf16", nw, nh, tout, v)
    _same(got, want, tout, "gamma %r" % (geom,))
    if tout == "bf16":
        # linear: the same call into a float32 image, narrowed
        lin = _resize(avir_amd.CImageResizer(bits), src, "bf16", nw, nh,
                      "f32", v)
        _same(got, narrow(lin), "bf16", "linear %r" % (geom,))


# ---- special values -------------------------------------------------------

def _special_bf16_source(sw, sh):
    """Every bfloat16 bit-pattern class, scattered in an ordinary frame."""
    src = _src((sh, sw, 4), "bf16", seed=9)
    # (the lower half: bfloat16 denormals, 0x0001 .. 0x007f of either sign)
    k = rb.lcg_u8((sh - 24, sw, 4), seed=5).astype(np.uint16)
    src[24:] = (k & 0x7f) | ((k & 0x80) << 8)
    src[2, 3] = [0x0000, 0x8000, 0x0000, 0x8000]          # +-0
    src[5, 7] = [0x0001, 0x007f, 0x8001, 0x807f]          # denormals
    src[9, 20] = [0x7f7f, 0xff7f, 0x7f7f, 0xff7f]         # largest finite
    src[14, 40] = [0x7f80, 0x3f80, 0x3f80, 0x3f80]        # +Inf
    src[3, 11] = [0x3f80, 0xff80, 0x3f80, 0x3f80]         # -Inf
    src[12, 50] = [0x3f80, 0x3f80, 0x7fc0, 0x3f80]        # quiet NaN
    src[16, 55] = [0x7f81, 0xffff, 0x3f80, 0xff81]        # other NaNs
    src[6:14, 24:32] = 0x0080                             # smallest normal
    return src


def _special_f32_source(sw, sh):
    """float32 pixels whose results land on float32 denormals, on the largest
    binades, on +-Inf (the sums of the 2.4e38 blocks overflow) and on NaN."""
    src = rb.lcg_f32((sh, sw, 4), seed=9)
    src[24:] = rb.lcg_f32((sh - 24, sw, 4), seed=5) * np.float32(1.1e-38)
    big = np.array([1.5e38, -1.6e38, 2.4e38, -2.4e38], np.float32)
    src[4:16, 8:24] = big
    src[4:16, 36:52] = -big
    src[40, 58] = [np.nan, 1.0, 1.0, 1.0]
    src[44, 6] = [1.0, np.inf, -np.inf, 1.0]
    return src


@pytest.mark.parametrize("path", [None, 4, 1], ids=["auto", "4", "1"])
def test_special_values(path):
    """Source side: +-0, bfloat16 denormals, the largest finite values, +-Inf
    and NaNs of several payloads, read as bfloat16. Result side: float32
    sources whose float32 results are denormal, above 2^127, infinite and NaN,
    stored as bfloat16. (Decides whether the hardware narrowing of k_up2's
    store form meets the contract: path 4 and the automatic path of these
    frames run it. FINITE results that narrow to Inf cannot come out of this
    geometry -- the reference's 2x upsampling holds twice the source in an
    intermediate buffer, so its finite results end near 2e38, below
    0x7f7f8000 = 3.396e38: test_lancir_finite_results_that_narrow_to_inf.)"""
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    sw, sh = 64, 48
    nw, nh = sw * 2, sh * 2
    for tin, src in (("bf16", _special_bf16_source(sw, sh)),
                     ("f32", _special_f32_source(sw, sh))):
        ref = H.checker_avir(_as_f32(src, tin), nw, nh, out_dtype=np.float32,
                             resbits=16)
        want = narrow(ref)
        wf = widen(want)
        fin = np.isfinite(ref)
        assert np.isnan(ref).any() and np.isinf(ref).any()
        # (denormal results: float32 denormals in, bfloat16 denormals out)
        assert (fin & (ref != 0) & (np.abs(ref) < 2.0 ** -126)).any()
        assert ((wf != 0) & (np.abs(wf) < 2.0 ** -126)).any()
        if tin == "f32":
            assert (fin & (np.abs(ref) > 2.0 ** 127)).any()
        r = avir_amd.CImageResizer(16)
        p = _plan(r, sw, sh, nw, nh, 4, tin, "bf16", path)
        assert p is not None
        print("special values, %s source: path %s runs path %d" % (
            tin, path, lib.avirhip_plan_get_path(p)))
        got = _resize(r, src, tin, nw, nh, "bf16")
        _same(got, want, "bf16", "special values, %s source, path %s" % (
            tin, path))
        gf = widen(got)
        assert np.array_equal(np.isinf(gf), np.isinf(wf))
        assert np.array_equal(np.isnan(gf), np.isnan(wf))


@pytest.mark.parametrize("path", [0, 1], ids=["auto", "generic"])
def test_lancir_finite_results_that_narrow_to_inf(path):
    """Finite float32 results from 0x7f7f8000 upwards (the bfloat16 halfway
    point above the largest finite value) become +-Inf: CLancIR, which keeps
    no scaled intermediate, on blocks of +-3.05e38 whose overshoot lands
    there."""
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    sw, sh, nw, nh = 96, 64, 125, 83
    src = rb.lcg_f32((sh, sw, 4), seed=9)
    blk = np.float32(3.05e38) * (1 - np.float32(0.004) *
                                 rb.lcg_f32((24, 32, 4), seed=4))
    src[4:28, 8:40] = blk
    src[4:28, 50:82] = -blk
    src[34:58, 8:40] = -blk
    ref = H.checker_lancir(src, nw, nh, out_dtype=np.float32)
    want = narrow(ref)
    wf = widen(want)
    fin = np.isfinite(ref)
    up, dn = int((fin & (wf == np.inf)).sum()), int((fin & (wf == -np.inf)).sum())
    print("finite results narrowed to +Inf: %d, to -Inf: %d" % (up, dn))
    assert up >= 10 and dn >= 10  # (23 and 29 with the reference)
    l = avir_amd.CLancIR()
    p = l.plan(sw, sh, nw, nh, 4, None, abi.F32, abi.BF16)
    abi.check(lib.avirhip_plan_set_path(p, path), "path")
    got = _lancir(l, src, "f32", nw, nh, "bf16")
    assert got is not None
    _same(got, want, "bf16", "lancir beyond the largest finite, path %d" % path)
    assert np.array_equal(np.isinf(widen(got)).reshape(wf.shape), np.isinf(wf))


# ---- windows ----------------------------------------------------------------

@pytest.mark.parametrize("geom,path", [((97, 130, 194, 260), 4),
                                       ((300, 200, 460, 307), 5)],
                         ids=["marching", "pass-kernels"])
def test_window_of_bf16_rows_between_nans(geom, path):
    """avirhip_resize_window from a device window of bfloat16 rows whose
    surroundings are NaNs (tests/test_gpu_window.py's manner)."""
    import torch
    sw, sh, nw, nh = geom
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    src = _src((sh, sw, 4), "bf16", seed=sw)
    want = _want_avir(src, "bf16", nw, nh, "bf16", 16)
    r = avir_amd.CImageResizer(16)
    p = _plan(r, sw, sh, nw, nh, 4, "bf16", "bf16", path)
    assert p is not None
    r0, r1 = nh // 3, nh // 3 + 41
    a, b = C.c_int(), C.c_int()
    abi.check(lib.avirhip_band_source_rows(p, r0, r1, C.byref(a), C.byref(b)),
              "rows")
    n = b.value - a.value + 1
    G = 16
    big = np.full((n + 2 * G, sw, 4), NAN, np.uint16)
    big[G:G + n] = src[a.value:b.value + 1]
    dbig = _dev_bytes(big)
    dst = torch.zeros((r1 - r0) * nw * 4 * 2, dtype=torch.uint8,
                      device="cuda:0")
    abi.check(lib.avirhip_resize_window(
        p, dbig.data_ptr() + G * sw * 4 * 2, abi.MEM_DEVICE, a.value, n,
        dst.data_ptr(), abi.MEM_DEVICE, r0, r1, None), "window")
    torch.cuda.synchronize()
    _same(dst.cpu().numpy().view(np.uint16), want[r0:r1], "bf16",
          "window band")


# ---- torch ------------------------------------------------------------------

def test_torch_bf16_tensor_on_a_side_stream():
    import torch
    sw, sh = 160, 120
    src = _src((sh, sw, 4), "bf16", seed=3)
    want = _want_avir(src, "bf16", 320, 240, "bf16", 16)
    # (the contract's formula is torch's own conversion)
    f = rb.lcg_f32((sh, sw, 4), seed=3)
    assert np.array_equal(
        torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy()
        .view(np.uint16), src)
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        dsrc = torch.from_numpy(src.view(np.int16)).view(torch.bfloat16).to(
            "cuda:0", non_blocking=False)
        got = avir_amd.CImageResizer(16).resize(dsrc, 320, 240)
        got8 = avir_amd.CImageResizer(8).resize(dsrc, 320, 240,
                                                out_dtype=torch.uint8)
        back = avir_amd.CImageResizer(16).resize(
            dsrc.to(torch.float32), 320, 240, out_dtype=torch.bfloat16)
    st.synchronize()
    assert got.dtype == torch.bfloat16 and got.is_cuda
    _same(got.view(torch.int16).cpu().numpy().view(np.uint16), want, "bf16",
          "torch bfloat16")
    _same(back.view(torch.int16).cpu().numpy().view(np.uint16), want, "bf16",
          "torch float32 -> bfloat16")
    _same(got8.cpu().numpy(), _want_avir(src, "bf16", 320, 240, "u8", 8),
          "u8", "torch bfloat16 -> uint8")
