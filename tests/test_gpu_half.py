"""Half-precision (float16) images on the GPU. The rule (include/avirhip.h,
AVIRHIP_F16): a call with half elements is the same call with float32 buffers
-- the source widened exactly, the float32 result narrowed to half with
round-to-nearest-even. The expected bits of every call here are therefore

    reference(float32(src_half)) -> float32 result -> numpy .astype(float16)

compared word for word, except that elements that are NaN on both sides count
as equal. The reference is the one every GPU test uses (tests/helpers.py)."""
import ctypes as C
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H

pytestmark = pytest.mark.gpu

F16, F32, U8 = np.float16, np.float32, np.uint8
_T = {np.dtype(F16): abi.F16, np.dtype(F32): abi.F32, np.dtype(U8): abi.U8}


def _src(shape, tin, seed):
    if np.dtype(tin) == np.dtype(U8):
        return rb.lcg_u8(shape, seed=seed)
    a = rb.lcg_f32(shape, seed=seed)
    return a.astype(F16) if np.dtype(tin) == np.dtype(F16) else a


def _widen(src):
    return src.astype(F32) if src.dtype == np.dtype(F16) else src


def _narrow(res, tout):
    if np.dtype(tout) == np.dtype(F16):
        with np.errstate(over="ignore", invalid="ignore"):
            return res.astype(F16)
    return res


def _want_avir(src, nw, nh, tout, bits=8, **kw):
    rt = F32 if np.dtype(tout) == np.dtype(F16) else tout
    return _narrow(H.checker_avir(_widen(src), nw, nh, out_dtype=rt,
                                  resbits=bits, **kw), tout)


def _want_lancir(src, nw, nh, tout, **kw):
    rt = F32 if np.dtype(tout) == np.dtype(F16) else tout
    return _narrow(H.checker_lancir(_widen(src), nw, nh, out_dtype=rt, **kw),
                   tout)


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    """Word for word; NaN == NaN whatever the payload."""
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype, what
    bad = _words(got) != _words(want)
    if want.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    n = int(bad.sum())
    print("%s: %d of %d elements differ" % (what, n, want.size))
    assert n == 0, "%s: %d of %d elements differ, first at %r" % (
        what, n, want.size, tuple(np.argwhere(bad)[0]))


def _plan(r, sw, sh, nw, nh, ch, tin, tout, path, variant=0):
    """The plan on a forced path; None when the path cannot run the plan
    (AVIRHIP_EUNSUPPORTED -- anything else fails)."""
    lib = abi.load()
    p = r.plan(sw, sh, nw, nh, ch, 0.0, None, _T[np.dtype(tin)],
               _T[np.dtype(tout)])
    rc = lib.avirhip_plan_set_path(p, path)
    if rc != 0:
        assert rc == abi.EUNSUPPORTED, rc
        return None
    abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
    return p


def _run(r, src, nw, nh, tout):
    """resize(); None when the forced path refused the call."""
    try:
        return r.resize(src, nw, nh, out_dtype=tout)
    except abi.AvirHipError as e:
        assert "(%d)" % abi.EUNSUPPORTED in str(e), e
        return None


def _dev_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)
                            ).to("cuda:0")


# ---- the marching kernel -------------------------------------------------

@pytest.mark.parametrize("tin", [F16, F32], ids=["f16", "f32"])
def test_marching_kernel_half_rgba(tin, monkeypatch):
    """k_up2< true, 6, 124 > / k_up2< true, 6 >: half RGBA pixels read where
    they lie and stored by the vertical phase, forced path 4: whole frames,
    bands, device sources the raw road must refuse (base 2 bytes off a dword,
    odd row pitch), and the same calls through the pack pass and the output
    stage (AVIRHIP_UP2_NO_RAW, AVIRHIP_VARIANT_UP2_UNFUSED_IO)."""
    import torch
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    ran = 0
    for (sw, sh) in [(97, 61), (333, 40), (1001, 9), (50, 50), (642, 361)]:
        src = _src((sh, sw, 4), tin, seed=sw + 4)
        nw, nh = sw * 2, sh * 2
        want = _want_avir(src, nw, nh, F16, 16)
        r = avir_amd.CImageResizer(16)
        p = _plan(r, sw, sh, nw, nh, 4, tin, F16, abi.PATH_UP2)
        if p is None:
            continue
        ran += 1
        got = r.resize(src, nw, nh, out_dtype=F16)
        _same(got, want, "frame %r" % ((sw, sh),))
        out = np.zeros((nh, nw, 4), F16)
        for a_, b_ in [(0, nh // 3), (nh // 3, nh - 5), (nh - 5, nh)]:
            abi.check(lib.avirhip_resize_band(
                p, src.ctypes.data, abi.MEM_HOST, out[a_:b_].ctypes.data,
                abi.MEM_HOST, a_, b_, None), "band")
        _same(out, want, "bands %r" % ((sw, sh),))
        # the same bytes without the raw source, and without any fused I/O
        monkeypatch.setenv("AVIRHIP_UP2_NO_RAW", "1")
        g2 = r.resize(src, nw, nh, out_dtype=F16)
        monkeypatch.delenv("AVIRHIP_UP2_NO_RAW")
        assert g2.tobytes() == got.tobytes(), ("pack pass", sw, sh)
        abi.check(lib.avirhip_plan_set_variant(
            p, abi.VARIANT_UP2_UNFUSED_IO), "variant")
        g3 = r.resize(src, nw, nh, out_dtype=F16)
        abi.check(lib.avirhip_plan_set_variant(p, 0), "variant")
        assert g3.tobytes() == got.tobytes(), ("unfused", sw, sh)
        # device images: a destination 2 bytes off dword alignment (the fused
        # store refuses it), a half source likewise (the raw road refuses it)
        dsrc = _dev_bytes(src)
        dst = torch.zeros(want.nbytes + 8, dtype=torch.uint8, device="cuda:0")
        calls = [(dsrc.data_ptr(), 2)]
        if tin == F16:
            buf = torch.zeros(src.nbytes + 8, dtype=torch.uint8,
                              device="cuda:0")
            buf[2:2 + src.nbytes] = dsrc
            calls.append((buf.data_ptr() + 2, 0))
        for sp, do in calls:
            abi.check(lib.avirhip_resize_band(
                p, sp, abi.MEM_DEVICE, dst.data_ptr() + do, abi.MEM_DEVICE, 0,
                nh, None), "device")
            torch.cuda.synchronize()
            g4 = dst.cpu().numpy()[do:do + want.nbytes].view(F16)
            _same(g4, want, "unaligned %s %r" % (
                "destination" if do else "source", (sw, sh)))
        if tin != F16:
            continue
        # an odd row pitch in elements: rows alternate in dword alignment
        pitch = sw * 4 + 1
        p2 = r.plan(sw, sh, nw, nh, 4, 0.0, None, abi.F16, abi.F16, pitch)
        abi.check(lib.avirhip_plan_set_path(p2, abi.PATH_UP2), "path")
        flat = np.full(sh * pitch, np.nan, F16)
        flat.reshape(sh, pitch)[:, :sw * 4] = src.reshape(sh, sw * 4)
        dflat = _dev_bytes(flat)
        abi.check(lib.avirhip_resize_band(
            p2, dflat.data_ptr(), abi.MEM_DEVICE, dst.data_ptr(),
            abi.MEM_DEVICE, 0, nh, None), "odd pitch")
        torch.cuda.synchronize()
        _same(dst.cpu().numpy()[:want.nbytes].view(F16), want,
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


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("tin,tout", [(F16, F16), (F16, U8), (U8, F16),
                                      (F16, F32)],
                         ids=["f16-f16", "f16-u8", "u8-f16", "f16-f32"])
def test_every_family_converts_half_pixels(ch, tin, tout):
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    bits = 8 if np.dtype(tout) == np.dtype(U8) else 16
    ran = 0
    for (sw, sh, nw, nh), runs in FAMILIES:
        src = _src((sh, sw, ch), tin, seed=sw + ch)
        want = _want_avir(src, nw, nh, tout, bits)
        for path, variant in runs:
            r = avir_amd.CImageResizer(bits)
            if _plan(r, sw, sh, nw, nh, ch, tin, tout, path, variant) is None:
                continue
            got = _run(r, src, nw, nh, tout)
            if got is None:
                continue
            ran += 1
            _same(got, want, "%r path %d variant %d" % (
                (sw, sh, nw, nh), path, variant))
    # (26 runs in the table; narrow plans of small frames may refuse a path)
    assert ran >= 13, ran


# ---- CLancIR --------------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("tin,tout", [(F16, F16), (F16, U8), (U8, F16),
                                      (F16, F32)],
                         ids=["f16-f16", "f16-u8", "u8-f16", "f16-f32"])
def test_lancir_half_pixels(ch, tin, tout):
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    for (sw, sh, nw, nh) in [(160, 120, 320, 240), (192, 108, 250, 140),
                             (300, 240, 100, 80)]:
        src = _src((sh, sw, ch), tin, seed=sw + ch)
        want = _want_lancir(src, nw, nh, tout)
        for path, variant in [(0, 0), (1, 0), (4, 0), (5, 0),
                              (5, abi.VARIANT_UPG_FUSED)]:
            l = avir_amd.CLancIR()
            p = l.plan(sw, sh, nw, nh, ch, None, _T[np.dtype(tin)],
                       _T[np.dtype(tout)])
            rc = lib.avirhip_plan_set_path(p, path)
            if rc != 0:
                assert rc == abi.EUNSUPPORTED
                continue
            abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
            try:
                got = l.resize(src, nw, nh, out_dtype=tout)
            except abi.AvirHipError as e:
                assert "(%d)" % abi.EUNSUPPORTED in str(e), e
                continue
            _same(got, want, "lancir %r path %d variant %d" % (
                (sw, sh, nw, nh), path, variant))
        # NewSSize larger than the row: the padding survives the call
        npad = 6
        wantp = _want_lancir(src, nw, nh, tout, npad=npad)
        P = avir_amd.CLancIRParams(aNewSSize=nw * ch + npad)
        dst = np.full((nh, nw * ch + npad), 5, tout)
        l = avir_amd.CLancIR()
        assert l.resizeImage(src, sw, sh, dst, nw, nh, ch, P) == nh
        _same(dst[:, :nw * ch].reshape(nh, nw, ch), wantp, "NewSSize")
        assert (dst[:, nw * ch:] == 5).all()


# ---- gamma ----------------------------------------------------------------

@pytest.mark.parametrize("tout", [F16, U8], ids=["f16", "u8"])
@pytest.mark.parametrize("geom", [(96, 70, 192, 140), (300, 200, 460, 307),
                                  (600, 402, 200, 134)])
def test_gamma_half_source(tout, geom):
    """UseSRGBGamma: the half source is linearised as the float source is; the
    half result is the narrowed LINEAR float result (a float-type result is
    not de-linearised, avir.h:4956-4979), the uint8 result is de-linearised."""
    sw, sh, nw, nh = geom
    src = _src((sh, sw, 4), F16, seed=sw)
    bits = 8 if tout == U8 else 16
    want = _want_avir(src, nw, nh, tout, bits, gamma=True, alpha=3)
    v = avir_amd.CImageResizerVars()
    v.UseSRGBGamma, v.AlphaIndex = 1, 3
    got = avir_amd.CImageResizer(bits).resize(src, nw, nh, out_dtype=tout,
                                              aVars=v)
    _same(got, want, "gamma %r" % (geom,))


# ---- special values -------------------------------------------------------

@pytest.mark.parametrize("path", [4, 1])
def test_special_values(path):
    """+-0, half denormals, +-65504, +-Inf, NaN, and a block near 6e4 whose
    overshoot crosses 65504: Inf / NaN positions and all finite bits match."""
    sw, sh = 64, 48
    src = _src((sh, sw, 4), F16, seed=9)
    # (the lower half: values under 2^-14, half denormals in and out)
    src[24:] = (rb.lcg_f32((sh - 24, sw, 4), seed=5) * 6e-5).astype(F16)
    src[2, 3] = [0.0, -0.0, 0.0, -0.0]
    src[5, 7] = np.array([1, 0x3ff, 0x8001, 0x83ff], np.uint16).view(F16)
    src[9, 20] = [65504, -65504, 65504, -65504]
    src[14, 40] = [np.inf, 1.0, 1.0, 1.0]
    src[3, 11] = [1.0, -np.inf, 1.0, 1.0]
    src[12, 50] = [1.0, 1.0, np.nan, 1.0]
    src[6:14, 24:32] = 6e4
    nw, nh = sw * 2, sh * 2
    want = _want_avir(src, nw, nh, F16, 16)
    assert np.isinf(want).any() and np.isnan(want).any()
    den = (np.abs(want.astype(F32)) < 2.0 ** -14) & (want != 0)
    assert den.any()  # (half denormals among the results)
    r = avir_amd.CImageResizer(16)
    assert _plan(r, sw, sh, nw, nh, 4, F16, F16, path) is not None
    got = r.resize(src, nw, nh, out_dtype=F16)
    _same(got, want, "special values, path %d" % path)
    assert np.array_equal(np.isinf(got), np.isinf(want))
    assert np.array_equal(np.isnan(got), np.isnan(want))


# ---- windows ----------------------------------------------------------------

@pytest.mark.parametrize("geom,path", [((97, 130, 194, 260), 4),
                                       ((300, 200, 460, 307), 5)],
                         ids=["marching", "pass-kernels"])
def test_window_of_half_rows_between_nans(geom, path):
    """avirhip_resize_window from a device window of half rows whose
    surroundings are NaN halves (tests/test_gpu_window.py's manner)."""
    import torch
    sw, sh, nw, nh = geom
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    src = _src((sh, sw, 4), F16, seed=sw)
    want = _want_avir(src, nw, nh, F16, 16)
    r = avir_amd.CImageResizer(16)
    p = _plan(r, sw, sh, nw, nh, 4, F16, F16, path)
    assert p is not None
    r0, r1 = nh // 3, nh // 3 + 41
    a, b = C.c_int(), C.c_int()
    abi.check(lib.avirhip_band_source_rows(p, r0, r1, C.byref(a), C.byref(b)),
              "rows")
    n = b.value - a.value + 1
    G = 16
    big = np.full((n + 2 * G, sw, 4), np.nan, F16)
    big[G:G + n] = src[a.value:b.value + 1]
    dbig = _dev_bytes(big)
    dst = torch.zeros((r1 - r0) * nw * 4 * 2, dtype=torch.uint8,
                      device="cuda:0")
    abi.check(lib.avirhip_resize_window(
        p, dbig.data_ptr() + G * sw * 4 * 2, abi.MEM_DEVICE, a.value, n,
        dst.data_ptr(), abi.MEM_DEVICE, r0, r1, None), "window")
    torch.cuda.synchronize()
    _same(dst.cpu().numpy().view(F16), want[r0:r1], "window band")


# ---- torch ------------------------------------------------------------------

def test_torch_half_tensor_on_a_side_stream():
    import torch
    sw, sh = 160, 120
    src = _src((sh, sw, 4), F16, seed=3)
    want = _want_avir(src, 320, 240, F16, 16)
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        dsrc = torch.from_numpy(src).to("cuda:0", non_blocking=False)
        got = avir_amd.CImageResizer(16).resize(dsrc, 320, 240)
    st.synchronize()
    assert got.dtype == torch.float16 and got.is_cuda
    _same(got.cpu().numpy(), want, "torch half")
