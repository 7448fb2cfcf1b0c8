"""CLancIR exact 2x with half / bfloat16 RGBA images: k_lanc2h (lanc2h.hip),
one launch over the caller's own images.

Expected bits, as tests/test_gpu_half.py and tests/test_gpu_bf16.py define
them: the reference's CLancIR (tests/helpers.py, checker_lancir) on the exactly
widened float32 source, its float32 result narrowed with numpy's
.astype(float16), or with (u + 0x7fff + ((u >> 16) & 1)) >> 16 for bfloat16,
compared word for word; NaNs on both sides count as equal.

The calls are made on device-resident torch tensors through the pointer-level
ABI (bfloat16 host images are np.uint16 bit arrays: numpy has no bfloat16).

Shapes: 128 output columns per strip and 26 source rows per chunk at these
sizes (lanc2h_run's chunk rule), so (333, 140) is six strips and six chunks; (3, 200), (200, 2) and (1, 1) clamp every halo."""
import ctypes as C
import threading
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
MIB = 1 << 20

# every instantiated (SRC, OUT) pair: all but float -> float (k_lanc2's)
PAIRS = [("f16", "f16"), ("f16", "bf16"), ("f16", "f32"), ("bf16", "f16"),
         ("bf16", "bf16"), ("bf16", "f32"), ("f32", "f16"), ("f32", "bf16")]
SHAPES = [(333, 140), (97, 61), (1001, 9), (3, 200), (200, 2), (1, 1)]


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


def _src(shape, t, seed):
    if t == "u8":
        return rb.lcg_u8(shape, seed=seed)
    a = rb.lcg_f32(shape, seed=seed)
    return narrow(a) if t == "bf16" else a.astype(_T[t][1])


_REF = {}


def _case(sw, sh, tin):
    """(source, the reference's float32 result): computed once per source
    type and shape, shared by every test, never written to."""
    key = (sw, sh, tin)
    if key not in _REF:
        src = _src((sh, sw, 4), tin, seed=sw + sh)
        ref = H.checker_lancir(_as_f32(src, tin), 2 * sw, 2 * sh,
                               out_dtype=np.float32)
        src.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (src, ref)
    return _REF[key]


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


def _lib():
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    return lib


def _plan(l, sw, sh, tin, tout, path, variant=0, P=None):
    """The plan of the exact-2x call on `path` (0: automatic). A forced path
    that cannot run the plan FAILS here."""
    lib = abi.load()
    p = l.plan(sw, sh, 2 * sw, 2 * sh, 4, P, _T[tin][0], _T[tout][0])
    abi.check(lib.avirhip_plan_set_path(p, path), "path %d" % path)
    abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
    return p


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
    return t.cpu().numpy().view(_T[tout][1]).reshape(shape)


def _bands(nh):
    """The thirds of tests/test_gpu_half.py, and one band with odd row0 and
    row1 inside a chunk (52 output rows) where the frame has one."""
    cuts = sorted({0, nh // 3, max(nh - 5, nh // 3), nh})
    bands = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    odd = (7, 29) if nh >= 30 else ((1, 3) if nh >= 4 else None)
    return bands, odd


def _frame_and_bands(lib, p, dsrc, want, tout, what):
    """Whole frame; the bands into one image; the odd band on its own."""
    import torch
    nh, nw = want.shape[:2]
    es = want.dtype.itemsize
    rb_ = nw * 4 * es
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    _call(lib, p, dsrc.data_ptr(), d.data_ptr(), 0, nh, what=what)
    _same(_host(d, tout, want.shape), want, tout, what + " frame")
    bands, odd = _bands(nh)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    for a, b in bands:
        _call(lib, p, dsrc.data_ptr(), d.data_ptr() + a * rb_, a, b, what=what)
    _same(_host(d, tout, want.shape), want, tout, what + " bands")
    if odd is not None:
        a, b = odd
        d = torch.zeros((b - a) * rb_, dtype=torch.uint8, device="cuda:0")
        _call(lib, p, dsrc.data_ptr(), d.data_ptr(), a, b, what=what)
        _same(_host(d, tout, want[a:b].shape), want[a:b], tout,
              what + " odd band")


# ---- 1. every pair ----------------------------------------------------------

@pytest.mark.parametrize("path", [0, 4], ids=["auto", "path4"])
@pytest.mark.parametrize("tin,tout", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_every_pair(tin, tout, path):
    lib = _lib()
    for sw, sh in SHAPES:
        src, ref = _case(sw, sh, tin)
        want = _from_f32(ref, tout)
        l = avir_amd.CLancIR()
        p = _plan(l, sw, sh, tin, tout, path)
        _frame_and_bands(lib, p, _dev(src), want, tout,
                         "%s->%s %r path %d" % (tin, tout, (sw, sh), path))
        # one launch over the caller's images: no float copy of either
        assert lib.avirhip_plan_device_bytes(p) < 2 * MIB


@pytest.mark.parametrize("path", [0, 4], ids=["auto", "path4"])
@pytest.mark.parametrize("tin,tout", [("f16", "f16"), ("bf16", "bf16"),
                                      ("f32", "f16"), ("f16", "f32")],
                         ids=["f16-f16", "bf16-bf16", "f32-f16", "f16-f32"])
def test_one_launch_no_float_copies(tin, tout, path):
    """640x360 -> 1280x720, device-resident: the plan holds neither the float
    copy of the source (3.7 MB) nor the float result (14.7 MB)."""
    import torch
    lib = _lib()
    sw, sh = 640, 360
    src, ref = _case(sw, sh, tin)
    want = _from_f32(ref, tout)
    l = avir_amd.CLancIR()
    p = _plan(l, sw, sh, tin, tout, path)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    dsrc = _dev(src)
    _call(lib, p, dsrc.data_ptr(), d.data_ptr(), 0, 2 * sh)
    _same(_host(d, tout, want.shape), want, tout,
          "%s->%s 640x360 path %d" % (tin, tout, path))
    held = lib.avirhip_plan_device_bytes(p)
    print("plan holds %d bytes" % held)
    assert held < 2 * MIB < sw * sh * 16


@pytest.mark.parametrize("path", [0, 4], ids=["auto", "path4"])
@pytest.mark.parametrize("tout", ["f16", "bf16"])
def test_uint8_source_behind_the_pack_pass(tout, path):
    """uint8 RGBA -> half / bfloat16: the kernel reads the pack pass's float
    copy and applies the plan's gain (1 / 255) in front of the narrowing."""
    lib = _lib()
    for sw, sh in [(333, 140), (97, 61)]:
        src, ref = _case(sw, sh, "u8")
        assert ref.max() <= 1.5  # (the gain is in the expected values)
        want = _from_f32(ref, tout)
        l = avir_amd.CLancIR()
        p = _plan(l, sw, sh, "u8", tout, path)
        _frame_and_bands(lib, p, _dev(src), want, tout,
                         "u8->%s %r path %d" % (tout, (sw, sh), path))
        # (the float copy of the source, no float result)
        assert lib.avirhip_plan_device_bytes(p) < sw * sh * 16 + 2 * MIB


# ---- 2. refusals ------------------------------------------------------------

@pytest.mark.parametrize("path", [0, 4], ids=["auto", "path4"])
@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_refused_images_take_the_general_road(t, path):
    """lanc2h_image_ok wants naturally aligned pixels: a base 2 bytes off and
    a row pitch that is no multiple of 4 elements are refused -- the same bits
    through the float copy / the float result, rc == 0, the destination's
    padding untouched. A pitch of whole pixels is admitted: no float copies."""
    import torch
    lib = _lib()
    pad_s = np.array([NAN], np.uint16).view(_T[t][1])[0] if t == "bf16" \
        else np.float16(np.nan)
    for sw, sh in [(97, 61), (333, 140)]:
        nw, nh = 2 * sw, 2 * sh
        src, ref = _case(sw, sh, t)
        want = _from_f32(ref, t)
        dsrc = _dev(src)
        # source base 2 bytes off
        l = avir_amd.CLancIR()
        p = _plan(l, sw, sh, t, t, path)
        off = _dev(src, off=2, tail=6)
        d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
        _call(lib, p, off.data_ptr() + 2, d.data_ptr(), 0, nh, what="src + 2")
        _same(_host(d, t, want.shape), want, t, "source base 2 bytes off")
        # destination base 2 bytes off
        d = torch.zeros(want.nbytes + 8, dtype=torch.uint8, device="cuda:0")
        _call(lib, p, dsrc.data_ptr(), d.data_ptr() + 2, 0, nh, what="dst + 2")
        g = _host(d, "u8", (want.nbytes + 8,))
        _same(g[2:2 + want.nbytes].view(_T[t][1]), want, t,
              "destination base 2 bytes off")
        assert (g[:2] == 0).all() and (g[2 + want.nbytes:] == 0).all()
        # odd source pitch, the padding elements NaN
        pitch = sw * 4 + 1
        flat = np.full((sh, pitch), pad_s, _T[t][1])
        flat[:, :sw * 4] = src.reshape(sh, sw * 4)
        l2 = avir_amd.CLancIR()
        p2 = _plan(l2, sw, sh, t, t, path,
                   P=avir_amd.CLancIRParams(aSrcSSize=pitch))
        dflat = _dev(flat)
        d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
        _call(lib, p2, dflat.data_ptr(), d.data_ptr(), 0, nh, what="odd pitch")
        _same(_host(d, t, want.shape), want, t, "odd source pitch")
        # NewSSize with padding: 6 elements (refused), 8 (whole pixels: admitted)
        for npad in (6, 8):
            np_ = nw * 4 + npad
            l3 = avir_amd.CLancIR()
            p3 = _plan(l3, sw, sh, t, t, path,
                       P=avir_amd.CLancIRParams(aNewSSize=np_))
            fill = np.full((nh, np_), 5, np.uint16)
            d = _dev(fill)
            _call(lib, p3, dsrc.data_ptr(), d.data_ptr(), 0, nh,
                  what="NewSSize + %d" % npad)
            g = _host(d, "bf16", (nh, np_))
            _same(np.ascontiguousarray(g[:, :nw * 4]).view(_T[t][1]),
                  want.reshape(nh, nw * 4), t, "NewSSize + %d" % npad)
            assert (g[:, nw * 4:] == 5).all(), "padding written"
            if npad == 8:
                assert lib.avirhip_plan_device_bytes(p3) < 2 * MIB


# ---- 3. the three roads -------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_three_roads_agree(t):
    """Fused (one launch), AVIRHIP_VARIANT_UP2_UNFUSED_IO (pack pass, k_lanc2,
    output stage) and forced path 1 (the generic kernels): the same bytes."""
    import torch
    lib = _lib()
    for sw, sh in [(333, 140), (97, 61)]:
        src, ref = _case(sw, sh, t)
        want = _from_f32(ref, t)
        dsrc = _dev(src)
        got = []
        for path, variant in [(4, 0), (4, abi.VARIANT_UP2_UNFUSED_IO),
                              (0, abi.VARIANT_UP2_UNFUSED_IO), (1, 0)]:
            l = avir_amd.CLancIR()
            p = _plan(l, sw, sh, t, t, path, variant)
            d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
            _call(lib, p, dsrc.data_ptr(), d.data_ptr(), 0, 2 * sh)
            got.append(_host(d, t, want.shape))
            held = lib.avirhip_plan_device_bytes(p)
            # (the variant took effect: the plan holds the float copy of the
            # source and the float result, which the fused road never makes)
            if variant:
                assert held >= sw * sh * 16 + 4 * sw * sh * 16, (path, held)
            elif path == 4:
                assert held < 2 * MIB, held
        _same(got[0], want, t, "fused %r" % ((sw, sh),))
        for g in got[1:]:
            assert g.tobytes() == got[0].tobytes(), (sw, sh)


# ---- 4. special values --------------------------------------------------------

def _special_f16_source(sw, sh):
    """tests/test_gpu_half.py::test_special_values' pattern."""
    src = _src((sh, sw, 4), "f16", seed=9)
    # (the lower half: values under 2^-14, half denormals in and out)
    src[24:] = (rb.lcg_f32((sh - 24, sw, 4), seed=5) * 6e-5).astype(np.float16)
    src[2, 3] = [0.0, -0.0, 0.0, -0.0]
    src[5, 7] = np.array([1, 0x3ff, 0x8001, 0x83ff], np.uint16).view(np.float16)
    src[9, 20] = [65504, -65504, 65504, -65504]
    src[14, 40] = [np.inf, 1.0, 1.0, 1.0]
    src[3, 11] = [1.0, -np.inf, 1.0, 1.0]
    src[12, 50] = [1.0, 1.0, np.nan, 1.0]
    src[6:14, 24:32] = 6e4
    return src


def special_f16_case():
    sw, sh = 64, 48
    src = _special_f16_source(sw, sh)
    ref = H.checker_lancir(src.astype(np.float32), 2 * sw, 2 * sh,
                           out_dtype=np.float32)
    want = _from_f32(ref, "f16")
    # a weak input fails here: Inf (the source's, and finite float32 results
    # beyond 65504: the 6e4 block's overshoot), NaN, half denormals
    assert np.isinf(want).any() and np.isnan(want).any()
    assert (np.isfinite(ref) & np.isinf(want)).any()
    assert ((np.abs(want.astype(np.float32)) < 2.0 ** -14) & (want != 0)).any()
    return src, want


def _special_f32_source(sw, sh):
    """float32 pixels whose CLancIR results land on float32 denormals, on NaN
    and +-Inf, and -- blocks of +-2.8e38 .. 3.2e38 whose overshoot partly stays
    finite in float32 -- on finite values from 0x7f7f8000 (3.396e38, the bfloat16
    halfway point above the largest finite value) upwards."""
    src = rb.lcg_f32((sh, sw, 4), seed=9)
    src[32:] = rb.lcg_f32((sh - 32, sw, 4), seed=5) * np.float32(1.1e-38)
    blk = np.float32(3.2e38) * (1 - np.float32(0.12) *
                                rb.lcg_f32((12, 16, 4), seed=4))
    src[4:16, 4:20] = blk
    src[4:16, 26:42] = -blk
    src[18:30, 4:20] = -blk
    src[40, 58] = [np.nan, 1.0, 1.0, 1.0]
    src[44, 6] = [1.0, np.inf, -np.inf, 1.0]
    return src


def special_bf16_case():
    sw, sh = 64, 48
    src = _special_f32_source(sw, sh)
    ref = H.checker_lancir(src, 2 * sw, 2 * sh, out_dtype=np.float32)
    want = narrow(ref)
    wf = widen(want)
    fin = np.isfinite(ref)
    up = int((fin & (wf == np.inf)).sum())
    dn = int((fin & (wf == -np.inf)).sum())
    print("finite results narrowed to +Inf: %d, to -Inf: %d" % (up, dn))
    assert up >= 3 and dn >= 3  # (5 and 10 with the reference)
    assert np.isnan(ref).any() and np.isinf(ref).any()
    assert ((wf != 0) & (np.abs(wf) < 2.0 ** -126)).any()  # denormal results
    return src, want


@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_special_values(t):
    """Half: +-0, denormals, +-65504, +-Inf, NaN and a 6e4 block whose
    overshoot crosses 65504, read and stored by k_lanc2h< F16, F16 >.
    bfloat16: k_lanc2h< F32, BF16 >'s own store narrows finite float32 results
    from 0x7f7f8000 upwards to +-Inf, keeps denormals, NaN and Inf."""
    import torch
    lib = _lib()
    src, want = special_f16_case() if t == "f16" else special_bf16_case()
    tin = "f16" if t == "f16" else "f32"
    sh, sw = src.shape[:2]
    l = avir_amd.CLancIR()
    p = _plan(l, sw, sh, tin, t, 4)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    dsrc = _dev(src)
    _call(lib, p, dsrc.data_ptr(), d.data_ptr(), 0, 2 * sh)
    got = _host(d, t, want.shape)
    _same(got, want, t, "special values, %s" % t)
    gf, wf = _as_f32(got, t), _as_f32(want, t)
    assert np.array_equal(np.isinf(gf), np.isinf(wf))
    assert np.array_equal(np.isnan(gf), np.isnan(wf))
    assert lib.avirhip_plan_device_bytes(p) < 2 * MIB  # (the fused kernel ran)


# ---- 5. far rows --------------------------------------------------------------

@pytest.mark.parametrize("side", ["source", "destination"])
def test_rows_beyond_4_gib(side):
    """A 64 x 40 half RGBA frame whose last source row (SrcSSize), or whose last
    destination row (NewSSize), starts more than 4 GiB from the base: 64-bit
    row addresses. Only the rows themselves are written and read; compared
    with the packed frame's result (and that with the reference)."""
    import torch
    lib = _lib()
    sw, sh = 64, 40
    nw, nh = 2 * sw, 2 * sh
    src, ref = _case(sw, sh, "f16")
    want = _from_f32(ref, "f16")
    l = avir_amd.CLancIR()
    p = _plan(l, sw, sh, "f16", "f16", 4)
    dsrc = _dev(src)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    _call(lib, p, dsrc.data_ptr(), d.data_ptr(), 0, nh)
    packed = _host(d, "f16", want.shape)
    _same(packed, want, "f16", "packed frame")
    # (row pitches in elements: whole pixels, the last row past 2^32 bytes)
    rows, row_el = (sh, sw * 4) if side == "source" else (nh, nw * 4)
    pitch = (-(-(1 << 32) // (2 * (rows - 1))) + 4) & ~3
    assert (rows - 1) * pitch * 2 > (1 << 32)
    big = torch.empty((rows - 1) * pitch + row_el, dtype=torch.float16,
                      device="cuda:0")
    view = big.as_strided((rows, row_el), (pitch, 1))
    if side == "source":
        view.copy_(torch.from_numpy(src.reshape(sh, sw * 4).copy()))
        P = avir_amd.CLancIRParams(aSrcSSize=pitch)
    else:
        view.zero_()
        P = avir_amd.CLancIRParams(aNewSSize=pitch)
    l2 = avir_amd.CLancIR()
    p2 = _plan(l2, sw, sh, "f16", "f16", 4, P=P)
    if side == "source":
        d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
        _call(lib, p2, big.data_ptr(), d.data_ptr(), 0, nh, what="far source")
        got = _host(d, "f16", want.shape)
    else:
        _call(lib, p2, dsrc.data_ptr(), big.data_ptr(), 0, nh,
              what="far destination")
        torch.cuda.synchronize()
        got = view.cpu().numpy().reshape(want.shape)
    assert lib.avirhip_plan_device_bytes(p2) < 2 * MIB
    assert got.tobytes() == packed.tobytes(), "far %s rows" % side


# ---- 6. threads ---------------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_four_threads_one_plan(t):
    """Four threads run fused whole-frame and band calls of ONE plan at once,
    each on its own stream into its own images."""
    import torch
    lib = _lib()
    sw, sh = 333, 140
    nw, nh = 2 * sw, 2 * sh
    src, ref = _case(sw, sh, t)
    want = _from_f32(ref, t)
    l = avir_amd.CLancIR()
    p = _plan(l, sw, sh, t, t, 0)
    dsrc = _dev(src)
    rb_ = nw * 4 * 2
    bands, odd = _bands(nh)
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
        _same(_host(out[i][0], t, want.shape), want, t, "thread %d frame" % i)
        _same(_host(out[i][1], t, want.shape), want, t, "thread %d bands" % i)
    # (spares of the plan, none with a float copy)
    assert lib.avirhip_plan_device_bytes(p) < 2 * MIB
