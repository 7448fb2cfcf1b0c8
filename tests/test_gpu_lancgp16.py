"""CLancIR at general ratios (path 5) with half / bfloat16 images: k_lf's and
k_gv's raw loaders read a 16-bit float source where it lies (kinds 4 / 5), and
the last pass (k_lf, k_gh) narrows and stores a 16-bit float result itself
(gp_store_lancir_row< 3 >) -- no float copy of either image on the plan.

Expected bits and inputs: tests/lancgp16_cases.py (the reference's CLancIR on
the exactly widened float32 source, its float32 result narrowed by numpy / by
the header's integer formula, integer results the reference's own; word for
word, NaN equal to NaN). The calls are made on device-resident torch tensors
through avirhip_resize_band."""
import threading
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import lancgp16_cases as G
from tests.gpass_route_cases import environment

pytestmark = pytest.mark.gpu

T = G.T
P5 = G.P5
MIB = G.MIB
NO_IO16 = {"AVIRHIP_GP_NO_IO16": "1"}


def _lib():
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    return lib


def _plan(geom, tin, tout, path=0, variant=0, ch=4, P=None):
    """(CLancIR object, plan) of the call on `path` (0: automatic). A forced
    path that cannot run the plan FAILS here."""
    lib = abi.load()
    sw, sh, nw, nh = geom
    l = avir_amd.CLancIR()
    p = l.plan(sw, sh, nw, nh, ch, P, T[tin][0], T[tout][0])
    abi.check(lib.avirhip_plan_set_path(p, path), "path %d" % path)
    abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
    return l, p


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


def _frame(lib, p, sptr, want, tout, what, off=0, pitch=0):
    """The whole frame into an image of 0x5a bytes `off` bytes into its
    allocation, with a guard row behind it (`pitch`: elements per row, the
    padding must survive too). -> the image's pixels."""
    import torch
    nh, nw, ch = want.shape
    es = want.dtype.itemsize
    pe = pitch if pitch else nw * ch
    nbytes = ((nh - 1) * pe + nw * ch) * es
    guard = pe * es
    d = torch.full((off + nbytes + guard,), 0x5a, dtype=torch.uint8,
                   device="cuda:0")
    _call(lib, p, sptr, d.data_ptr() + off, 0, nh, what=what)
    g = _host(d, "u8", (off + nbytes + guard,))
    assert (g[:off] == 0x5a).all() and (g[off + nbytes:] == 0x5a).all(), \
        what + ": stored outside the image"
    img = np.full(nh * pe * es, 0x5a, np.uint8)
    img[:nbytes] = g[off:off + nbytes]
    rows = img.reshape(nh, pe * es)
    assert (rows[:, nw * ch * es:] == 0x5a).all(), what + ": row padding"
    got = np.ascontiguousarray(rows[:, :nw * ch * es]).view(
        T[tout][1]).reshape(want.shape)
    G.same(got, want, tout, what)
    return got


def _frame_and_bands(lib, p, dsrc, want, tout, what, soff=0):
    """Whole frame (guard row behind it); thirds into one image; the odd band
    on its own."""
    import torch
    nh, nw, ch = want.shape
    rb_ = nw * ch * want.dtype.itemsize
    sp = dsrc.data_ptr() + soff
    _frame(lib, p, sp, want, tout, what + " frame")
    bands, odd = G.bands(nh)
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    for a, b in bands:
        _call(lib, p, sp, d.data_ptr() + a * rb_, a, b, what=what)
    G.same(_host(d, tout, want.shape), want, tout, what + " bands")
    if odd is not None:
        a, b = odd
        d = torch.zeros((b - a) * rb_, dtype=torch.uint8, device="cuda:0")
        _call(lib, p, sp, d.data_ptr(), a, b, what=what)
        G.same(_host(d, tout, want[a:b].shape), want[a:b], tout,
               what + " odd band")


def _held(lib, p):
    import torch
    torch.cuda.synchronize()
    return int(lib.avirhip_plan_device_bytes(p))


_FLOAT_BYTES = {}


def _float_plan_bytes(lib, geom, path, variant):
    """Device bytes of the float32 -> float32 RGBA plan of the same geometry,
    path and variant after a whole-frame call: float RGBA is the kernels' own
    format, that plan holds `mid` at most."""
    import torch
    key = (geom, path, variant)
    if key not in _FLOAT_BYTES:
        src, want = G.case(geom, "f32", "f32")
        l, p0 = _plan(geom, "f32", "f32", path, variant)
        d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
        dsrc = _dev(src)
        _call(lib, p0, dsrc.data_ptr(), d.data_ptr(), 0, geom[3], what="float")
        _FLOAT_BYTES[key] = _held(lib, p0)
    return _FLOAT_BYTES[key]


def _copies(geom):
    """Bytes of the float copy of the source (`packed`) and of the float
    result (`lres`)."""
    sw, sh, nw, nh = geom
    return sw * sh * 16, nw * nh * 16


# ---- 1. every pair ------------------------------------------------------------

@pytest.mark.parametrize("tin,tout", G.PAIRS,
                         ids=["%s-%s" % pr for pr in G.PAIRS])
def test_every_pair(tin, tout):
    lib = _lib()
    for geom in G.SHAPES:
        src, want = G.case(geom, tin, tout)
        dsrc = _dev(src)
        for path, variant in G.roads(geom):
            l, p = _plan(geom, tin, tout, path, variant)
            what = "%s->%s %r path %d variant %d" % (tin, tout, geom, path,
                                                     variant)
            _frame_and_bands(lib, p, dsrc, want, tout, what)


# ---- 2. channels ----------------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_channels(t, ch):
    lib = _lib()
    for geom in G.CH_SHAPES:
        src, want = G.case(geom, t, t, ch)
        dsrc = _dev(src)
        for path, variant in [(0, 0), (P5, 0), (P5, G.V_UPG2)]:
            l, p = _plan(geom, t, t, path, variant, ch=ch)
            what = "%s x%d %r path %d variant %d" % (t, ch, geom, path, variant)
            _frame_and_bands(lib, p, dsrc, want, t, what)
        # width * channels * 2 bytes is a multiple of 4 at these shapes: read
        # and stored where they lie
        pk, lr = _copies(geom)
        assert _held(lib, p) < _float_plan_bytes(lib, geom, P5, G.V_UPG2) + \
            min(pk, lr), (geom, ch)


# ---- 3. chunk seams -------------------------------------------------------------

@pytest.mark.parametrize("chunk", G.LF_CHUNKS)
@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_chunk_seams_of_the_fused_kernel(t, chunk):
    lib = _lib()
    src, want = G.case(G.UP, t, t)
    l, p = _plan(G.UP, t, t, P5, G.V_UPGF)
    with environment({"AVIRHIP_LF_CHUNK": str(chunk)}):
        _frame_and_bands(lib, p, _dev(src), want, t,
                         "k_lf %s chunk %d" % (t, chunk))


@pytest.mark.parametrize("chunk", G.GV_CHUNKS)
@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_chunk_seams_of_the_vertical_pass(t, chunk):
    lib = _lib()
    for geom, variant in ((G.DN18, 0), (G.UP, G.V_UPG2)):
        src, want = G.case(geom, t, t)
        l, p = _plan(geom, t, t, P5, variant)
        with environment({"AVIRHIP_GV_CHUNK": str(chunk)}):
            _frame_and_bands(lib, p, _dev(src), want, t,
                             "k_gv %s %r chunk %d" % (t, geom, chunk))


# ---- 4. held memory -------------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_no_float_copies_on_the_plan(t):
    """k_lf: the plan holds nothing frame-sized. The two pass kernels: `mid`
    only, what the float32 -> float32 RGBA plan holds."""
    lib = _lib()
    src, want = G.case(G.HELD_UP, t, t)
    dsrc = _dev(src)
    for path in (0, P5):
        l, p = _plan(G.HELD_UP, t, t, path)
        _frame(lib, p, dsrc.data_ptr(), want, t, "k_lf %s path %d" % (t, path))
        held = _held(lib, p)
        print("k_lf %s path %d: %d bytes (packed %d, lres %d)" %
              ((t, path, held) + _copies(G.HELD_UP)))
        assert held < 2 * MIB
    for geom, variant in ((G.HELD_UP, G.V_UPG2), (G.HELD_DN, 0)):
        src, want = G.case(geom, t, t)
        dsrc = _dev(src)
        l, p = _plan(geom, t, t, P5, variant)
        _frame(lib, p, dsrc.data_ptr(), want, t, "two passes %s %r" % (t, geom))
        held = _held(lib, p)
        fl = _float_plan_bytes(lib, geom, P5, variant)
        print("two passes %s %r: %d bytes, the float plan %d" %
              (t, geom, held, fl))
        assert held <= fl + MIB


# ---- 5. the roads agree ---------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_roads_agree(t):
    """The fused call; AVIRHIP_VARIANT_UP2_UNFUSED_IO; AVIRHIP_GP_NO_IO16: the
    same words, and under either switch the plan holds the float copies."""
    lib = _lib()
    for geom, variant in ((G.UP, 0), (G.UP, G.V_UPG2), (G.DN18, 0),
                          (G.MIXED, 0)):
        for ch in (4, 3) if geom != G.UP else (4,):
            src, want = G.case(geom, t, t, ch)
            dsrc = _dev(src)
            pk, lr = _copies(geom)
            what = "%s %r x%d variant %d" % (t, geom, ch, variant)
            l, p = _plan(geom, t, t, P5, variant, ch=ch)
            got = _frame(lib, p, dsrc.data_ptr(), want, t, what)
            if ch == 4:
                assert _sides(lib, p, geom, variant) == (False, False), what
            l2, p2 = _plan(geom, t, t, P5, variant | G.V_UNFUSED, ch=ch)
            g = _frame(lib, p2, dsrc.data_ptr(), want, t, what + " unfused")
            assert g.tobytes() == got.tobytes(), what
            assert _held(lib, p2) >= pk + lr, what
            with environment(NO_IO16):
                l3, p3 = _plan(geom, t, t, P5, variant, ch=ch)
                g = _frame(lib, p3, dsrc.data_ptr(), want, t,
                           what + " no io16")
                assert g.tobytes() == got.tobytes(), what
                assert _held(lib, p3) >= pk + lr, what


# ---- 6. refusals ----------------------------------------------------------------

def _sides(lib, p, geom, variant):
    """-> (the plan holds the float copy of the source, the float result), by
    its bytes over the float plan's (`mid` and tables: the same on both)."""
    pk, lr = _copies(geom)
    over = _held(lib, p) - _float_plan_bytes(lib, geom, P5, variant)
    slack = min(pk, lr) // 2
    for s_, d_ in ((0, 0), (1, 0), (0, 1), (1, 1)):
        if abs(over - (s_ * pk + d_ * lr)) <= slack:
            return bool(s_), bool(d_)
    raise AssertionError("%r: %d bytes over the float plan (packed %d, lres "
                         "%d)" % (geom, over, pk, lr))


@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_refused_sources_take_the_pack_pass(t):
    """The source is refused, the fused store still runs: the plan holds the
    float copy of the source and no float result; the same bits."""
    lib = _lib()
    # a base 2 bytes into a dword
    src, want = G.case(G.UP, t, t)
    for variant in (0, G.V_UPG2):
        l, p = _plan(G.UP, t, t, P5, variant)
        d = _dev(src, off=2, tail=6)
        _frame_and_bands(lib, p, d, want, t, "%s base 2 mod 4" % t, soff=2)
        assert _sides(lib, p, G.UP, variant) == (True, False), variant
    # RGB of odd width: a pitch of 582 bytes
    src, want = G.case(G.UP, t, t, 3)
    l, p = _plan(G.UP, t, t, P5, ch=3)
    _frame_and_bands(lib, p, _dev(src), want, t, "%s RGB pitch 582" % t)
    assert _sides(lib, p, G.UP, 0) == (True, False)
    # an explicit odd SrcSSize
    src, want = G.case(G.UP, t, t)
    pitch = G.UP[0] * 4 + 1
    P = avir_amd.CLancIRParams(aSrcSSize=pitch)
    l, p = _plan(G.UP, t, t, P5, P=P)
    _frame_and_bands(lib, p, _dev(G.padded(src, pitch, t)), want, t,
                     "%s odd SrcSSize" % t)
    assert _sides(lib, p, G.UP, 0) == (True, False)
    # ... and an even one, read where it lies
    pitch = G.UP[0] * 4 + 6
    P = avir_amd.CLancIRParams(aSrcSSize=pitch)
    l, p = _plan(G.UP, t, t, P5, P=P)
    _frame_and_bands(lib, p, _dev(G.padded(src, pitch, t)), want, t,
                     "%s SrcSSize + 6" % t)
    assert _sides(lib, p, G.UP, 0) == (False, False)
    # 40 source columns; 28 vertical taps
    for geom in (G.NARROW, G.TALL):
        src, want = G.case(geom, t, t)
        l, p = _plan(geom, t, t, P5)
        _frame_and_bands(lib, p, _dev(src), want, t, "%s %r" % (t, geom))
        assert _sides(lib, p, geom, 0) == (True, False), geom


@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_refused_destinations_take_the_output_stage(t):
    """A destination at an odd byte offset: elements are stored whole, so the
    call goes through the float result and the output stage (rc == 0, the same
    bits), while the source is still read where it lies. An RGBA destination
    2 bytes into 8, or with NewSSize no multiple of 4, is stored by the last
    pass."""
    lib = _lib()
    src, want = G.case(G.UP, t, t)
    dsrc = _dev(src)
    for variant in (0, G.V_UPG2):
        l, p = _plan(G.UP, t, t, P5, variant)
        _frame(lib, p, dsrc.data_ptr(), want, t, "%s odd destination" % t,
               off=1)
        assert _sides(lib, p, G.UP, variant) == (False, True), variant
        for off in (2, 6):
            l, p = _plan(G.UP, t, t, P5, variant)
            _frame(lib, p, dsrc.data_ptr(), want, t,
                   "%s destination %d mod 8" % (t, off), off=off)
            assert _sides(lib, p, G.UP, variant) == (False, False)
        for extra in (1, 2, 3):
            pitch = G.UP[2] * 4 + extra
            P = avir_amd.CLancIRParams(aNewSSize=pitch)
            l, p = _plan(G.UP, t, t, P5, variant, P=P)
            _frame(lib, p, dsrc.data_ptr(), want, t,
                   "%s NewSSize + %d" % (t, extra), pitch=pitch)
            assert _sides(lib, p, G.UP, variant) == (False, False)


# ---- 7. special values ----------------------------------------------------------

@pytest.mark.parametrize("geom", [G.SPECIAL_UP, G.SPECIAL_DN],
                         ids=["up", "down"])
@pytest.mark.parametrize("tin,tout", [("f16", "f16"), ("bf16", "bf16"),
                                      ("f16", "bf16"), ("bf16", "f16"),
                                      ("bf16", "u8")])
def test_special_values(tin, tout, geom):
    lib = _lib()
    src, ref, want = G.special_case(tin, tout, geom)
    if tout in G.H16:
        c = G.special_classes(tout, ref, want)
        print(tin, tout, geom, c)
        assert c["pos_inf"] > 0 and c["neg_inf"] > 0 and c["nan"] > 0
        # (a half source has nothing that small: bfloat16's denormals are
        # float32's)
        assert c["denormal"] > 0 or (tin, tout) == ("f16", "bf16")
    dsrc = _dev(src)
    for path, variant in [(0, 0), (P5, 0)] + (
            [(P5, G.V_UPG2)] if geom == G.SPECIAL_UP else []):
        l, p = _plan(geom, tin, tout, path, variant)
        got = _frame(lib, p, dsrc.data_ptr(), want, tout,
                     "special %s->%s %r path %d variant %d" %
                     (tin, tout, geom, path, variant))
        if tout in G.H16:
            gf, wf = G.as_f32(got, tout), G.as_f32(want, tout)
            assert np.array_equal(np.isinf(gf), np.isinf(wf))
            assert np.array_equal(np.isnan(gf), np.isnan(wf))
            assert np.array_equal(np.signbit(gf) & (gf == 0),
                                  np.signbit(wf) & (wf == 0))


# ---- 8. gain and clamp ----------------------------------------------------------

@pytest.mark.parametrize("tin,tout,ch", [("f16", "u8", 4), ("u16", "bf16", 4),
                                         ("bf16", "u8", 3), ("u16", "f16", 3)])
def test_gain_and_clamp(tin, tout, ch):
    """Non-unity plans: out_mul in the 16-bit float store, the integer rule
    (clamp, nearest-even, the + 0.5 tail of a scanline whose length is no
    multiple of 4) behind a 16-bit float source."""
    lib = _lib()
    for geom in (G.DN18, G.UP):
        src, want = G.case(geom, tin, tout, ch)
        dsrc = _dev(src)
        for path, variant in G.roads(geom):
            l, p = _plan(geom, tin, tout, path, variant, ch=ch)
            _frame_and_bands(lib, p, dsrc, want, tout,
                             "%s->%s x%d %r path %d variant %d" %
                             (tin, tout, ch, geom, path, variant))


# ---- 9. threads -----------------------------------------------------------------

def test_four_threads_one_plan():
    """Four threads run whole-frame and band calls of ONE plan at once, each
    on its own stream into its own images."""
    import torch
    lib = _lib()
    t = "f16"
    sw, sh, nw, nh = G.UP
    src, want = G.case(G.UP, t, t)
    l, p = _plan(G.UP, t, t, P5)
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
    assert _held(lib, p) < 2 * MIB


# ---- 10. the Python front end ---------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_python_front_end_torch(t):
    import torch
    src, want = G.case(G.UP, t, t)
    if t == "f16":
        x = torch.from_numpy(src.copy()).to("cuda:0")
    else:
        x = torch.from_numpy(src.copy().view(np.int16)).to("cuda:0").view(
            torch.bfloat16)
    assert x.dtype == (torch.float16 if t == "f16" else torch.bfloat16)
    got = avir_amd.CLancIR().resize(x, G.UP[2], G.UP[3])
    torch.cuda.synchronize()
    assert got.dtype == x.dtype and tuple(got.shape) == want.shape
    g = got.view(torch.int16).cpu().numpy().view(T[t][1])
    G.same(g, want, t, "CLancIR.resize torch %s" % t)


def test_python_front_end_numpy():
    src, want = G.case(G.DN18, "f16", "f16", 3)
    got = avir_amd.CLancIR().resize(src.copy(), G.DN18[2], G.DN18[3])
    assert got.dtype == np.float16
    G.same(got, want, "f16", "CLancIR.resize numpy float16 RGB")
