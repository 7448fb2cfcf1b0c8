"""avirhip_resize_window (include/avirhip.h): a band computed from the source
rows it reads and nothing else is bit-identical to the same rows of a whole
resize -- on every kernel family, from device and host windows whose
surroundings are poison; refusals leave the destination alone; window calls
and lock-free whole-frame calls share a plan across threads; a device window
may overlap its destination band.

Expected pixels are the reference's (tests/helpers.py: checker_avir /
checker_lancir), one whole frame per case; a band's expectation is
want[row0:row1]. Raw words are compared, the bar is 0 differing elements."""
import ctypes as C
import threading
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import helpers as H
from tests import refbind as rb
from tests import window_cases as W

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
SENTINEL = 0xA5


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def _image(c, seed=0):
    """The real source image of a case, (sh, sw, ch)."""
    fe, sw, sh, nw, nh, ch, tin, tout = c[:8]
    tin = np.dtype(tin)
    if tin.kind == "u":
        raw = rb.lcg_u8((sh, sw, ch, tin.itemsize), seed=sw + ch + seed)
        return np.ascontiguousarray(raw).view(tin).reshape(sh, sw, ch)
    a = rb.lcg_f32((sh, sw, ch), seed=7 * sw + ch + seed)
    if tin == np.float64:
        # (mantissa bits a float does not hold)
        b = rb.lcg_f32((sh, sw, ch), seed=sh + seed)
        return a.astype(np.float64) + b.astype(np.float64) * 2.0 ** -25
    return a


def _poison(img):
    """NaN for float images; the bitwise complement of an integer image, so
    that every stale element differs from the true one."""
    if img.dtype.kind == "f":
        return np.full_like(img, np.nan)
    return ~img


def _flat(img, pitch, fill):
    """(rows, sw, ch) -> the rows at `pitch` elements, exactly
    (rows - 1) * pitch + sw * ch elements long; padding = `fill`."""
    rows, sw, ch = img.shape
    out = np.full(rows * pitch, fill, img.dtype)
    out.reshape(rows, pitch)[:, :sw * ch] = img.reshape(rows, sw * ch)
    return np.ascontiguousarray(out[:(rows - 1) * pitch + sw * ch])


def _want(c, img):
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = c
    if fe == "lancir":
        k = float(ex.get("k", 0.0))
        return H.checker_lancir(img, nw, nh, out_dtype=tout, kx=k, ky=k,
                                ox=float(ex.get("ox", 0.0)),
                                oy=float(ex.get("oy", 0.0)))
    kw = {}
    if ex.get("fp") == abi.FPCLASS_DOUBLE:
        assert H.need_ref("the double class")
        kw["variant"] = 4
    return H.checker_avir(img, nw, nh, k=float(ex.get("k", 0.0)),
                          out_dtype=tout, resbits=bits,
                          ox=float(ex.get("ox", 0.0)),
                          oy=float(ex.get("oy", 0.0)),
                          build_mode=ex.get("build_mode", -1), threads=8,
                          gamma=bool(ex.get("gamma", 0)),
                          alpha=ex.get("alpha", -1), **kw)


def _plan(c, obj, arg):
    """The device plan of a case on its forced path / variant. A refusal
    fails the test: the table has to hold geometries its families take."""
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = c
    lib = abi.load()
    ti, to = avir_amd._NP2T[np.dtype(tin)], avir_amd._NP2T[np.dtype(tout)]
    if fe == "lancir":
        p = obj.plan(sw, sh, nw, nh, ch, arg, ti, to)
    else:
        p = obj.plan(sw, sh, nw, nh, ch, float(ex.get("k", 0.0)), arg, ti, to,
                     W.pitch(c) if ex.get("pad") else 0)
    abi.check(lib.avirhip_plan_set_path(p, path), "set_path %d" % path)
    abi.check(lib.avirhip_plan_set_variant(p, variant),
              "set_variant %d" % variant)
    if path != 0:
        assert lib.avirhip_plan_get_path(p) == path
    elif "auto_path" in ex:
        assert lib.avirhip_plan_get_path(p) == ex["auto_path"]
    return p


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)
                            ).to("cuda:0")


def _dev_sentinel(nbytes):
    import torch
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda:0")


def _rows_of(lib, p, r0, r1):
    a, b = C.c_int(), C.c_int()
    abi.check(lib.avirhip_band_source_rows(p, r0, r1, C.byref(a), C.byref(b)),
              "band_source_rows")
    return a.value, b.value


def _differ(got_bytes, want_band):
    """Differing elements of a band (raw words)."""
    w = _bits(want_band).reshape(-1)
    g = np.ascontiguousarray(got_bytes).view(w.dtype)
    assert g.size == w.size
    return int((g != w).sum())


@pytest.mark.parametrize("case", W.CASES, ids=W.IDS)
def test_window_differential(case):
    """A1: every band of the case from a compact device window, a compact
    host window and one wider device window; the plan's frame-sized staging
    buffer and packed float copy are filled with poison before each call."""
    import torch
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = case
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    img = _image(case)
    want = _want(case, img)
    assert want.shape == (nh, nw, ch) and want.dtype == np.dtype(tout)
    obj, arg = W.front_end(case)
    p = _plan(case, obj, arg)
    pitch = W.pitch(case)
    esz = np.dtype(tin).itemsize
    osz = np.dtype(tout).itemsize
    pfill = np.nan if img.dtype.kind == "f" else np.iinfo(img.dtype).max
    frame = _flat(img, pitch, pfill)
    d_poison = _dev(_flat(_poison(img), pitch, pfill))
    d_scratch = _dev_sentinel(nh * nw * ch * osz)
    native = bool(ex.get("native"))
    problems = []

    def poison():
        abi.check(lib.avirhip_resize_window(
            p, d_poison.data_ptr(), abi.MEM_DEVICE, 0, sh,
            d_scratch.data_ptr(), abi.MEM_DEVICE, 0, nh, None), "poison call")

    def run(what, first, n, ptr, mem, r0, r1, host_dst):
        """One window call -> the band's bytes; checks the plan's growth."""
        nbytes = (r1 - r0) * nw * ch * osz
        win_bytes = ((n - 1) * pitch + sw * ch) * esz
        poison()
        before = lib.avirhip_plan_device_bytes(p)
        if host_dst:
            out = np.full(nbytes, SENTINEL, np.uint8)
            abi.check(lib.avirhip_resize_window(
                p, ptr, mem, first, n, out.ctypes.data, abi.MEM_HOST, r0, r1,
                None), what)
            torch.cuda.synchronize()
        else:
            d = _dev_sentinel(nbytes)
            abi.check(lib.avirhip_resize_window(
                p, ptr, mem, first, n, d.data_ptr(), abi.MEM_DEVICE, r0, r1,
                None), what)
            torch.cuda.synchronize()
            out = d.cpu().numpy()
        grow = lib.avirhip_plan_device_bytes(p) - before
        if native and not host_dst and grow > win_bytes + 4096:
            problems.append("%s: the plan grew by %d bytes, the window has %d"
                            % (what, grow, win_bytes))
        nd = _differ(out, want[r0:r1])
        print("%s: window rows [%d, %d) of %d, %d of %d elements differ"
              % (what, first, first + n, sh, nd, (r1 - r0) * nw * ch))
        if nd:
            problems.append("%s: %d elements differ" % (what, nd))

    for name, r0, r1 in W.bands(nh):
        a, b = _rows_of(lib, p, r0, r1)
        assert (a, b) == W.host_source_rows(case, obj, arg, r0, r1), name
        win = [(name, a, b - a + 1)]
        if name == "frame":
            win = [(name, 0, sh)]
        elif name == "inner":
            wa, wb = max(0, a - 3), min(sh - 1, b + 5)
            win.append((name + "-wide", wa, wb - wa + 1))
        for wname, first, n in win:
            rows = frame[first * pitch:(first + n - 1) * pitch + sw * ch]
            rows = np.ascontiguousarray(rows)
            assert rows.nbytes == ((n - 1) * pitch + sw * ch) * esz
            dsts = [False] + ([True] if ex.get("host_dst") else [])
            for host_dst in dsts:
                tag = "%s%s" % (wname, " host dst" if host_dst else "")
                d_rows = _dev(rows)
                run(tag + " device window", first, n, d_rows.data_ptr(),
                    abi.MEM_DEVICE, r0, r1, host_dst)
                if wname.endswith("-wide"):
                    continue
                run(tag + " host window", first, n, rows.ctypes.data,
                    abi.MEM_HOST, r0, r1, host_dst)
            if native and not wname.endswith("-wide"):
                # the window in the middle of a larger tensor whose other
                # rows are NaN: every byte the kernels may touch is mapped, a
                # wrong row index shows as a wrong pixel
                G = 16
                big = np.full((n + 2 * G) * pitch, np.nan, img.dtype)
                big[G * pitch:G * pitch + rows.size] = rows
                d_big = _dev(big)
                run(wname + " device window between NaN rows", first, n,
                    d_big.data_ptr() + G * pitch * esz, abi.MEM_DEVICE, r0, r1,
                    False)
    assert not problems, "\n".join(problems)


def _refusal_plans():
    """(case, ...) of one staged and one native plan."""
    return [("avir", 600, 800, 300, 400, 4, np.float32, np.float32, 16, 0, 0,
             {}),
            ("avir", 320, 416, 640, 832, 4, np.float32, np.float32, 16, 0, 0,
             dict(native=1, auto_path=4))]


def test_window_refusals_leave_the_destination_alone():
    """A2: windows that do not cover the band's rows or the frame are refused
    with EINVAL and a message before anything is stored; an empty band stores
    nothing; the error-diffusion ditherer takes whole frames only."""
    import torch
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    for case in _refusal_plans():
        fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = case
        img = _image(case)
        obj, arg = W.front_end(case)
        p = _plan(case, obj, arg)
        pitch = W.pitch(case)
        rowb = pitch * 4
        # (two rows of slack behind the frame: a call that is wrongly NOT
        # refused still reads mapped memory)
        d_frame = _dev(np.concatenate([img.reshape(-1),
                                       np.zeros(2 * pitch, np.float32)]))
        base = d_frame.data_ptr()
        r0, r1 = 2 * (nh // 5), 3 * (nh // 5)
        a, b = _rows_of(lib, p, r0, r1)
        assert 3 < a <= b < sh - 3
        nbytes = (r1 - r0) * nw * ch * 4
        bad = [("starts one row late", a + 1, b - a),
               ("ends one row early", a, b - a),
               ("first_row -1", -1, b + 2),
               ("past the frame", a, sh + 1 - a),
               ("no rows", a, 0),
               ("INT_MAX rows", 1, INT_MAX)]
        for what, first, n in bad:
            ptr = base + max(first, 0) * rowb
            for mem, src in ((abi.MEM_DEVICE, ptr),
                             (abi.MEM_HOST, img.ctypes.data +
                              max(first, 0) * rowb)):
                if mem == abi.MEM_HOST and first + n > sh:
                    continue  # (no host rows to point at behind the frame)
                d = _dev_sentinel(nbytes)
                rc = lib.avirhip_resize_window(p, src, mem, first, n,
                                               d.data_ptr(), abi.MEM_DEVICE,
                                               r0, r1, None)
                msg = lib.avirhip_last_error()
                torch.cuda.synchronize()
                assert rc == abi.EINVAL, (what, mem, rc)
                assert msg, (what, mem)
                assert bool((d == SENTINEL).all()), (what, mem)
        # an empty band with a valid window: OK, nothing stored
        d = _dev_sentinel(nbytes)
        rc = lib.avirhip_resize_window(p, base + a * rowb, abi.MEM_DEVICE, a,
                                       b - a + 1, d.data_ptr(), abi.MEM_DEVICE,
                                       r0, r0, None)
        torch.cuda.synchronize()
        assert rc == 0
        assert bool((d == SENTINEL).all())

    # the error-diffusion ditherer is recursive over rows
    sw, sh, nw, nh, ch = 300, 400, 460, 613, 3
    img = rb.lcg_u8((sh, sw, ch), seed=5)
    want = H.checker_avir(img, nw, nh, out_dtype=np.uint8, resbits=8,
                          errd=True, threads=8)
    r = avir_amd.CImageResizer(8, aDitherer="errd")
    p = r.plan(sw, sh, nw, nh, ch, 0.0, None, abi.U8, abi.U8)
    d_img = _dev(img)
    r0, r1 = 2 * (nh // 5), 3 * (nh // 5)
    a, b = _rows_of(lib, p, r0, r1)
    d = _dev_sentinel((r1 - r0) * nw * ch)
    rc = lib.avirhip_resize_window(
        p, d_img.data_ptr() + a * sw * ch, abi.MEM_DEVICE, a, b - a + 1,
        d.data_ptr(), abi.MEM_DEVICE, r0, r1, None)
    msg = lib.avirhip_last_error()
    torch.cuda.synchronize()
    assert rc == abi.EUNSUPPORTED and msg
    assert bool((d == SENTINEL).all())
    d = _dev_sentinel(nh * nw * ch)
    abi.check(lib.avirhip_resize_window(
        p, d_img.data_ptr(), abi.MEM_DEVICE, 0, sh, d.data_ptr(),
        abi.MEM_DEVICE, 0, nh, None), "errd whole frame through a window")
    torch.cuda.synchronize()
    assert _differ(d.cpu().numpy(), want) == 0


# Iterations of each of A3's threads. On the library that kept the window on
# the plan (NOTEBOOK.md section 12) 129 of 2000 whole-frame results and 31 of
# 2000 band results were wrong, the first in iteration 0 of both threads: one
# wrong result per 15 iterations of the whole-frame thread. 400 iterations are
# some 25 times that, and run in under a second.
A3_ITERS = 400


@pytest.mark.parametrize("fe,path", [("avir", 0), ("lancir", 0),
                                     ("lancir", 4)])
def test_window_calls_and_lock_free_calls_share_a_plan(fe, path):
    """A3: four threads on one exact-2x float RGBA plan, each on its own
    stream: two avirhip_resize_window calls for different inner bands, one
    avirhip_resize, one avirhip_resize_band for rows outside both windows.
    Every result of every iteration is compared with the reference's rows.

    CImageResizer: k_up2, whose whole-frame and band calls take no lock.
    CLancIR: every call takes the plan's lock; at this size its automatic
    path is the pass kernels (5), k_lanc2 is path 4 -- both are run.

    The windows are VIEWS into the whole-frame device tensor: the virtual
    frame base the kernels get is the real one, so a library that mixes up
    the calls' row clamps shows wrong pixels and reads nothing unmapped."""
    import torch
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    sw, sh = 640, 480
    nw, nh = 2 * sw, 2 * sh
    img = rb.lcg_f32((sh, sw, 4), seed=640)
    if fe == "avir":
        obj = avir_amd.CImageResizer(16)
        want = H.checker_avir(img, nw, nh, resbits=16, threads=8)
        p = obj.plan(sw, sh, nw, nh, 4)
        assert lib.avirhip_plan_get_path(p) == abi.PATH_UP2
    else:
        obj = avir_amd.CLancIR()
        want = H.checker_lancir(img, nw, nh)
        p = obj.plan(sw, sh, nw, nh, 4)
        abi.check(lib.avirhip_plan_set_path(p, path), "set_path")
        assert lib.avirhip_plan_get_path(p) == (path or abi.PATH_GPASS)
    d_frame = torch.from_numpy(img).to("cuda:0")
    d_want = torch.from_numpy(_bits(want).view(np.int32)).to("cuda:0")
    rowb = sw * 16
    f = nh // 5
    jobs = [("window A", f, 2 * f, True), ("window B", 3 * f, 4 * f, True),
            ("whole frame", 0, nh, None), ("band", 0, nh // 10, False)]
    wins = [_rows_of(lib, p, r0, r1) for _, r0, r1, w in jobs if w]
    ba, bb = _rows_of(lib, p, 0, nh // 10)
    assert all(bb < a for a, b in wins), "the band must lie outside the windows"
    torch.cuda.synchronize()
    flags, errors = {}, []
    start = threading.Barrier(len(jobs))

    def work(name, r0, r1, windowed):
        try:
            abi.check(lib.avirhip_init(0), "init")
            s = torch.cuda.Stream(device="cuda:0")
            st = s.cuda_stream
            with torch.cuda.stream(s):
                dst = torch.empty((r1 - r0, nw, 4), dtype=torch.float32,
                                  device="cuda:0")
                bad = torch.zeros(A3_ITERS, dtype=torch.int32, device="cuda:0")
                a, b = _rows_of(lib, p, r0, r1)
                src = d_frame[a:b + 1]  # a view: no copy
                assert src.data_ptr() == d_frame.data_ptr() + a * rowb
                s.synchronize()
                start.wait()
                for it in range(A3_ITERS):
                    dst.zero_()
                    if windowed:
                        rc = lib.avirhip_resize_window(
                            p, src.data_ptr(), abi.MEM_DEVICE, a, b - a + 1,
                            dst.data_ptr(), abi.MEM_DEVICE, r0, r1, st)
                    elif windowed is None:
                        rc = lib.avirhip_resize(
                            p, d_frame.data_ptr(), abi.MEM_DEVICE,
                            dst.data_ptr(), abi.MEM_DEVICE, st)
                    else:
                        rc = lib.avirhip_resize_band(
                            p, d_frame.data_ptr(), abi.MEM_DEVICE,
                            dst.data_ptr(), abi.MEM_DEVICE, r0, r1, st)
                    abi.check(rc, name)
                    bad[it] = (dst.view(torch.int32) != d_want[r0:r1]).any()
                s.synchronize()
                flags[name] = bad.cpu().numpy()
        except BaseException as e:  # noqa: B902 (reported by the main thread)
            errors.append((name, repr(e)))
            start.abort()

    ts = [threading.Thread(target=work, args=j) for j in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    report = {}
    for name in flags:
        w = np.flatnonzero(flags[name])
        report[name] = (int(w.size), int(w[0]) if w.size else None)
    print("wrong results of %d iterations (count, first): %r"
          % (A3_ITERS, report))
    assert all(n == 0 for n, _ in report.values()), report


@pytest.mark.parametrize("case", _refusal_plans(),
                         ids=["staged-k_dnf", "native-k_up2"])
def test_device_window_that_overlaps_its_destination_band(case):
    """A4: source window and dst_band in one device tensor -- dst_band at the
    window's first byte, in its middle, adjacent but disjoint. The library's
    answer to an overlap (include/avirhip.h, avirhip_resize_window): the
    window is copied aside first, so every layout gives the reference's bits,
    on every repeat."""
    import torch
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = case
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    img = _image(case, seed=3)
    want = _want(case, img)
    obj, arg = W.front_end(case)
    p = _plan(case, obj, arg)
    # (a band long enough that rows stored early lie on window rows that are
    # read late: the marching kernels hold some twenty source rows in flight)
    r0 = nh // 3
    r1 = r0 + min(160, nh // 3)
    a, b = _rows_of(lib, p, r0, r1)
    rows = np.ascontiguousarray(img[a:b + 1]).view(np.uint8).reshape(-1)
    win_bytes = rows.size
    dst_bytes = (r1 - r0) * nw * ch * 4
    up = (win_bytes + 255) & ~255
    layouts = [("dst at the window's first byte", 0),
               ("dst in the middle of the window", (win_bytes // 2) & ~255),
               ("dst behind the window", up)]
    h_rows = torch.from_numpy(rows)
    problems = []
    for what, off in layouts:
        for rep in range(3):
            buf = _dev_sentinel(up + dst_bytes + 256)
            buf[:win_bytes] = h_rows.to("cuda:0")
            torch.cuda.synchronize()
            rc = lib.avirhip_resize_window(
                p, buf.data_ptr(), abi.MEM_DEVICE, a, b - a + 1,
                buf.data_ptr() + off, abi.MEM_DEVICE, r0, r1, None)
            torch.cuda.synchronize()
            if rc != 0:
                problems.append("%s, repeat %d: error %d (%s)" % (
                    what, rep, rc, lib.avirhip_last_error()))
                continue
            got = buf[off:off + dst_bytes].cpu().numpy()
            nd = _differ(got, want[r0:r1])
            print("%s, repeat %d: %d of %d elements differ"
                  % (what, rep, nd, dst_bytes // 4))
            if nd:
                problems.append("%s, repeat %d: %d of %d elements differ"
                                % (what, rep, nd, dst_bytes // 4))
            # (what lies behind the band is not the call's to write)
            tail = buf[max(off + dst_bytes, up):]
            if not bool((tail == SENTINEL).all()):
                problems.append("%s, repeat %d: bytes behind the band were "
                                "written" % (what, rep))
    assert not problems, "\n".join(problems)
