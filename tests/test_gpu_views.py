"""Plane views of the planar calls on the device (include/avirhip.h, "Plane
views"): channel-last images, RGBX results, batches of images, planes in
separate allocations -- each ONE call of CLancIR (k_lancp) or CImageResizer
(k_avirp) over views, between guard bytes.

Bars of every case: the raw bytes of every result element equal the
reference's one-channel result of its plane (0 differing); every other byte of
every result allocation -- between strided neighbours, between rows, in front
and behind -- is still the guard byte; AVIRHIP_VERBOSE shows exactly one
k_lancp / k_avirp line and no per-plane line (the declined cases: the
per-plane line and no kernel line). The view arrays are overwritten with
garbage as soon as the call returns, before the device is waited for.

Geometries, sources and expected bits are those of tests/planes_cases.py and
tests/avir_planes_cases.py (the reference runs once per distinct plane)."""
import ctypes as C
import re
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import planes_cases as P
from tests import avir_planes_cases as A
from tests import dnf16_cases as D16
from tests.gpass_route_cases import environment

pytestmark = pytest.mark.gpu

MEM_VIEWS, PlaneView = abi.MEM_VIEWS, abi.PlaneView   # (the feature itself)
GUARD, FRONT = P.GUARD, P.FRONT
LINE = re.compile(r"^(k_lancp|k_avirp|planes: per-plane road)\b", re.M)
KERNEL = {"lancir": "k_lancp", "avir": "k_avirp"}

# ---- geometries -----------------------------------------------------------------
# CLancIR: two tiles across, five down, partial tiles both ways; a downsizing
# row of planes_cases; one pixel wide; one row high
L_GEOMS = {"up2x5": (64, 48, 100, 77), "dn3": P.DN3, "w1": (1, 23, 1, 40),
           "h1": (37, 1, 61, 1)}
A_GEOMS = {"upf_both": A.GEOMS["upf_both"][0], "dn3": A.GEOMS["dn3"][0],
           "dn_zs": A.GEOMS["dn_zs"][0], "mix_ud": A.GEOMS["mix_ud"][0],
           "w1": (1, 23, 1, 40), "h1": (37, 1, 61, 1)}


def case_row(cls, geom, tin="u8", tout="u8", planes=3):
    if cls == "lancir":
        return dict(P.row("tap_up"), geom=L_GEOMS[geom], tin=tin, tout=tout,
                    planes=planes)
    return dict(A.row("upf_both"), geom=A_GEOMS[geom], tin=tin, tout=tout,
                planes=planes, bits=8 if tout == "u8" else 16)


def cases_of(cls):
    return P if cls == "lancir" else A


def source_plane(cls, r, i):
    return cases_of(cls).sources(r)[i]


# ---- layouts ---------------------------------------------------------------------
# A layout places n planes of (w, h) elements into allocations: -> (sizes in
# bytes, [(allocation, byte offset, row pitch, element stride)] per plane),
# pitch and stride in elements.

def lay_dense(n, w, h, es):
    """Tightly packed channel-first planes in one allocation: passed as a
    device pointer, not as views."""
    return [2 * FRONT + n * h * w * es], [(0, FRONT + i * h * w * es, w, 1)
                                          for i in range(n)]


def lay_dense_gap(n, w, h, es):
    """Channel-first planes 7 elements apart in one allocation: a device
    pointer and a plane stride, beside views on the other side."""
    st = h * w + 7
    return [2 * FRONT + ((n - 1) * st + h * w) * es], [
        (0, FRONT + i * st * es, w, 1) for i in range(n)]


def lay_hwc_row(n, w, h, es):
    """One row high: interleaved views that give different row pitches, one
    of them none -- a pitch that addresses nothing."""
    assert h == 1 and n == 3
    return [2 * FRONT + (w * 3 + 5) * es], [
        (0, FRONT + i * es, (0, w * 3, w * 3 + 11)[i], 3) for i in range(n)]


def _interleaved(e, pad):
    def lay(n, w, h, es):
        assert n % 3 == 0
        pitch = w * e + pad
        img = (h * pitch + 5) * es          # images a few elements apart
        return [2 * FRONT + (n // 3) * img], [
            (0, FRONT + (i // 3) * img + (i % 3) * es, pitch, e)
            for i in range(n)]
    return lay


lay_hwc = _interleaved(3, 0)       # H x W x 3, rows tight
lay_hwc_pad = _interleaved(3, 6)   # ... rows padded (P % E == 0)
lay_rgbx = _interleaved(4, 0)      # H x W x 4, the fourth element no plane's


def lay_sep(n, w, h, es):
    """One allocation a plane, listed in shuffled order, every plane with a
    row pitch of its own."""
    order = [(i * 2 + 1) % n for i in range(n)] if n % 2 else list(
        reversed(range(n)))
    sizes = [0] * n
    out = []
    for i in range(n):
        pitch = w + (i % 3) * 2
        sizes[order[i]] = 2 * FRONT + ((h - 1) * pitch + w + 3) * es
        out.append((order[i], FRONT, pitch, 1))
    return sizes, out


LAYOUTS = {"dense": lay_dense, "dense_gap": lay_dense_gap,
           "hwc_row": lay_hwc_row, "hwc": lay_hwc, "hwc_pad": lay_hwc_pad,
           "rgbx": lay_rgbx, "sep": lay_sep}


class Side(object):
    """One side of a call on the device: allocations full of guard bytes with
    `planes` placed in them (None: guards only), and its argument."""

    def __init__(self, layout, n, w, h, dtype, planes=None, twice=False):
        import torch
        self.n, self.w, self.h, self.dtype = n, w, h, np.dtype(dtype)
        self.dense = layout in ("dense", "dense_gap")
        # the plane stride argument: 0 beside views and for tight planes
        self.stride = h * w + 7 if layout == "dense_gap" else 0
        sizes, self.at = LAYOUTS[layout](n, w, h, self.dtype.itemsize)
        if twice:
            # the first view given twice: plane 1 reads plane 0's elements
            self.at[1] = self.at[0]
        self.sizes = [(s + 7) & ~7 for s in sizes]
        host = self.image(planes)
        self.dev = [torch.from_numpy(b).to("cuda:0") for b in host]

    def image(self, planes):
        """The allocations as byte arrays: guards, `planes` placed."""
        out = [np.full(s, GUARD, np.uint8) for s in self.sizes]
        if planes is not None:
            for (b, off, pitch, e), pl in zip(self.at, planes):
                a = out[b][off:off + ((self.sizes[b] - off) //
                                      self.dtype.itemsize) * self.dtype.itemsize]
                a = a.view(self.dtype)
                for y in range(self.h):
                    a[y * pitch:y * pitch + (self.w - 1) * e + 1:e] = pl[y]
        return out

    def arg(self):
        """(pointer, mem kind, what to keep alive)"""
        if self.dense:
            return (C.c_void_p(self.dev[0].data_ptr() + self.at[0][1]),
                    abi.MEM_DEVICE, None)
        v = (PlaneView * self.n)()
        for x, (b, off, pitch, e) in zip(v, self.at):
            x.base = self.dev[b].data_ptr() + off
            x.row_pitch, x.elem_stride = pitch, e
        return C.cast(v, C.c_void_p), MEM_VIEWS, v

    def check(self, planes, what):
        """Every byte of every allocation: elements and guards."""
        want = self.image(planes)
        mask = self.image([np.zeros_like(p) for p in planes])
        bad_px = bad_guard = 0
        for t, w_, m in zip(self.dev, want, mask):
            g = t.cpu().numpy()
            px = (m != GUARD) | (w_ != GUARD)
            d = g != w_
            bad_px += int((d & px).sum())
            bad_guard += int((d & ~px).sum())
        print("%s: %d element bytes differ, %d guard bytes written" % (
            what, bad_px, bad_guard))
        assert bad_guard == 0, "%s: %d bytes that are no element written" % (
            what, bad_guard)
        assert bad_px == 0, "%s: %d element bytes differ" % (what, bad_px)


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    return lib


class front(object):
    """with front(lib, cls, r) as call: the front end object of the row; it is
    destroyed behind the block, where the device has been waited for."""

    def __init__(self, lib, cls, r):
        self.lib, self.cls, self.r = lib, cls, r

    def __enter__(self):
        if self.cls == "lancir":
            self.h = C.c_void_p()
            abi.check(self.lib.avirhip_lancir_create(C.byref(self.h)), "create")
        else:
            self.h = A.resizer(self.lib, self.r)
        return self.call

    def __exit__(self, *a):
        if self.cls == "lancir":
            self.lib.avirhip_lancir_destroy(self.h)
        else:
            self.lib.avirhip_resizer_destroy(self.h)

    def call(self, sarg, darg, stream=None, sps=0, dps=0):
        r, lib = self.r, self.lib
        sw, sh, nw, nh = r["geom"]
        ti, to = P.T[r["tin"]][0], P.T[r["tout"]][0]
        if self.cls == "lancir":
            p = P.params(dict(r, spad=0, npad=0))
            rc = lib.avirhip_lancir_resize_planes(
                self.h, sarg[0], sarg[1], sw, sh, darg[0], darg[1], nw, nh,
                r["planes"], sps, dps, C.byref(p), ti, to, stream)
            return 0 if rc == nh else (rc if rc < 0 else -100 - rc)
        v = A.vars_of(r)
        return lib.avirhip_resizer_resize_planes(
            self.h, sarg[0], sarg[1], sw, sh, 0, darg[0], darg[1], nw, nh,
            r["planes"], sps, dps, float(r["k"]), C.byref(v), ti, to, stream)


def run(lib, capfd, cls, r, slay, dlay, road=None, env=None, twice=False):
    """One call over the layouts, every bar."""
    import torch
    sw, sh, nw, nh = r["geom"]
    n = r["planes"]
    cs = cases_of(cls)
    smap = [0 if (twice and i == 1) else i for i in range(n)]
    S = Side(slay, n, sw, sh, P.T[r["tin"]][1],
             [source_plane(cls, r, smap[i]) for i in range(n)], twice=twice)
    D = Side(dlay, n, nw, nh, P.T[r["tout"]][1])
    sarg, darg = S.arg(), D.arg()
    torch.cuda.synchronize()
    with environment(dict(env or {}, AVIRHIP_VERBOSE="1")), \
            front(lib, cls, r) as call:
        capfd.readouterr()
        rc = call(sarg, darg, sps=S.stride, dps=D.stride)
        # the arrays are the caller's again: garbage, before the device is done
        for a in (sarg, darg):
            if a[2] is not None:
                C.memset(a[2], 0xa5, C.sizeof(a[2]))
        torch.cuda.synchronize()
        lines = LINE.findall(capfd.readouterr().err)
    what = "%s %s %s %s->%s %s->%s" % (cls, r["geom"], n, slay, dlay,
                                       r["tin"], r["tout"])
    print(what, rc, lines)
    assert rc == 0, (rc, lib.avirhip_last_error())
    D.check([cs.expected(r, smap[i]) for i in range(n)], what)
    assert lines == [road or KERNEL[cls]], (what, lines)
    return D


GEOM_CASES = ([("lancir", g) for g in L_GEOMS] + [("avir", g) for g in A_GEOMS])
LAYOUT_CASES = [("hwc", "dense", 3), ("dense", "hwc", 3), ("dense", "rgbx", 3),
                ("hwc", "hwc", 3), ("hwc", "hwc", 6), ("sep", "sep", 5),
                ("hwc_pad", "sep", 3), ("sep", "hwc_pad", 3),
                # the side without views keeps its plane stride
                ("hwc", "dense_gap", 3), ("dense_gap", "hwc", 3),
                ("dense_gap", "rgbx", 6)]


@pytest.mark.parametrize("cls,geom", GEOM_CASES)
def test_geometry_hwc(cls, geom, lib, capfd):
    """Every geometry: a channel-last image in, a channel-last image out."""
    run(lib, capfd, cls, case_row(cls, geom), "hwc", "hwc")


@pytest.mark.parametrize("cls", ["lancir", "avir"])
@pytest.mark.parametrize("slay,dlay,n", LAYOUT_CASES)
def test_layout(cls, slay, dlay, n, lib, capfd):
    geom = "up2x5" if cls == "lancir" else "upf_both"
    run(lib, capfd, cls, case_row(cls, geom, planes=n), slay, dlay)


@pytest.mark.parametrize("cls", ["lancir", "avir"])
def test_one_row_pitches_differ(cls, lib, capfd):
    """Interleaved result views of one row: their pitches address nothing and
    need not agree."""
    run(lib, capfd, cls, case_row(cls, "h1"), "hwc_row", "hwc_row")


@pytest.mark.parametrize("cls", ["lancir", "avir"])
def test_source_view_twice(cls, lib, capfd):
    geom = "dn3"
    run(lib, capfd, cls, case_row(cls, geom), "hwc", "rgbx", twice=True)


TYPES = [(t, t) for t in ("u8", "u16", "f16", "bf16", "f32")] + [
    ("u8", "f32"), ("f32", "u8")]


@pytest.mark.parametrize("cls", ["lancir", "avir"])
@pytest.mark.parametrize("tin,tout", TYPES)
def test_types_hwc(cls, tin, tout, lib, capfd):
    geom = "up2x5" if cls == "lancir" else "mix_ud"
    run(lib, capfd, cls, case_row(cls, geom, tin, tout), "hwc", "hwc")


# ---- declined views: the per-plane road, strided on both sides -------------------

@pytest.mark.parametrize("cls", ["lancir", "avir"])
def test_declined_f64(cls, lib, capfd):
    geom = "dn3"
    run(lib, capfd, cls, case_row(cls, geom, "f64", "f64"), "hwc", "rgbx",
        road="planes: per-plane road")


def test_declined_by_pixels(lib, capfd):
    run(lib, capfd, "avir", case_row("avir", "dn_zs"), "hwc_pad", "hwc",
        road="planes: per-plane road",
        env={"AVIRHIP_AVIRP_MAX_PIXELS": "1"})


@pytest.mark.parametrize("slay,dlay", [("hwc", "dense_gap"),
                                       ("dense_gap", "rgbx")])
def test_declined_plane_stride(slay, dlay, lib, capfd):
    """The per-plane road beside a dense side at a plane stride."""
    run(lib, capfd, "avir", case_row("avir", "dn_zs"), slay, dlay,
        road="planes: per-plane road",
        env={"AVIRHIP_AVIRP_MAX_PIXELS": "1"})


@pytest.mark.parametrize("cls", ["lancir", "avir"])
def test_zero_sized_source(cls, lib):
    """A zero-sized source zero-fills the elements of every result view and
    nothing else; a host result beside views is refused before the fill."""
    import torch
    r = case_row(cls, "dn3")
    nw, nh = r["geom"][2:]
    r = dict(r, geom=(0, 5, nw, nh))
    zero = [np.zeros((nh, nw), np.uint8)] * 3
    S = Side("hwc", 3, 4, 5, np.uint8)
    for dlay in ("rgbx", "sep", "dense_gap"):
        D = Side(dlay, 3, nw, nh, np.uint8)
        sarg, darg = S.arg(), D.arg()
        with front(lib, cls, r) as call:
            rc = call(sarg, darg, dps=D.stride)
            torch.cuda.synchronize()
        assert rc == 0, (rc, lib.avirhip_last_error())
        D.check(zero, "%s zero-sized source -> %s" % (cls, dlay))
    host = np.full(3 * nh * nw, GUARD, np.uint8)
    with front(lib, cls, r) as call:
        rc = call(S.arg(), (C.c_void_p(host.ctypes.data), 2, None))  # MEM_AUTO
    assert rc == abi.EINVAL, rc
    assert b"device memory" in lib.avirhip_last_error()
    assert (host == GUARD).all()


def test_declined_dense_views_pass_their_base(lib, capfd):
    """Views that are tight planes at the plan's pitch need no staging: the
    same bits through the per-plane road."""
    run(lib, capfd, "avir", case_row("avir", "dn_zs", planes=5), "sep", "sep",
        road="planes: per-plane road",
        env={"AVIRHIP_AVIRP_MAX_PIXELS": "1"})


# ---- against today's dense call of the same library ------------------------------

@pytest.mark.parametrize("cls", ["lancir", "avir"])
def test_equals_dense_call(cls, lib, capfd):
    """The views call on HWC data equals the dense call on the de-interleaved
    copy, word for word."""
    r = case_row(cls, "dn3", "f16", "f16", planes=6)
    a = run(lib, capfd, cls, r, "hwc", "hwc")
    b = run(lib, capfd, cls, r, "dense", "dense")
    nw, nh = r["geom"][2:]
    for i in range(6):
        planes = []
        for side in (a, b):
            blk, off, pitch, e = side.at[i]
            g = side.dev[blk].cpu().numpy()
            g = g[off:off + ((g.size - off) // 2) * 2].view(np.uint16)
            planes.append(np.stack([g[y * pitch:y * pitch + (nw - 1) * e + 1:e]
                                    for y in range(nh)]))
        assert planes[0].shape == (nh, nw)
        assert np.array_equal(planes[0], planes[1]), i


# ---- the plan level ---------------------------------------------------------------

def test_plan_level(lib):
    """avirhip_resize_planes takes views too, and validates them."""
    import torch
    r = case_row("avir", "dn_zs")
    sw, sh, nw, nh = r["geom"]
    h = A.resizer(lib, r)
    try:
        p = C.c_void_p()
        abi.check(lib.avirhip_resizer_get_plan(
            h, sw, sh, 0, nw, nh, 1, 0.0, None, abi.U8, abi.U8, C.byref(p)),
            "get_plan")
        S = Side("hwc", 3, sw, sh, np.uint8,
                 [source_plane("avir", r, i) for i in range(3)])
        D = Side("hwc", 3, nw, nh, np.uint8)
        sarg, darg = S.arg(), D.arg()

        def go(sps=0, dps=0, d=darg):
            return lib.avirhip_resize_planes(p, sarg[0], sarg[1], sps, d[0],
                                             d[1], dps, 3, None)
        assert go(sps=64) == abi.EINVAL
        assert b"plane stride" in lib.avirhip_last_error()
        assert go(d=sarg) == abi.EINVAL
        assert b"share bytes" in lib.avirhip_last_error()
        bad = (PlaneView * 3)()
        C.memmove(bad, darg[2], C.sizeof(bad))
        bad[2].base = bad[0].base + 3           # 3 elements on: 3 % E == 0
        assert go(d=(C.cast(bad, C.c_void_p), MEM_VIEWS)) == abi.EINVAL
        assert b"interleaved" in lib.avirhip_last_error()
        bad[2].base = bad[0].base + 2
        bad[2].row_pitch = 2 * nw * 3           # another pitch
        assert go(d=(C.cast(bad, C.c_void_p), MEM_VIEWS)) == abi.EINVAL
        assert b"interleaved" in lib.avirhip_last_error()
        for v in bad:
            v.row_pitch = nw * 3 + 1            # P % E != 0
        assert go(d=(C.cast(bad, C.c_void_p), MEM_VIEWS)) == abi.EINVAL
        assert b"interleaved" in lib.avirhip_last_error()
        C.memmove(bad, darg[2], C.sizeof(bad))
        bad[2].row_pitch = (nw - 1) * 3         # one element short
        assert go(d=(C.cast(bad, C.c_void_p), MEM_VIEWS)) == abi.EINVAL
        assert b"row pitch" in lib.avirhip_last_error()
        torch.cuda.synchronize()
        D.check([np.full((nh, nw), GUARD, np.uint8)] * 3, "refused calls")
        assert go() == 0, lib.avirhip_last_error()
        torch.cuda.synchronize()
        D.check([A.expected(r, i) for i in range(3)], "plan level")
    finally:
        lib.avirhip_resizer_destroy(h)


# ---- Python ------------------------------------------------------------------------

def _resizer(cls):
    return avir_amd.CLancIR() if cls == "lancir" else avir_amd.CImageResizer(8)


def _batch(cls, r):
    """A channels_last (2, 3, H, W) uint8 tensor of the row's first planes."""
    import torch
    sw, sh = r["geom"][:2]
    src = np.stack([source_plane(cls, r, i) for i in range(6)])
    nhwc = np.ascontiguousarray(src.reshape(2, 3, sh, sw).transpose(0, 2, 3, 1))
    x = torch.from_numpy(nhwc).to("cuda:0").permute(0, 3, 1, 2)
    assert not x.is_contiguous()
    assert x.is_contiguous(memory_format=torch.channels_last)
    return x


@pytest.mark.parametrize("cls", ["lancir", "avir"])
def test_python_channels_last(cls):
    import torch
    r = case_row(cls, "dn3", planes=6)
    nw, nh = r["geom"][2:]
    x = _batch(cls, r)
    R = _resizer(cls)
    got = R.resize_planes(x, nw, nh)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 3, nh, nw)
    assert got.is_contiguous(memory_format=torch.channels_last)
    g = got.cpu().numpy().reshape(6, nh, nw)
    for i in range(6):
        D16.same(g[i], cases_of(cls).expected(r, i), "u8", "plane %d" % i)
    # out=: a channels_last float32 tensor
    rf = dict(r, tout="f32", bits=16)
    out = torch.full((2, 3, nh, nw), -1.0, device="cuda:0").contiguous(
        memory_format=torch.channels_last)
    ret = R.resize_planes(x, nw, nh, out=out)
    torch.cuda.synchronize()
    assert ret is out
    g = out.cpu().numpy().reshape(6, nh, nw)
    for i in range(6):
        D16.same(np.ascontiguousarray(g[i]), cases_of(cls).expected(rf, i),
                 "f32", "out= plane %d" % i)
    # x[:, 1:3]: no single plane stride
    got = R.resize_planes(x[:, 1:3], nw, nh)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    for b in range(2):
        for c in range(2):
            D16.same(np.ascontiguousarray(g[b, c]),
                     cases_of(cls).expected(r, b * 3 + 1 + c), "u8",
                     "slice %d %d" % (b, c))


@pytest.mark.parametrize("cls", ["lancir", "avir"])
def test_python_list_of_tensors_other_stream(cls):
    """A list of separately allocated frames in, a list of planes of one HWC
    tensor out, on a non-default stream."""
    import torch
    r = case_row(cls, "dn3")
    sw, sh, nw, nh = r["geom"]
    src = [torch.from_numpy(np.array(source_plane(cls, r, i))).to("cuda:0")
           for i in range(3)]
    out = torch.full((nh, nw, 3), GUARD, dtype=torch.uint8, device="cuda:0")
    R = _resizer(cls)
    s = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        if cls == "lancir":
            rc = R.resizePlanes(src, sw, sh, [out[:, :, c] for c in range(3)],
                                nw, nh, 3)
            assert rc == nh
        else:
            R.resizePlanes(src, sw, sh, 0, [out[:, :, c] for c in range(3)],
                           nw, nh, 3)
    s.synchronize()
    g = out.cpu().numpy()
    for i in range(3):
        D16.same(np.ascontiguousarray(g[:, :, i]),
                 cases_of(cls).expected(r, i), "u8", "plane %d" % i)
