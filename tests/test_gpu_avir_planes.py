"""CImageResizer over single-channel planes (avirhip_resizer_resize_planes,
k_avirp): every row of tests/avir_planes_cases.py as ONE call from and into
device memory between guard bytes, against the reference's ElCountIO = 1 call
on each plane. Raw bytes are compared, the bar is 0 differing; every byte that
is no pixel of a result row stays a guard byte; and the AVIRHIP_VERBOSE line
says which road the call took -- k_avirp, or the per-plane road for the rows
named for it and for no other. Then the plan level, the Python front end (a
(2, 3, H, W) tensor, a non-default stream, host arrays) and the cross-check
against today's resizeImage.

Figures of a run (MI355X): see NOTEBOOK.md, "CImageResizer planes"."""
import ctypes as C
import re
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import avir_planes_cases as A
from tests import dnf16_cases as D16
from tests.gpass_route_cases import environment

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^(k_avirp|planes: per-plane road)\b", re.M)
TAGS = {"k_avirp": ["k_avirp"], "fallback": ["planes: per-plane road"]}


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    return lib


@pytest.mark.parametrize("name", A.NAMES)
def test_row(name, lib, capfd):
    import torch
    r = A.row(name)
    keep_s, sptr = A.device_side(r, "src", A.source_planes(r))
    keep_d, dptr = A.device_side(r, "dst", None)
    h = A.resizer(lib, r)
    try:
        with environment({"AVIRHIP_VERBOSE": "1"}):
            capfd.readouterr()
            rc = A.call(lib, h, r, sptr, dptr)
            torch.cuda.synchronize()
            lines = LINE.findall(capfd.readouterr().err)
    finally:
        lib.avirhip_resizer_destroy(h)
    print(name, rc, lines)
    assert rc == 0, (rc, lib.avirhip_last_error())
    A.compare(r, A.read_back(r, keep_d), name)
    assert lines == TAGS[A.road(r)], (name, lines)
    if name not in A.FALLBACK_MAY + A.DECLINED:
        assert "planes: per-plane road" not in lines


def _to_torch(a, t):
    import torch
    a = np.array(a)   # (a writable copy: the shared sources are read-only)
    if t == "bf16":
        return torch.from_numpy(a.view(np.int16)).to("cuda:0").view(
            torch.bfloat16)
    return torch.from_numpy(a).to("cuda:0")


def _from_torch(x, t):
    import torch
    if t == "bf16":
        x = x.view(torch.int16)
    a = x.cpu().numpy()
    return a.view(np.uint16) if t == "bf16" else a


@pytest.mark.parametrize("name", A.CROSS)
def test_equals_todays_road(name):
    """Each result plane equals CImageResizer.resizeImage( plane,
    ElCountIO = 1 ) of the same library, word for word."""
    import torch
    r = A.row(name)
    sw, sh, nw, nh = r["geom"]
    n, tin, tout = r["planes"], r["tin"], r["tout"]
    R = avir_amd.CImageResizer(r["bits"])
    src = _to_torch(np.stack(A.source_planes(r)), tin)
    odt = _to_torch(np.zeros(1, A.T[tout][1]), tout).dtype
    got = R.resize_planes(src, nw, nh, out_dtype=odt)
    for i in range(n):
        one = torch.empty((nh, nw), dtype=odt, device="cuda:0")
        R.resizeImage(src[i].contiguous(), sw, sh, 0, one, nw, nh, 1, 0.0)
        torch.cuda.synchronize()
        D16.same(_from_torch(got[i], tout), _from_torch(one, tout), tout,
                 "%s plane %d against resizeImage" % (name, i))
        D16.same(_from_torch(got[i], tout), A.expected(r, i), tout,
                 "%s plane %d against the reference" % (name, i))


def test_plan_level(lib):
    """avirhip_resize_planes on a CImageResizer plan of one channel works; on
    a plan of three channels it is AVIRHIP_EUNSUPPORTED."""
    import torch
    r = A.row("dn_zs")
    sw, sh, nw, nh = r["geom"]
    n = r["planes"]
    h = A.resizer(lib, r)
    try:
        p = C.c_void_p()
        abi.check(lib.avirhip_resizer_get_plan(
            h, sw, sh, 0, nw, nh, 1, 0.0, None, abi.U8, abi.U8, C.byref(p)),
            "get_plan")
        src = _to_torch(np.stack(A.source_planes(r)), "u8")
        dst = torch.zeros((n, nh, nw), dtype=torch.uint8, device="cuda:0")
        rc = lib.avirhip_resize_planes(
            p, C.c_void_p(src.data_ptr()), abi.MEM_DEVICE, 0,
            C.c_void_p(dst.data_ptr()), abi.MEM_DEVICE, 0, n, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.avirhip_last_error()
        for i in range(n):
            D16.same(dst[i].cpu().numpy(), A.expected(r, i), "u8",
                     "plan level plane %d" % i)
        p3 = C.c_void_p()
        abi.check(lib.avirhip_resizer_get_plan(
            h, sw, sh, 0, nw, nh, 3, 0.0, None, abi.U8, abi.U8, C.byref(p3)),
            "get_plan")
        rc = lib.avirhip_resize_planes(
            p3, C.c_void_p(src.data_ptr()), abi.MEM_DEVICE, 0,
            C.c_void_p(dst.data_ptr()), abi.MEM_DEVICE, 0, 1, None)
        assert rc == abi.EUNSUPPORTED
    finally:
        lib.avirhip_resizer_destroy(h)


def test_batch_tensor():
    """A (2, 3, H, W) tensor: six planes through resize_planes."""
    import torch
    r = A.row("planes6_packed")
    sw, sh, nw, nh = r["geom"]
    src = _to_torch(A.sources(r)[:6].reshape(2, 3, sh, sw), "u8")
    got = avir_amd.CImageResizer(8).resize_planes(src, nw, nh)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 3, nh, nw)
    g = got.cpu().numpy().reshape(6, nh, nw)
    for i in range(6):
        D16.same(g[i], A.expected(r, i), "u8", "batch plane %d" % i)


def test_other_stream():
    import torch
    r = A.row(A.STREAM_ROW)
    sw, sh, nw, nh = r["geom"]
    n = r["planes"]
    s = torch.cuda.Stream(device="cuda:0")
    src = _to_torch(np.stack(A.source_planes(r)), r["tin"])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = avir_amd.CImageResizer(8).resize_planes(src, nw, nh)
    s.synchronize()
    for i in range(n):
        D16.same(got[i].cpu().numpy(), A.expected(r, i), r["tout"],
                 "stream plane %d" % i)


def test_host_arrays():
    r = A.row(A.NUMPY_ROW)
    sw, sh, nw, nh = r["geom"]
    n = r["planes"]
    src = np.ascontiguousarray(np.stack(A.source_planes(r)))
    v = avir_amd.CImageResizerVars()
    got = avir_amd.CImageResizer(8).resize_planes(src, nw, nh, aVars=v)
    assert got.shape == (n, nh, nw)
    for i in range(n):
        D16.same(got[i], A.expected(r, i), r["tout"], "host plane %d" % i)
    # the caller's fields of aVars are what the one-channel call leaves
    w = avir_amd.CImageResizerVars()
    one = np.empty((nh, nw), np.uint8)
    avir_amd.CImageResizer(8).resizeImage(src[0], sw, sh, 0, one, nw, nh, 1,
                                          0.0, w)
    assert bytes(v) == bytes(w)
    D16.same(got[0], one, "u8", "host plane 0 against resizeImage")
    # rows and planes apart, guards in between: only the rows are written
    q = dict(r, gap=7, spad=2)
    sreg = A.regions(q, "src", A.source_planes(q))[0][1]
    dreg = A.regions(q, "dst", None)[0][1]
    avir_amd.CImageResizer(8).resizePlanes(
        sreg[A.FRONT:], sw, sh, sw + 2, dreg[A.FRONT:], nw, nh, n,
        A.side(q, "src")[3], A.side(q, "dst")[3])
    A.compare(q, [dreg], "host planes with padding")
