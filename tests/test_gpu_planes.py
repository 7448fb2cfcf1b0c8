"""CLancIR over single-channel planes (avirhip_lancir_resize_planes, k_lancp):
every row of tests/planes_cases.py as ONE call from and into device memory
between guard bytes, against the reference's ElCount = 1 call on each plane.
Raw bytes are compared, the bar is 0 differing; every byte that is no pixel of
a result row stays a guard byte; and the AVIRHIP_VERBOSE line says which road
the call took -- k_lancp, or the per-plane road for the rows named for it and
for no other. Then the Python front end: a (2, 3, H, W) tensor, a non-default
stream, host arrays, and the cross-check against today's resizeImage.

Figures of a run (MI355X): see NOTEBOOK.md, "Planes"."""
import ctypes as C
import re
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import planes_cases as P
from tests import dnf16_cases as D16
from tests.gpass_route_cases import environment

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^(k_lancp|planes: per-plane road)\b", re.M)
TAGS = {"k_lancp": ["k_lancp"], "fallback": ["planes: per-plane road"]}


@pytest.fixture(scope="module")
def lancir():
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    h = C.c_void_p()
    abi.check(lib.avirhip_lancir_create(C.byref(h)), "lancir_create")
    yield lib, h
    lib.avirhip_lancir_destroy(h)


@pytest.mark.parametrize("name", P.NAMES)
def test_row(name, lancir, capfd):
    import torch
    lib, h = lancir
    r = P.row(name)
    n = r["planes"]
    keep_s, sptr = P.device_side(r, "src", P.sources(r)[:n])
    keep_d, dptr = P.device_side(r, "dst", None)
    with environment({"AVIRHIP_VERBOSE": "1"}):
        capfd.readouterr()
        rc = P.call(lib, h, r, sptr, dptr)
        torch.cuda.synchronize()
        lines = LINE.findall(capfd.readouterr().err)
    print(name, rc, lines)
    assert rc == r["geom"][3], (rc, lib.avirhip_last_error())
    P.compare(r, P.read_back(r, keep_d), name)
    assert lines == TAGS[P.road(r)], (name, lines)
    if name not in P.FALLBACK_MAY:
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


@pytest.mark.parametrize("name", P.CROSS)
def test_equals_todays_road(name):
    """Each result plane equals CLancIR.resizeImage( plane, ElCount = 1 ) of
    the same library, word for word."""
    import torch
    r = P.row(name)
    sw, sh, nw, nh = r["geom"]
    n, tin, tout = r["planes"], r["tin"], r["tout"]
    L = avir_amd.CLancIR()
    src = _to_torch(P.sources(r)[:n], tin)
    odt = _to_torch(np.zeros(1, P.T[tout][1]), tout).dtype
    got = L.resize_planes(src, nw, nh, out_dtype=odt, aParams=P.params(r))
    for i in range(n):
        one = torch.empty((nh, nw), dtype=odt, device="cuda:0")
        assert L.resizeImage(src[i].contiguous(), sw, sh, one, nw, nh, 1,
                             P.params(r)) == nh
        torch.cuda.synchronize()
        D16.same(_from_torch(got[i], tout), _from_torch(one, tout), tout,
                 "%s plane %d against resizeImage" % (name, i))
        D16.same(_from_torch(got[i], tout), P.expected(r, i), tout,
                 "%s plane %d against the reference" % (name, i))


def test_batch_tensor():
    """A (2, 3, H, W) tensor: six planes through resize_planes."""
    import torch
    r = dict(P.row("planes5_packed"), planes=6)
    sw, sh, nw, nh = r["geom"]
    src = _to_torch(P.sources(r)[:6].reshape(2, 3, sh, sw), "u8")
    got = avir_amd.CLancIR().resize_planes(src, nw, nh)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 3, nh, nw)
    g = got.cpu().numpy().reshape(6, nh, nw)
    for i in range(6):
        D16.same(g[i], P.expected(r, i), "u8", "batch plane %d" % i)


def test_other_stream():
    import torch
    r = P.row(P.STREAM_ROW)
    sw, sh, nw, nh = r["geom"]
    n = r["planes"]
    s = torch.cuda.Stream(device="cuda:0")
    src = _to_torch(P.sources(r)[:n], r["tin"])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = avir_amd.CLancIR().resize_planes(src, nw, nh)
    s.synchronize()
    for i in range(n):
        D16.same(got[i].cpu().numpy(), P.expected(r, i), r["tout"],
                 "stream plane %d" % i)


def test_host_arrays():
    r = P.row(P.NUMPY_ROW)
    sw, sh, nw, nh = r["geom"]
    n = r["planes"]
    src = np.ascontiguousarray(P.sources(r)[:n])
    got = avir_amd.CLancIR().resize_planes(src, nw, nh)
    assert got.shape == (n, nh, nw)
    for i in range(n):
        D16.same(got[i], P.expected(r, i), r["tout"], "host plane %d" % i)
    # rows and planes apart, guards in between: only the rows are written
    q = dict(r, gap=7, npad=3, spad=2)
    sreg = P.regions(q, "src", P.sources(q)[:n])[0][1]
    dreg = P.regions(q, "dst", None)[0][1]
    rc = avir_amd.CLancIR().resizePlanes(
        sreg[P.FRONT:], sw, sh, dreg[P.FRONT:], nw, nh, n,
        P.side(q, "src")[3], P.side(q, "dst")[3], P.params(q))
    assert rc == nh
    P.compare(q, [dreg], "host planes with padding")
