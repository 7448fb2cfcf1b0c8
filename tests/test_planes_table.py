"""tests/planes_cases.py is consistent (host only): every tap class, every
new_w % 4 residue, the seam rows at the tile read from lancp.hip, rounding rows
that can tell the two rounding rules apart, the two ABI symbols, and the
parameter errors of the planar calls, which need no device."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from avir_amd import abi
from tests import planes_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_unique():
    assert len(set(P.NAMES)) == len(P.NAMES)
    assert set(P.FALLBACK_MAY) <= set(P.NAMES)
    assert set(P.CROSS) <= set(P.NAMES)
    for r in P.ROWS:
        if r["road"] != "k_lancp":
            assert r["name"] in P.FALLBACK_MAY, r["name"]


@pytest.mark.parametrize("name", sorted(P.TAPS))
def test_tap_classes(name):
    (klx, _), (kly, _) = P.axes(P.row(name))
    assert (klx, kly) == P.TAPS[name]


def test_tap_rows():
    want = {"tap_up", "tap_dn2", "tap_dn15", "tap_dn3", "tap_up_la2",
            "tap_down_x_up_y", "tap_up_x_down_y", "tap_crop", "tap_tiny"}
    assert want == set(P.TAP_ROWS)
    sw, sh, nw, nh = P.row("tap_down_x_up_y")["geom"]
    assert nw < sw and nh > sh
    sw, sh, nw, nh = P.row("tap_up_x_down_y")["geom"]
    assert nw > sw and nh < sh
    assert P.row("tap_crop")["par"][1:] != (0.0, 0.0, 0.0, 0.0)
    sw, sh, nw, nh = P.row("tap_tiny")["geom"]
    assert max(sw, nw) < P.TW and max(sh, nh) < P.TR
    # la = 2: 4 taps, the loop over further groups of four never runs
    assert P.TAPS["tap_up_la2"] == (4, 4)
    assert P.TAPS["tap_up"][0] % 4 == 2 and P.TAPS["tap_dn2"][0] % 4 == 0


def test_residues():
    res = {r["geom"][2] % 4 for r in P.ROWS
           if r["tout"] in ("u8", "u16") and r["road"] == "k_lancp"}
    assert res == {0, 1, 2, 3}


def test_seams_follow_the_source():
    k = P.parse_constants(os.path.join(ROOT, "avir_amd", "csrc"))
    tw, tr = k["LP_TW"], k["LP_TR"]
    sizes = {(P.row(n)["geom"][2], P.row(n)["geom"][3]) for n, _, _ in P.SEAMS}
    assert {(tw - 1, tr - 1), (tw, tr), (tw + 1, tr + 1)} <= sizes
    assert any(w > 2 * tw and h > 2 * tr for w, h in sizes)
    # more than one block in the plane-count rows, too
    assert P.UP[3] > 2 * tr


def test_types_and_counts():
    for g, _ in P.TYPE_GEOMS:
        for a, b in P.PAIRS:
            assert "type_%s_%s_%s" % (g, a, b) in P.NAMES
    assert len(P.PAIRS) == 11
    for n in (1, 3, 5):
        for way in ("packed", "gap7", "pitch1", "pitch2", "pitch3"):
            assert "planes%d_%s" % (n, way) in P.NAMES
    # 7 elements of padding: odd byte bases for uint8 result planes (61 x 40
    # + 7); the source planes' 37 x 23 + 7 is even
    r = P.row("planes3_gap7")
    assert P.side(r, "src")[4] == 37 * 23 + 7
    assert (P.side(r, "dst")[4] * P.side(r, "dst")[5]) % 2 == 1
    r = P.row("far_planes")
    assert P.side(r, "src")[4] * P.side(r, "src")[5] == 2 ** 31 + 64
    assert P.side(r, "dst")[4] * P.side(r, "dst")[5] == 2 ** 31 + 64


def test_declined_classes():
    k = P.parse_constants()
    assert P.lds_of(P.row("long_kernel")) > k["LP_LDS"]
    (klx, _), (kly, _) = P.axes(P.row("k16"))
    assert (klx, kly) == (96, 96)
    assert P.road(P.row("k16")) in ("k_lancp", "fallback")
    for r in P.ROWS:
        if r["road"] == "k_lancp":
            assert P.lds_of(r) <= k["LP_LDS"] or r["far"], r["name"]


@pytest.mark.parametrize("i", range(len(P.ROUNDING)))
def test_rounding_rows_discriminate(i):
    geom, n, groups, tail = P.ROUNDING[i]
    r = P.row("round_%dx%d_n%d" % (geom[2], geom[3], n))
    got = P.wrong_rule_counts(r)
    print(r["name"], got)
    assert got[0] > 0 and got[1] > 0, (r["name"], got)
    assert got == (groups, tail), (r["name"], got)


# ---- the ABI ------------------------------------------------------------------

SYMS = ["avirhip_resize_planes", "avirhip_lancir_resize_planes"]


def test_abi_symbols():
    hdr = open(os.path.join(ROOT, "include", "avirhip.h")).read()
    lib = abi.load()
    for s in SYMS:
        assert re.search(r"^int %s\(" % s, hdr, re.M), s
        assert s in abi.PROTOTYPES, s
        assert getattr(lib, s) is not None
    assert len(abi.PROTOTYPES["avirhip_resize_planes"][1]) == 9
    assert len(abi.PROTOTYPES["avirhip_lancir_resize_planes"][1]) == 16


def _call(lib, h, src, dst, sw, sh, nw, nh, n, sps, dps, p=None):
    return lib.avirhip_lancir_resize_planes(
        h, C.c_void_p(src), abi.MEM_HOST, sw, sh, C.c_void_p(dst), abi.MEM_HOST,
        nw, nh, n, sps, dps, C.byref(p) if p is not None else None, abi.U8,
        abi.U8, None)


def test_parameter_errors_need_no_device():
    import avir_amd
    lib = abi.load()
    h = C.c_void_p()
    abi.check(lib.avirhip_lancir_create(C.byref(h)), "lancir_create")
    try:
        src = np.zeros(3 * 8 * 8, np.uint8)
        dst = np.zeros(3 * 16 * 16, np.uint8)
        s, d = src.ctypes.data, dst.ctypes.data
        assert _call(lib, h, s, d, 8, 8, 16, 16, 0, 0, 0) == abi.EINVAL
        # a plane needs 64 / 256 elements
        assert _call(lib, h, s, d, 8, 8, 16, 16, 3, 63, 0) == abi.EINVAL
        assert b"plane stride" in lib.avirhip_last_error()
        assert _call(lib, h, s, d, 8, 8, 16, 16, 3, 0, 255) == abi.EINVAL
        assert _call(lib, h, s, d, 8, 8, 16, 16, 3, -64, 0) == abi.EINVAL
        # with row pitches: ( h - 1 ) * pitch + w
        p = avir_amd.CLancIRParams(10, 20)
        assert _call(lib, h, s, d, 8, 8, 16, 16, 1, 77, 0, p) == abi.EINVAL
        assert _call(lib, h, s, d, 8, 8, 16, 16, 1, 0, 315, p) == abi.EINVAL
        # the reference's parameter errors return 0
        assert _call(lib, h, s, s, 8, 8, 16, 16, 3, 0, 0) == 0
        p = avir_amd.CLancIRParams()
        p.la = 1.5
        assert _call(lib, h, s, d, 8, 8, 16, 16, 3, 0, 0, p) == 0
        assert _call(lib, h, s, d, 8, 8, 0, 16, 3, 0, 0) == 0
        assert _call(lib, h, s, d, -1, 8, 16, 16, 3, 0, 0) == 0
        # spans that share bytes
        both = np.zeros(3 * 16 * 16 + 64, np.uint8)
        assert _call(lib, h, both.ctypes.data, both.ctypes.data + 32, 8, 8, 16,
                     16, 3, 0, 0) == abi.EINVAL
        assert b"share bytes" in lib.avirhip_last_error()
        # plan level: no plan
        assert lib.avirhip_resize_planes(None, C.c_void_p(s), abi.MEM_HOST, 0,
                                         C.c_void_p(d), abi.MEM_HOST, 0, 1,
                                         None) == abi.EINVAL
    finally:
        lib.avirhip_lancir_destroy(h)


def test_zero_sized_source_host():
    """Zero-filled rows, plane by plane, and nothing else (host buffers: no
    device)."""
    import avir_amd
    lib = abi.load()
    h = C.c_void_p()
    abi.check(lib.avirhip_lancir_create(C.byref(h)), "lancir_create")
    try:
        src = np.zeros(16, np.uint8)
        nw, nh, pitch, stride, n = 5, 3, 7, 30, 2
        dst = np.full((n - 1) * stride + (nh - 1) * pitch + nw + 9, P.GUARD,
                      np.uint8)
        p = avir_amd.CLancIRParams(0, pitch)
        rc = _call(lib, h, src.ctypes.data, dst.ctypes.data, 0, 4, nw, nh, n, 0,
                   stride, p)
        assert rc == nh
        want = np.full_like(dst, P.GUARD)
        for i in range(n):
            for y in range(nh):
                o = i * stride + y * pitch
                want[o:o + nw] = 0
        assert np.array_equal(dst, want)
    finally:
        lib.avirhip_lancir_destroy(h)
