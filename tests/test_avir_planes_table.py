"""tests/avir_planes_cases.py is consistent (host only): every row is in the
class the planner answers for it, the seam rows follow the tile read from
avirp.hip, the LDS formula restated from avirp.hip's constants predicts the
kernel for every row outside FALLBACK_MAY and for every class, the new ABI
symbol, and the parameter errors and the zero-sized source of the planar
call, which need no device."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from avir_amd import abi
from tests import avir_planes_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_unique():
    assert len(set(A.NAMES)) == len(A.NAMES)
    assert set(A.FALLBACK_MAY) <= set(A.NAMES)
    assert A.FALLBACK_MAY == ["long_kernel", "f64", "odd_base", "gamma_u8",
                              "errd_u8", "fp4"]
    assert set(A.CROSS) <= set(A.NAMES)
    for r in A.ROWS:
        if r["road"] == "fallback":
            assert r["name"] in A.FALLBACK_MAY + A.DECLINED, r["name"]


@pytest.mark.parametrize("name", A.CLASS_ROWS)
def test_class(name):
    """The row's class is the planner's answer for one channel."""
    r = A.row(name)
    got = A.steps(r)
    print(name, r["geom"], got)
    want = A.GEOMS[name][1]
    if want is not None:
        assert got == want
    h, v = got.split(" | ")
    sw, sh, nw, nh = r["geom"]
    if name in A.FIRST_FIR:
        ff = A.first_fir(r)
        for got_ax, want_ax in zip(ff, A.FIRST_FIR[name]):
            if want_ax is not None:
                assert got_ax == want_ax, (name, ff)
    if name in ("mix_du", "mix_ud"):
        assert (nw < sw) != (nh < sh)
        # one axis of each kind: filtered upsample, zero-stuffed downsizing
        assert sorted("UP_FILTERED" in a for a in (h, v)) == [False, True]
    if name == "tiny":
        assert max(sw, nw) < A.TW and max(sh, nh) < A.TR
    if name in ("dn_zs", "dn_near1"):
        assert 1 < sw / nw < 2 and h.startswith("UP_ZEROSTUFF RESIZE2")
    # every chain lowers to at most three ops an axis
    for a in (h, v):
        assert len([s for s in a.split() if s != "UP_ZEROSTUFF"]) <= 3


def test_all_three_op_types_and_views():
    kinds = set()
    for name in A.CLASS_ROWS:
        kinds |= set(re.sub(r"[\d()/]", "", A.steps(A.row(name))).split())
    assert {"FIR", "UP_ZEROSTUFF", "UP_FILTERED", "RESIZE", "RESIZE"} <= kinds
    assert "RESIZE" in kinds


def test_seams_follow_the_source():
    k = A.parse_constants(os.path.join(ROOT, "avir_amd", "csrc"))
    tw, tr = k["AP_TW"], k["AP_TR"]
    assert k["CAND"][0] == (tw, tr)
    for src, tag in ((A.SEAM_UP, "up"), (A.SEAM_DN, "dn")):
        sizes = {A.row(n)["geom"][2:] for n in A.SEAM_ROWS
                 if n.startswith("seam_" + tag)}
        assert sizes == {(w, h) for w in (tw - 1, tw, tw + 1, 2 * tw + 1)
                         for h in (tr - 1, tr, tr + 1, 2 * tr + 1)}
        for n in A.SEAM_ROWS:
            if n.startswith("seam_" + tag):
                assert A.row(n)["geom"][:2] == src
    assert (140, 80, tw - 1, tr - 1) in [A.row(n)["geom"] for n in A.SEAM_ROWS]


def test_crop_rows():
    for n, cls in (("crop_zs", "UP_ZEROSTUFF"), ("crop_upf", "UP_FILTERED"),
                   ("crop_dn", "RESIZE(")):
        r = A.row(n)
        assert r["k"] > 0 and r["ox"] != 0 and r["oy"] != 0
        assert cls in A.steps(r), (n, A.steps(r))


def test_types_counts_layout():
    for g in A.TYPE_GEOMS:
        for a, b in A.PAIRS:
            assert "type_%s_%s_%s" % (g, a, b) in A.NAMES
    assert len(A.PAIRS) == 11
    assert {A.row("planes%d_packed" % n)["planes"] for n in (1, 3, 5, 6)} == {
        1, 3, 5, 6}
    r = A.row("planes3_gap7")
    assert A.side(r, "src")[4] == 37 * 23 + 7
    assert (A.side(r, "dst")[4] * A.side(r, "dst")[5]) % 2 == 1
    r = A.row("scanline_pad")
    assert A.side(r, "src")[2] == r["geom"][0] + 3
    assert A.side(r, "dst")[2] == r["geom"][2]      # result rows are tight
    r = A.row("far_planes")
    assert A.side(r, "src")[4] * A.side(r, "src")[5] == 2 ** 31 + 64
    assert A.side(r, "dst")[4] * A.side(r, "dst")[5] == 2 ** 31 + 64
    r = A.row("many_planes")
    assert r["planes"] == 70000 > 65535 and A.DISTINCT == 6
    assert A.row("res16_u16")["bits"] == 16
    # bit-depth truncation: ResBitDepth under the element's width
    for n in ("trunc_u8", "trunc_f32_u8"):
        with A.desc(A.row(n)) as d:
            assert d.tr_mul != 1.0, n
    with A.desc(A.row("upf_both")) as d:
        assert d.tr_mul == 1.0


def test_road_prediction():
    """No row outside FALLBACK_MAY is predicted to fall back, every class
    has a row predicted on the kernel, and the LDS formula stays within
    avirp.hip's bounds."""
    k = A.parse_constants()
    assert k["AP_LDS_PREF"] <= 65536 and k["AP_LDS_MAX"] <= 150 * 1024
    for r in A.ROWS:
        if r["name"] in A.FALLBACK_MAY + A.DECLINED and r["road"] == "fallback":
            continue
        lds, tile = A.lds_of(r)
        print(r["name"], r["geom"], lds, tile)
        if r["name"] not in A.FALLBACK_MAY:
            assert A.road(r) == "k_avirp", r["name"]
            assert lds is not None and lds <= k["AP_LDS_MAX"], r["name"]
            assert tile in k["CAND"]
    on_kernel = {r["cls"] for r in A.ROWS if A.road(r) == "k_avirp"}
    assert set(A.CLASS_ROWS) - {"long_kernel"} <= on_kernel
    # a row on each side of the measured threshold, and no other row above it
    assert A.pixels(A.row("px_at")) == k["AP_MAX_PIXELS"]
    assert A.pixels(A.row("px_above")) > k["AP_MAX_PIXELS"]
    assert A.lds_of(A.row("px_above"))[0] is not None   # (it is the threshold)
    assert A.DECLINED == ["px_above"]
    for r in A.ROWS:
        if r["name"] not in A.DECLINED:
            assert A.pixels(r) <= k["AP_MAX_PIXELS"], r["name"]
    # the first tile wherever it stays within the preferred bound
    lds, tile = A.lds_of(A.row("upf_both"))
    assert tile == (k["AP_TW"], k["AP_TR"]) and lds <= k["AP_LDS_PREF"]
    # a decimating first filter leaves it
    assert A.lds_of(A.row("dn_rf4"))[1] != (k["AP_TW"], k["AP_TR"])
    assert A.lds_of(A.row("dn_rf4"), (k["AP_TW"], k["AP_TR"]))[0] > k[
        "AP_LDS_PREF"]


# ---- the ABI ------------------------------------------------------------------

SYM = "avirhip_resizer_resize_planes"


def test_abi_symbol():
    hdr = open(os.path.join(ROOT, "include", "avirhip.h")).read()
    lib = abi.load()
    assert re.search(r"^int %s\(" % SYM, hdr, re.M)
    assert SYM in abi.PROTOTYPES
    assert getattr(lib, SYM) is not None
    assert len(abi.PROTOTYPES[SYM][1]) == 18
    # one more export than before it (44, avirhip_lancir_resize_planes the last)
    assert len(abi.PROTOTYPES) == 45
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(avirhip_[a-z_0-9]+)\s*\(", code))) == 45


def _call(lib, h, src, dst, sw, sh, nw, nh, n, sps, dps, ss=0, tin=abi.U8,
          tout=abi.U8, k=0.0):
    return lib.avirhip_resizer_resize_planes(
        h, C.c_void_p(src), abi.MEM_HOST, sw, sh, ss, C.c_void_p(dst),
        abi.MEM_HOST, nw, nh, n, sps, dps, k, None, tin, tout, None)


def _one(lib, h, src, dst, sw, sh, nw, nh, tin=abi.U8, tout=abi.U8, k=0.0):
    return lib.avirhip_resizer_resize(
        h, C.c_void_p(src), abi.MEM_HOST, sw, sh, 0, C.c_void_p(dst),
        abi.MEM_HOST, nw, nh, 1, k, None, tin, tout, None)


@pytest.fixture()
def resizer():
    lib = abi.load()
    h = C.c_void_p()
    abi.check(lib.avirhip_resizer_create(8, 0, None, C.byref(h)), "create")
    yield lib, h
    lib.avirhip_resizer_destroy(h)


def test_parameter_errors_need_no_device(resizer):
    lib, h = resizer
    src = np.zeros(3 * 8 * 8, np.uint8)
    dst = np.zeros(3 * 16 * 16, np.uint8)
    s, d = src.ctypes.data, dst.ctypes.data
    assert _call(lib, h, s, d, 8, 8, 16, 16, 0, 0, 0) == abi.EINVAL
    assert _call(lib, h, s, d, 8, 8, 16, 16, -1, 0, 0) == abi.EINVAL
    # a plane needs 64 / 256 elements
    assert _call(lib, h, s, d, 8, 8, 16, 16, 3, 63, 0) == abi.EINVAL
    assert b"plane stride" in lib.avirhip_last_error()
    assert _call(lib, h, s, d, 8, 8, 16, 16, 3, 0, 255) == abi.EINVAL
    assert _call(lib, h, s, d, 8, 8, 16, 16, 3, -64, 0) == abi.EINVAL
    assert _call(lib, h, s, d, 8, 8, 16, 16, 3, 0, -256) == abi.EINVAL
    # with a source row pitch: ( h - 1 ) * pitch + w
    assert _call(lib, h, s, d, 8, 8, 16, 16, 1, 77, 0, ss=10) == abi.EINVAL
    assert _call(lib, h, s, d, 8, 8, 16, 16, 1, 0, 0, ss=7) == abi.EINVAL
    assert b"row pitch" in lib.avirhip_last_error()
    # spans that share bytes
    both = np.zeros(3 * 16 * 16 + 64, np.uint8)
    assert _call(lib, h, both.ctypes.data, both.ctypes.data + 32, 8, 8, 16,
                 16, 3, 0, 0) == abi.EINVAL
    assert b"share bytes" in lib.avirhip_last_error()
    # no object, no plan
    assert _call(lib, None, s, d, 8, 8, 16, 16, 3, 0, 0) == abi.EINVAL
    assert lib.avirhip_resize_planes(None, C.c_void_p(s), abi.MEM_HOST, 0,
                                     C.c_void_p(d), abi.MEM_HOST, 0, 1,
                                     None) == abi.EINVAL
    # the reference's own parameter errors: what avirhip_resizer_resize returns
    for geom, kw in (((-1, 8, 16, 16), {}), ((8, -3, 16, 16), {}),
                     ((8, 8, -16, 16), {}), ((8, 8, 16, -1), {}),
                     ((8, 8, 16, 16), dict(tout=99)),
                     ((8, 8, 16, 16), dict(tin=abi.U32))):
        one = _one(lib, h, s, d, *geom, **kw)
        got = _call(lib, h, s, d, *(geom + (3, 0, 0)), **kw)
        print(geom, kw, one, got)
        assert one != 0 and got == one, (geom, kw, one, got)
    # a zero-sized destination is a no-op
    dst[:] = A.GUARD
    assert _call(lib, h, s, d, 8, 8, 0, 16, 3, 0, 0) == 0
    assert _call(lib, h, s, d, 8, 8, 16, 0, 3, 0, 0) == 0
    assert (dst == A.GUARD).all()


def test_zero_sized_source_host(resizer):
    """Zero-filled rows of new_w elements, plane by plane, and nothing else
    (host buffers: no device)."""
    lib, h = resizer
    src = np.zeros(16, np.uint16)
    nw, nh, stride, n = 5, 3, 22, 3
    dst = np.full(9 + (n - 1) * stride + nh * nw + 9, 0x5a5a, np.uint16)
    rc = _call(lib, h, src.ctypes.data, dst.ctypes.data + 18, 0, 4, nw, nh, n,
               0, stride, tin=abi.U16, tout=abi.U16)
    assert rc == 0
    want = np.full_like(dst, 0x5a5a)
    for i in range(n):
        want[9 + i * stride:9 + i * stride + nh * nw] = 0
    assert np.array_equal(dst, want)
    # ... tightly packed, and with the other side empty
    dst[:] = 0x5a5a
    rc = _call(lib, h, src.ctypes.data, dst.ctypes.data + 18, 4, 0, nw, nh, 2,
               0, 0, tin=abi.U16, tout=abi.U16)
    assert rc == 0
    want[:] = 0x5a5a
    want[9:9 + 2 * nh * nw] = 0
    assert np.array_equal(dst, want)


def test_cpp_front_end_compiles(tmp_path):
    """CImageResizer<>::resizeImagePlanes of include/avir_hip/avir.h, with and
    without aVars (syntax and types only: no device here)."""
    import subprocess
    src = tmp_path / "planes.cpp"
    src.write_text(
        '#include "avir.h"\n'
        'int main() {\n'
        '\tavir::CImageResizer<> R( 8 );\n'
        '\tunsigned char a[ 3 * 64 ] = { 0 };\n'
        '\tfloat b[ 3 * 256 ];\n'
        '\tavir::CImageResizerVars v;\n'
        '\tR.resizeImagePlanes( a, 8, 8, 0, b, 16, 16, 3, 0, 0, 0.0, &v );\n'
        '\tR.resizeImagePlanes( a, 8, 8, 8, b, 16, 16, 3, 64, 256, 0.5 );\n'
        '\treturn( v.ElCountIO == 1 ? 0 : 1 );\n'
        '}\n')
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include", "avir_hip"),
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)
