"""Plane views of the planar calls (include/avirhip.h, "Plane views"), host
only: the ABI adds a struct, a constant and a macro and no function; every
validation and overlap rule answers AVIRHIP_EINVAL with a message before any
device call, through both front ends (the plan-level call takes a plan, which
only a device can make: tests/test_gpu_views.py runs the same rules through
it); the C++ overloads compile.

The bases of these views are numbers, never memory: a call that passed
validation would go on to the device with them. So the one accepted layout,
interleaved result planes, is called only where no device exists, and must
then fail for the missing device and not for its views."""
import ctypes as C
import os
import re
import subprocess
import pytest
from avir_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEM_VIEWS, PlaneView = abi.MEM_VIEWS, abi.PlaneView   # (the feature itself)

SW, SH, NW, NH, N = 8, 8, 16, 16, 3
SRC, DST = 0x7f0000100000, 0x7f0000200000   # far apart, multiples of 8


def test_abi_struct_and_macros():
    hdr = open(os.path.join(ROOT, "include", "avirhip.h")).read()
    assert C.sizeof(PlaneView) == 24
    assert [f[0] for f in PlaneView._fields_] == ["base", "row_pitch",
                                                  "elem_stride"]
    assert PlaneView.row_pitch.offset == 8 and PlaneView.elem_stride.offset == 16
    m = re.search(r"typedef struct avirhip_plane_view \{(.*?)\} "
                  r"avirhip_plane_view;", hdr, re.S)
    assert m, "include/avirhip.h: no avirhip_plane_view"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\S+)\s*;", body) == ["base", "row_pitch",
                                              "elem_stride"]
    assert re.search(r"^#define AVIRHIP_MEM_VIEWS 3\b", hdr, re.M)
    assert re.search(r"^#define AVIRHIP_HAS_VIEWS 1\b", hdr, re.M)
    assert MEM_VIEWS == 3
    # no new export
    assert len(abi.PROTOTYPES) == 45
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(avirhip_[a-z_0-9]+)\s*\(", code))) == 45


def views(rows):
    a = (PlaneView * len(rows))()
    for v, (base, pitch, stride) in zip(a, rows):
        v.base, v.row_pitch, v.elem_stride = base, pitch, stride
    return a


def hwc(base, w, e=3, es=1):
    """The planes of one interleaved image: { base + c, w * e, e }."""
    return [(base + c * es, w * e, e) for c in range(N)]


class Front(object):
    """One of the two front ends behind one call signature."""

    def __init__(self, kind):
        self.kind, self.lib, self.h = kind, abi.load(), C.c_void_p()
        if kind == "lancir":
            abi.check(self.lib.avirhip_lancir_create(C.byref(self.h)), "create")
        else:
            abi.check(self.lib.avirhip_resizer_create(8, 0, None,
                                                      C.byref(self.h)), "create")

    def close(self):
        if self.kind == "lancir":
            self.lib.avirhip_lancir_destroy(self.h)
        else:
            self.lib.avirhip_resizer_destroy(self.h)

    def call(self, src, dst, sps=0, dps=0, tin=abi.U8, tout=abi.U8,
             geom=(SW, SH, NW, NH), n=N):
        """src / dst: a list of view rows, or (address, mem kind)."""
        keep = []

        def side(x):
            if isinstance(x, list):
                keep.append(views(x))
                return C.cast(keep[-1], C.c_void_p), MEM_VIEWS
            return C.c_void_p(x[0]), x[1]
        (sp, sm), (dp, dm) = side(src), side(dst)
        sw, sh, nw, nh = geom
        if self.kind == "lancir":
            return self.lib.avirhip_lancir_resize_planes(
                self.h, sp, sm, sw, sh, dp, dm, nw, nh, n, sps, dps, None,
                tin, tout, None)
        return self.lib.avirhip_resizer_resize_planes(
            self.h, sp, sm, sw, sh, 0, dp, dm, nw, nh, n, sps, dps, 0.0, None,
            tin, tout, None)

    def refused(self, word, *a, **kw):
        rc = self.call(*a, **kw)
        msg = self.lib.avirhip_last_error()
        print(self.kind, word, rc, msg)
        assert rc == abi.EINVAL, (rc, msg)
        assert word.encode() in msg, msg


@pytest.fixture(params=["lancir", "resizer"])
def front(request):
    f = Front(request.param)
    yield f
    f.close()


def test_plane_stride_with_views(front):
    front.refused("plane stride", hwc(SRC, SW), hwc(DST, NW), sps=64)
    front.refused("plane stride", hwc(SRC, SW), hwc(DST, NW), dps=256)
    front.refused("plane stride", hwc(SRC, SW), (DST, abi.MEM_DEVICE), sps=1)
    front.refused("plane stride", (SRC, abi.MEM_DEVICE), hwc(DST, NW), dps=-1)
    # the side without views keeps its own stride rule (a plane needs 256)
    front.refused("plane stride", hwc(SRC, SW), (DST, abi.MEM_DEVICE), dps=255)
    front.refused("device memory", hwc(SRC, SW), (DST, abi.MEM_HOST))
    front.refused("device memory", (SRC, abi.MEM_HOST), hwc(DST, NW))


def test_view_fields(front):
    ok_s, ok_d = hwc(SRC, SW), hwc(DST, NW)
    # a row of 8 elements at stride 3 is 22 elements long
    front.refused("row pitch", [(SRC, 21, 3)] + ok_s[1:], ok_d)
    front.refused("row pitch", ok_s, ok_d[:2] + [(DST + 2, 45, 3)])
    front.refused("row pitch", [(SRC, 7, 1)] * 3, ok_d)
    front.refused("null base", [(None, 24, 3)] + ok_s[1:], ok_d)
    front.refused("null base", ok_s, ok_d[:1] + [(None, 48, 3)] + ok_d[2:])
    front.refused("negative", [(SRC, -24, 3)] + ok_s[1:], ok_d)
    front.refused("negative", ok_s, [(DST, 48, -3)] + ok_d[1:])
    front.refused("element size", [(SRC + 1, 24, 3)] + ok_s[1:], ok_d,
                  tin=abi.U16)
    front.refused("element size", ok_s, [(DST + 2, 48, 3)] + ok_d[1:],
                  tout=abi.F32)
    front.refused("address space", [(2 ** 64 - 64, 24, 3)] + ok_s[1:], ok_d)
    front.refused("address space", ok_s, [(DST, 2 ** 62, 3)] + ok_d[1:],
                  tout=abi.F32)
    front.refused("address space", [(SRC, 0, 2 ** 62)] + ok_s[1:], ok_d,
                  tin=abi.F32)


def test_result_meets_source(front):
    # the last byte of the first source view is the first of a result view
    last = SRC + (SH - 1) * SW * 3 + (SW - 1) * 3
    front.refused("share bytes", hwc(SRC, SW), hwc(last, NW))
    front.refused("share bytes", hwc(SRC, SW), hwc(DST, NW)[:2] + [(SRC + 5, 0, 1)])
    front.refused("share bytes", hwc(SRC, SW), (SRC + 100, abi.MEM_DEVICE))
    front.refused("share bytes", (DST + 100, abi.MEM_DEVICE), hwc(DST, NW))
    # ... among many views, the source ones overlapping each other
    n = 64
    front.refused("share bytes", [(SRC + 7 * i, 0, 1) for i in range(n)],
                  [(DST + 4096 * i, 0, 1) for i in range(n - 1)] +
                  [(SRC + 7 * 40 + 3, 0, 1)], n=n)


def test_result_views_meet(front):
    s = hwc(SRC, SW)
    # bases a multiple of E apart: the same base, and E elements on
    front.refused("interleaved", s, [(DST, 48, 3), (DST + 1, 48, 3), (DST, 48, 3)])
    front.refused("interleaved", s, [(DST, 48, 3), (DST + 1, 48, 3),
                                     (DST + 3, 48, 3)])
    front.refused("interleaved", s, [(DST, 192, 12), (DST + 4, 192, 12),
                                     (DST + 48, 192, 12)], tout=abi.F32)
    # different pitches
    front.refused("interleaved", s, [(DST, 48, 3), (DST + 1, 96, 3),
                                     (DST + 2, 48, 3)])
    # different strides
    front.refused("interleaved", s, [(DST, 48, 3), (DST + 1, 48, 2),
                                     (DST + 2, 48, 3)])
    # P % E != 0
    front.refused("interleaved", s, [(DST, 49, 3), (DST + 1, 49, 3),
                                     (DST + 2, 49, 3)])
    # dense planes that meet
    front.refused("interleaved", s, [(DST, 0, 1), (DST + 255, 0, 1),
                                     (DST + 4096, 0, 1)])
    # ... found among many, listed in any order
    n = 200
    d = [(DST + 4096 * ((i * 77) % n), 0, 1) for i in range(n)]
    d[123] = (d[17][0] + 8, 0, 1)
    front.refused("interleaved", [(SRC, 0, 1)] * n, d, n=n)


def test_interleaved_result_passes_validation(front):
    """Accepted views go on to the device, so this runs only without one:
    the call must then fail for the device, not for its views."""
    if front.lib.avirhip_device_count() > 0:
        pytest.skip("a device exists: the call would reach it with these "
                    "made-up bases; tests/test_gpu_views.py runs the layouts")
    for src, dst, kw in (
            (hwc(SRC, SW), hwc(DST, NW), {}),
            ([(SRC, 24, 3)] * 3, hwc(DST, NW, 4), {}),           # RGBX
            (hwc(SRC, SW, 3, 4), hwc(DST, NW, 3, 2),
             dict(tin=abi.F32, tout=abi.U16)),
            ([(SRC, 22, 3)] * 3, [(DST + 4096 * i, 0, 1) for i in (2, 0, 1)],
             {}),
            # one row: pitches address nothing and need not agree
            (hwc(SRC, SW), [(DST, 0, 3), (DST + 1, 48, 3), (DST + 2, 59, 3)],
             dict(geom=(SW, 1, NW, 1))),
            # a dense side at a plane stride beside views
            (hwc(SRC, SW), (DST, abi.MEM_DEVICE), dict(dps=300))):
        rc = front.call(src, dst, **kw)
        msg = front.lib.avirhip_last_error()
        print(front.kind, rc, msg)
        assert rc < 0 and rc != abi.EINVAL, (rc, msg)
        assert b"planes:" not in msg


def test_plan_level_without_a_plan():
    lib = abi.load()
    v = views(hwc(SRC, SW))
    rc = lib.avirhip_resize_planes(None, C.cast(v, C.c_void_p), MEM_VIEWS, 0,
                                   C.c_void_p(DST), abi.MEM_DEVICE, 0, N, None)
    assert rc == abi.EINVAL


def test_cpp_overloads_compile(tmp_path):
    """resizeImagePlanes over avirhip_plane_view of both classes (syntax and
    types only: no device here)."""
    src = tmp_path / "views.cpp"
    src.write_text(
        '#include <stdint.h>\n'
        '#include "avir.h"\n'
        '#include "lancir.h"\n'
        '#if !defined( AVIRHIP_HAS_VIEWS ) || AVIRHIP_MEM_VIEWS != 3\n'
        '#error "no plane views"\n'
        '#endif\n'
        'int main() {\n'
        '\tstatic_assert( sizeof( avirhip_plane_view ) == 24, "size" );\n'
        '\tunsigned char* img = nullptr; float* out = nullptr;\n'
        '\tavirhip_plane_view s[ 3 ], d[ 3 ];\n'
        '\tfor( int c = 0; c < 3; c++ ) {\n'
        '\t\ts[ c ].base = img + c; s[ c ].row_pitch = 8 * 3;\n'
        '\t\ts[ c ].elem_stride = 3;\n'
        '\t\td[ c ].base = out + c * 256; d[ c ].row_pitch = 0;\n'
        '\t\td[ c ].elem_stride = 1; }\n'
        '\tavir::CImageResizer<> R( 8 );\n'
        '\tavir::CImageResizerVars v;\n'
        '\tR.resizeImagePlanes< uint8_t, float >( s, 8, 8, d, 16, 16, 3, 0.0 );\n'
        '\tR.resizeImagePlanes< uint8_t, float >( s, 8, 8, d, 16, 16, 3, 0.5,\n'
        '\t\t&v, nullptr );\n'
        '\tavir::CLancIR L;\n'
        '\tavir::CLancIRParams p;\n'
        '\tint rc = L.resizeImagePlanes< uint8_t, float >( s, 8, 8, d, 16, 16,\n'
        '\t\t3 );\n'
        '\trc += L.resizeImagePlanes< uint8_t, float >( s, 8, 8, d, 16, 16, 3,\n'
        '\t\t&p, nullptr );\n'
        '\t// the dense overloads still resolve\n'
        '\tR.resizeImagePlanes( img, 8, 8, 0, out, 16, 16, 3, 0, 0, 0.0 );\n'
        '\trc += L.resizeImagePlanes( img, 8, 8, out, 16, 16, 3 );\n'
        '\treturn( rc );\n'
        '}\n')
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only",
                    "-I" + os.path.join(ROOT, "include", "avir_hip"),
                    "-I" + os.path.join(ROOT, "include"), str(src)], check=True)
