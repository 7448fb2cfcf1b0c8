"""bfloat16 elements, host side (no GPU): the type code and the buffer map of
the Python front end, the planner -- an AVIRHIP_BF16 call plans exactly as the
float32 call that defines it (include/avirhip.h), in every field and table
except the two type fields, with the other side float32, integer or half --
the refusal under fpclass_float4 / fpclass_def<double>, and the C++ front
ends' type maps."""
import ctypes as C
import os
import subprocess
import pytest
import avir_amd
from avir_amd import abi
from tests import helpers as H
from tests import plancmp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (sw, sh, nw, nh, ch): exact 2x, 3x down, 2x down, non-integer up and down,
# mixed axes, 1-4 channels
GEOMS = [
    (97, 61, 194, 122, 4), (160, 120, 320, 240, 3), (50, 50, 100, 100, 1),
    (300, 240, 100, 80, 4), (303, 241, 101, 80, 2), (320, 240, 160, 120, 3),
    (192, 108, 250, 140, 4), (101, 77, 333, 200, 1), (640, 480, 237, 178, 3),
    (500, 300, 412, 250, 4), (200, 90, 100, 244, 2), (64, 48, 173, 20, 4),
]


def test_type_code_and_buffer_maps():
    assert abi.BF16 == 6
    assert avir_amd.BF16 == abi.BF16
    import torch
    t = torch.zeros((4, 4, 4), dtype=torch.bfloat16)
    assert avir_amd._buf(t) == (t.data_ptr(), abi.MEM_HOST, abi.BF16, None)


def _not_types(bad):
    return [b for b in bad if not b.startswith(("in_type:", "out_type:"))]


def _avir_desc(ti, to, sw, sh, nw, nh, ch, gamma, bits=8):
    lib = abi.load()
    r = C.c_void_p()
    abi.check(lib.avirhip_resizer_create(bits, 0, None, C.byref(r)), "create")
    v = abi.Vars()
    lib.avirhip_vars_default(C.byref(v))
    v.UseSRGBGamma, v.AlphaIndex = gamma, 3
    d = C.POINTER(abi.PlanDesc)()
    abi.check(lib.avirhip_resizer_build_desc(
        r, sw, sh, 0, nw, nh, ch, 0.0, C.byref(v), ti, to, C.byref(d)),
        "build_desc")
    return r, d


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d-%dx%dx%d" % g)
@pytest.mark.parametrize("gamma", [0, 1])
def test_avir_desc_equals_float32_desc(geom, gamma):
    sw, sh, nw, nh, ch = geom
    descs = [_avir_desc(t, t, sw, sh, nw, nh, ch, gamma)
             for t in (abi.BF16, abi.F32)]
    try:
        a, b = descs[0][1].contents, descs[1][1].contents
        assert (a.in_type, a.out_type) == (abi.BF16, abi.BF16)
        assert (b.in_type, b.out_type) == (abi.F32, abi.F32)
        assert _not_types(plancmp.compare_desc(a, b)) == []
        for f in ("use_srgb_gamma", "alpha_index", "dither", "work_f64"):
            assert getattr(a, f) == getattr(b, f), f
    finally:
        for r, d in descs:
            H.free_product_desc(r, d)


@pytest.mark.parametrize("gamma", [0, 1])
@pytest.mark.parametrize("other", [abi.U8, abi.U16, abi.F32, abi.F16],
                         ids=["u8", "u16", "f32", "f16"])
def test_avir_mixed_desc_equals_float32_desc(other, gamma):
    """Each side follows its own rule: BF16 -> X plans as F32 -> X, X -> BF16
    as X -> F32 (input scale, pk_out, tr_mul), whatever X is."""
    for (ti, to), (fi, fo) in (((abi.BF16, other), (abi.F32, other)),
                               ((other, abi.BF16), (other, abi.F32))):
        r1, d1 = _avir_desc(ti, to, 192, 108, 250, 140, 3, gamma, 6)
        r2, d2 = _avir_desc(fi, fo, 192, 108, 250, 140, 3, gamma, 6)
        try:
            assert (d1.contents.in_type, d1.contents.out_type) == (ti, to)
            assert _not_types(plancmp.compare_desc(d1.contents,
                                                   d2.contents)) == []
            assert d1.contents.dither == d2.contents.dither
        finally:
            H.free_product_desc(r1, d1)
            H.free_product_desc(r2, d2)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d-%dx%dx%d" % g)
def test_lancir_desc_equals_float32_desc(geom):
    sw, sh, nw, nh, ch = geom
    lib = abi.load()
    l = C.c_void_p()
    abi.check(lib.avirhip_lancir_create(C.byref(l)), "lancir_create")
    P = abi.LancirParams()
    lib.avirhip_lancir_params_default(C.byref(P))
    P.NewSSize = nw * ch + 6
    made = []
    try:
        for ti, to in ((abi.BF16, abi.BF16), (abi.F32, abi.F32),
                       (abi.U8, abi.BF16), (abi.U8, abi.F32),
                       (abi.BF16, abi.U16), (abi.F32, abi.U16),
                       (abi.BF16, abi.F16), (abi.F32, abi.F16),
                       (abi.F16, abi.BF16), (abi.F16, abi.F32),
                       (abi.BF16, abi.F32), (abi.F32, abi.F32)):
            d = C.POINTER(abi.LancirDesc)()
            abi.check(lib.avirhip_lancir_build_desc(
                l, sw, sh, nw, nh, ch, C.byref(P), ti, to, C.byref(d)),
                "lancir_build_desc")
            made.append(d)
        for i in range(0, len(made), 2):
            assert _not_types(plancmp.compare_lancir_desc(
                made[i].contents, made[i + 1].contents)) == []
        assert made[0].contents.in_type == abi.BF16
        assert made[0].contents.out_type == abi.BF16
    finally:
        for d in made:
            lib.avirhip_lancir_desc_free(d)
        lib.avirhip_lancir_destroy(l)


@pytest.mark.parametrize("fpclass", [4, abi.FPCLASS_DOUBLE])
@pytest.mark.parametrize("types", [(abi.BF16, abi.BF16), (abi.BF16, abi.U8),
                                   (abi.F32, abi.BF16)])
def test_other_fpclasses_refuse_bf16(fpclass, types):
    lib = abi.load()
    r = C.c_void_p()
    abi.check(lib.avirhip_resizer_create(8, 0, None, C.byref(r)), "create")
    try:
        abi.check(lib.avirhip_resizer_set_fpclass(r, fpclass), "set_fpclass")
        d = C.POINTER(abi.PlanDesc)()
        rc = lib.avirhip_resizer_build_desc(r, 64, 48, 0, 128, 96, 4, 0.0, None,
                                            types[0], types[1], C.byref(d))
        assert rc == abi.EUNSUPPORTED
        assert len(lib.avirhip_last_error()) > 0
        # float32 keeps working on the same object
        abi.check(lib.avirhip_resizer_build_desc(
            r, 64, 48, 0, 128, 96, 4, 0.0, None, abi.F32, abi.F32,
            C.byref(d)), "build_desc")
        lib.avirhip_plan_desc_free(d)
    finally:
        lib.avirhip_resizer_destroy(r)


def test_type_codes_beyond_bf16_stay_invalid():
    lib = abi.load()
    r = C.c_void_p()
    abi.check(lib.avirhip_resizer_create(8, 0, None, C.byref(r)), "create")
    try:
        d = C.POINTER(abi.PlanDesc)()
        assert lib.avirhip_resizer_build_desc(
            r, 64, 48, 0, 128, 96, 4, 0.0, None, 7, abi.F32,
            C.byref(d)) == abi.EINVAL
        assert lib.avirhip_resizer_build_desc(
            r, 64, 48, 0, 128, 96, 4, 0.0, None, abi.F32, 7,
            C.byref(d)) == abi.EINVAL
    finally:
        lib.avirhip_resizer_destroy(r)


def test_band_source_rows_accept_bf16():
    ir = avir_amd.CImageResizer(8)
    assert ir.band_source_rows(97, 61, 194, 122, 4, 10, 50, in_type=abi.BF16,
                               out_type=abi.BF16) == \
        ir.band_source_rows(97, 61, 194, 122, 4, 10, 50)
    lr = avir_amd.CLancIR()
    assert lr.band_source_rows(97, 61, 194, 122, 4, 10, 50, in_type=abi.BF16,
                               out_type=abi.BF16) == \
        lr.band_source_rows(97, 61, 194, 122, 4, 10, 50)


def test_bf16_program_compiles_and_links(tmp_path):
    """resizeImage< __bf16, __bf16 > through the drop-in C++ headers (compile
    and link only: running it needs the GPU)."""
    lib = os.path.join(ROOT, "avir_amd", "lib")
    exe = str(tmp_path / "bf16_frontend")
    # (a host compiler that knows __bf16 in C++: the HIP toolchain's clang)
    cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([cxx, "-O1", "-std=c++11",
                    "-I" + os.path.join(ROOT, "include", "avir_hip"),
                    os.path.join(ROOT, "tests", "cpp", "bf16_frontend.cpp"),
                    "-L" + lib, "-lavirhip", "-Wl,-rpath," + lib,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    assert os.path.exists(exe)
