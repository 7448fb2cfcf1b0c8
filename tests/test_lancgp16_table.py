"""Host-only checks of the inputs of tests/test_gpu_lancgp16.py
(tests/lancgp16_cases.py): a half / bfloat16 CLancIR description is the float32
one but for the type fields, the shapes have the tap counts they were chosen
for, and the special-value frames produce, with the reference alone, every
class of result the GPU test is there to compare."""
import ctypes as C
import math
import numpy as np
import pytest
from avir_amd import abi
from tests import plancmp
from tests import lancgp16_cases as G

_SHAPES = G.SHAPES + [G.TALL, G.NARROW, G.HELD_UP, G.HELD_DN, G.SPECIAL_DN] + \
    G.CH_SHAPES


def _descs(geom, ch, pairs):
    sw, sh, nw, nh = geom
    lib = abi.load()
    l = C.c_void_p()
    abi.check(lib.avirhip_lancir_create(C.byref(l)), "lancir_create")
    made = []
    for ti, to in pairs:
        d = C.POINTER(abi.LancirDesc)()
        abi.check(lib.avirhip_lancir_build_desc(
            l, sw, sh, nw, nh, ch, None, ti, to, C.byref(d)),
            "lancir_build_desc")
        made.append(d)
    return lib, l, made


def _free(lib, l, made):
    for d in made:
        lib.avirhip_lancir_desc_free(d)
    lib.avirhip_lancir_destroy(l)


def _not_types(bad):
    return [b for b in bad if not b.startswith(("in_type:", "out_type:"))]


@pytest.mark.parametrize("geom", _SHAPES, ids=lambda g: "%dx%d-%dx%d" % g)
def test_desc_equals_float32_desc(geom):
    F16, BF16, F32 = abi.F16, abi.BF16, abi.F32
    for ch in (4, 3):
        lib, l, made = _descs(geom, ch, [(F32, F32), (F16, F16), (BF16, BF16),
                                         (abi.U8, F32), (abi.U8, F16),
                                         (F32, abi.U16), (BF16, abi.U16)])
        try:
            for i, j in ((1, 0), (2, 0), (4, 3), (6, 5)):
                assert _not_types(plancmp.compare_lancir_desc(
                    made[i].contents, made[j].contents)) == [], (geom, ch, i)
            assert (made[1].contents.in_type, made[1].contents.out_type) == \
                (F16, F16)
            assert (made[2].contents.in_type, made[2].contents.out_type) == \
                (BF16, BF16)
            # the gain behind a 16-bit float type is the float32 call's
            for i, j in ((1, 0), (2, 0), (4, 3), (6, 5)):
                a, b = made[i].contents, made[j].contents
                assert (a.out_mul, a.clamp, a.is_unity_mul) == \
                    (b.out_mul, b.clamp, b.is_unity_mul)
            assert made[4].contents.is_unity_mul == 0
            assert made[6].contents.is_unity_mul == 0
        finally:
            _free(lib, l, made)


def _lancir_taps(src, new):
    """LANCIR's kernel: 2 * ceil(3 * k) taps when downsizing, 6 when not."""
    k = src / float(new)
    return 2 * int(math.ceil(3.0 * k)) if k > 1.0 else 6


@pytest.mark.parametrize("geom,taps", [
    (G.DN18, (18, 18)), (G.DN10, (10, 10)), (G.TALL, (None, 28)),
    (G.UP, (6, 6)), (G.MIXED, (10, 6))],
    ids=["18", "10", "28v", "up", "mixed"])
def test_tap_counts_are_the_planners(geom, taps):
    lib, l, made = _descs(geom, 4, [(abi.F16, abi.F16)])
    try:
        d = made[0].contents
        sw, sh, nw, nh = geom
        assert d.h.kernel_len == _lancir_taps(sw, nw)
        assert d.v.kernel_len == _lancir_taps(sh, nh)
        if taps[0] is not None:
            assert d.h.kernel_len == taps[0]
        assert d.v.kernel_len == taps[1]
        if geom in G.TAPS:
            assert G.TAPS[geom] == (d.h.kernel_len, d.v.kernel_len)
    finally:
        _free(lib, l, made)


def test_cases_cover_the_issue():
    assert len(G.PAIRS) == 16
    for a, b in G.PAIRS:
        assert a in G.H16 or b in G.H16
    assert set(G.SAME) <= set(G.PAIRS)
    assert G.LF_CHUNKS == [1, 7, 9, 13] and G.GV_CHUNKS == [1, 4, 5]
    assert G.UP == (97, 61, 233, 150) and G.NARROW[0] == 40
    assert (G.UP[0] * 3 * 2) % 4 == 2      # RGB half: a pitch of 582 bytes
    assert len(G.roads(G.UP)) == 4 and len(G.roads(G.DN18)) == 2
    # the l4 tail rule: width * channels not a multiple of 4
    assert (G.UP[2] * 3) % 4 != 0


@pytest.mark.parametrize("geom", [G.SPECIAL_UP, G.SPECIAL_DN],
                         ids=["up", "down"])
def test_half_frame_has_every_class(geom):
    src, ref, want = G.special_case("f16", "f16", geom)
    assert src.dtype == np.float16 and want.dtype == np.float16
    c = G.special_classes("f16", ref, want)
    print(geom, c)
    assert c["finite"] > c["size"] // 2
    assert c["fin_to_inf"] > 0           # overflow on narrowing
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    assert c["denormal"] > 0
    # (-0 comes from the narrowing of a negative result under half the smallest
    # denormal: the edge of a field of zeros, which 16-tap windows do not
    # resolve -- the upsizing frame has the class)
    assert c["neg_zero"] > 0 or geom == G.SPECIAL_DN


@pytest.mark.parametrize("geom", [G.SPECIAL_UP, G.SPECIAL_DN],
                         ids=["up", "down"])
def test_bfloat16_frame_has_every_class(geom):
    src, ref, want = G.special_case("bf16", "bf16", geom)
    assert src.dtype == np.uint16 and want.dtype == np.uint16
    c = G.special_classes("bf16", ref, want)
    print(geom, c)
    assert c["finite"] > c["size"] // 2
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    assert c["denormal"] > 0
    assert c["neg_zero"] > 0 or geom == G.SPECIAL_DN
    # every exponent is in the source, with four mantissas and both signs
    e = (src.astype(np.uint32) >> 7) & 0xff
    assert len(np.unique(e)) == 256
    assert np.array_equal(np.isnan(G.widen(want)), np.isnan(ref))
    # the largest finite value times the gain of an integer result: clamped
    s8, r8, w8 = G.special_case("bf16", "u8", geom)
    assert w8.dtype == np.uint8 and (w8 == 255).any() and (w8 == 0).any()
    # a half result of the same frame overflows where bfloat16 does not
    s, r, wh = G.special_case("bf16", "f16", geom)
    ch = G.special_classes("f16", r, wh)
    assert ch["fin_to_inf"] > 0


def test_source_denormals_reach_the_result():
    """The half frame's block of denormals: a loader that flushed them would
    read zeros there, and the reference's result of that frame is another."""
    from tests import helpers as H
    src, ref, want = G.special_case("f16", "f16", G.SPECIAL_UP)
    blk = src[G.DENORMALS].astype(np.float32)
    assert (np.abs(blk) < 2.0 ** -14).all()
    assert int((blk != 0).sum()) > blk.size // 2
    flushed = src.copy()
    flushed[G.DENORMALS] = 0
    fref = H.checker_lancir(flushed.astype(np.float32), G.SPECIAL_UP[2],
                            G.SPECIAL_UP[3], out_dtype=np.float32)
    differ = int((G.words(want) != G.words(G.from_f32(fref, "f16"))).sum())
    print("elements that differ from the flushed frame's:", differ)
    assert differ > 0
