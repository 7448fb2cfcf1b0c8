"""Host-only checks of the inputs of tests/test_gpu_dnsrgb8.py
(tests/dnsrgb8_cases.py): the shapes are k_dnf's plans for the uint8 gamma
call as for the float32 call, and the frames hold, by the reference alone,
what the GPU tests are there to compare."""
import ctypes as C
import numpy as np
import pytest
from avir_amd import abi
from tests import dnsrgb8_cases as D
from tests import plancmp


def _desc(geom, t, gamma, alpha=-1):
    """The product planner's description of the call (resbits 8)."""
    lib = abi.load()
    sw, sh, nw, nh = geom
    r = C.c_void_p()
    abi.check(lib.avirhip_resizer_create(8, 0, None, C.byref(r)), "create")
    v = abi.Vars()
    lib.avirhip_vars_default(C.byref(v))
    v.UseSRGBGamma, v.AlphaIndex = (1 if gamma else 0), alpha
    d = C.POINTER(abi.PlanDesc)()
    abi.check(lib.avirhip_resizer_build_desc(
        r, sw, sh, 0, nw, nh, 4, 0.0, C.byref(v), D.T[t][0], D.T[t][0],
        C.byref(d)), "build_desc")
    return r, d


def _free(r, d):
    lib = abi.load()
    lib.avirhip_plan_desc_free(d)
    lib.avirhip_resizer_destroy(r)


@pytest.mark.parametrize("geom", D.SHAPES + D.EXTRA_SHAPES +
                         [D.SPECIAL, D.SPECIAL_BIG, D.RAMP],
                         ids=lambda g: "%dx%d-%dx%d" % g)
def test_the_gamma_call_has_the_float_calls_plan(geom):
    """Everything but the type and gamma fields: the axes of the uint8 gamma
    call are the float32 call's; two steps each (resize, correction filter)
    are k_dnf's plan, which at ResBitDepth 8 all but NOT_DNF have."""
    rf, df = _desc(geom, "f32", False)
    rg, dg = _desc(geom, "u8", True, 3)
    try:
        a, b = df.contents, dg.contents
        bad = []
        for f in ("src_w", "src_h", "src_stride_elems", "new_w", "new_h",
                  "channels"):
            if getattr(a, f) != getattr(b, f):
                bad.append(f)
        bad += plancmp.compare_axis(a.h, b.h, "h")
        bad += plancmp.compare_axis(a.v, b.v, "v")
        assert not bad, bad
        assert ((a.h.n_steps, a.v.n_steps) == (2, 2)) == (
            geom not in D.NOT_DNF), geom
        assert (b.use_srgb_gamma, b.alpha_index) == (1, 3)
        assert b.in_type == abi.U8 and b.out_type == abi.U8
        assert a.use_srgb_gamma == 0
    finally:
        _free(rf, df)
        _free(rg, dg)


def test_shapes_have_every_form():
    forms = set((g[0] // g[2], g[1] // g[3]) for g in D.DNF_SHAPES)
    assert forms == {(2, 2), (3, 3), (2, 3), (3, 2)}
    for sw, sh, nw, nh in D.SHAPES + D.EXTRA_SHAPES + [D.SPECIAL,
                                                        D.SPECIAL_BIG, D.RAMP]:
        assert sw % nw == 0 and sh % nh == 0
    # a last strip one column wide, for K = 2 and for K = 3
    assert sorted((g[0] // g[2], g[2] % 42) for g in D.DNF_SHAPES
                  if g[2] % 42 == 1) == [(2, 1), (3, 1)]


@pytest.mark.parametrize("alpha", D.ALPHAS)
@pytest.mark.parametrize("geom", [D.SHAPES[0], D.SHAPES[1], D.SHAPES[5]],
                         ids=lambda g: "%dx%d-%dx%d" % g)
def test_lcg_results_stay_inside_the_byte_range(geom, alpha):
    """The comparison is of the stage's steps, not of its clamps."""
    src, want = D.case(geom, "u8", "u8", 4, alpha)
    inside = float(((want != 0) & (want != 255)).mean())
    print(geom, alpha, inside)
    assert inside >= 0.99


def test_ramp_frame_has_every_byte_and_both_clamps():
    src, want = D.ramp_case()
    assert src.shape == (400, 600, 4) and want.shape == (200, 300, 4)
    n = np.bincount(want.reshape(-1), minlength=256)
    print(int((n > 0).sum()), int(n[0]), int(n[255]))
    assert (n > 0).all()
    assert n[0] >= 5000 and n[255] >= 5000


def test_special_frame_leaves_the_searched_range():
    """The linear float32 result of the special-value frame: what reaches the
    store's direct branch."""
    src, lin = D.special_case(D.SPECIAL, "f32")
    assert lin.size == 12288
    fin = np.isfinite(lin)
    with np.errstate(invalid="ignore"):
        far = int((fin & (np.abs(lin) > 16)).sum())
    inf, nan = int(np.isinf(lin).sum()), int(np.isnan(lin).sum())
    print(far, inf, nan)
    assert far >= 1000 and inf >= 10 and nan >= 100
