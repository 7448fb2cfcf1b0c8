"""Host-only checks of the inputs of tests/test_gpu_up2srgb8.py
(tests/up2srgb8_cases.py): the shapes are k_up2's plans for the uint8 gamma
call as for the float32 call, and the frames hold, by the reference alone,
what the GPU tests are there to compare."""
import ctypes as C
import numpy as np
import pytest
from avir_amd import abi
from tests import up2srgb8_cases as U
from tests import plancmp


def _desc(geom, t, gamma, alpha=-1, ch=4):
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
        r, sw, sh, 0, nw, nh, ch, 0.0, C.byref(v), U.T[t][0], U.T[t][0],
        C.byref(d)), "build_desc")
    return r, d


def _free(r, d):
    lib = abi.load()
    lib.avirhip_plan_desc_free(d)
    lib.avirhip_resizer_destroy(r)


@pytest.mark.parametrize("geom", U.ALL_SHAPES + [U.RAMP],
                         ids=lambda g: "%dx%d-%dx%d" % g)
def test_the_gamma_call_has_the_float_calls_plan(geom):
    """Everything but the type and gamma fields: the axes of the uint8 gamma
    call are the float32 call's, three steps each, kinds 0, 1, 4 -- the plan
    k_up2 matches."""
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
        for ax in (b.h, b.v):
            assert ax.n_steps == 3, geom
            assert [ax.steps[i].kind for i in range(3)] == [0, 1, 4], geom
        assert (b.use_srgb_gamma, b.alpha_index) == (1, 3)
        assert b.in_type == abi.U8 and b.out_type == abi.U8
        assert a.use_srgb_gamma == 0
    finally:
        _free(rf, df)
        _free(rg, dg)


@pytest.mark.parametrize("ch", [1, 3])
def test_which_shapes_are_the_kernels_plans_for_fewer_channels(ch):
    """The planner's cost model sees the channel count: RGB pixels get the
    plan k_up2 matches at every shape, grey pixels at the two larger ones."""
    for geom in U.ALL_SHAPES:
        r, d = _desc(geom, "u8", True, -1, ch)
        try:
            k = [[ax.steps[i].kind for i in range(ax.n_steps)]
                 for ax in (d.contents.h, d.contents.v)]
        finally:
            _free(r, d)
        assert (k == [[0, 1, 4], [0, 1, 4]]) == (geom in U.shapes(ch) or
                                                  ch == 3), (geom, k)


def test_shapes_reach_every_edge_of_the_march():
    for sw, sh, nw, nh in U.ALL_SHAPES + [U.RAMP]:
        assert (nw, nh) == (2 * sw, 2 * sh)
    # last strips of 2 and of 16 columns, a frame under the smallest chunk
    # (62 source rows), frames of several chunks
    assert sorted(g[2] % 64 for g in U.SMALL) == [2, 16, 16]
    assert min(g[1] for g in U.SMALL) < 62
    assert U.RGBA_BIG[1] > 4 * 62 and U.RGB_BIG[1] > 4 * 62
    assert U.RGB_BIG[0] % 4 != 0  # a row pitch of 963 bytes


@pytest.mark.parametrize("alpha", (-1, 3, 0))
@pytest.mark.parametrize("geom", [U.SMALL[0], U.RGBA_BIG],
                         ids=lambda g: "%dx%d-%dx%d" % g)
def test_results_stay_inside_the_byte_range(geom, alpha):
    """The comparison is of the stage's steps, not of its clamps."""
    src, want = U.case(geom, "u8", "u8", 4, alpha)
    inside = float(((want != 0) & (want != 255)).mean())
    print(geom, alpha, inside)
    assert inside >= 0.99


def test_which_shapes_run_the_transposed_form():
    """The fused loads and stores live in the transposed form (up2_vt). At
    ResBitDepth 8 the three small shapes and the ramp frame get an order-1
    bank at x = 0.5 on an axis: the plain form, the road from before."""
    for ch in (4, 3):
        assert [U.transposed(g, ch) for g in U.SMALL + [U.RAMP]] == \
            [False] * 4, ch
        assert U.transposed(U.RGBA_BIG, ch) and U.transposed(U.RGB_BIG, ch)
    assert U.transposed(U.RGBA_BIG, 1) and U.transposed(U.RGB_BIG, 1)
    assert U.road(U.SMALL[0], 4, True) == U.PARENT
    assert U.road(U.RGBA_BIG, 4, True) == ["k_up2"]
    assert U.road(U.RGB_BIG, 1, False) == ["pack pass", "k_up2"]


def test_small_shapes_of_the_transposed_form():
    """What 322x420 and 321x420 do not reach in the kernel's gamma kinds: a
    frame under the smallest chunk whose last marching step holds fewer than 8
    source rows, and a 16-column last strip -- both the transposed form's."""
    sw, sh, nw, nh = U.SHORT
    assert sh < 62 and sh % 8 != 0 and U.transposed(U.SHORT, 4)
    assert U.STRIP16[2] % 64 == 16
    assert U.transposed(U.STRIP16, 4) and U.transposed(U.STRIP16, 3)
    for g in (U.RGBA_BIG, U.RGB_BIG):
        assert g[2] % 64 not in (0, 16) and g[1] >= 62


@pytest.mark.parametrize("geom", [U.RAMP, U.RAMP_BIG],
                         ids=lambda g: "%dx%d-%dx%d" % g)
def test_ramp_frame_has_every_byte_and_both_clamps(geom):
    src, want = U.ramp_case(geom)
    assert want.shape == (geom[3], geom[2], 4)
    n = np.bincount(want.reshape(-1), minlength=256)
    print(int((n > 0).sum()), int(n.min()), int(n[0]), int(n[255]))
    assert (n > 0).all()
    assert n[0] >= 5000 and n[255] >= 5000


@pytest.mark.parametrize("geom", [U.SPECIAL, U.SPECIAL_BIG],
                         ids=lambda g: "%dx%d-%dx%d" % g)
def test_special_frame_leaves_the_searched_range(geom):
    """The linear float32 result of the special-value frame: what reaches the
    store's direct branch."""
    src, lin = U.special_case("f32", geom)
    assert lin.shape == (geom[3], geom[2], 4)
    fin = np.isfinite(lin)
    with np.errstate(invalid="ignore"):
        far = int((fin & (np.abs(lin) > 16)).sum())
    inf, nan = int(np.isinf(lin).sum()), int(np.isnan(lin).sum())
    print(far, inf, nan)
    assert far >= 1000 and inf >= 10 and nan >= 100
