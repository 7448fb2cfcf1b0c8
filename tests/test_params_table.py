"""Host-only: the chain shapes the parameter sets of tests/param_cases.py give
on its geometry classes, read from the product planner's PlanDesc (pinned to
the reference planner by tests/plancmp.py, here and in test_planner.py) -- the
facts the expectations of tests/test_gpu_params.py rest on. These are
assertions about the reference's arithmetic, not about the kernels.

TABLE (set -> class -> one (horizontal, vertical) shape per frame of the class,
in param_cases.CLASSES order) is derived once, at import; the GPU file imports
it. It is keyed by frame, not by geometry: the reference picks a build mode by
cost, and channel count, element type and bit depth enter the cost."""
import numpy as np
import pytest
from avir_amd import abi
from tests import param_cases as PC
from tests import plancmp as pc
from tests import refbind as rb
from tests.helpers import product_desc, free_product_desc


def _desc(name, frame):
    sw, sh, nw, nh, ch, t, tout, bits, fp = frame
    ty = {np.uint8: abi.U8, np.uint16: abi.U16, np.float32: abi.F32,
          np.float64: abi.F64}[t]
    return product_desc(sw, sh, nw, nh, ch, in_type=ty, out_type=ty,
                        resbits=bits, params=PC.SETS[name], fpclass=fp)


def _shape(name, frame):
    r, d = _desc(name, frame)
    try:
        return PC.desc_shape(d.contents)
    finally:
        free_product_desc(r, d)


TABLE = {s: {c: tuple(_shape(s, f) for f, _ in PC.CLASSES[c])
             for c in PC.CLASS_NAMES} for s in PC.SET_NAMES}


def shape_of(name, cls, frame):
    return TABLE[name][cls][[f for f, _ in PC.CLASSES[cls]].index(frame)]


def _axes(name):
    for cls in PC.CLASS_NAMES:
        for hv in TABLE[name][cls]:
            for ax in hv:
                yield cls, ax


def test_default_values_are_the_librarys():
    import ctypes as C
    P = abi.Params()
    abi.load().avirhip_params_preset(0, C.byref(P))
    assert tuple(getattr(P, n) for n in PC.NAMES) == PC.DEF
    assert sorted(PC.SEVEN_TAP + PC.OTHER_TAP) == PC.SET_NAMES


@pytest.mark.parametrize("name", PC.SET_NAMES)
def test_correction_filter_follows_calc_filter_length(name):
    """2 * ceil(CorrFltLen / 2) - 1 taps, latency (taps - 1) / 2, on every
    axis of every class, exactly one per axis, never resampling."""
    want = PC.corr_len_lat(name)
    for cls, ax in _axes(name):
        firs = [s for s in ax if s[0] == "FIR"]
        assert len(firs) == 1, (cls, ax)
        assert firs[0][1] == 1 and (firs[0][2], firs[0][3]) == want, (cls, ax)
    split = {"ulr": (5, 2), "lr": (5, 2), "corr8.2": (9, 4),
             "corr4.0": (3, 1)}
    assert want == split.get(name, (7, 3))
    assert (name in PC.SEVEN_TAP) == (want == (7, 3))


def test_default_set_gives_the_shapes_the_kernels_name():
    T = TABLE["def"]
    fir7 = ("FIR", 1, 7, 3, 0)
    zs = ("UP_ZEROSTUFF", 2, 0, 0, 0)
    up = (fir7, zs, ("RESIZE2", 0, 0, 0, 24))  # FIR7 -> 12-tap bank over ZS
    for cls in ("x2", "upg"):
        assert all(hv == (up, up) for hv in T[cls]), T[cls]
    assert [PC.gather_taps(hv[0]) for hv in T["dn12"]] == [19, 16]
    for hv in T["dn12"]:
        assert hv[0] == hv[1] and PC._kinds(hv[0]) == PC.DN12
        assert hv[0][2] == fir7
    # whole ratios: the two (K, NT) dn.hip is written for
    assert T["whole"] == tuple(((("RESIZE", 0, 0, 0, n), fir7),) * 2
                               for n in (24, 38, 24, 38))
    assert T["dn2p"] == (((("RESIZE", 0, 0, 0, 36), fir7),) * 2,) * 3
    assert T["mixed"] == ((up, (("RESIZE", 0, 0, 0, 34), fir7)),)
    assert [PC._kinds(hv[0]) for hv in T["dbl"]] == [PC.UP, PC.UP,
                                                     PC.DN12] * 2


def test_custom_sets_land_where_they_were_aimed():
    def taps(name, cls):
        return [tuple(PC.gather_taps(ax) for ax in hv)
                for i, hv in enumerate(TABLE[name][cls])
                if (name, cls, i) != FILTERED]
    # the zero-stuffed bank of the upsizing side: IntFltLen moves it off 12 in
    # both directions, LPFltBaseLen too; `high` / `ultra` give 13
    for name, n in (("int14", 10), ("int22", 14), ("lp5.2", 11),
                    ("lp10.4", 14), ("high", 13), ("ultra", 13),
                    ("low", 12), ("ulr", 12), ("lr", 12), ("corr8.2", 12),
                    ("corr4.0", 12), ("int_a2_c0.7", 12)):
        assert set(taps(name, "x2") + taps(name, "upg")) == {(n, n)}, name
    # whole ratios 2 and 3: only the default's tap counts are dn.hip's
    whole = {name: [t[0] for t in taps(name, "whole")]
             for name in PC.SET_NAMES}
    assert whole["lp5.2"] == [22, 34] * 2 and whole["lp10.4"] == [28, 42] * 2
    assert whole["int14"] == [20, 32] * 2 and whole["int22"] == [28, 44] * 2
    assert whole["high"] == whole["ultra"] == [26, 40] * 2
    for name in ("def", "low", "lr", "corr8.2", "corr4.0", "int_a2_c0.7"):
        assert whole[name] == [24, 38] * 2, name
    # 1 < k < 2: every set stays inside the 13 .. 25 taps of the register-
    # window vertical kernel and of k_gh2, on both sides of k_gh2's automatic
    # threshold of 22
    seen = set()
    for name in PC.SET_NAMES:
        for t in taps(name, "dn12"):
            assert 13 <= t[0] <= 25 and t[0] == t[1], (name, t)
            seen.add(t[0])
    assert min(seen) < 22 <= max(seen), seen
    # k >= 2: 24 .. 64 taps, below the 51 the vertical ring could hold
    for name in PC.SET_NAMES:
        for cls in ("whole", "dn2p"):
            for t in taps(name, cls):
                assert 20 <= t[0] <= 44, (name, cls, t)


# The one frame of the table whose build mode is not the zero-stuffed one: the
# reference's cost model gives the horizontal axis of this 1-channel exact 2x a
# FILTERED upsample (which only the generic kernels run).
FILTERED = ("lp10.4", "x2", 4)


def test_one_frame_takes_a_filtered_upsample():
    found = [(s, c, i) for s in PC.SET_NAMES for c in PC.CLASS_NAMES
             for i, hv in enumerate(TABLE[s][c])
             if any("UP_FILTERED" in PC._kinds(ax) for ax in hv)]
    assert found == [FILTERED]
    h, v = TABLE["lp10.4"]["x2"][4]
    assert PC._kinds(h) == ("FIR", "UP_FILTERED", "RESIZE")
    assert PC._kinds(v) == PC.UP
    for path in (2, 4, 5):
        assert PC.expect((h, v), PC.CLASSES["x2"][4][0], path) is not None


@pytest.mark.parametrize("name", PC.SET_NAMES)
def test_shape_depends_on_the_geometry_alone_otherwise(name):
    """uint8 / 8-bit, uint16, 1-3 channel and double-pipeline frames have the
    shape of the float RGBA 16-bit frame of their geometry."""
    for cls in PC.CLASS_NAMES:
        for i, (frame, _) in enumerate(PC.CLASSES[cls]):
            if (name, cls, i) == FILTERED:
                continue
            base = frame[:4] + (4, np.float32, np.float32, 16, 1)
            assert TABLE[name][cls][i] == _shape(name, base), (cls, frame)


def _phase_rows(s, j):
    """The coefficients api.cpp lower_axis gives output j of a RESIZE2 step:
    ftp[i] + ftp2[i] * x in float, every second tap."""
    rp = s.rpos[j]
    fl = s.bank_filter_len
    base = rp.phase * fl * (s.bank_order + 1) + rp.ftp_off
    out = []
    for i in range(0, rp.fl, 2):
        a = np.float32(s.phase_taps[base + i])
        if s.bank_order == 1:
            t = np.float32(np.float32(s.phase_taps[base + fl + i]) *
                           np.float32(rp.x))
            a = np.float32(a + t)
        out.append(a)
    return np.array(out, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", PC.SET_NAMES)
def test_exact_2x_bank_phases_are_bit_symmetric(name):
    """fo[t] == fe[nt-1-t] in bits, which up2.hip's transposed form needs:
    holds for every set, so parameters never select the plain form."""
    for frame, _ in PC.CLASSES["x2"]:
        ch = frame[4]
        r, d = _desc(name, frame)
        try:
            for ax in (d.contents.h, d.contents.v):
                s = ax.steps[ax.n_steps - 1]
                if s.kind != abi.STEP_RESIZE2:
                    assert (name, "x2", 4) == FILTERED and ch == 1
                    continue
                j = (s.out_len // 2) & ~1
                fe, fo = _phase_rows(s, j), _phase_rows(s, j + 1)
                assert len(fe) == len(fo) == PC.gather_taps(
                    PC.axis_shape(ax))
                assert np.array_equal(fo, fe[::-1]), (name, frame)
        finally:
            free_product_desc(r, d)


def _combos(name):
    for cls in PC.CLASS_NAMES:
        for frame, runs in PC.CLASSES[cls]:
            for path, variant, env in runs:
                yield cls, frame, path, PC.expect(shape_of(name, cls, frame),
                                                  frame, path)


def test_expectation_table_meets_the_stated_conditions():
    # the default set: every listed combination runs
    assert [c for c in _combos("def") if c[3] is not None] == []
    for name in PC.SET_NAMES:
        ran = {}
        for (cls, frame, path, why), (_, _, _, dwhy) in zip(_combos(name),
                                                           _combos("def")):
            hv = shape_of(name, cls, frame)
            filtered = any("UP_FILTERED" in PC._kinds(ax) for ax in hv)
            if why is None:
                # (path 0 counts as the fast path it may land on)
                ran.setdefault(cls, set()).update(
                    PC.expect_auto(hv, frame) if path == 0 else [path])
            if path in (0, 1, 2):
                assert (why is None) == (path != 2 or not filtered), (
                    name, cls, frame, path, why)
            seven = name in PC.SEVEN_TAP and not filtered
            if path == 5:
                # the pass kernels take every 7-tap set and no other
                assert (why is None) == seven, (name, cls, frame, why)
            if path == 4:
                nt = PC.gather_taps(shape_of(name, cls, frame)[0])
                assert (why is None) == (seven and nt == 12), (name, why)
        if name in PC.SEVEN_TAP:
            # no (set, class) pair in which nothing but path 1 may run
            assert all(ran[c] - {1} for c in PC.CLASS_NAMES), (name, ran)
    for name in ("low", "high", "ultra"):
        nt = PC.gather_taps(TABLE[name]["x2"][0][0])
        assert nt == (12 if name == "low" else 13)
    for name in ("ulr", "lr"):
        bad = [c for c in _combos(name) if c[2] in (4, 5) and c[3] is None]
        assert bad == []


@pytest.mark.skipif(not rb.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", PC.SET_NAMES)
def test_reference_takes_the_set_and_the_planners_agree(name):
    """The real reference resizes with the set (no assertion of its own
    trips: an abort would end the run), and the product planner's plans of
    the class geometries equal the reference planner's bit for bit."""
    src = rb.lcg_f32((30, 40, 4), seed=3)
    for nw, nh in ((80, 60), (61, 47), (27, 20), (20, 10), (13, 7)):
        out = rb.ref_avir(src, nw, nh, resbits=16, params=PC.SETS[name])
        assert np.isfinite(out).all()
    for cls in PC.CLASS_NAMES:
        sw, sh, nw, nh = PC.geometries(cls)[0]
        rd = rb.ref_avir_plan(sw, sh, nw, nh, 4, resbits=16,
                              params=PC.SETS[name])
        r, d = product_desc(sw, sh, nw, nh, 4, resbits=16,
                            params=PC.SETS[name])
        try:
            assert pc.compare_desc(rd.contents, d.contents) == []
        finally:
            free_product_desc(r, d)
            rb.ref().ref_avir_plan_free(rd)
