"""Host-only check of the case table of tests/test_gpu_placement.py
(tests/placement_cases.py): the product planner agrees with the reference
planner on every placed call, every case is placed as its name says -- by the
windows of the planner's own description --, band_source_rows stays inside the
frame and holds every row the band's windows reach after the edge clamp, and
the real reference and the plain-C restatement (which tests/test_oracle.py
pins on covering grids only) agree bit for bit on the case."""
import numpy as np
import pytest
from avir_amd import abi
from tests import helpers as H
from tests import placement_cases as P
from tests import plancmp as pc
from tests import refbind as rb
from tests import window_cases as W

needs_ref = pytest.mark.skipif(not rb.have_ref(),
                               reason="oracle/_ref not built")


def test_the_table_names_its_cases_once():
    assert len(set(P.IDS)) == len(P.IDS)
    assert {c[0] for c in P.CASES} == set(P.ROWS)
    for c in P.CASES:
        assert set(c[2]) <= set(P.PLACEMENTS), c[2]
        # (a placed case states its step; the offsets of the shifts are the
        # 37 .. 130 -- or, past the far edge, more -- the table promises)
        assert c[1][11]["k"] != 0


@needs_ref
@pytest.mark.parametrize("case", P.CASES, ids=P.IDS)
def test_planners_agree(case):
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = case[1]
    ti, to = P._ty(tin), P._ty(tout)
    with P.Desc(case) as d:
        if fe == "lancir":
            rd = rb.ref_lancir_plan(sw, sh, nw, nh, ch, ti, to, kx=ex["k"],
                                    ky=ex["k"], ox=ex["ox"], oy=ex["oy"])
            try:
                assert pc.compare_lancir_desc(rd.contents, d) == []
            finally:
                rb.ref().ref_lancir_plan_free(rd)
            return
        if ex.get("fp") == abi.FPCLASS_DOUBLE:
            # (the reference planner's dump is of the float class; the double
            # pipeline's plans are pinned by tests/test_planner.py -- here the
            # chain and the positions, which the classes share)
            ti = to = abi.F32
            with P.Desc((case[0], case[1][:6] + (np.float32, np.float32) +
                         case[1][8:11] + (dict(ex, fp=1),), case[2])) as d1:
                assert P.windows(case, d, "v")[0].tolist() == \
                    P.windows(case, d1, "v")[0].tolist()
                assert P.windows(case, d, "h")[1].tolist() == \
                    P.windows(case, d1, "h")[1].tolist()
            return
        rd = rb.ref_avir_plan(sw, sh, nw, nh, ch, k=ex["k"], in_type=ti,
                              out_type=to, resbits=bits, ox=ex["ox"],
                              oy=ex["oy"],
                              sstride=W.pitch(case[1]) if ex.get("pad") else 0)
        try:
            assert pc.compare_desc(rd.contents, d) == []
        finally:
            rb.ref().ref_avir_plan_free(rd)


@pytest.mark.parametrize("case", P.CASES, ids=P.IDS)
def test_case_is_placed_as_named(case):
    sh, nh = case[1][2], case[1][4]
    obj, arg = W.front_end(case[1])
    with P.Desc(case) as d:
        for axis in "hv":
            assert P.placement_holds(case, d, axis) is None
        lo, hi = P.windows(case, d, "v")
        clo, chi = P.windows(case, d, "v", clamped=True)
        rows = {}
        for name, r0, r1 in P.bands(case, d):
            a, b = W.host_source_rows(case[1], obj, arg, r0, r1)
            rows[name] = (a, b)
            assert 0 <= a <= b < sh, (name, a, b)
            # every row the band's windows reach after the clamp
            reach = np.clip(np.concatenate([clo[r0:r1], chi[r0:r1]]), 0,
                            sh - 1)
            assert a <= reach.min() and reach.max() <= b, (name, a, b)
        if case[2][1] == "outside":
            which = P.outside_fifth(lo, hi, sh)
            edge = 0 if which == "first" else sh - 1
            assert rows[which] == (edge, edge), rows
        print(case[2], "windows h [%d .. %d] v [%d .. %d], rows %r" % (
            P.windows(case, d, "h")[0][0], P.windows(case, d, "h")[1][-1],
            lo[0], hi[-1], rows))


def test_expectation_names_the_refusals_it_should():
    """Whole-pixel shifts of an exact 2x are refused by path 4 and taken by
    path 5 and the automatic path; the un-shifted explicit form is path 4's;
    every other case of the table is expected to run on its path."""
    refused = []
    for c in P.CASES:
        with P.Desc(c) as d:
            why = P.expect(c, d)
            if why is not None:
                refused.append(P.case_id(c))
                assert c[0] in ("x2", "lanc2") and c[1][9] == 4, (c, why)
                assert "starts at sample" in why, why
                assert P.expect(c, d, 0) is None
                assert P.expect(c, d, 5) is None
            if c[2] == ("cover", "cover"):
                assert why is None and c[1][9] == 4
    assert len(refused) == 3, refused
    for row in P.ROWS:
        runs = [c for c in P.CASES if c[0] == row and c[2][0] != "cover"]
        assert len(runs) >= 2, row


@needs_ref
@pytest.mark.parametrize("case", P.CASES, ids=P.IDS)
def test_reference_and_restatement_agree(case):
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = case[1]
    if ex.get("fp") == abi.FPCLASS_DOUBLE:
        # (the restatement has no double class: the reference alone runs the
        # call, and trips no assertion of its own)
        src = rb.lcg_f32((sh, sw, ch), seed=sw).astype(np.float64)
        out = rb.ref_avir(src, nw, nh, k=ex["k"], resbits=bits, ox=ex["ox"],
                          oy=ex["oy"], variant=4, threads=8)
        assert np.isfinite(out).all()
        return
    t = np.dtype(tin)
    if t.kind == "u":
        src = rb.lcg_u8((sh, sw, ch), seed=sw + ch)
    else:
        src = rb.lcg_f32((sh, sw, ch), seed=7 * sw + ch)
    if fe == "lancir":
        kw = dict(out_dtype=tout, kx=ex["k"], ky=ex["k"], ox=ex["ox"],
                  oy=ex["oy"])
        a, b = rb.ref_lancir(src, nw, nh, **kw), rb.orc_lancir(src, nw, nh,
                                                               **kw)
    else:
        kw = dict(k=ex["k"], out_dtype=tout, resbits=bits, ox=ex["ox"],
                  oy=ex["oy"], gamma=bool(ex.get("gamma", 0)),
                  alpha=ex.get("alpha", -1))
        a = rb.ref_avir(src, nw, nh, threads=8, **kw)
        b = rb.orc_avir(src, nw, nh, **kw)
    assert a.shape == (nh, nw, ch)
    va = a.view(np.uint32) if a.dtype == np.float32 else a
    vb = b.view(np.uint32) if b.dtype == np.float32 else b
    assert np.array_equal(va, vb), int((va != vb).sum())
