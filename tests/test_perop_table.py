"""tests/perop_cases.py held to the product planner (host only): every row's
horizontal axis lowers to the step kinds the row is there for, with the fields
it names, in the float class and in the double class."""
import pytest
from avir_amd import abi
from tests import helpers as H
from tests import perop_cases as PC
from tests import plancmp


@pytest.mark.parametrize("fp", [PC.FLT, PC.DBL], ids=["flt", "dbl"])
@pytest.mark.parametrize("r", PC.ROWS, ids=[r[0] for r in PC.ROWS])
def test_rows_lower_to_their_op_kinds(r, fp):
    name, geom, mode, bits, chans, steps = r
    rz, d = H.product_desc(*geom, 3, resbits=bits, build_mode=mode,
                           fpclass=fp)
    try:
        ax = d.contents.h
        what = "%s: %s" % (name, plancmp.axis_summary(ax))
        assert d.contents.work_f64 == (1 if fp == PC.DBL else 0), what
        assert [abi.STEP_NAMES[ax.steps[i].kind]
                for i in range(ax.n_steps)] == [k for k, _ in steps], what
        for i, (_, fields) in enumerate(steps):
            for f, want in fields.items():
                got = getattr(ax.steps[i], f)
                assert (got > 0 if want == ">0" else got == want), (what, i, f)
        # (both axes run the same chain: the vertical loop of the driver too)
        assert [ax.steps[i].kind for i in range(ax.n_steps)] == \
            [d.contents.v.steps[i].kind for i in range(d.contents.v.n_steps)]
    finally:
        H.free_product_desc(rz, d)


def test_cases_name_rows_and_both_classes():
    for c in PC.CASES:
        assert c[1] in PC.row(c[0])[4], c
    for r in PC.ROWS:
        for fp in (PC.FLT, PC.DBL):
            assert [c for c in PC.CASES if c[0] == r[0] and c[2] == fp], r[0]
    extra = [c for c in PC.CASES if c[3] != PC.np.float32]
    assert sorted(PC.np.dtype(c[3]).name for c in extra) == \
        ["float64", "uint8"] and all(c[2] == PC.DBL for c in extra)
