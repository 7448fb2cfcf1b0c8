"""Host-only checks of the inputs of tests/test_gpu_sacc16.py
(tests/sacc16_cases.py): every shape plans as the accumulation kernels'
material on the axes it names, a half / bfloat16 description is the float32
one but for the two type fields, the shapes stand on the side of the floor
they are there for, and the special-value frame produces, with the reference
alone, every class of result the GPU test compares."""
import numpy as np
import pytest
from avir_amd import abi
from tests import helpers as H
from tests import plancmp
from tests import sacc16_cases as S

_names = sorted(S.SHAPES)


def _desc(geom, ti, to, ch=4):
    sw, sh, nw, nh = geom
    return H.product_desc(sw, sh, nw, nh, ch, in_type=ti, out_type=to,
                          resbits=16)


@pytest.mark.parametrize("name", _names)
def test_step_kinds_per_axis_and_channel_count(name):
    """Resize-then-filter ([3, 0]) where the accumulation kernels run the axis,
    at 1-4 channels (whether the forced path accepts the plan takes a device
    to tell: the GPU test asserts it)."""
    for ch in (1, 2, 3, 4):
        r, d = _desc(S.geom(name), abi.F32, abi.F32, ch)
        try:
            c = d.contents
            got = tuple([ax.steps[i].kind for i in range(ax.n_steps)]
                        for ax in (c.h, c.v))
            assert got == S.SHAPES[name][1], (name, ch, got)
        finally:
            H.free_product_desc(r, d)


def _not_types(bad):
    return [b for b in bad if not b.startswith(("in_type:", "out_type:"))]


@pytest.mark.parametrize("t", ["f16", "bf16"])
@pytest.mark.parametrize("ch", [4, 3])
@pytest.mark.parametrize("name", _names)
def test_desc_equals_float32_desc(name, ch, t):
    geom = S.geom(name)
    r1, d1 = _desc(geom, S.T[t][0], S.T[t][0], ch)
    r2, d2 = _desc(geom, abi.F32, abi.F32, ch)
    try:
        a, b = d1.contents, d2.contents
        assert (a.in_type, a.out_type) == (S.T[t][0], S.T[t][0])
        assert (b.in_type, b.out_type) == (abi.F32, abi.F32)
        assert _not_types(plancmp.compare_desc(a, b)) == []
    finally:
        H.free_product_desc(r1, d1)
        H.free_product_desc(r2, d2)


def test_shapes_stand_on_their_side_of_the_floor():
    assert S.FLOOR == 65536
    for name in _names:
        if name == "floor":
            assert S.pixels(name) < S.FLOOR
            assert S.geom(name) == (300, 200, 100, 67)
        else:
            assert S.pixels(name) >= S.FLOOR, name
    for name in S.NARROW:
        assert S.geom(name)[0] in (9, 8, 7, 5)
    assert S.CHUNKS == [1, 2, 3, 5, 17]
    assert set(S.PAIR_SHAPES + S.HELD_SHAPES + S.NARROW) <= set(S.SHAPES)
    assert len(S.PAIRS) == 11 and set(S.SAME) <= set(S.PAIRS)


@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_special_frame_has_every_class(t):
    """384x288 -> 150x113: every class special_classes names for the type is
    there at this size (nothing had to be enlarged)."""
    src, ref, want = S.special_case(t)
    assert src.dtype == S.T[t][1] and want.dtype == S.T[t][1]
    c = S.special_classes(t, ref, want)
    print(t, c)
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    assert c["denormal"] > 0
    if t == "f16":
        assert c["fin_to_inf"] > 0
        blk = src[44:84, 100:160].astype(np.float32)
        assert ((blk != 0) & (np.abs(blk) < 2.0 ** -14)).all()
    # the frame with its non-finite elements replaced is finite, and another
    fin = S.finite_of(src, t)
    assert np.isfinite(S.as_f32(fin, t)).all()
    assert int((S.words(fin) != S.words(src)).sum()) > 0
