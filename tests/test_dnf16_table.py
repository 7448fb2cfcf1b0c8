"""Host-only checks of the inputs of tests/test_gpu_dnf16.py
(tests/dnf16_cases.py): the special-value frames produce, with the reference
alone, every class of result the GPU test is there to compare; and the variant
switch of the Python ABI is the header's."""
import os
import re
import numpy as np
import pytest
from avir_amd import abi
from tests import dnf16_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("out", D.SPECIAL_OUT, ids=["22", "33", "23", "32"])
def test_half_frame_has_every_class(out):
    src, ref, want = D.special_case("f16", out)
    assert src.dtype == np.float16 and src.shape == (144, 192, 4)
    c = D.special_classes("f16", ref, want)
    print(out, c)
    # finite float32 results beyond 65504 that the narrowing turns into Inf,
    # the source's own +-Inf, NaN (but not a frame of them), half denormals
    assert c["fin_to_inf"] >= 16
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    assert c["denormal"] >= 1000
    assert want.dtype == np.float16


@pytest.mark.parametrize("out", D.SPECIAL_OUT, ids=["22", "33", "23", "32"])
def test_bfloat16_frame_has_every_class(out):
    src, ref, want = D.special_case("bf16", out)
    assert src.dtype == np.float32
    c = D.special_classes("bf16", ref, want)
    print(out, c)
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    assert c["denormal"] >= 1536
    # (the narrowing itself: Inf and NaN stay what they are)
    wf = D.widen(want)
    assert np.array_equal(np.isnan(wf), np.isnan(ref))
    assert np.array_equal(np.isinf(wf) & np.isinf(ref), np.isinf(ref))


@pytest.mark.parametrize("t", ["f16", "bf16"])
@pytest.mark.parametrize("out", D.SPECIAL_BIG_OUT, ids=["22", "33", "23", "32"])
def test_big_frame_has_every_class(out, t):
    """The frame whose four results all are k_dnfh's."""
    src, ref, want = D.special_case(t, out, D.SPECIAL_BIG_SRC)
    c = D.special_classes(t, ref, want)
    print(t, out, c)
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0 and c["denormal"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    if t == "f16":
        assert c["fin_to_inf"] > 0


def _steps(geom):
    from tests import helpers as H
    r, d = H.product_desc(geom[0], geom[1], geom[2], geom[3], 4, resbits=16)
    n = (d.contents.h.n_steps, d.contents.v.n_steps)
    H.free_product_desc(r, d)
    return n


def test_which_shapes_are_the_kernels():
    """k_dnf / k_dnfh match a two-step axis (resize, correction filter)."""
    for g in D.DNF_SHAPES:
        assert _steps(g) == (2, 2), g
    for nw, nh in D.SPECIAL_BIG_OUT:
        assert _steps(D.SPECIAL_BIG_SRC + (nw, nh)) == (2, 2)
    assert _steps(D.SPECIAL_SRC + (64, 48)) == (2, 2)
    # (a filter in front of the resize: the tiles' plan)
    assert _steps((170, 122, 85, 61)) == (3, 3)
    assert _steps((384, 216, 128, 108)) == (2, 3)
    forms = set((g[0] // g[2], g[1] // g[3]) for g in D.DNF_SHAPES)
    assert forms == {(2, 2), (3, 3), (2, 3), (3, 2)}
    assert _steps(D.SPECIAL_SRC + (96, 72)) == (3, 3)


def test_shapes_are_whole_ratios():
    forms = set()
    assert D.EXTRA_SHAPES[0][2] % 42 == 1 and D.EXTRA_SHAPES[0][0] == 254
    for sw, sh, nw, nh in D.SHAPES:
        assert sw % nw == 0 and sh % nh == 0
        kh, kv = sw // nw, sh // nh
        assert kh in (2, 3) and kv in (2, 3)
        forms.add((kh, kv))
    assert forms == {(2, 2), (3, 3), (2, 3), (3, 2)}
    # a last strip one column wide, for K = 2 and for K = 3
    assert [g[2] % 42 for g in D.SHAPES[4:6]] == [1, 1]
    for (nw, nh) in D.SPECIAL_OUT:
        assert D.SPECIAL_SRC[0] // nw in (2, 3)
        assert D.SPECIAL_SRC[1] // nh in (2, 3)


def test_variant_is_the_headers():
    with open(os.path.join(ROOT, "include", "avirhip.h")) as fh:
        m = re.search(r"#define\s+AVIRHIP_VARIANT_DN_UNFUSED_IO\s+(\d+)",
                      fh.read())
    assert m is not None
    assert abi.VARIANT_DN_UNFUSED_IO == int(m.group(1)) == 128
