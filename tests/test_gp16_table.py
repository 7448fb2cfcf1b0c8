"""Host-only checks of the inputs of tests/test_gpu_gp16.py
(tests/gp16_cases.py): every shape plans as the pass kernels' material (two
steps per axis: a filter and a resize, in either order), a half / bfloat16
description is the float32 one but for the two type fields, and the special-
value frames produce, with the reference alone, every class of result the GPU
test is there to compare."""
import numpy as np
import pytest
from avir_amd import abi
from tests import helpers as H
from tests import plancmp
from tests import gp16_cases as G

_names = sorted(G.ROUTES)


def _desc(geom, ti, to, ch=4):
    sw, sh, nw, nh = geom
    return H.product_desc(sw, sh, nw, nh, ch, in_type=ti, out_type=to,
                          resbits=16)


@pytest.mark.parametrize("name", _names)
def test_shapes_are_the_pass_kernels(name):
    """Each axis has the steps gpass.hip's match_avir_axis takes (whether the
    forced path accepts the plan takes a device to tell: the GPU test asserts
    it for every shape)."""
    geom = G.geom(name)
    assert G.CHANNELS[name][0] == 4
    for ch in G.CHANNELS[name]:
        r, d = _desc(geom, abi.F32, abi.F32, ch)
        try:
            c = d.contents
            got = tuple([ax.steps[i].kind for i in range(ax.n_steps)]
                        for ax in (c.h, c.v))
            assert got == G.AXES[name], (name, ch)
        finally:
            H.free_product_desc(r, d)
    for which in (G.SPECIAL_UP, G.SPECIAL_DN):
        r, d = _desc(which[0] + which[1], abi.F32, abi.F32)
        try:
            c = d.contents
            got = [ax.steps[i].kind for ax in (c.h, c.v)
                   for i in range(ax.n_steps)]
            assert got == 2 * (G.AX_UP if which is G.SPECIAL_UP
                               else G.AX_BETWEEN)
        finally:
            H.free_product_desc(r, d)


def test_tiny_and_thin_sources():
    """Which of the smallest sources plan as the pass kernels' material."""
    def kinds(g):
        sw, sh, nw, nh, ch = g
        r, d = _desc((sw, sh, nw, nh), abi.F32, abi.F32, ch)
        try:
            c = d.contents
            return tuple([ax.steps[i].kind for i in range(ax.n_steps)]
                         for ax in (c.h, c.v))
        finally:
            H.free_product_desc(r, d)
    for g in G.THIN:
        assert kinds(g) == (G.AX_UP, G.AX_UP), g
        assert g[0] * g[4] == 3
    ours = (G.AX_UP, G.AX_BETWEEN, G.AX_DOWN)
    for g in G.TINY:
        k = kinds(g)
        assert not (k[0] in ours and k[1] in ours), g


def _not_types(bad):
    return [b for b in bad if not b.startswith(("in_type:", "out_type:"))]


@pytest.mark.parametrize("t", ["f16", "bf16"])
@pytest.mark.parametrize("ch", [4, 3])
@pytest.mark.parametrize("name", _names)
def test_desc_equals_float32_desc(name, ch, t):
    geom = G.geom(name)
    r1, d1 = _desc(geom, G.T[t][0], G.T[t][0], ch)
    r2, d2 = _desc(geom, abi.F32, abi.F32, ch)
    try:
        a, b = d1.contents, d2.contents
        assert (a.in_type, a.out_type) == (G.T[t][0], G.T[t][0])
        assert (b.in_type, b.out_type) == (abi.F32, abi.F32)
        assert _not_types(plancmp.compare_desc(a, b)) == []
        for f in ("use_srgb_gamma", "alpha_index", "dither", "work_f64"):
            assert getattr(a, f) == getattr(b, f), f
    finally:
        H.free_product_desc(r1, d1)
        H.free_product_desc(r2, d2)


def test_cases_cover_the_issue():
    assert set(G.BOTH_FUSED + G.STORE_ONLY) <= set(G.ROUTES)
    assert len(G.PAIRS) == 11 and set(G.SAME) <= set(G.PAIRS)
    assert G.geom("last_strip")[2] % 64 == 1
    assert G.geom("narrow")[0] == 49
    assert G.GH_CHUNKS == [1, 2, 3, 5]
    for a, b in G.PAIRS:
        assert a in ("f16", "bf16") or b in ("f16", "bf16")


@pytest.mark.parametrize("which", [G.SPECIAL_UP, G.SPECIAL_DN],
                         ids=["up", "down"])
def test_half_frame_has_every_class(which):
    src, ref, want = G.special_case("f16", which)
    assert src.dtype == np.float16 and want.dtype == np.float16
    c = G.special_classes("f16", ref, want)
    print(which, c)
    assert c["fin_to_inf"] > 0
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    assert c["denormal"] > 0


@pytest.mark.parametrize("src_t", ["f32", "bf16"])
@pytest.mark.parametrize("which", [G.SPECIAL_UP, G.SPECIAL_DN],
                         ids=["up", "down"])
def test_bfloat16_frame_has_every_class(which, src_t):
    if src_t == "f32":
        src, ref, want = G.special_case("bf16", which)
        assert src.dtype == np.float32
    else:
        src, ref, want = G.special_bf16_case(which)
        assert src.dtype == np.uint16
    c = G.special_classes("bf16", ref, want)
    print(which, src_t, c)
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    assert c["denormal"] > 0
    wf = G.widen(want)
    assert np.array_equal(np.isnan(wf), np.isnan(ref))


@pytest.mark.parametrize("which", [G.SPECIAL_UP, G.SPECIAL_DN],
                         ids=["up", "down"])
def test_source_denormals_reach_the_result(which):
    """The half frame's block of denormals: a loader that flushed them would
    give the flushed frame's result, which is another."""
    src, ref, want = G.special_case("f16", which)
    blk = src[44:84, 100:160].astype(np.float32)
    assert ((blk != 0) & (np.abs(blk) < 2.0 ** -14)).all()
    fsrc, fref, fwant = G.special_case("f16", which, flushed=True)
    assert (fsrc[44:84, 100:160] == 0).all()
    differ = int((G.words(want) != G.words(fwant)).sum())
    print(which, "elements that differ from the flushed frame's:", differ)
    assert differ > 0
