"""gpass_run's routes (avir_amd/csrc/gpass.hip, gpass_route): every row of
tests/gpass_route_cases.py on a plan forced to PATH_GPASS, as a whole frame and
as three bands (one of a single row), from and into device memory, against the
reference (tests/helpers.py). Raw words are compared, the bar is 0 differing
words; where an Inf and a NaN are planted a NaN only has to be a NaN. That a
row's shapes take the kernels it is named after is what
tools/gpass_route_trace.py records (profiles/gpass_route/)."""
import numpy as np
import pytest
from avir_amd import abi
from tests import helpers as H
from tests import gpass_route_cases as G
from tests import window_cases as W

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if want.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), "%s: NaNs in other places (%d vs %d)" % (
            what, int(gn.sum()), int(wn.sum()))
        got, want = np.where(gn, 0, got), np.where(wn, 0, want)
    n = int((_bits(got) != _bits(want)).sum())
    assert n == 0, "%s: %d of %d raw words differ" % (what, n, want.size)


def _want(c, img):
    fe, sw, sh, nw, nh, ch, tin, tout, bits = c[:9]
    if fe == "lancir":
        return H.checker_lancir(img, nw, nh, out_dtype=tout)
    return H.checker_avir(img, nw, nh, out_dtype=tout, resbits=bits, threads=8)


@pytest.mark.parametrize("name", G.NAMES)
def test_route(name):
    lib = abi.load()
    for (c, env, images) in G.row(name)[1]:
        nh = c[4]
        wants = {k: _want(c, G.image(c, k)) for k in set(images)}
        srcs = {k: G.to_device(G.flat(G.image(c, k), W.pitch(c)))
                for k in set(images)}
        with G.environment(env):
            obj, p = G.plan(c)
            for i, kind in enumerate(images):
                for how, rows in (("frame", [(0, nh)]), ("bands", G.bands(nh))):
                    what = "%s %s %s %d:%s %s" % (name, W.case_id(c), env, i,
                                                  kind, how)
                    rcs, got = G.run_device(lib, p, c, srcs[kind], rows)
                    assert rcs == [0] * len(rows), "%s: %r %s" % (
                        what, rcs, lib.avirhip_last_error())
                    _same(got, wants[kind], what)


def test_route_refusal():
    """A float RGBA two-pass plan called with a destination that is 4 bytes off
    16-byte alignment: the forced path refuses the call, the automatic path
    runs it on kernels that take it."""
    lib = abi.load()
    c = G._c("avir", 64, 48, 100, 77, 4, np.float32, np.float32,
             abi.VARIANT_UPG_TWO_PASS)[0]
    img = G.image(c, "clean")
    want = _want(c, img)
    dsrc = G.to_device(img)
    obj, p = G.plan(c)
    rcs, got = G.run_device(lib, p, c, dsrc, [(0, c[4])], dst_off=4)
    assert rcs == [abi.EUNSUPPORTED], rcs
    assert lib.avirhip_last_error() == \
        b"path 5 cannot run this call (unaligned buffers?)"
    assert not got.any(), "a refused call wrote its destination"
    obj0, p0 = G.plan(c, path=0)
    rcs, got = G.run_device(lib, p0, c, dsrc, [(0, c[4])], dst_off=4)
    assert rcs == [0], (rcs, lib.avirhip_last_error())
    _same(got, want, "automatic path, destination at +4")
