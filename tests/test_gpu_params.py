"""Every kernel family under non-default CImageResizerParams: for each
parameter set and geometry class of tests/param_cases.py, every frame of the
class on every path / variant / environment the class names. A combination
avirhip_plan_set_path accepts gives the reference's whole frame and three row
bands (one of them a single row) bit for bit; whether it is accepted is
asserted against param_cases.expect(), which is derived from the chain shape
of tests/test_params_table.py's TABLE -- an unexpected refusal fails, and so
does an unexpected acceptance.

Expected pixels are the real reference's (tests/helpers.py checker_avir with
params=; the double pipeline against its variant 4). Raw words are compared,
the bar is 0 differing elements."""
import os
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import helpers as H
from tests import param_cases as PC
from tests import refbind as rb
from tests.test_params_table import shape_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    lib = abi.load()
    assert lib.avirhip_device_count() >= 1, "no gfx950 device"
    abi.check(lib.avirhip_init(0), "init")


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def _same(got, want, what, problems):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        problems.append("%s: %d of %d elements differ; first at %s: got %r "
                        "want %r" % (what, len(bad), g.size, i, got[i],
                                     want[i]))


_IMAGES = {}


def _image(frame):
    """The source image of a frame: one per (size, channels, type), shared by
    every parameter set and never written."""
    sw, sh, nw, nh, ch, tin, tout, bits, fp = frame
    key = (sw, sh, ch, np.dtype(tin).name)
    if key not in _IMAGES:
        t = np.dtype(tin)
        if t.kind == "u":
            raw = rb.lcg_u8((sh, sw, ch, t.itemsize), seed=sw + ch)
            a = np.ascontiguousarray(raw).view(t).reshape(sh, sw, ch)
        else:
            a = rb.lcg_f32((sh, sw, ch), seed=7 * sw + ch)
            if t == np.float64:
                # (mantissa bits a float does not hold)
                b = rb.lcg_f32((sh, sw, ch), seed=sh)
                a = a.astype(np.float64) + b.astype(np.float64) * 2.0 ** -25
        a.setflags(write=False)
        _IMAGES[key] = a
    return _IMAGES[key]


def _want(name, frame, img):
    sw, sh, nw, nh, ch, tin, tout, bits, fp = frame
    kw = {}
    if fp == PC.DBL:
        assert H.need_ref("the double class")
        kw["variant"] = 4
    return H.checker_avir(img, nw, nh, out_dtype=tout, resbits=bits,
                          params=PC.SETS[name], threads=8, **kw)


class _Env(object):
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.keep = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bands(nh):
    return [(0, nh // 3), (nh // 3, nh // 3 + 1), (nh // 3 + 1, nh)]


# (set, class) -> the paths that executed; filled by the parametrised test,
# read by the test behind it
RAN = {}
COUNTS = {}


@pytest.mark.parametrize("cls", PC.CLASS_NAMES)
@pytest.mark.parametrize("name", PC.SET_NAMES)
def test_parameter_set_on_every_path(name, cls):
    lib = abi.load()
    problems = []
    ran = set()
    n_ran = n_refused = 0
    for frame, runs in PC.CLASSES[cls]:
        sw, sh, nw, nh, ch, tin, tout, bits, fp = frame
        shape = shape_of(name, cls, frame)
        img = _image(frame)
        want = _want(name, frame, img)
        assert want.shape == (nh, nw, ch) and want.dtype == np.dtype(tout)
        r = avir_amd.CImageResizer(bits, 0, PC.product_params(name),
                                   aFpPack=fp)
        ti, to = avir_amd._NP2T[np.dtype(tin)], avir_amd._NP2T[np.dtype(tout)]
        p = r.plan(sw, sh, nw, nh, ch, 0.0, None, ti, to)
        for path, variant, env in runs:
            what = "%s %s" % (name, PC.case_id(frame, path, variant, env))
            why = PC.expect(shape, frame, path)
            rc = lib.avirhip_plan_set_path(p, path)
            if rc != 0:
                assert rc == abi.EUNSUPPORTED, (what, rc)
                n_refused += 1
                print("%s: refused (%s)" % (what, why))
                if why is None:
                    problems.append("%s: refused, the table says it runs"
                                    % what)
                continue
            if why is not None:
                # (not executed: the chain is foreign to the path's kernels)
                problems.append("%s: accepted, the table says refused: %s"
                                % (what, why))
                continue
            abi.check(lib.avirhip_plan_set_variant(p, variant), "set_variant")
            took = lib.avirhip_plan_get_path(p)
            assert took == path or path == 0, (what, took)
            if path == 0:
                fast = PC.expect_auto(shape, frame)
                if (took in fast) != bool(fast) or (not fast and took != 1):
                    problems.append("%s: automatic path %d, the table allows "
                                    "%r" % (what, took, fast or [1]))
            with _Env(env):
                got = np.zeros((nh, nw, ch), tout)
                abi.check(lib.avirhip_resize(
                    p, img.ctypes.data, abi.MEM_HOST, got.ctypes.data,
                    abi.MEM_HOST, None), what)
                out = np.zeros((nh, nw, ch), tout)
                for a_, b_ in _bands(nh):
                    abi.check(lib.avirhip_resize_band(
                        p, img.ctypes.data, abi.MEM_HOST,
                        out[a_:b_].ctypes.data, abi.MEM_HOST, a_, b_, None),
                        what + " band")
            _same(got, want, what, problems)
            for a_, b_ in _bands(nh):
                _same(out[a_:b_], want[a_:b_],
                      "%s rows [%d, %d)" % (what, a_, b_), problems)
            ran.add(took)
            n_ran += 1
            print("%s: ran on path %d" % (what, took))
        abi.check(lib.avirhip_plan_set_variant(p, 0), "set_variant")
    RAN[(name, cls)] = ran
    COUNTS[(name, cls)] = (n_ran, n_refused)
    print("%s / %s: %d combinations ran, %d refused" % (name, cls, n_ran,
                                                        n_refused))
    assert not problems, "\n".join(problems)
    if name in PC.SEVEN_TAP:
        # (each such pair asserts it here: their count is zero)
        assert ran - {1}, "nothing but the generic kernels ran: %r" % ran


def test_no_seven_tap_set_is_left_to_the_generic_kernels():
    """Behind the cases above: the number of (7-tap set, class) pairs in
    which nothing but path 1 executed is zero (every case asserts its own
    pair too); prints what each set ran / was refused."""
    for s in PC.SET_NAMES:
        got = [COUNTS[(s, c)] for c in PC.CLASS_NAMES if (s, c) in COUNTS]
        print("%s: %d ran, %d refused" % (s, sum(g[0] for g in got),
                                          sum(g[1] for g in got)))
    only1 = [k for k in RAN if k[0] in PC.SEVEN_TAP and not RAN[k] - {1}]
    assert len(only1) == 0, only1


@pytest.mark.parametrize("name", PC.SET_NAMES)
def test_automatic_path_at_real_sizes(name):
    """Plans only, nothing executed: a 7-tap set lands on a fast path whose
    kernels take its chain (never on the generic kernels), the default where
    the automatic choice's comments say, the other sets on the tiles."""
    lib = abi.load()
    from tests.helpers import product_desc, free_product_desc
    for (sw, sh, nw, nh, ch, t, bits), dflt in zip(PC.BIG,
                                                   PC.BIG_DEFAULT_PATHS):
        ty = avir_amd._NP2T[np.dtype(t)]
        rh, d = product_desc(sw, sh, nw, nh, ch, in_type=ty, out_type=ty,
                             resbits=bits, params=PC.SETS[name])
        try:
            shape = PC.desc_shape(d.contents)
        finally:
            free_product_desc(rh, d)
        frame = (sw, sh, nw, nh, ch, t, t, bits, 1)
        fast = PC.expect_auto(shape, frame)
        r = avir_amd.CImageResizer(bits, 0, PC.product_params(name))
        p = r.plan(sw, sh, nw, nh, ch, 0.0, None, ty, ty)
        took = lib.avirhip_plan_get_path(p)
        print("%s %dx%d -> %dx%d: path %d of %r" % (name, sw, sh, nw, nh,
                                                    took, fast))
        assert fast and took in fast, (name, frame, took, fast)
        for path in (2, 4, 5):
            rc = lib.avirhip_plan_set_path(p, path)
            assert (rc == 0) == (path in fast), (name, frame, path, rc)
        if name == "def":
            assert took == dflt, (frame, took)
        if name in PC.SEVEN_TAP and dflt != abi.PATH_TILED:
            # upsizing plans: k_up2 where its predicate holds (float RGBA
            # output), the pass kernels otherwise -- float RGBA sources
            # always, RGB uint8 from 2 Mpixel outputs on (gpass_preferred);
            # the downsizing README frame may take any path that runs it
            if nw > sw:
                assert took == (abi.PATH_UP2 if abi.PATH_UP2 in fast
                                else abi.PATH_GPASS), (name, frame, took)
        if name in PC.OTHER_TAP:
            assert fast == [abi.PATH_TILED] and took == abi.PATH_TILED
