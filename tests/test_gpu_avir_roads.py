"""avir_road's outcomes (avir_amd/csrc/api.cpp): every row of
tests/avir_road_cases.py as a whole frame and as bands, from and into device
memory between guard bytes, against the reference. Raw words are compared, the
bar is 0 differing words; the guard bytes stay untouched; and the stages and
kernels the whole-frame call names under AVIRHIP_VERBOSE are the row's list, in
order -- the road the call took, recorded from the library before avir_road
(tools/avir_road_trace.py, profiles/avir_road/).

check_road is the body of this test and of tests/test_gpu_lanc_roads.py's: `R`
is the case module, `same` its comparison."""
import re
import pytest
from avir_amd import abi
from tests import avir_road_cases as R
from tests import dnf16_cases as D16

pytestmark = pytest.mark.gpu

TAG = re.compile(r"^(k_\w+|pack pass|output stage):", re.M)


def _same(r, got, want, what):
    if want.size == 0:
        return  # (no reference for this class on this machine: H.need_ref)
    D16.same(got.view(want.dtype), want, r["tout"], what)


def _frame(R, lib, r, p, sptr, capfd):
    with R.environment(dict(r["env"], AVIRHIP_VERBOSE="1")):
        capfd.readouterr()
        rcs, got, clean = R.run(lib, p, r, sptr, [(0, r["geom"][3])])
        tags = TAG.findall(capfd.readouterr().err)
    return rcs[0], got, clean, tags


def check_road(R, name, capfd, same):
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    r = R.row(name)
    src, want = R.case(r)
    keep, sptr = R.device_source(r, src)
    with R.environment(r["env"]):
        obj, p = R.plan(r)
    rc, got, clean, tags = _frame(R, lib, r, p, sptr, capfd)
    print(name, rc, tags)
    assert clean, name + ": stored outside the image"
    if r["rc"] != 0:
        # the forced path refuses these pointers and writes nothing; the
        # automatic path serves them
        assert rc == r["rc"], (rc, lib.avirhip_last_error())
        assert lib.avirhip_last_error() == (
            b"path %d cannot run this call (unaligned buffers?)" % r["path"])
        assert (got == R.GUARD).all(), "a refused call wrote its destination"
        obj, p = R.plan(r, 0)
        rc, got, clean, tags = _frame(R, lib, r, p, sptr, capfd)
        assert clean, name + ": stored outside the image (automatic path)"
    assert rc == 0, (rc, lib.avirhip_last_error())
    same(r, got, want, name + " frame")
    assert tags == r["tags"], (name, tags)
    calls = R.bands(r)
    if calls:
        with R.environment(r["env"]):
            rcs, got, clean = R.run(lib, p, r, sptr, calls)
        assert rcs == [0] * len(calls), (rcs, lib.avirhip_last_error())
        assert clean, name + ": a band stored outside the image"
        same(r, got, want, name + " bands")


@pytest.mark.parametrize("name", R.NAMES)
def test_road(name, capfd):
    check_road(R, name, capfd, _same)
