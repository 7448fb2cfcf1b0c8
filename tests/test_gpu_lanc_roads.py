"""lanc_road's attempts (avir_amd/csrc/api.cpp): every row of
tests/lanc_road_cases.py as a whole frame and as bands, from and into device
memory between guard bytes, against the reference's CLancIR. Raw words are
compared, the bar is 0 differing words; the guard bytes stay untouched; and the
stages and kernels the whole-frame call names under AVIRHIP_VERBOSE are the
row's list, in order -- the road the call took, recorded from the library
before lanc_road (tools/avir_road_trace.py --cases lanc, profiles/lanc_road/).
The body is tests/test_gpu_avir_roads.py's."""
import pytest
from tests import lanc_road_cases as R
from tests.test_gpu_avir_roads import check_road

pytestmark = pytest.mark.gpu


def _same(r, got, want, what):
    R.same(got, want, r["tout"], what)


@pytest.mark.parametrize("name", R.NAMES)
def test_road(name, capfd):
    check_road(R, name, capfd, _same)
