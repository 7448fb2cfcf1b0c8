"""Host-only check of the case table of tests/test_gpu_window.py: a band whose
source window is the whole frame would test nothing, so every case has to be
a true window -- by the planner's own answer (the band_source_rows queries of
the front ends need no device)."""
import pytest
from tests import window_cases as W


@pytest.mark.parametrize("case", W.CASES, ids=W.IDS)
def test_every_case_is_a_true_window(case):
    sh, nh, ex = case[2], case[4], case[11]
    obj, arg = W.front_end(case)
    need = {}
    for name, r0, r1 in W.bands(nh):
        a, b = W.host_source_rows(case, obj, arg, r0, r1)
        assert 0 <= a <= b < sh, (name, a, b)
        need[name] = b - a + 1
    assert need["inner"] < need["frame"] <= sh  # (k given: maybe not all)
    if ex.get("small"):
        # (the one k_up2 frame below a chunk height: bands of a 48-row frame
        # with 9 rows of halo a side cannot meet the shares, and say so here)
        assert sh < 62
        return
    assert need["inner"] * 2 < sh, need
    assert need["row"] * 2 < sh, need
    assert need["first"] * 4 < sh * 3, need
    assert need["last"] * 4 < sh * 3, need


def test_the_table_names_its_cases_once():
    assert len(set(W.IDS)) == len(W.IDS)
