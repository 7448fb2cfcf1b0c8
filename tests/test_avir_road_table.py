"""Host-only check of the road table of tests/test_gpu_avir_roads.py
(tests/avir_road_cases.py): every attempt named in the comment table above
avir_road (avir_amd/csrc/api.cpp) has a row, every row's shape lies in the case
module it claims, and no source is larger than 600x402 pixels."""
import os
import re
from tests import avir_road_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    """The first column of the comment table above avir_road."""
    with open(os.path.join(ROOT, "avir_amd", "csrc", "api.cpp")) as fh:
        text = fh.read()
    head = text.index("//   attempt        path   condition")
    body = text[head:text.index("static Road avir_road(", head)]
    names = []
    for line in body.split("\n")[1:]:
        m = re.match(r"^//   (\S.*?)\s{2,}\S", line)
        if not m:
            if line.strip() == "//":
                break
            continue
        names.append(m.group(1))
    return names


def test_every_outcome_of_the_comment_table_has_a_row():
    names = _table()
    assert names == R.OUTCOMES, names
    have = set(r["outcome"] for r in R.ROWS)
    for n in names:
        assert n in have, n
    assert have <= set(names), have - set(names)
    assert len(set(R.NAMES)) == len(R.NAMES)


def test_every_shape_lies_in_its_case_module():
    for r in R.ROWS:
        assert r["geom"] in R.module_shapes(r["module"]), r["name"]
        assert r["tin"] in R.T and r["tout"] in R.T, r["name"]


def test_no_row_is_larger_than_600x402():
    for r in R.ROWS:
        sw, sh, nw, nh = r["geom"]
        assert sw * sh <= R.MAX_SRC_PIXELS, r["name"]


def test_tag_lists_are_stages_and_kernels():
    for r in R.ROWS:
        assert isinstance(r["tags"], list), r["name"]
        for t in r["tags"]:
            assert t in (R.PACK, R.OUT) or re.match(r"^k_\w+$", t), r["name"]
