"""Host-only check of the road table of tests/test_gpu_lanc_roads.py
(tests/lanc_road_cases.py): every attempt named in the comment table above
lanc_road (avir_amd/csrc/api.cpp) has a row, every row's shape lies in the
module it claims, and no source is larger than 600x402 pixels -- but the one
row that stands at the automatic path's threshold."""
import os
import re
from tests import lanc_road_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    """The first column of the comment table above lanc_road."""
    with open(os.path.join(ROOT, "avir_amd", "csrc", "api.cpp")) as fh:
        text = fh.read()
    end = text.index("static Road lanc_road(")
    head = text.rindex("//   attempt        path   sides and condition", 0,
                       end)
    names = []
    for line in text[head:end].split("\n")[1:]:
        m = re.match(r"^//   (\S.*?)\s{2,}\S", line)
        if not m:
            if line.strip() == "//":
                break
            continue
        names.append(m.group(1))
    return names


def test_every_attempt_of_the_comment_table_has_a_row():
    names = _table()
    assert names == R.OUTCOMES, names
    have = set(r["outcome"] for r in R.ROWS)
    for n in names:
        assert n in have, n
    assert have <= set(names), have - set(names)
    assert len(set(R.NAMES)) == len(R.NAMES)


def test_every_shape_lies_in_its_module():
    for r in R.ROWS:
        assert r["geom"] in R.module_shapes(r["module"]), r["name"]
        assert r["tin"] in R.T and r["tout"] in R.T, r["name"]


def test_no_row_is_larger_than_600x402_but_the_threshold_row():
    large = []
    for r in R.ROWS:
        sw, sh, nw, nh = r["geom"]
        if sw * sh > R.MAX_SRC_PIXELS:
            large.append(r["name"])
    assert large == R.LARGE == ["auto4_u8c4"], large
    # (finalize_lancir_plan: the automatic path is 4 from here on)
    sw, sh, nw, nh = R.row("auto4_u8c4")["geom"]
    assert sw * sh == 1500000 and (nw, nh) == (2 * sw, 2 * sh)
    assert R.row("auto4_u8c4")["path"] == 0


def test_tag_lists_are_stages_and_kernels():
    for r in R.ROWS:
        assert isinstance(r["tags"], list), r["name"]
        for t in r["tags"]:
            assert t in (R.PACK, R.OUT) or re.match(r"^k_\w+$", t), r["name"]
