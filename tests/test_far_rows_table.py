"""Host-only check of the case table of tests/test_gpu_far_rows.py
(tests/far_row_cases.py): every derived pitch stands on the side of the row's
own limit it is meant to, is a 16-byte multiple that fits int32 elements and
implies an allocation under the cap; every family's file has a row; and the
text each row quotes still stands at the file:line it names -- a guard edited
later fails here and sends the reader back to the row."""
import os
import re
import pytest
from tests import far_row_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _norm(s):
    return " ".join(s.split())


@pytest.mark.parametrize("name", F.NAMES)
def test_levels_stand_where_they_are_meant_to(name):
    r = F.row(name)
    es = F.esz_of(r)
    q = 16 // es
    lv = {l.name: l for l in F.levels(r)}
    assert list(lv) == list(F.LEVELS)
    under, over, wrap = lv["under"], lv["over"], lv["wrap"]
    # on the intended side of the row's own expression, and adjacent: nothing
    # lies between the two
    assert under.inside and not over.inside
    assert F.inside(r, under.pitch, under.sh)
    assert not F.inside(r, over.pitch, over.sh)
    if r["by"] == "rows":
        assert over.sh == under.sh + 1 and over.pitch == under.pitch
        # the largest pitch k_up2 admits (up2.hip: below 1 << 22 bytes)
        assert under.pitch * es == (1 << 22) - 16
        assert F.span(r, wrap.pitch, wrap.sh) > F.GIB4
        assert F.span(r, wrap.pitch, wrap.sh - 1) <= F.GIB4
        # the frame of ADVICE.md's third item is one of the levels
        assert wrap.sh == 1026
    else:
        assert over.pitch == under.pitch + q and over.sh == under.sh
        assert F.span(r, wrap.pitch) > F.GIB4
        assert F.span(r, wrap.pitch - q) <= F.GIB4
    width = (r["nw"] if r["by"] == "dst" else r["sw"]) * r["ch"]
    for l in lv.values():
        assert l.pitch >= width, l
        assert (l.pitch * es) % 16 == 0, l
        assert 0 < l.pitch <= 2 ** 31 - 1, l
        assert l.alloc == F.span(r, l.pitch, l.sh)
        # a level over the cap is dropped, and says so; the others fit
        assert (l.dropped is None) == (l.alloc + (64 << 20) <= F.CAP), l
    # a row none of whose levels can run would test nothing
    assert any(l.dropped is None and (l.inside or not r["limit"]["guard"])
               for l in lv.values()), name


def test_only_the_cap_drops_levels():
    dropped = [(r["name"], l.name) for r in F.ROWS for l in F.levels(r)
               if l.dropped]
    # k_lanc2's float rows: its limit is 2^31 ELEMENTS, 8 GiB of floats
    assert dropped == [("lanc2_f32", "under"), ("lanc2_f32", "over")]
    assert F.level(F.row("lanc2_f32"), "wrap").inside


def test_every_family_file_has_a_row():
    have = set(f for r in F.ROWS for f in r["files"])
    for f in F.FILES:
        assert f in have or len(F.LEFT_OUT.get(f, "")) > 20, f
        assert os.path.exists(os.path.join(ROOT, F.CSRC, f)), f
    assert len(set(F.NAMES)) == len(F.NAMES)
    for g in F.GROUPS:
        assert F.group(g)


def test_element_types_the_families_read_themselves():
    def types(prefix):
        return set(r["tin"] for r in F.ROWS if r["name"].startswith(prefix))
    assert types("up2_raw") == {"u8", "u16", "f16", "bf16"}
    assert types("lanc2_raw") == {"u8", "u16"}
    assert {"u8", "u16"} <= types("sacc2")
    assert {"u8", "u16"} <= types("dn_two_pass")
    assert {"u8", "u16"} <= types("tiles_")
    assert {"u8", "u16"} <= types("lanc_fused_owner")
    assert "f64" in types("lanc_f64") and "f64" in types("tile64")
    assert "f64" in types("up64")
    # float32 wherever the family takes it
    for p in ("generic_", "tiles_", "tile_fused", "dnf_", "dn_two_pass",
              "up2_f32", "gpass_", "sacc_", "lanc_fused_f32", "lanc_two_pass",
              "lanc2_f32", "generic64"):
        assert "f32" in types(p), p


_quotes = sorted(set(
    [(r["limit"]["where"], r["limit"]["quote"]) for r in F.ROWS] +
    [q for r in F.ROWS for q in r["also"]]))


@pytest.mark.parametrize("where,quote", _quotes,
                         ids=[w for w, _ in _quotes])
def test_quoted_code_still_stands(where, quote):
    assert re.match(r"^[a-z0-9_]+\.(hip|h):[0-9]+$", where), where
    f, ln = where.split(":")
    with open(os.path.join(ROOT, F.CSRC, f)) as fh:
        lines = fh.read().split("\n")
    assert len(_norm(quote)) >= 20, quote
    assert _norm(quote) in _norm(lines[int(ln) - 1]), (
        "%s no longer reads %r: re-read the row(s) that lean on it (now at "
        "lines %r)" % (where, quote, [i + 1 for i, l in enumerate(lines)
                                      if _norm(quote) in _norm(l)]))


def test_rows_carry_a_note_and_a_limit():
    for r in F.ROWS:
        l = r["limit"]
        assert len(r["note"]) > 40, r["name"]
        assert l["op"] in ("<", "<=") and l["bound"] > 0 and l["unit"]
        assert r["by"] in ("pitch", "rows", "dst")
        assert r["tin"] in F.TYPES and r["tout"] in F.TYPES
        if r["by"] == "dst":
            assert r["fe"] == "lancir"  # (avir has no destination pitch)
        if r["window"]:
            assert r["path"] == 4 and r["tin"] == "f32" and r["ch"] == 4


def test_design_md_holds_the_table():
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        doc = fh.read()
    for line in F.design_table():
        assert line in doc, line
