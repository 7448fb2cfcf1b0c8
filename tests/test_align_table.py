"""Host-only check of the case table of tests/test_gpu_align.py
(tests/align_cases.py): every family's file has a row and every row states all
its sides; the text each row quotes still stands at the file:line it names --
a predicate edited later fails here and sends the reader back to the row;
every derived level lies on the side of the row's own moduli that it claims,
and each side with a modulus above the element size has levels on both; the
second geometries' rows are no multiple of 4 bytes; every allocation is small;
DESIGN.md holds the table of moduli."""
import os
import re
import pytest
from tests import align_cases as A
from tests import window_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _norm(s):
    return " ".join(s.split())


def test_every_family_file_has_a_row_with_all_sides():
    have = set(f for r in A.ROWS for f in r["files"])
    for f in A.FILES:
        assert f in have, f
        assert os.path.exists(os.path.join(ROOT, A.CSRC, f)), f
    assert len(set(A.NAMES)) == len(A.NAMES)
    for r in A.ROWS:
        want = ["src_base", "src_pitch", "dst_base"]
        if r["fe"] == "lancir":
            want.append("dst_pitch")
        if r["window"]:
            want.append("window")
        assert sorted(r["sides"]) == sorted(want), r["name"]
        for k, s in r["sides"].items():
            es = A.esz_out(r) if k.startswith("dst") else A.esz_in(r)
            if s["mod"] == 0:
                assert k.endswith("pitch") and s["tell"], (r["name"], k)
                continue
            assert s["mod"] >= es and s["mod"] % es == 0, (r["name"], k)
            assert s["mod"] in (1, 2, 4, 8, 16), (r["name"], k)
            assert len(s["aside"]) > 10, (r["name"], k)
            assert s["tell"] in ("refused", "pack", "out", "bytes", None)
            # a side that steps aside to another road says how that shows,
            # one that asks whole elements has nothing to show
            if s["mod"] == es:
                assert s["tell"] is None, (r["name"], k)
        assert len(r["note"]) > 80, r["name"]
        assert r["tin"] in A.TYPES and r["tout"] in A.TYPES
        if r["window"]:
            assert r["path"] == 4 and r["tin"] == "f32" and r["ch"] == 4
            assert r["sides"]["window"]["tell"] == "bytes"
        assert r["base"] is None or r["base"] <= {"pack", "out"}
    # bases 1 byte off: decided row by row, each with its reason
    for r in A.ROWS:
        wide = A.esz_in(r) > 1 or A.esz_out(r) > 1
        assert (r["name"] in A.LEFT_OUT) == wide, r["name"]
        if wide:
            why = A.LEFT_OUT[r["name"]]
            assert len(why) > 120, r["name"]
            assert ("source:" in why) == (A.esz_in(r) > 1)
            assert ("destination:" in why) == (A.esz_out(r) > 1)
    assert set(A.LEFT_OUT) <= set(A.NAMES)


def test_store_forms_of_the_inventory_have_rows():
    """The store forms the far-row table does not distinguish."""
    def have(prefix, **kw):
        return [r for r in A.ROWS if r["name"].startswith(prefix) and
                all(r[k] == v for k, v in kw.items())]
    for ch, t in ((3, "u8"), (4, "u8"), (4, "u16")):
        assert have("up2_raw", ch=ch, tout=t), (ch, t)        # k_up2< true, IO >
    for ch, t in ((3, "u8"), (4, "u8"), (3, "u16"), (4, "u16")):
        assert have("gpass_gv", ch=ch, tout=t), (ch, t)       # gp_store_int_row
    for t in ("u8", "u16"):
        assert have("gpass_gf", ch=4, tout=t), t              # ... behind k_gf
    for ch, t in ((3, "u8"), (4, "u8"), (4, "u16")):
        assert have("sacc2", ch=ch, tout=t)                   # the vertical k_sacc
        assert have("dn_two_pass", ch=ch, tout=t)             # dn.hip
        assert have("lanc2_raw", ch=ch, tout=t)               # dst2
        assert have("lanc_fused_owner", ch=ch, tout=t)        # gp_store_lancir_row
        assert have("tiles", ch=ch, tout=t)                   # the tiles
    assert have("generic_", tout="u8") and have("generic_", tout="u16")
    assert have("up64", tout="f64")                           # vec_st
    assert have("up2_", ch=3, tin="f32", tout="f32", path=4)  # k_up2< true, 3 >
    for ch, t in ((3, "u8"), (4, "u8"), (3, "u16"), (4, "u16")):
        e = have("errd_", ch=ch, tout=t)                      # k_errd_mp
        assert e and e[0]["ex"].get("errd") and e[0]["frames"], (ch, t)


def test_ditherer_rows_reach_the_chained_kernel():
    """launch_errd takes k_errd_mp for padded RGBA results of 65536 pixels and
    more (the row quotes nothing of that line: it is no alignment predicate),
    and the ditherer runs whole frames only."""
    with open(os.path.join(ROOT, A.CSRC, "generic.hip")) as fh:
        lines = fh.read().split("\n")
    assert "(long) w * h >= 65536 &&" in lines[1737 - 1]
    for r in A.ROWS:
        if not r["ex"].get("errd"):
            assert not r["frames"], r["name"]
            continue
        for g in ((0, 1) if r["geom2"] else (0,)):
            sw, sh, nw, nh = A.geom(r, g)
            assert nw * nh >= 65536, r["name"]
        assert not [l for l in A.levels(r) if l.call in ("bands", "window")]
        assert r["sides"]["dst_base"]["mod"] == 16


_quotes = sorted(set((s["where"], s["quote"], r["name"])
                     for r in A.ROWS for s in r["sides"].values()))
_by_quote = {}
for _w, _q, _n in _quotes:
    _by_quote.setdefault((_w, _q), []).append(_n)


@pytest.mark.parametrize("where,quote", sorted(_by_quote),
                         ids=["%s-%d" % (w, i) for i, (w, _) in
                              enumerate(sorted(_by_quote))])
def test_quoted_code_still_stands(where, quote):
    assert re.match(r"^[a-z0-9_]+\.(hip|h|cpp):[0-9]+$", where), where
    f, ln = where.split(":")
    with open(os.path.join(ROOT, A.CSRC, f)) as fh:
        lines = fh.read().split("\n")
    assert len(_norm(quote)) >= 20, quote
    assert _norm(quote) in _norm(lines[int(ln) - 1]), (
        "%s no longer reads %r: re-read the row(s) %r that lean on it (now at "
        "lines %r)" % (where, quote, _by_quote[(where, quote)],
                       [i + 1 for i, l in enumerate(lines)
                        if _norm(quote) in _norm(l)]))


@pytest.mark.parametrize("name", A.NAMES)
def test_levels_stand_where_they_claim(name):
    r = A.row(name)
    es, ed = A.esz_in(r), A.esz_out(r)
    lv = A.levels(r)
    names = [l.name for l in lv]
    assert len(set(names)) == len(names)
    assert lv[0].name == "aligned"
    # the aligned, packed call is on the fast road on every side
    assert all(A.on_fast_road(r, lv[0]).values()), name
    assert not A.tells(r, lv[0])
    # the levels of the issue, by count
    frames = [l for l in lv if l.call == "frame" and l.g == 0]
    assert sum(1 for l in frames if l.soff and not l.doff and not l.spad) == \
        16 // es - 1
    assert sum(1 for l in frames if l.doff and not l.soff) == 16 // ed - 1
    assert [(l.soff, l.doff) for l in frames if l.name.startswith("both")] == \
        [(es, ed), (16 - es, 16 - ed)]
    assert [l.spad for l in frames if l.spad and not l.soff] == \
        [1, 2, 3, 4, 5, 8]
    assert [(l.soff, l.spad) for l in frames if l.spad and l.soff] == [(es, 1)]
    assert [l.dpad for l in frames if l.dpad] == \
        ([1, 2, 3, 4] if r["fe"] == "lancir" else [])
    assert [l.soff for l in lv if l.call == "window"] == \
        ([0, 4, 8, 12] if r["window"] else [])
    assert [(l.soff, l.doff) for l in lv if l.call == "host"] == [(es, ed)]
    assert sum(1 for l in lv if l.call == "bands") == (0 if r["frames"]
                                                        else 1)
    for l in lv:
        assert l.soff % es == 0 and l.doff % ed == 0 and l.soff < 16 and \
            l.doff < 16, l
        # what on_fast_road claims is the modulus' own arithmetic
        sp, dp = A.pitches(r, l)
        sw, sh, nw, nh = A.geom(r, l.g)
        assert sp >= sw * r["ch"] and dp >= nw * r["ch"]
        if l.call == "window":
            assert A.on_fast_road(r, l) == {
                "window": l.soff % r["sides"]["window"]["mod"] == 0}
            continue
        got = A.on_fast_road(r, l)
        s = r["sides"]
        assert got["src_base"] == (l.soff % s["src_base"]["mod"] == 0)
        assert got["dst_base"] == (l.doff % s["dst_base"]["mod"] == 0)
        assert got["src_pitch"] == ((sp * es) % s["src_pitch"]["mod"] == 0)
        if "dst_pitch" in s:
            m = s["dst_pitch"]["mod"]
            assert got["dst_pitch"] == ((dp * ed) % m == 0 if m else
                                        l.dpad == 0)
        assert A.alloc_bytes(r, l) < A.CAP, l
    # both sides of every modulus above the element size: otherwise the row
    # tests nothing
    for side, s in r["sides"].items():
        es_ = ed if side.startswith("dst") else es
        if 0 < s["mod"] <= es_:
            continue
        which = [A.on_fast_road(r, l)[side] for l in lv
                 if l.call in ("frame", "window") and
                 side in A.on_fast_road(r, l) and
                 l.name != "aligned"]
        assert True in which and False in which, (name, side)


@pytest.mark.parametrize("name", A.NAMES)
def test_second_geometries_have_rows_of_no_whole_dwords(name):
    r = A.row(name)
    es, ed = A.esz_in(r), A.esz_out(r)
    if not A.wants_geom2(r):
        # RGBA pixels of 1, 2, 4 or 8 bytes: rows are whole dwords at any width
        # (... where a second geometry still moves the rows off the 16-byte
        # grid: float RGB, whose bands then start 4, 8 or 12 bytes off it)
        assert (r["ch"] * es) % 4 == 0 and (r["ch"] * ed) % 4 == 0
        if r["geom2"] is not None:
            sw, sh, nw, nh = r["geom2"]
            assert (sw * r["ch"] * es) % 16 and (nw * r["ch"] * ed) % 16
            assert [l.g for l in A.levels(r) if l.call == "bands"] == [1]
        return
    assert r["geom2"] is not None, name
    sw, sh, nw, nh = r["geom2"]
    assert (sw * r["ch"] * es) % 4 != 0, name
    assert (nw * r["ch"] * ed) % 4 != 0, name
    # widths next to the first geometry's, the same heights
    assert abs(sw - r["sw"]) <= 2 and abs(nw - r["nw"]) <= 2
    assert (sh, nh) == (r["sh"], r["nh"])
    # the bands run there, and their bases take every residue mod 4 a row of
    # that length can give them: 1, 2, 3 for an odd byte count, 2 otherwise
    if r["frames"]:
        assert [l.g for l in A.levels(r) if l.name == "aligned-g2"] == [1]
        return
    band = [l for l in A.levels(r) if l.call == "bands"][0]
    assert band.g == 1
    rb = nw * r["ch"] * ed
    res = set((a * rb) % 4 for a, b in A.bands(r, 1))
    assert res == ({0, 1, 2, 3} if rb % 2 else {0, 2}), (name, res)
    assert [x for x in A.bands(r, 1)[:5]] == [(a, b) for _, a, b in
                                              W.bands(nh)]


def test_geometries_are_the_far_rows():
    """The first geometries are those of tests/far_row_cases.py: the smallest
    frames each family takes on its forced path."""
    from tests import far_row_cases as F
    far = set((r["sw"], r["sh"], r["nw"], r["nh"]) for r in F.ROWS)
    for r in A.ROWS:
        assert (r["sw"], r["sh"], r["nw"], r["nh"]) in far, r["name"]


def test_design_md_holds_the_table():
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        doc = fh.read()
    for line in A.design_table():
        assert line in doc, line
