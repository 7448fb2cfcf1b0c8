"""Host-only check of tests/chunk_cases.py, the table of
tests/test_gpu_chunks.py: every stage's list of forced lengths holds what the
seam tests are about, the geometry gives those lengths seams to be wrong at,
and the constants the table restates are the sources'."""
import os
import pytest
from tests import chunk_cases as CC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "avir_amd", "csrc")
STAGES = [(name, st) for name, call, stages in CC.ROWS for st in stages]
IDS = ["%s-%s%s" % (n, s.kernel, "-" + s.tag if s.tag else "")
       for n, s in STAGES]
KNOBBED = [(n, s) for n, s in STAGES if s.knob is not None]
KIDS = [i for i, (n, s) in zip(IDS, STAGES) if s.knob is not None]


def test_restated_constants_are_the_sources():
    parsed = CC.parse_constants(CSRC)
    assert parsed == CC.CONSTANTS
    # (the constants the seam lengths hang on, by name)
    for n in ("LF_NB", "GF_NB", "GH_NB", "LF_TE", "GF_TE", "DF_W", "LH_MINQ",
              "L2_RB"):
        assert n in parsed
    assert (CC.LF_CLAMP, CC.GF_CLAMP, CC.GV_RING) == (192, 170, 6)


def test_every_family_of_the_issue_has_a_row():
    kernels = {s.kernel for n, s in STAGES}
    assert kernels >= {"k_lanc2", "k_lanc2h", "k_dnf", "k_dnfh", "k_dnh",
                       "k_dnv", "k_gh", "k_gh2", "k_gv", "k_gf", "k_lf",
                       "k_sacc", "k_sacc2", "k_sacc2v"}
    assert len(CC.NAMES) == len(set(CC.NAMES))
    assert [r[1][5] for r in CC.UP64_ROWS] == [4, 3]
    assert CC.UP64_RH == (4, 8) and CC.UP64_EPL == (1, 2)


@pytest.mark.parametrize("name,st", KNOBBED, ids=KIDS)
def test_lengths_straddle_the_ring_and_hold_the_real_ones(name, st):
    L = st.lengths
    assert L == sorted(set(L)) and L[0] >= 1
    # requested: 1, 2, 3, today's, ring - 1, ring, ring + 1, 2 ring + 1
    assert {1, 2, 3, st.today, st.ring - 1, st.ring, st.ring + 1,
            2 * st.ring + 1} <= set(L)
    # in force (a rounding rule moves them): below, and above the ring; at
    # the ring wherever the rule can give that length at all
    eff = {st.in_force(v, 1 << 20) for v in L}
    assert any(e < st.ring for e in eff) and any(e > st.ring for e in eff)
    if st.rule != "cq":
        assert st.ring in eff
    else:
        assert all(e % 8 == 2 for e in eff)
        assert min(e for e in eff if e > st.ring) == st.ring + 2
    # the lengths real frames run at
    assert st.real, st.kernel
    assert set(st.real.values()) <= set(L), st.real
    # the clamp, and a value above it that must come back clamped
    if st.clamp is not None:
        assert {st.clamp, st.clamp + 8} <= set(L)
        assert st.in_force(st.clamp + 8) == st.clamp
    if st.rule == "gv":
        assert max(L) > CC.gv_clamp(1, False)  # above every possible clamp


@pytest.mark.parametrize("name,st", KNOBBED, ids=KIDS)
def test_geometry_leaves_seams(name, st):
    """At least three chunks at the ring-depth length and exactly one at the
    longest -- or, where the launcher's clamp is shorter than the pass, the
    two the clamp leaves: the seam of the longest chunk a real frame runs."""
    assert st.rows is not None
    ring_len = st.in_force(st.ring, 1 << 20)
    assert st.chunks(ring_len) >= 3
    longest = max(st.in_force(v, 1 << 20) for v in L_(st))
    if st.clamp is not None and st.clamp < st.rows:
        assert longest == st.clamp and st.chunks(longest) == 2
    else:
        assert longest >= st.rows and st.chunks(longest) == 1
    assert st.above_ring() is not None


@pytest.mark.parametrize("name", [r[0] for r in CC.ROWS if r[2][-1].knob])
def test_every_family_has_a_last_chunk_of_one_row(name):
    n, call, stages = CC.row(name)
    assert any(st.rows % e == 1 and e > 1 for st in stages
               for e in (st.in_force(v, 1 << 20) for v in L_(st)))


def L_(st):
    return st.lengths


def test_dnf_rows_hold_a_216_row_chunk_and_a_remainder():
    for name in ("dnf_2x2", "dnf_3x3", "dnf_2x3", "dnfh_f16", "dnfh_bf16_u16"):
        n, call, stages = CC.row(name)
        st = stages[0]
        assert st.real == {"cfg4": 90, "4k_1080p": 216}
        assert call[4] > 216 and st.chunks(216) == 2
        assert st.today == CC.dnf_crows(call[4], call[3])


def test_todays_lengths_are_what_the_rules_give_small_frames():
    """The `today` column against the restated rules at the table's shapes
    (nominal strip counts: both give the floor)."""
    assert CC.balanced_chunk(241, 2, 4, 192, 3, 9, True) == 4
    assert CC.balanced_chunk(241, 2, 4, 170, 5, 8, True) == 4
    assert CC.balanced_chunk(150, 2, 4, 150, 2, 16, False) == 4
    assert CC.sacc_chunk(241, 2, 54, 3.0, 13376) == 4
    assert CC.lanc2_cq(121, 200, CC.L2_MINQ) == 58
    assert CC.lanc2_cq(121, 200, CC.K["LH_MINQ"]) == 26
    # ... and far below the lengths of real frames
    assert CC.real_lengths("k_lf")["1080p_2500"] > 2 * CC.K["LF_NB"]
    assert CC.real_lengths("k_gf")["1080p_5760"] > 2 * CC.K["GF_NB"]


def test_up64_rules():
    assert CC.up64_crows_h(121, 2, 2, 8) == 128
    assert CC.up64_crows_h(121, 2, 2000, 4) == 16
    assert CC.up64_crows_h(121, 2, 4, 8) == 64
    assert CC.up64_crows_v(242, 4, 4) == 242
    assert CC.up64_crows_v(242, 4, 4000) == 48
