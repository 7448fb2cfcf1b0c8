"""The chunk split of the 2x marching kernel (avir_amd/csrc/up2_chunks.h: the
forward map, its inverse and the choice of (n, cq, nlong)), on the CPU: the
header is plain C++, compiled here with g++ into tests/cpp/up2_chunks_dump.cpp,
which prints the split of every band height and walks the inverse over every
row.

The parent rule (one height cq = 8k - 18 per launch, the last chunk gets what
is left) is restated below from up2_run's former loop, not taken from the code
under test."""
import math
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB = 8
NSTRIPS = [1, 2, 7, 30, 60, 120, 240]
MAXROWS = 4400
THR = [1.0, 0.3, 0.57, 0.8, 0.9, 0.9, 0.9, 0.97, 1.0]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("up2_chunks") / "up2_chunks_dump")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "avir_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "up2_chunks_dump.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe, str(MAXROWS)] + [str(n) for n in NSTRIPS],
                         check=True, capture_output=True, text=True,
                         timeout=600).stdout
    res = {}
    for ln in out.splitlines():
        f = [int(x) for x in ln.split()]
        res[(f[0], f[1])] = dict(n=f[2], cq=f[3], nlong=f[4], inv_bad=f[5],
                                 first=f[6:])
    assert len(res) == MAXROWS * len(NSTRIPS)
    return res


def steps_of(h):
    """marching steps of a chunk of h source rows: 6 rows of preload and 12 of
    warm-up in front of them, RB rows per step."""
    return (h + 18 + RB - 1) // RB


def parent_rule(rows, nstrips):
    """up2_run's loop before the split: (cq, chunk heights) of a whole frame
    of `rows` source rows (2 * rows output rows)."""
    r = (2 * rows + 1) // 2 + 1
    best, cq = -1.0, 0
    for k in range(10, 65):
        c = RB * k - 18
        nch = (r + c - 1) // c
        items = nch * nstrips
        m = (items + 255) // 256
        cost = m * k / THR[m] if m <= 8 else items * k / 256.0 * 1.06
        if best < 0.0 or cost < best:
            best, cq = cost, c
        if nch == 1:
            break
    return cq, [min(q + cq, rows) - q for q in range(0, rows, cq)]


def modelled(steps, ns):
    """step-times of a launch whose strips are cut into chunks of `steps`: see
    test_total_steps_no_more_than_the_parent_rule"""
    n, m = len(steps), math.ceil(len(steps) * ns / 256)
    if m > 8:
        return ns * sum(steps) / 256.0 * 1.08
    return max(sum(steps[(c + 32 * t) % n] for t in range(m))
               for c in range(n)) / THR[m]


def heights(c, rows):
    f = c["first"]
    return [min(f[i + 1], rows) - f[i] for i in range(c["n"])]


def test_chunks_tile_the_band_exactly(cases):
    for (rows, ns), c in cases.items():
        f = c["first"]
        assert len(f) == c["n"] + 1 and f[0] == 0, (rows, ns, c)
        assert all(a < b for a, b in zip(f, f[1:])), (rows, ns, c)
        # n chunks, no fewer and no more: the last one begins inside the band
        # and ends at or beyond its end (where the frame clips it)
        assert f[c["n"] - 1] < rows <= f[c["n"]], (rows, ns, c)


def test_heights_are_whole_steps_and_one_step_apart(cases):
    for (rows, ns), c in cases.items():
        f = c["first"]
        full = [b - a for a, b in zip(f, f[1:])]  # before the clip
        for h in full:
            assert (h + 18) % RB == 0 and (h + 18) // RB >= 3, (rows, ns, c)
        assert max(full) - min(full) <= RB, (rows, ns, c)
        assert 0 <= c["nlong"] < max(c["n"], 2), (rows, ns, c)
        # long chunks first
        assert full == sorted(full, reverse=True), (rows, ns, c)
        # only the last chunk is clipped
        assert heights(c, rows)[:-1] == full[:-1], (rows, ns, c)


def test_inverse_agrees_with_forward_map_at_every_row(cases):
    bad = [(k, c["inv_bad"]) for k, c in cases.items() if c["inv_bad"]]
    assert not bad, bad[:5]


def test_total_steps_no_more_than_the_parent_rule(cases):
    """A strip's marching steps under the split against the parent rule's.
    More steps in total are allowed for one reason only, which is asserted: the
    launch is modelled to end SOONER than the parent's, by the parent's own
    formula with the exact load of the most loaded CU in it:
    - every item resident at once (at most 8 x 256): the launch ends with its
      most loaded CU, after steps / thr[m] (thr: the VALU throughput of a CU
      that runs m workgroups, restated from up2_run's former loop). A CU holds
      m = ceil(items / 256) items; items are strip-major and an XCD deals its
      workgroups over its 32 CUs in turn, so they are the chunks c, c + 32,
      c + 64 ... modulo the chunk count, for the worst c;
    - more items than that: the mean steps of a CU and 8 % on top (partial
      rounds; the parent took 6 %, cfg3 cut into 18-20 chunks measured 7-8 %:
      the larger figure is the stricter one for a split of more chunks).
    (cfg2 is such a case: 17 chunks of 10-11 steps, 174 steps a strip, at most
    42 on a CU, against 16 chunks of 11 and 6 steps, 171 a strip, where a CU
    holds the same chunk of four strips and marches 44.)"""
    worse = 0
    for (rows, ns), c in cases.items():
        new = [steps_of(h) for h in heights(c, rows)]
        old = [steps_of(h) for h in parent_rule(rows, ns)[1]]
        if sum(new) <= sum(old):
            continue
        worse += 1
        assert modelled(new, ns) < modelled(old, ns), (
            rows, ns, c, sum(new), sum(old))
    print("cases with more steps than the parent rule: %d of %d" % (
        worse, len(cases)))


@pytest.mark.parametrize("rows,ns", [(2160, 120), (1080, 60)])
def test_headline_shapes_have_no_short_chunk(cases, rows, ns):
    """cfg3 and cfg2: no chunk, the clipped last one included, is shorter than
    the longest by more than one marching step."""
    new = [steps_of(h) for h in heights(cases[(rows, ns)], rows)]
    assert max(new) - min(new) <= 1, new
