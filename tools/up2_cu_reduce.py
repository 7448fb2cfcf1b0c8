#!/usr/bin/env python3
"""Per-CU figures of one k_up2 launch, from the per-item clocks the debug
build dumps (make -C avir_amd/csrc dbg; AVIRHIP_UP2_CLKDUMP=FILE: one line per
workgroup: blockIdx, shader cycles, start, end in 10 ns ticks from the
launch's first start, and HW_ID | XCC_ID << 32 in hex).

For every CU (XCC, SE, SH, CU of the hardware id): the items it held, their
marching steps if the chunk split is given, its first start and last end, and
the slot-time it stood idle (SLOTS resident workgroups x the launch's span,
minus its items' own times). Then the launch's summary: how far apart the
CUs' last ends lie is what a better split of the work has to narrow.

usage: python tools/up2_cu_reduce.py DUMP [--split ROWS,CQ,NLONG] [--slots 8]
                                     [--per-cu]
"""
import argparse
import collections
import statistics

RB = 8  # source rows per marching step (U2_RB)


def cu_of(hw):
    """(xcc, se, sh, cu) of HW_ID (gfx9 layout: cu 11:8, sh 12, se 15:13) with
    XCC_ID 3:0 in the upper word."""
    return ((hw >> 32) & 15, (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15)


def item_of(b, nwg):
    """blockIdx -> work item: the kernel's XCD-aware dealing."""
    xcd, qd, rm = b & 7, nwg >> 3, nwg & 7
    base = xcd * (qd + 1) if xcd < rm else rm * (qd + 1) + (xcd - rm) * qd
    return base + (b >> 3)


def chunk_steps(rows, cq, nlong):
    """marching steps of every chunk of a strip of `rows` source rows."""
    out, c = [], 0
    while True:
        q0 = c * cq + RB * min(c, nlong)
        if q0 >= rows:
            return out
        h = min(q0 + cq + (RB if c < nlong else 0), rows) - q0
        out.append((h + 18 + RB - 1) // RB)
        c += 1


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dump")
    ap.add_argument("--split", help="ROWS,CQ,NLONG of the launch")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--per-cu", action="store_true")
    a = ap.parse_args()
    rec = []
    for line in open(a.dump):
        f = line.split()
        rec.append((int(f[0]), int(f[2]) / 100.0, int(f[3]) / 100.0,
                    int(f[4], 16)))
    nwg = len(rec)
    steps = chunk_steps(*map(int, a.split.split(","))) if a.split else None
    span0 = min(r[1] for r in rec)
    span1 = max(r[2] for r in rec)
    span = span1 - span0
    cus = collections.defaultdict(list)
    for b, t0, t1, hw in rec:
        k = steps[item_of(b, nwg) % len(steps)] if steps else 0
        cus[cu_of(hw)].append((t0, t1, k))
    rows = []
    for cu, it in sorted(cus.items()):
        busy = sum(t1 - t0 for t0, t1, _ in it)
        rows.append((cu, len(it), sum(k for _, _, k in it),
                     max(k for _, _, k in it) if steps else 0,
                     sum(1 for _, _, k in it if steps and k == max(steps)),
                     min(t0 for t0, _, _ in it), max(t1 for _, t1, _ in it),
                     a.slots * span - busy))
    if a.per_cu:
        print("xcc se sh cu  items steps longest n_longest  first_start_us "
              "last_end_us idle_slot_us")
        for cu, n, s, mx, nl, f, l, idle in rows:
            print("%3d %2d %2d %2d  %5d %5d %7d %9d  %14.2f %11.2f %12.2f" % (
                cu + (n, s, mx, nl, f, l, idle)))
    dur = [r[2] - r[1] for r in rec]
    ends = [r[6] for r in rows]
    print("launch: %d items on %d CUs, span %.2f us; item time mean %.2f "
          "max %.2f us" % (nwg, len(rows), span, statistics.mean(dur),
                           max(dur)))
    print("items per CU: " + " ".join("%d:%d" % kv for kv in sorted(
        collections.Counter(r[1] for r in rows).items())))
    if steps:
        print("chunks of a strip, steps: %s" % " ".join(map(str, steps)))
        print("steps per CU: min %d mean %.1f max %d; longest chunks on one "
              "CU: max %d" % (min(r[2] for r in rows),
                              statistics.mean(r[2] for r in rows),
                              max(r[2] for r in rows),
                              max(r[4] for r in rows)))
        byk = collections.defaultdict(list)
        for it in cus.values():
            for t0, t1, k in it:
                byk[k].append(t1 - t0)
        print("item time by steps: " + "  ".join(
            "%d: %.2f us (%d)" % (k, statistics.mean(v), len(v))
            for k, v in sorted(byk.items())))
    print("CU first start: max %.2f us" % max(r[5] for r in rows))
    print("CU last end: min %.2f  p10 %.2f  median %.2f  p90 %.2f  max %.2f "
          "us; spread (max - min) %.2f us, (max - median) %.2f us" % (
              min(ends), pct(ends, 0.1), statistics.median(ends),
              pct(ends, 0.9), max(ends), max(ends) - min(ends),
              max(ends) - statistics.median(ends)))
    idle = sum(r[7] for r in rows)
    print("idle slot-time: %.0f us of %.0f (%d slots x %d CUs x span): "
          "%.1f %%" % (idle, a.slots * len(rows) * span, a.slots, len(rows),
                       100.0 * idle / (a.slots * len(rows) * span)))
    if steps:
        # does the CU that ends last hold the most steps?
        rows.sort(key=lambda r: r[6])
        n = max(1, len(rows) // 8)
        print("steps held by the %d CUs that end first: %.1f, last: %.1f" % (
            n, statistics.mean(r[2] for r in rows[:n]),
            statistics.mean(r[2] for r in rows[-n:])))


if __name__ == "__main__":
    main()
