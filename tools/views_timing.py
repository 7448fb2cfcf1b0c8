#!/usr/bin/env python3
"""What plane views cost and buy (AVIRHIP_MEM_VIEWS of the planar calls;
k_lancp / k_avirp reading each plane's base, pitch and stride from a table), by
the method of tools/planes_timing.py: device-resident torch tensors, every
figure over a ring of distinct source / result pairs of more than 512 MiB in
all (twice the Infinity Cache), one process, the roads alternating REPS times;
a figure is the time between two events around one pass over the ring, divided
by the ring's length -- launches and the host's calls included, as a caller
sees them.

Shapes: those of the two planar README rows that have three channels, uint8:
CLancIR 3 planes 1920x1080 -> 2500x1400, 3840x2160 -> 1280x720, 640x480 ->
1024x768, 64 x 3 planes 500x375 -> 224x224; CImageResizer 64 x 3 planes
500x375 -> 224x224 and 128x96 -> 256x192, 3 planes 512x512 -> 360x360 and
360x360 -> 512x512. Then the preprocessing step, HWC uint8 -> CHW float32 at
64 x 3 x 500x375 -> 224x224, and a declined call (CImageResizer 3 planes
640x480 -> 1024x768, above AVIRHIP_AVIRP_MAX_PIXELS), whose views are
gathered and scattered around the per-plane road.

Roads:
  (v)  the views call on channel-last data, both sides (preprocessing: the
       source side; the result is dense CHW); the view tables are made once
       per buffer, outside the clock, as a caller with a ring of surfaces
       would keep them
  (v+) resize_planes( x, out= ) on the same tensors: the tables made per call
  (d)  today's dense call on data that is channel-first already: the price of
       the strided accesses is (v) - (d)
  (p)  what a caller of channel-last data does today: permute().contiguous()
       on each side that needs it, around the dense call
Prints median [min .. max] ms per road and shape and the spread of each road
( max / min - 1 ); --json FILE keeps the rows."""
import argparse
import json
import statistics
import subprocess
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import avir_amd  # noqa: E402

U8, F32 = torch.uint8, torch.float32
# (name, class, images, source type, result type, result channel-last, sw, sh,
#  nw, nh)
SHAPES = [
    ("CLancIR 3 x u8 1920x1080 -> 2500x1400", "L", 1, U8, U8, 1, 1920, 1080,
     2500, 1400),
    ("CLancIR 3 x u8 3840x2160 -> 1280x720", "L", 1, U8, U8, 1, 3840, 2160,
     1280, 720),
    ("CLancIR 3 x u8 640x480 -> 1024x768", "L", 1, U8, U8, 1, 640, 480, 1024,
     768),
    ("CLancIR 64 x 3 x u8 500x375 -> 224x224", "L", 64, U8, U8, 1, 500, 375,
     224, 224),
    ("CImageResizer 64 x 3 x u8 500x375 -> 224x224", "A", 64, U8, U8, 1, 500,
     375, 224, 224),
    ("CImageResizer 64 x 3 x u8 128x96 -> 256x192", "A", 64, U8, U8, 1, 128,
     96, 256, 192),
    ("CImageResizer 3 x u8 512x512 -> 360x360", "A", 1, U8, U8, 1, 512, 512,
     360, 360),
    ("CImageResizer 3 x u8 360x360 -> 512x512", "A", 1, U8, U8, 1, 360, 360,
     512, 512),
    ("preprocessing CLancIR 64 x HWC u8 500x375 -> CHW f32 224x224", "L", 64,
     U8, F32, 0, 500, 375, 224, 224),
    ("preprocessing CImageResizer 64 x HWC u8 500x375 -> CHW f32 224x224",
     "A", 64, U8, F32, 0, 500, 375, 224, 224),
    ("declined: CImageResizer 3 x u8 640x480 -> 1024x768 (per-plane road)",
     "A", 1, U8, U8, 1, 640, 480, 1024, 768),
]
RING_BYTES = 512 << 20


def timed(fn, ring):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(ring):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ring


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="",
                    help="comma-separated shape indices (default: all)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    only = [int(x) for x in args.only.split(",") if x]
    objs = {"L": avir_amd.CLancIR(), "A": avir_amd.CImageResizer(8)}
    rows = []
    print("device  %s" % torch.cuda.get_device_name(0))
    try:   # (tools/half_timing.py's header: read-only)
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"],
                             capture_output=True, text=True, timeout=60).stdout
        for ln in out.split("\n"):
            if "sclk" in ln or "mclk" in ln or "fclk" in ln:
                print("clocks  " + ln.strip())
    except Exception as e:  # (the table stands without them)
        print("clocks  unavailable: %r" % (e,))
    for si, (name, cls, nb, dt, odt, ocl, sw, sh, nw, nh) in enumerate(SHAPES):
        if only and si not in only:
            continue
        R = objs[cls]
        es = torch.empty(0, dtype=dt).element_size()
        oes = torch.empty(0, dtype=odt).element_size()
        # (the ring holds both the channel-last and the channel-first copy)
        per = 2 * nb * 3 * (sw * sh * es + nw * nh * oes)
        ring = max(2, RING_BYTES // per + 1)
        n = nb * 3
        # channel-last data, seen as (N, C, H, W); channel-first copies
        hsrc = [torch.randint(0, 256, (nb, sh, sw, 3), dtype=dt,
                              device="cuda:0").permute(0, 3, 1, 2)
                for _ in range(ring)]
        csrc = [h.contiguous() for h in hsrc]
        cdst = [torch.empty((nb, 3, nh, nw), dtype=odt, device="cuda:0")
                for _ in range(ring)]
        if ocl:
            hdst = [torch.empty((nb, nh, nw, 3), dtype=odt,
                                device="cuda:0").permute(0, 3, 1, 2)
                    for _ in range(ring)]
        else:
            hdst = cdst
        sv = [avir_amd._Views.of_tensor(h, "src") for h in hsrc]
        dv = [avir_amd._Views.of_tensor(h, "out") for h in hdst] if ocl \
            else cdst

        def planes(s, d):
            if cls == "L":
                R.resizePlanes(s, sw, sh, d, nw, nh, n)
            else:
                R.resizePlanes(s, sw, sh, 0, d, nw, nh, n)

        def road_v(i):
            planes(sv[i], dv[i])

        def road_vp(i):
            R.resize_planes(hsrc[i], nw, nh, out=hdst[i])

        def road_d(i):
            planes(csrc[i], cdst[i])

        def road_p(i):
            planes(hsrc[i].contiguous(), cdst[i])
            if ocl:
                hdst[i].copy_(cdst[i])

        roads = [("v", road_v), ("v+", road_vp), ("d", road_d), ("p", road_p)]
        for _, fn in roads:   # warm-up: plans, table slots
            fn(0)
            fn(1)
        torch.cuda.synchronize()
        t = {k: [] for k, _ in roads}
        for _ in range(args.reps):
            for k, fn in roads:
                t[k].append(timed(fn, ring))
        print("%s (ring %d)" % (name, ring))
        row = {"shape": name, "ring": ring}
        for k, _ in roads:
            med, lo, hi = statistics.median(t[k]), min(t[k]), max(t[k])
            row[k] = {"median_ms": med, "min_ms": lo, "max_ms": hi}
            print("  (%-2s) %9.4f ms  [%9.4f .. %9.4f]  spread %5.1f %%" % (
                k, med, lo, hi, (hi / lo - 1.0) * 100.0))
        row["v_over_d"] = row["v"]["median_ms"] / row["d"]["median_ms"]
        row["p_over_v"] = row["p"]["median_ms"] / row["v"]["median_ms"]
        print("  (v) / (d) = %.2f   (p) / (v) = %.2f" % (
            row["v_over_d"], row["p_over_v"]), flush=True)
        rows.append(row)
        del hsrc, csrc, cdst, hdst, sv, dv
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
