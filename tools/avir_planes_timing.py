#!/usr/bin/env python3
"""What the planar call buys for CImageResizer (resizePlanes, k_avirp) on
channel-first images and batches, by the method of tools/planes_timing.py
(which times CLancIR's): device-resident
torch tensors, every figure over a ring of distinct source / result pairs of
more than 512 MiB in all (twice the Infinity Cache), one process, the roads
alternating REPS times; a figure is the time between two events around one
pass over the ring, divided by the ring's length -- launches and the host's
calls included, as a caller sees them.

Shapes: 3 planes uint8 1920x1080 -> 2500x1400; 3 planes uint8 3840x2160 ->
1280x720; 1 plane float32 1920x1080 -> 3840x2160 and 3840x2160 -> 7680x4320
(exact 2x); 64 x 3 planes float16 500x375 -> 224x224; 64 x 3 planes uint8
128x96 -> 256x192 (the filtered-upsample class); 3 planes uint8 640x480 ->
1024x768.

Roads:
  (a)  the planar call, one launch for all planes: k_avirp at every size
       (the tool sets AVIRHIP_AVIRP_MAX_PIXELS beyond any frame, so that the
       threshold itself can be measured)
  (b)  the unchanged road for the same planes: resizeImage( ...,
       ElCountIO = 1 ) per plane
  (c)  the interleaved call of the same pixel count (H x W x 3 per image)
  (c+) the same with the two permute().contiguous() passes a channel-first
       caller has to add
Prints median [min .. max] ms per road and shape, (b) / (a), and the spread of
each road ( max / min - 1 ); --json FILE keeps the rows."""
import argparse
import json
import statistics
import subprocess
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import avir_amd  # noqa: E402

SHAPES = [
    ("3 x u8 1920x1080 -> 2500x1400", 1, 3, torch.uint8, 1920, 1080, 2500, 1400),
    ("3 x u8 3840x2160 -> 1280x720", 1, 3, torch.uint8, 3840, 2160, 1280, 720),
    ("1 x f32 1920x1080 -> 3840x2160", 1, 1, torch.float32, 1920, 1080, 3840,
     2160),
    ("1 x f32 3840x2160 -> 7680x4320", 1, 1, torch.float32, 3840, 2160, 7680,
     4320),
    ("64 x 3 x f16 500x375 -> 224x224", 64, 3, torch.float16, 500, 375, 224,
     224),
    ("64 x 3 x u8 128x96 -> 256x192", 64, 3, torch.uint8, 128, 96, 256, 192),
    ("3 x u8 640x480 -> 1024x768", 1, 3, torch.uint8, 640, 480, 1024, 768),
    # at the kernel's threshold (AP_MAX_PIXELS of avirp.hip), both directions
    ("3 x u8 512x512 -> 360x360", 1, 3, torch.uint8, 512, 512, 360, 360),
    ("3 x u8 360x360 -> 512x512", 1, 3, torch.uint8, 360, 360, 512, 512),
]
RING_BYTES = 512 << 20


def fill(shape, dtype):
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, dtype=dtype, device="cuda:0")
    return torch.rand(shape, dtype=torch.float32, device="cuda:0").to(dtype)


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
    os.environ["AVIRHIP_AVIRP_MAX_PIXELS"] = str(1 << 62)
    L = avir_amd.CImageResizer(8)
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
    for si, (name, nb, c, dt, sw, sh, nw, nh) in enumerate(SHAPES):
        if only and si not in only:
            continue
        es = torch.empty(0, dtype=dt).element_size()
        per = nb * c * (sw * sh + nw * nh) * es
        ring = max(2, RING_BYTES // per + 1)
        srcs = [fill((nb, c, sh, sw), dt) for _ in range(ring)]
        dsts = [torch.empty((nb, c, nh, nw), dtype=dt, device="cuda:0")
                for _ in range(ring)]
        n = nb * c

        def road_a(i):
            L.resizePlanes(srcs[i], sw, sh, 0, dsts[i], nw, nh, n)

        def road_b(i):
            s, d = srcs[i].view(n, sh, sw), dsts[i].view(n, nh, nw)
            for p in range(n):
                L.resizeImage(s[p], sw, sh, 0, d[p], nw, nh, 1, 0.0)

        roads = [("a", road_a), ("b", road_b)]
        if c == 3:
            hsrc = [s.permute(0, 2, 3, 1).contiguous() for s in srcs]
            hdst = [torch.empty((nb, nh, nw, c), dtype=dt, device="cuda:0")
                    for _ in range(ring)]

            def road_c(i):
                for k in range(nb):
                    L.resizeImage(hsrc[i][k], sw, sh, 0, hdst[i][k], nw, nh, c,
                                  0.0)

            def road_cp(i):
                h = srcs[i].permute(0, 2, 3, 1).contiguous()
                for k in range(nb):
                    L.resizeImage(h[k], sw, sh, 0, hdst[i][k], nw, nh, c, 0.0)
                dsts[i].copy_(hdst[i].permute(0, 3, 1, 2))

            roads += [("c", road_c), ("c+", road_cp)]
        for _, fn in roads:   # warm-up: plans, scratch
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
        row["b_over_a"] = row["b"]["median_ms"] / row["a"]["median_ms"]
        print("  (b) / (a) = %.2f" % row["b_over_a"], flush=True)
        rows.append(row)
        del srcs, dsts
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
