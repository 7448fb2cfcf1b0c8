#!/usr/bin/env python3
"""What half (float16) pixels buy on the exact-2x marching kernel: cfg3
(3840x2160 -> 7680x4320 RGBA) and cfg2 (1920x1080 -> 3840x2160) as
  (a) float32 -> float32 (the baseline; with PARENT.so also on that build),
  (b) half -> half, read and stored by k_up2 itself (k_up2< true, 6, 124 >),
  (c) half -> half through the pack pass and the output stage
      (AVIRHIP_VARIANT_UP2_UNFUSED_IO),
  (d) float32 -> half (k_up2< true, 6 >),
one process, avirhip_time_resize, every figure over a ring of distinct source /
destination pairs of more than 512 MiB in all (twice the Infinity Cache), the
rows alternating REPS times. Prints the table with the achieved bytes/s, the
library's md5 and the device clocks.
--bf16 adds the bfloat16 rows beside them, in the same process and rotation:
  (e) bfloat16 -> bfloat16, read and stored by k_up2 (k_up2< true, 7, 224 >),
  (f) bfloat16 -> bfloat16 through the pack pass and the output stage,
  (g) float32 -> bfloat16 (k_up2< true, 7 >).
--lancir measures CLancIR's exact-2x kernels instead, by the same method: cfg5
(3840x2160 -> 7680x4320 RGBA) and 1920x1080 -> 3840x2160 as
  (a) float32 -> float32 (k_lanc2; with PARENT.so also on that build),
  (b) half -> half, one launch of k_lanc2h< F16, F16 >,
  (c) half -> half through the pack pass, k_lanc2 and the output stage
      (AVIRHIP_VARIANT_UP2_UNFUSED_IO: the road before k_lanc2h),
  (d) float32 -> half, (e) half -> float32,
  (f) - (i) the bfloat16 twins of (b) - (e).
--dnf measures whole-ratio downsizing on path 2 by the same method: cfg4
(3840x2160 -> 1280x720 RGBA) and 3840x2160 -> 1920x1080 as
  (a) float32 -> float32 (k_dnf; with PARENT.so also on that build),
  (b) half -> half, one launch of k_dnfh< F16, F16 >,
  (c) half -> half through the pack pass, k_dnf and the output stage
      (AVIRHIP_VARIANT_DN_UNFUSED_IO: the road before k_dnfh),
  (d) bfloat16 -> bfloat16 fused, (e) the same unfused,
  (f) float32 -> half, (g) half -> float32.
--gpass measures general ratios on the pass kernels (path 5, the automatic
path of every shape it runs) by the same method -- 1920x1080 -> 2500x1400,
3840x2160 -> 2560x1440 and -> 2000x1125, 1920x1080 -> 5760x3240, 3840x2160 ->
6144x3456, 5184x3456 -> 1920x1280 -- as float32, the 16-bit call as it runs
automatically, the same call under AVIRHIP_GP_NO_IO16 (pack pass and output
stage: the road before the typed k_gh and the narrowing store), and the typed
k_gh forced where k_gf / k_gh2 keep the pack pass; with PARENT.so also RGB
uint8 on both builds (the store function the integer stage shares).

--lancgp measures CLancIR at general ratios (path 5: k_lf, or k_gv + k_gh) by
the same method -- 1920x1080 -> 2500x1400, 3840x2160 -> 1280x720, 1920x1080 ->
5760x3240, RGBA half and bfloat16 in and out, plus RGB half at the first shape
-- as float32, the 16-bit call as it runs automatically (the fused road: the
raw loaders' kinds 4 / 5 and gp_store_lancir_row< 3 >) and the same call with
AVIRHIP_VARIANT_UP2_UNFUSED_IO (pack pass, kernels, output stage: the road
before). Then the `lf_pays` sweep: k_lf (AVIRHIP_VARIANT_UPG_FUSED) against
k_gv + k_gh (AVIRHIP_VARIANT_UPG_TWO_PASS) with a half RGBA result at x1.5,
x2.5, x3 and x4 from 1920x1080. With PARENT.so also README's CLancIR rows of
uint8 / float32 images on both builds, alternating.

--sacc measures downsizing by a non-integer ratio of 2 or more with 16-bit
sources by the same method -- 5184x3456 -> 1920x1280 (RGBA and RGB), 3840x2160
-> 1500x844, 1920x1080 -> 700x394, 640x480 -> 233x175, the mixed 3840x1080 ->
1500x1400, half and bfloat16 -- as float32 on path 5; the 16-bit call on
forced path 5 on the typed exact road (k_sacc< 4 / 5 >), the typed optimistic
one (k_sacc2< 4 / 5 > first), the branch-free launches alone and the pack road
(AVIRHIP_GP_NO_IO16); and the automatic path before and with path 5 admitted
(AVIRHIP_SA16_AUTO_MINPIX). With PARENT.so also README's uint8 and float32
accumulation rows on both builds, alternating.

--dnsrgb measures whole-ratio downsizing of 8-bit images with sRGB gamma
(CImageResizer(8), UseSRGBGamma, AlphaIndex 3) on path 2 by the same method --
3840x2160 -> 1920x1080 and -> 1280x720 -- each call as it runs (k_dnfh's DH_S8
kinds) and under AVIRHIP_VARIANT_DN_UNFUSED_IO (pack pass, k_dnf, output
stage: the road before, the yardstick), alternating: RGBA uint8 -> uint8, RGBA
uint8 -> float32, RGB uint8 -> uint8 (the store side only), and the RGBA uint8
call without gamma for scale.

--up2srgb measures exact-2x upsizing of 8-bit images with sRGB gamma
(CImageResizer(8), UseSRGBGamma, AlphaIndex 3 for RGBA) on path 4 by the same
method -- 1920x1080 -> 3840x2160 and 3840x2160 -> 7680x4320 -- RGBA and RGB
uint8 -> uint8 as they run (k_up2's SRC 313 / 314 and IO 9 kinds), under
AVIRHIP_VARIANT_UP2_UNFUSED_IO (pack pass, k_up2, output stage: the road
before, with PARENT.so also on that build) and without gamma (k_up2< true, 4,
13 / 14 >); float32 -> uint8 RGBA and RGB with gamma, the store side alone
(IO 8 behind the pack pass) against the road before; the residency of the
gamma kinds under AVIRHIP_UP2_LDSPAD (1 KB on the store kind: seven -> six
workgroups a CU; 4 KB on the raw kind: six -> five) and, with THR1K.so (`make
thr1k`: the colour thresholds alone in LDS, alpha by its direct expression),
of that form (raw kinds: seven workgroups; store kinds: eight); and float32 ->
float32 RGBA in this library, with PARENT.so beside the parent's.

usage: python tools/half_timing.py [--bf16 | --lancir | --dnf | --dnsrgb |
       --up2srgb | --gpass | --lancgp | --sacc] [PARENT.so] [REPS=5] [ONLY]
(--up2srgb: [PARENT.so] [REPS=5] [THR1K.so] [bounds]; `bounds`: the fused roads
against the road before at six frame sizes from 640x360 to 3840x2160)
(ONLY, with --gpass, --lancgp and --sacc: the shapes whose names hold one of
these comma-separated words, e.g. "u8")"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def header(lib, parent):
    import torch
    from avir_amd import abi
    print("library %s md5 %s" % (abi.LIB_PATH, md5(abi.LIB_PATH)))
    print("version %s" % lib.avirhip_version().decode())
    if parent:
        print("parent  %s md5 %s" % (parent, md5(parent)))
    print("device  %s" % torch.cuda.get_device_name(0))
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"],
                             capture_output=True, text=True, timeout=60).stdout
        for l in out.split("\n"):
            if "sclk" in l or "mclk" in l or "fclk" in l:
                print("clocks  " + l.strip())
    except Exception as e:  # (the table stands without them)
        print("clocks  unavailable: %r" % (e,))


def lancir_main(argv):
    """--lancir: the rows of the module docstring, CLancIR plans on path 4."""
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    parent = argv[1] if len(argv) > 1 and argv[1] != "-" else None
    reps = int(argv[2]) if len(argv) > 2 else 5
    lib = abi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    header(lib, parent)
    TD = {abi.F32: torch.float32, abi.F16: torch.float16,
          abi.BF16: torch.bfloat16}
    ES = {abi.F32: 4, abi.F16: 2, abi.BF16: 2}
    U = abi.VARIANT_UP2_UNFUSED_IO
    for name, (sw, sh) in (("cfg5", (3840, 2160)), ("1080p", (1920, 1080))):
        nw, nh = 2 * sw, 2 * sh
        base = synth.lcg_f32((sh, sw, 4))
        rows = [("a  f32->f32 k_lanc2", lib, abi.F32, abi.F32, 0),
                ("b  f16->f16 fused", lib, abi.F16, abi.F16, 0),
                ("c  f16->f16 pack + output stage", lib, abi.F16, abi.F16, U),
                ("d  f32->f16", lib, abi.F32, abi.F16, 0),
                ("e  f16->f32", lib, abi.F16, abi.F32, 0),
                ("f  bf16->bf16 fused", lib, abi.BF16, abi.BF16, 0),
                ("g  bf16->bf16 pack + output stage", lib, abi.BF16, abi.BF16,
                 U),
                ("h  f32->bf16", lib, abi.F32, abi.BF16, 0),
                ("i  bf16->f32", lib, abi.BF16, abi.F32, 0)]
        pairs = [(rows[1][0], rows[2][0]), (rows[5][0], rows[6][0])]
        if parent:
            rows.insert(0, ("a' f32->f32 parent build", abi.load_path(parent),
                            abi.F32, abi.F32, 0))
        run, keep, first = {}, [], {}
        for tag, L, ti, to, variant in rows:
            pair = sw * sh * 4 * ES[ti] + nw * nh * 4 * ES[to]
            n = max(2, -(-(512 << 20) // pair))
            ring = []
            for i in range(n):
                s = torch.from_numpy(np.roll(base, i, axis=0)).to(dev).to(TD[ti])
                d = torch.empty((nh, nw, 4), dtype=TD[to], device=dev)
                ring.append((s, d))
            with abi.using(L):
                r = avir_amd.CLancIR()
                p = r.plan(sw, sh, nw, nh, 4, None, ti, to)
            abi.check(L.avirhip_plan_set_path(p, abi.PATH_UP2), "path 4")
            if variant:
                abi.check(L.avirhip_plan_set_variant(p, variant), "variant")
            keep.append((r, ring))

            def once(L=L, p=p, ring=ring):
                t = 0.0
                ms = C.c_double()
                for s, d in ring:
                    abi.check(L.avirhip_time_resize(
                        p, s.data_ptr(), d.data_ptr(), 1, st, C.byref(ms)),
                        "time_resize")
                    t += ms.value
                return t / len(ring)
            run[tag] = (once, pair, n, L, p)
            first[tag] = ring[0][1]
        for tag in run:  # warm-up, clocks
            for _ in range(20):
                run[tag][0]()
        torch.cuda.synchronize()
        same = [torch.equal(first[x].view(torch.uint8),
                            first[y].view(torch.uint8)) for x, y in pairs]
        res = {tag: [] for tag in run}
        loops = 30 if name == "cfg5" else 60
        for _ in range(reps):
            for tag in run:
                res[tag].append(sum(run[tag][0]() for _ in range(loops)) / loops)
        print("%s (%dx%d -> %dx%d RGBA, CLancIR), %d reps x %d ring passes:" % (
            name, sw, sh, nw, nh, reps, loops))
        for tag in run:
            v = sorted(res[tag])
            med = v[len(v) // 2]
            print("  %-34s %.4f ms  (min %.4f max %.4f)  %6.1f MB/call  "
                  "%.2f TB/s  ring %d  plan holds %.1f MB" % (
                      tag, med, v[0], v[-1], run[tag][1] / 1e6,
                      run[tag][1] / med / 1e9, run[tag][2],
                      run[tag][3].avirhip_plan_device_bytes(run[tag][4]) / 1e6),
                  flush=True)
        print("  (b) and (c) bit-identical: %s" % same[0], flush=True)
        print("  (f) and (g) bit-identical: %s" % same[1], flush=True)
        del keep, run, first
        torch.cuda.empty_cache()


def dnf_main(argv):
    """--dnf: the rows of the module docstring, CImageResizer plans on path 2."""
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    parent = argv[1] if len(argv) > 1 and argv[1] != "-" else None
    reps = int(argv[2]) if len(argv) > 2 else 5
    lib = abi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    header(lib, parent)
    TD = {abi.F32: torch.float32, abi.F16: torch.float16,
          abi.BF16: torch.bfloat16}
    ES = {abi.F32: 4, abi.F16: 2, abi.BF16: 2}
    U = abi.VARIANT_DN_UNFUSED_IO
    sw, sh = 3840, 2160
    base = synth.lcg_f32((sh, sw, 4))
    for name, (nw, nh) in (("cfg4", (1280, 720)), ("1080p", (1920, 1080))):
        rows = [("a  f32->f32 k_dnf", lib, abi.F32, abi.F32, 0),
                ("b  f16->f16 fused", lib, abi.F16, abi.F16, 0),
                ("c  f16->f16 pack + k_dnf + output stage", lib, abi.F16,
                 abi.F16, U),
                ("d  bf16->bf16 fused", lib, abi.BF16, abi.BF16, 0),
                ("e  bf16->bf16 pack + k_dnf + output stage", lib, abi.BF16,
                 abi.BF16, U),
                ("f  f32->f16", lib, abi.F32, abi.F16, 0),
                ("g  f16->f32", lib, abi.F16, abi.F32, 0)]
        pairs = [(rows[1][0], rows[2][0]), (rows[3][0], rows[4][0])]
        if parent:
            rows.insert(0, ("a' f32->f32 parent build", abi.load_path(parent),
                            abi.F32, abi.F32, 0))
        run, keep, first = {}, [], {}
        for tag, L, ti, to, variant in rows:
            pair = sw * sh * 4 * ES[ti] + nw * nh * 4 * ES[to]
            n = max(2, -(-(512 << 20) // pair))
            ring = []
            for i in range(n):
                s = torch.from_numpy(np.roll(base, i, axis=0)).to(dev).to(TD[ti])
                d = torch.empty((nh, nw, 4), dtype=TD[to], device=dev)
                ring.append((s, d))
            with abi.using(L):
                r = avir_amd.CImageResizer(16)
                p = r.plan(sw, sh, nw, nh, 4, 0.0, None, ti, to)
            abi.check(L.avirhip_plan_set_path(p, 2), "path 2")
            if variant:
                abi.check(L.avirhip_plan_set_variant(p, variant), "variant")
            keep.append((r, ring))

            def once(L=L, p=p, ring=ring):
                t = 0.0
                ms = C.c_double()
                for s, d in ring:
                    abi.check(L.avirhip_time_resize(
                        p, s.data_ptr(), d.data_ptr(), 1, st, C.byref(ms)),
                        "time_resize")
                    t += ms.value
                return t / len(ring)
            run[tag] = (once, pair, n, L, p)
            first[tag] = ring[0][1]
        for tag in run:  # warm-up, clocks
            for _ in range(20):
                run[tag][0]()
        torch.cuda.synchronize()
        same = [torch.equal(first[x].view(torch.uint8),
                            first[y].view(torch.uint8)) for x, y in pairs]
        res = {tag: [] for tag in run}
        loops = 40
        for _ in range(reps):
            for tag in run:
                res[tag].append(sum(run[tag][0]() for _ in range(loops)) / loops)
        print("%s (%dx%d -> %dx%d RGBA, path 2), %d reps x %d ring passes:" % (
            name, sw, sh, nw, nh, reps, loops))
        for tag in run:
            v = sorted(res[tag])
            med = v[len(v) // 2]
            print("  %-42s %.4f ms  (min %.4f max %.4f)  %6.1f MB/call  "
                  "%.2f TB/s  ring %d  plan holds %.1f MB" % (
                      tag, med, v[0], v[-1], run[tag][1] / 1e6,
                      run[tag][1] / med / 1e9, run[tag][2],
                      run[tag][3].avirhip_plan_device_bytes(run[tag][4]) / 1e6),
                  flush=True)
        print("  (b) and (c) bit-identical: %s" % same[0], flush=True)
        print("  (d) and (e) bit-identical: %s" % same[1], flush=True)
        del keep, run, first
        torch.cuda.empty_cache()


def dnsrgb_main(argv):
    """--dnsrgb: the rows of the module docstring, CImageResizer(8) plans with
    UseSRGBGamma on path 2. The unfused rows (AVIRHIP_VARIANT_DN_UNFUSED_IO)
    are the road before k_dnfh's DH_S8 kinds and the yardstick of each pair."""
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    reps = int(argv[2]) if len(argv) > 2 else 5
    lib = abi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    header(lib, None)
    TD = {abi.F32: torch.float32, abi.U8: torch.uint8}
    ES = {abi.F32: 4, abi.U8: 1}
    U = abi.VARIANT_DN_UNFUSED_IO
    sw, sh = 3840, 2160
    gv = avir_amd.CImageResizerVars()
    gv.UseSRGBGamma, gv.AlphaIndex = 1, 3
    for name, (nw, nh) in (("1080p", (1920, 1080)), ("720p", (1280, 720))):
        rows = [("a  RGBA u8->u8 gamma fused", 4, abi.U8, abi.U8, 0, gv),
                ("b  RGBA u8->u8 gamma pack + k_dnf + output stage", 4,
                 abi.U8, abi.U8, U, gv),
                ("c  RGBA u8->f32 gamma fused", 4, abi.U8, abi.F32, 0, gv),
                ("d  RGBA u8->f32 gamma pack + k_dnf", 4, abi.U8, abi.F32, U,
                 gv),
                ("e  RGB u8->u8 gamma pack + fused store", 3, abi.U8, abi.U8,
                 0, gv),
                ("f  RGB u8->u8 gamma pack + k_dnf + output stage", 3, abi.U8,
                 abi.U8, U, gv),
                ("g  RGBA u8->u8 no gamma", 4, abi.U8, abi.U8, 0, None)]
        pairs = [(rows[0][0], rows[1][0]), (rows[2][0], rows[3][0]),
                 (rows[4][0], rows[5][0])]
        run, keep, first = {}, [], {}
        for tag, ch, ti, to, variant, vars_ in rows:
            base = synth.lcg_u8((sh, sw, ch))
            pair = sw * sh * ch * ES[ti] + nw * nh * ch * ES[to]
            n = max(2, -(-(512 << 20) // pair))
            ring = []
            for i in range(n):
                s = torch.from_numpy(np.roll(base, i, axis=0)).to(dev)
                d = torch.empty((nh, nw, ch), dtype=TD[to], device=dev)
                ring.append((s, d))
            r = avir_amd.CImageResizer(8)
            p = r.plan(sw, sh, nw, nh, ch, 0.0, vars_, ti, to)
            abi.check(lib.avirhip_plan_set_path(p, 2), "path 2")
            if variant:
                abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
            keep.append((r, ring))

            def once(p=p, ring=ring):
                t = 0.0
                ms = C.c_double()
                for s, d in ring:
                    abi.check(lib.avirhip_time_resize(
                        p, s.data_ptr(), d.data_ptr(), 1, st, C.byref(ms)),
                        "time_resize")
                    t += ms.value
                return t / len(ring)
            run[tag] = (once, pair, n, p)
            first[tag] = ring[0][1]
        # (row e: the store side alone, forced at this size)
        with _env({"AVIRHIP_DNSRGB_STORE_MAXPIX": str(1 << 40)}):
            for tag in run:  # warm-up, clocks
                for _ in range(20):
                    run[tag][0]()
            torch.cuda.synchronize()
            same = [torch.equal(first[x].view(torch.uint8),
                                first[y].view(torch.uint8)) for x, y in pairs]
            res = {tag: [] for tag in run}
            loops = 20
            for _ in range(reps):
                for tag in run:
                    res[tag].append(
                        sum(run[tag][0]() for _ in range(loops)) / loops)
        print("%s (%dx%d -> %dx%d, ResBitDepth 8, path 2), %d reps x %d ring "
              "passes:" % (name, sw, sh, nw, nh, reps, loops))
        for tag in run:
            v = sorted(res[tag])
            med = v[len(v) // 2]
            print("  %-50s %.4f ms  (min %.4f max %.4f)  %6.1f MB/call  "
                  "%.2f TB/s  ring %d  plan holds %.1f MB" % (
                      tag, med, v[0], v[-1], run[tag][1] / 1e6,
                      run[tag][1] / med / 1e9, run[tag][2],
                      lib.avirhip_plan_device_bytes(run[tag][3]) / 1e6),
                  flush=True)
        for (x, y), ok in zip(pairs, same):
            print("  (%s) and (%s) bit-identical: %s" % (x[0], y[0], ok),
                  flush=True)
        del keep, run, first
        torch.cuda.empty_cache()
    # the store side alone (RGB uint8 -> uint8: pack pass + k_dnfh< F32, S8 >
    # against pack pass + k_dnf + output stage) by frame size: where
    # dnsrgb_store_maxpix (api.cpp) belongs. AVIRHIP_DNSRGB_STORE_MAXPIX is
    # read per call; every shape is a two-step plan at ResBitDepth 8.
    gv3 = avir_amd.CImageResizerVars()
    gv3.UseSRGBGamma = 1
    print("store side alone, RGB u8->u8 gamma, fused store / output stage:")
    for sw, sh, nw, nh in ((3840, 2160, 1920, 1080), (2560, 1440, 1280, 720),
                           (1920, 1080, 960, 540), (1920, 1080, 640, 360),
                           (1200, 800, 600, 400), (1200, 801, 400, 267),
                           (600, 400, 300, 200), (600, 402, 200, 134)):
        base = synth.lcg_u8((sh, sw, 3))
        pair = sw * sh * 3 + nw * nh * 3
        n = max(2, -(-(512 << 20) // pair))
        ring = [(torch.from_numpy(np.roll(base, i, axis=0)).to(dev),
                 torch.empty((nh, nw, 3), dtype=torch.uint8, device=dev))
                for i in range(min(n, 64))]
        keep, run = [], {}
        for tag, variant in (("fused", 0), ("unfused", U)):
            r = avir_amd.CImageResizer(8)
            p = r.plan(sw, sh, nw, nh, 3, 0.0, gv3, abi.U8, abi.U8)
            abi.check(lib.avirhip_plan_set_path(p, 2), "path 2")
            abi.check(lib.avirhip_plan_set_variant(p, variant), "variant")
            keep.append(r)

            def once(p=p):
                t = 0.0
                ms = C.c_double()
                for s, d in ring:
                    abi.check(lib.avirhip_time_resize(
                        p, s.data_ptr(), d.data_ptr(), 1, st, C.byref(ms)),
                        "time_resize")
                    t += ms.value
                return t / len(ring)
            run[tag] = once
        res = {tag: [] for tag in run}
        with _env({"AVIRHIP_DNSRGB_STORE_MAXPIX": str(1 << 40)}):
            for tag in run:
                for _ in range(5):
                    run[tag]()
            for _ in range(reps):
                for tag in run:
                    res[tag].append(sum(run[tag]() for _ in range(10)) / 10)
        out = []
        for tag in run:
            v = sorted(res[tag])
            out.append("%s %.4f ms (min %.4f max %.4f)" % (
                tag, v[len(v) // 2], v[0], v[-1]))
        print("  %dx%d -> %dx%d (%d source pixels): %s" % (
            sw, sh, nw, nh, sw * sh, ", ".join(out)), flush=True)
        del keep, run, ring
        torch.cuda.empty_cache()


def up2srgb_main(argv):
    """--up2srgb: the rows of the module docstring, CImageResizer(8) plans on
    path 4; every row of a shape in one rotation."""
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    parent = argv[1] if len(argv) > 1 and argv[1] != "-" else None
    reps = int(argv[2]) if len(argv) > 2 else 5
    lib = abi.load()
    plib = abi.load_path(parent) if parent else None
    alib = abi.load_path(argv[3]) if len(argv) > 3 else None
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    header(lib, parent)
    TD = {abi.F32: torch.float32, abi.U8: torch.uint8}
    ES = {abi.F32: 4, abi.U8: 1}
    U = abi.VARIANT_UP2_UNFUSED_IO
    g4 = avir_amd.CImageResizerVars()
    g4.UseSRGBGamma, g4.AlphaIndex = 1, 3
    g3 = avir_amd.CImageResizerVars()
    g3.UseSRGBGamma = 1
    # the kernel's gamma kinds whatever the frame size (the library routes by
    # up2srgb_raw_minpix / _maxpix and up2srgb_store_maxpix, read per call)
    F = {"AVIRHIP_UP2SRGB_RAW_MINPIX": "0",
         "AVIRHIP_UP2SRGB_RAW_MAXPIX": "1000000000",
         "AVIRHIP_UP2SRGB_STORE_MAXPIX": "1000000000"}
    # BOUNDS: the fused roads against the road before over a ladder of frame
    # sizes, which is where those two bounds come from
    bounds = len(argv) > 4 and argv[4] == "bounds"
    shapes = (("1080p", (1920, 1080)), ("2160p", (3840, 2160)))
    if bounds:
        shapes = tuple(("%dx%d" % g, g) for g in (
            (640, 360), (1280, 720), (1920, 1080), (2560, 1440),
            (3200, 1800), (3840, 2160)))
    for name, (sw, sh) in shapes:
        nw, nh = 2 * sw, 2 * sh
        # (tag, library, channels, in, out, variant, vars, environment)
        rows = []
        for ch, gv in ((4, g4), (3, g3)):
            c = "RGBA" if ch == 4 else "RGB"
            rows += [("%s u8->u8 gamma, one launch" % c, lib, ch, abi.U8,
                      abi.U8, 0, gv, F),
                     ("%s u8->u8 gamma, pack + k_up2 + output stage" % c, lib,
                      ch, abi.U8, abi.U8, U, gv, {})]
            if bounds:
                continue
            if plib is not None:
                rows.append(("%s u8->u8 gamma, parent build" % c, plib, ch,
                             abi.U8, abi.U8, 0, gv, {}))
            rows.append(("%s u8->u8 no gamma" % c, lib, ch, abi.U8, abi.U8, 0,
                         None, {}))
        for ch, gv in ((4, g4), (3, g3)):
            c = "RGBA" if ch == 4 else "RGB"
            rows += [("%s f32->u8 gamma, pack + k_up2 store" % c, lib, ch,
                      abi.F32, abi.U8, 0, gv, F),
                     ("%s f32->u8 gamma, pack + k_up2 + output stage" % c,
                      lib, ch, abi.F32, abi.U8, U, gv, {})]
        if not bounds:
            rows += [("RGBA f32->u8 gamma, store, LDS + 1 KB (6 workgroups)",
                      lib, 4, abi.F32, abi.U8, 0, g4,
                      dict(F, AVIRHIP_UP2_LDSPAD="1024")),
                     ("RGBA u8->u8 gamma, one launch, LDS + 4 KB "
                      "(5 workgroups)", lib, 4, abi.U8, abi.U8, 0, g4,
                      dict(F, AVIRHIP_UP2_LDSPAD="4096")),
                     ("RGBA f32->f32", lib, 4, abi.F32, abi.F32, 0, None, {})]
        if alib is not None and not bounds:
            rows += [("RGBA u8->u8 gamma, one launch, 1 KB thresholds "
                      "(7 workgroups)", alib, 4, abi.U8, abi.U8, 0, g4, F),
                     ("RGB u8->u8 gamma, one launch, 1 KB thresholds "
                      "(7 workgroups)", alib, 3, abi.U8, abi.U8, 0, g3, F),
                     ("RGBA f32->u8 gamma, store, 1 KB thresholds "
                      "(8 workgroups)", alib, 4, abi.F32, abi.U8, 0, g4, F)]
        if plib is not None and not bounds:
            rows.append(("RGBA f32->f32, parent build", plib, 4, abi.F32,
                         abi.F32, 0, None, {}))
        pairs = [(rows[i][0], rows[i + 1][0]) for i in range(len(rows) - 1)
                 if "one launch" in rows[i][0] or "k_up2 store" in rows[i][0]]
        pairs = [(x, y) for x, y in pairs if "output stage" in y]
        run, keep, first = {}, [], {}
        for tag, L, ch, ti, to, variant, vars_, env in rows:
            base = synth.lcg_u8((sh, sw, ch))
            if ti == abi.F32:
                base = (base.astype(np.float32) / np.float32(255.0))
            pair = sw * sh * ch * ES[ti] + nw * nh * ch * ES[to]
            n = max(2, -(-(512 << 20) // pair))
            ring = []
            for i in range(n):
                s = torch.from_numpy(np.roll(base, i, axis=0)).to(dev)
                d = torch.empty((nh, nw, ch), dtype=TD[to], device=dev)
                ring.append((s, d))
            with abi.using(L):
                r = avir_amd.CImageResizer(8 if to == abi.U8 else 16)
                p = r.plan(sw, sh, nw, nh, ch, 0.0, vars_, ti, to)
            abi.check(L.avirhip_plan_set_path(p, abi.PATH_UP2), "path 4")
            abi.check(L.avirhip_plan_set_variant(p, variant), "variant")
            keep.append((r, ring))

            def once(L=L, p=p, ring=ring, env=env):
                t = 0.0
                ms = C.c_double()
                with _env(env):
                    for s, d in ring:
                        abi.check(L.avirhip_time_resize(
                            p, s.data_ptr(), d.data_ptr(), 1, st,
                            C.byref(ms)), "time_resize")
                        t += ms.value
                return t / len(ring)
            run[tag] = (once, pair, n, p, L)
            first[tag] = ring[0][1]
        for tag in run:  # warm-up, clocks
            for _ in range(10):
                run[tag][0]()
        torch.cuda.synchronize()
        same = [torch.equal(first[x], first[y]) for x, y in pairs]
        res = {tag: [] for tag in run}
        loops = 10 if sw * sh > 4000000 else 20
        for _ in range(reps):
            for tag in run:
                res[tag].append(
                    sum(run[tag][0]() for _ in range(loops)) / loops)
        print("%s (%dx%d -> %dx%d, path 4), %d reps x %d ring passes:" % (
            name, sw, sh, nw, nh, reps, loops))
        for tag in run:
            v = sorted(res[tag])
            med = v[len(v) // 2]
            print("  %-58s %.4f ms  (min %.4f max %.4f)  %6.1f MB/call  "
                  "%.2f TB/s  ring %d  plan holds %.1f MB" % (
                      tag, med, v[0], v[-1], run[tag][1] / 1e6,
                      run[tag][1] / med / 1e9, run[tag][2],
                      run[tag][4].avirhip_plan_device_bytes(run[tag][3]) /
                      1e6), flush=True)
        for (x, y), ok in zip(pairs, same):
            print("  (%s) and (%s) bit-identical: %s" % (x, y, ok),
                  flush=True)
        del keep, run, first
        torch.cuda.empty_cache()


class _env(object):
    """`with _env(d):` -- the variables of a call (read per call by the
    library), put back after."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.keep = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def gpass_main(argv):
    """--gpass: general ratios on the automatic path (the pass kernels, path 5,
    at every shape below). Rows per shape and type: float32; the 16-bit call
    as it runs automatically; the same call under AVIRHIP_GP_NO_IO16 (the road
    before the typed k_gh and the narrowing store: pack pass, kernels, output
    stage -- the baseline); and, where the float RGBA kernel of the shape has
    no typed form (k_gf, k_gh2), the typed k_gh road forced
    (AVIRHIP_GP_IO16_GF / AVIRHIP_GP_IO16_GH2 = 1).
    With PARENT.so: RGB uint8 through the shared store function, both builds
    alternating (cfg1 640x480 -> 1024x768, 1920x1080 -> 2500x1400)."""
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    parent = argv[1] if len(argv) > 1 and argv[1] != "-" else None
    reps = int(argv[2]) if len(argv) > 2 else 5
    lib = abi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    header(lib, parent)
    TD = {abi.F32: torch.float32, abi.F16: torch.float16,
          abi.BF16: torch.bfloat16, abi.U8: torch.uint8}
    ES = {abi.F32: 4, abi.F16: 2, abi.BF16: 2, abi.U8: 1}
    NO = {"AVIRHIP_GP_NO_IO16": "1"}
    GF = {"AVIRHIP_GP_IO16_GF": "1"}
    GH2 = {"AVIRHIP_GP_IO16_GH2": "1"}
    F32, F16, BF16, U8 = abi.F32, abi.F16, abi.BF16, abi.U8

    def same16(tag, ti, to, ch=4, alt=None, altname=""):
        rows = [("%s fused (automatic)" % tag, lib, ti, to, ch, {}),
                ("%s pack + output stage" % tag, lib, ti, to, ch, NO)]
        if alt is not None:
            rows.append(("%s %s" % (tag, altname), lib, ti, to, ch, alt))
        return rows

    shapes = [
        ("1080p x1.3", (1920, 1080, 2500, 1400),
         same16("f16->f16", F16, F16) + same16("bf16->bf16", BF16, BF16) +
         same16("f32->bf16", F32, BF16) + same16("RGB f16->f16", F16, F16, 3)),
        ("4K k1.5", (3840, 2160, 2560, 1440),
         same16("f16->f16", F16, F16) + same16("bf16->bf16", BF16, BF16) +
         same16("f32->bf16", F32, BF16)),
        ("4K k1.92", (3840, 2160, 2000, 1125),
         same16("f16->f16", F16, F16, 4, GH2, "typed k_gh forced") +
         same16("bf16->bf16", BF16, BF16, 4, GH2, "typed k_gh forced")),
        ("1080p x3", (1920, 1080, 5760, 3240),
         same16("f16->f16", F16, F16, 4, GF, "typed k_gh + k_gv forced") +
         same16("bf16->bf16", BF16, BF16, 4, GF, "typed k_gh + k_gv forced")),
        ("4K x1.6", (3840, 2160, 6144, 3456),
         same16("f16->f16", F16, F16, 4, GF, "typed k_gh + k_gv forced")),
        ("5184 k2.7", (5184, 3456, 1920, 1280),
         same16("f16->f16", F16, F16) + same16("bf16->bf16", BF16, BF16)),
    ]
    if parent:
        P = abi.load_path(parent)
        for name, g in (("cfg1 RGB u8", (640, 480, 1024, 768)),
                        ("1080p x1.3 RGB u8", (1920, 1080, 2500, 1400))):
            shapes.append((name, g, [("u8->u8 this build", lib, U8, U8, 3, {}),
                                     ("u8->u8 parent build", P, U8, U8, 3, {}),
                                     ("u8->u8 this build again", lib, U8, U8, 3,
                                      {})]))
    only = argv[3].split(",") if len(argv) > 3 else None  # (--gpass: ONLY)
    for name, (sw, sh, nw, nh), rows in shapes:
        if only is not None and not any(o in name for o in only):
            continue
        base = synth.lcg_f32((sh, sw, 4))
        if not name.endswith("u8"):
            rows = [("f32->f32", lib, F32, F32, 4, {})] + rows
        run, keep, first = {}, [], {}
        for tag, L, ti, to, ch, env in rows:
            pair = sw * sh * ch * ES[ti] + nw * nh * ch * ES[to]
            n = max(2, -(-(512 << 20) // pair))
            ring = []
            for i in range(n):
                b = np.roll(base, i, axis=0)[:, :, :ch]
                if ti == U8:
                    b = b * 255.0
                s = torch.from_numpy(np.ascontiguousarray(b)).to(dev).to(TD[ti])
                d = torch.empty((nh, nw, ch), dtype=TD[to], device=dev)
                ring.append((s, d))
            with abi.using(L):
                r = avir_amd.CImageResizer(8 if to == U8 else 16)
                p = r.plan(sw, sh, nw, nh, ch, 0.0, None, ti, to)
            keep.append((r, ring))

            def once(L=L, p=p, ring=ring, env=env):
                t = 0.0
                ms = C.c_double()
                with _env(env):
                    for s, d in ring:
                        abi.check(L.avirhip_time_resize(
                            p, s.data_ptr(), d.data_ptr(), 1, st, C.byref(ms)),
                            "time_resize")
                        t += ms.value
                return t / len(ring)
            run[tag] = (once, pair, n, L, p)
            first[tag] = ring[0][1]
        for tag in run:  # warm-up, clocks
            for _ in range(10):
                run[tag][0]()
        torch.cuda.synchronize()
        res = {tag: [] for tag in run}
        loops = 20
        for _ in range(reps):
            for tag in run:
                res[tag].append(sum(run[tag][0]() for _ in range(loops)) / loops)
        print("%s (%dx%d -> %dx%d), path %d, %d reps x %d ring passes:" % (
            name, sw, sh, nw, nh, lib.avirhip_plan_get_path(run[rows[-1][0]][4]),
            reps, loops))
        for tag in run:
            v = sorted(res[tag])
            med = v[len(v) // 2]
            print("  %-44s %.4f ms  (min %.4f max %.4f)  %6.1f MB/call  "
                  "ring %d  plan holds %.1f MB" % (
                      tag, med, v[0], v[-1], run[tag][1] / 1e6, run[tag][2],
                      run[tag][3].avirhip_plan_device_bytes(run[tag][4]) / 1e6),
                  flush=True)
        tags = [t for t in run if t != "f32->f32"]
        for i in range(0, len(tags) - 1):
            a, b = tags[i], tags[i + 1]
            if a.split(" fused")[0] == b.split(" pack")[0] or "u8" in a:
                print("  %s / %s bit-identical: %s" % (a, b, torch.equal(
                    first[a].view(torch.uint8), first[b].view(torch.uint8))),
                    flush=True)
        del keep, run, first
        torch.cuda.empty_cache()


def lancgp_main(argv):
    """--lancgp: the rows of the module docstring, CLancIR plans on their
    automatic path (5 at every shape below)."""
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    parent = argv[1] if len(argv) > 1 and argv[1] != "-" else None
    reps = int(argv[2]) if len(argv) > 2 else 5
    only = argv[3].split(",") if len(argv) > 3 else None
    lib = abi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    header(lib, parent)
    TD = {abi.F32: torch.float32, abi.F16: torch.float16,
          abi.BF16: torch.bfloat16, abi.U8: torch.uint8}
    ES = {abi.F32: 4, abi.F16: 2, abi.BF16: 2, abi.U8: 1}
    F32, F16, BF16, U8 = abi.F32, abi.F16, abi.BF16, abi.U8
    U = abi.VARIANT_UP2_UNFUSED_IO
    VF, V2 = abi.VARIANT_UPG_FUSED, abi.VARIANT_UPG_TWO_PASS

    def both(tag, ti, to, ch=4):
        return [("%s fused (automatic)" % tag, lib, ti, to, ch, 0),
                ("%s pack + output stage" % tag, lib, ti, to, ch, U)]

    f32 = [("f32->f32", lib, F32, F32, 4, 0)]
    shapes = [
        ("1080p x1.3", (1920, 1080, 2500, 1400),
         f32 + both("f16->f16", F16, F16) + both("bf16->bf16", BF16, BF16) +
         both("RGB f16->f16", F16, F16, 3)),
        ("4K k3", (3840, 2160, 1280, 720),
         f32 + both("f16->f16", F16, F16) + both("bf16->bf16", BF16, BF16)),
        ("1080p x3", (1920, 1080, 5760, 3240),
         f32 + both("f16->f16", F16, F16) + both("bf16->bf16", BF16, BF16)),
    ]
    for name, (nw, nh) in (("sweep x1.5", (2880, 1620)),
                           ("sweep x2.5", (4800, 2700)),
                           ("sweep x3", (5760, 3240)),
                           ("sweep x4", (7680, 4320))):
        shapes.append((name, (1920, 1080, nw, nh),
                       [("f16->f16 k_lf", lib, F16, F16, 4, VF),
                        ("f16->f16 k_gv + k_gh", lib, F16, F16, 4, V2),
                        ("f32->f16 k_lf", lib, F32, F16, 4, VF),
                        ("f32->f16 k_gv + k_gh", lib, F32, F16, 4, V2)]))
    if parent:
        P = abi.load_path(parent)

        def ab(ti, ch):
            return [("this build", lib, ti, ti, ch, 0),
                    ("parent build", P, ti, ti, ch, 0),
                    ("this build again", lib, ti, ti, ch, 0)]
        shapes += [
            ("parent 5184 RGB u8", (5184, 3456, 1920, 1280), ab(U8, 3)),
            ("parent 4K k3 RGBA u8", (3840, 2160, 1280, 720), ab(U8, 4)),
            ("parent 1080p x1.3 RGB u8", (1920, 1080, 2500, 1400), ab(U8, 3)),
            ("parent 1080p x1.3 RGBA u8", (1920, 1080, 2500, 1400), ab(U8, 4)),
            ("parent 1080p x1.3 RGBA f32", (1920, 1080, 2500, 1400),
             ab(F32, 4))]
    for name, (sw, sh, nw, nh), rows in shapes:
        if only is not None and not any(o in name for o in only):
            continue
        base = synth.lcg_f32((sh, sw, 4))
        run, keep, first = {}, [], {}
        for tag, L, ti, to, ch, variant in rows:
            pair = sw * sh * ch * ES[ti] + nw * nh * ch * ES[to]
            n = max(2, -(-(512 << 20) // pair))
            ring = []
            for i in range(n):
                b = np.roll(base, i, axis=0)[:, :, :ch]
                if ti == U8:
                    b = b * 255.0
                s = torch.from_numpy(np.ascontiguousarray(b)).to(dev).to(TD[ti])
                d = torch.empty((nh, nw, ch), dtype=TD[to], device=dev)
                ring.append((s, d))
            with abi.using(L):
                r = avir_amd.CLancIR()
                p = r.plan(sw, sh, nw, nh, ch, None, ti, to)
            if variant:
                abi.check(L.avirhip_plan_set_variant(p, variant), "variant")
            keep.append((r, ring))

            def once(L=L, p=p, ring=ring):
                t = 0.0
                ms = C.c_double()
                for s, d in ring:
                    abi.check(L.avirhip_time_resize(
                        p, s.data_ptr(), d.data_ptr(), 1, st, C.byref(ms)),
                        "time_resize")
                    t += ms.value
                return t / len(ring)
            run[tag] = (once, pair, n, L, p)
            first[tag] = ring[0][1]
        for tag in run:  # warm-up, clocks
            for _ in range(10):
                run[tag][0]()
        torch.cuda.synchronize()
        res = {tag: [] for tag in run}
        loops = 20
        for _ in range(reps):
            for tag in run:
                res[tag].append(sum(run[tag][0]() for _ in range(loops)) / loops)
        print("%s (%dx%d -> %dx%d, CLancIR), path %d, %d reps x %d ring "
              "passes:" % (name, sw, sh, nw, nh,
                           lib.avirhip_plan_get_path(run[rows[0][0]][4]),
                           reps, loops))
        for tag in run:
            v = sorted(res[tag])
            med = v[len(v) // 2]
            print("  %-36s %.4f ms  (min %.4f max %.4f)  %6.1f MB/call  "
                  "ring %d  plan holds %.1f MB" % (
                      tag, med, v[0], v[-1], run[tag][1] / 1e6, run[tag][2],
                      run[tag][3].avirhip_plan_device_bytes(run[tag][4]) / 1e6),
                  flush=True)
        tags = list(run)
        for i in range(0, len(tags) - 1):
            a, b = tags[i], tags[i + 1]
            if (a.split(" fused")[0] == b.split(" pack")[0] or
                    a.split(" k_lf")[0] == b.split(" k_gv")[0] or
                    a == "this build"):
                print("  %s / %s bit-identical: %s" % (a, b, torch.equal(
                    first[a].view(torch.uint8), first[b].view(torch.uint8))),
                    flush=True)
        del keep, run, first
        torch.cuda.empty_cache()


def sacc_main(argv):
    """--sacc: downsizing by a non-integer ratio of 2 or more with 16-bit
    sources (the accumulation kernels' typed loaders 4 / 5). Rows per shape and
    type, all in this process and alternating: float32 on forced path 5; the
    16-bit call on forced path 5 as the typed exact road, as the typed
    optimistic road (AVIRHIP_VARIANT_SACC_OPTIMISTIC), with the branch-free
    launches alone (AVIRHIP_SACC_OPT_ONLY) and on the pack road
    (AVIRHIP_GP_NO_IO16); and the automatic path as built, as it chose before
    the typed road (a plan made under AVIRHIP_SA16_AUTO_MINPIX = never) and
    with path 5 admitted (= 0). With PARENT.so: README's uint8 and float32 accumulation
    rows on both builds."""
    import torch
    import avir_amd
    from avir_amd import abi, synth
    parent = argv[1] if len(argv) > 1 and argv[1] != "-" else None
    reps = int(argv[2]) if len(argv) > 2 else 5
    only = argv[3].split(",") if len(argv) > 3 else None
    lib = abi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    header(lib, parent)
    F32, F16, BF16, U8 = abi.F32, abi.F16, abi.BF16, abi.U8
    TD = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16,
          U8: torch.uint8}
    ES = {F32: 4, F16: 2, BF16: 2, U8: 1}
    NM = {F32: "f32", F16: "f16", BF16: "bf16", U8: "u8"}
    NO = {"AVIRHIP_GP_NO_IO16": "1"}
    ALONE = {"AVIRHIP_SACC_OPT_ONLY": "1"}
    OPT = abi.VARIANT_SACC_OPTIMISTIC
    NEVER = {"AVIRHIP_SA16_AUTO_MINPIX": str(1 << 60)}
    ALWAYS = {"AVIRHIP_SA16_AUTO_MINPIX": "0"}

    # a row: (tag, library, tin, tout, channels, forced path, variant,
    #         environment of the plan's making, environment of the call)
    def rows16(ti, to, ch=4, auto=True):
        t = "%s->%s" % (NM[ti], NM[to]) + (" RGB" if ch == 3 else "")
        # (AVIRHIP_VARIANT_SACC_LADDER: the exact kernels whatever the size)
        r = [(t + " typed exact", lib, ti, to, ch, 5, abi.VARIANT_SACC_LADDER,
              {}, {}),
             (t + " typed optimistic", lib, ti, to, ch, 5, OPT, {}, {}),
             (t + " branch-free alone", lib, ti, to, ch, 5, OPT, {}, ALONE),
             (t + " pack road", lib, ti, to, ch, 5, 0, {}, NO)]
        if auto:
            r += [(t + " auto as built", lib, ti, to, ch, 0, 0, {}, {}),
                  (t + " auto before", lib, ti, to, ch, 0, 0, NEVER, {}),
                  (t + " auto, path 5 admitted", lib, ti, to, ch, 0, 0, ALWAYS,
                   {})]
        return r

    def f32row(ch=4):
        return [("f32->f32" + (" RGB" if ch == 3 else "") + " path 5", lib, F32,
                 F32, ch, 5, 0, {}, {})]

    shapes = [
        ("5184 RGBA", (5184, 3456, 1920, 1280),
         f32row() + rows16(F16, F16) + rows16(BF16, BF16)),
        ("5184 RGB", (5184, 3456, 1920, 1280),
         f32row(3) + rows16(F16, F16, 3) + rows16(BF16, BF16, 3)),
        ("4K", (3840, 2160, 1500, 844),
         f32row() + rows16(F16, F16) + rows16(BF16, BF16) +
         rows16(F16, F16, 3)),
        ("4K pairs", (3840, 2160, 1500, 844),
         [("f32->f16 path 5", lib, F32, F16, 4, 5, 0, {}, {})] +
         rows16(F16, F32, 4, False)),
        ("1080p", (1920, 1080, 700, 394),
         f32row() + rows16(F16, F16) + rows16(BF16, BF16) +
         rows16(F16, F16, 3)),
        ("480p", (640, 480, 233, 175),
         f32row() + rows16(F16, F16) + rows16(BF16, BF16) +
         rows16(F16, F16, 3)),
        ("mixed", (3840, 1080, 1500, 1400),
         f32row() + rows16(F16, F16, 4, False) + rows16(BF16, BF16, 4, False)),
        # between the shapes above: where the automatic path and the
        # optimistic form cross, and the smallest frames over the floor
        ("1800p", (3200, 1800, 1200, 675),
         rows16(F16, F16) + rows16(BF16, BF16) + rows16(F16, F16, 3)),
        ("1440p", (2560, 1440, 1000, 563),
         rows16(F16, F16) + rows16(BF16, BF16) + rows16(F16, F16, 3)),
        ("240p", (320, 240, 117, 88),
         rows16(F16, F16, 4, False) + rows16(BF16, BF16, 4, False) +
         rows16(F16, F16, 3, False)),
    ]
    if parent:
        P = abi.load_path(parent)
        for name, g, ti, ch in (
                ("parent 5184 RGB u8", (5184, 3456, 1920, 1280), U8, 3),
                ("parent 5184 RGBA f32", (5184, 3456, 1920, 1280), F32, 4),
                ("parent 4K RGBA f32", (3840, 2160, 1500, 844), F32, 4)):
            shapes.append((name, g, [
                ("this build", lib, ti, ti, ch, 0, 0, {}, {}),
                ("parent build", P, ti, ti, ch, 0, 0, {}, {}),
                ("this build again", lib, ti, ti, ch, 0, 0, {}, {})]))
    for name, (sw, sh, nw, nh), rows in shapes:
        if only is not None and not any(o in name for o in only):
            continue
        base = torch.from_numpy(synth.lcg_f32((sh, sw, 4))).to(dev)
        run, keep, rings = {}, [], {}
        for tag, L, ti, to, ch, path, variant, penv, env in rows:
            pair = sw * sh * ch * ES[ti] + nw * nh * ch * ES[to]
            n = max(2, -(-(512 << 20) // pair))
            if (ti, to, ch) not in rings:  # (rows of a kind share their ring)
                ring = []
                for i in range(n):
                    b = torch.roll(base, i, 0)[:, :, :ch]
                    if ti == U8:
                        b = b * 255.0
                    s = b.contiguous().to(TD[ti])
                    d = torch.empty((nh, nw, ch), dtype=TD[to], device=dev)
                    ring.append((s, d))
                rings[(ti, to, ch)] = ring
            ring = rings[(ti, to, ch)]
            with abi.using(L), _env(penv):
                r = avir_amd.CImageResizer(8 if to == U8 else 16)
                p = r.plan(sw, sh, nw, nh, ch, 0.0, None, ti, to)
                abi.check(L.avirhip_plan_set_path(p, path), "set_path")
                abi.check(L.avirhip_plan_set_variant(p, variant), "variant")
            keep.append(r)

            def once(L=L, p=p, ring=ring, env=env):
                t = 0.0
                ms = C.c_double()
                with _env(env):
                    for s, d in ring:
                        abi.check(L.avirhip_time_resize(
                            p, s.data_ptr(), d.data_ptr(), 1, st, C.byref(ms)),
                            "time_resize")
                        t += ms.value
                return t / len(ring)
            run[tag] = (once, pair, n, L, p)
        for tag in run:  # warm-up, clocks
            for _ in range(5):
                run[tag][0]()
        torch.cuda.synchronize()
        res = {tag: [] for tag in run}
        loops = 10
        for _ in range(reps):
            for tag in run:
                res[tag].append(sum(run[tag][0]() for _ in range(loops)) / loops)
        print("%s (%dx%d -> %dx%d), %d reps x %d ring passes:" % (
            name, sw, sh, nw, nh, reps, loops))
        for tag in run:
            v = sorted(res[tag])
            print("  %-36s %.4f ms  (min %.4f max %.4f)  path %d  ring %d  "
                  "plan holds %.1f MB" % (
                      tag, v[len(v) // 2], v[0], v[-1],
                      run[tag][3].avirhip_plan_get_path(run[tag][4]),
                      run[tag][2],
                      run[tag][3].avirhip_plan_device_bytes(run[tag][4]) / 1e6),
                  flush=True)
        del keep, run, rings
        torch.cuda.empty_cache()


def main():
    if "--sacc" in sys.argv:
        return sacc_main([a for a in sys.argv if a != "--sacc"])
    if "--lancgp" in sys.argv:
        return lancgp_main([a for a in sys.argv if a != "--lancgp"])
    if "--gpass" in sys.argv:
        return gpass_main([a for a in sys.argv if a != "--gpass"])
    if "--lancir" in sys.argv:
        return lancir_main([a for a in sys.argv if a != "--lancir"])
    if "--dnf" in sys.argv:
        return dnf_main([a for a in sys.argv if a != "--dnf"])
    if "--dnsrgb" in sys.argv:
        return dnsrgb_main([a for a in sys.argv if a != "--dnsrgb"])
    if "--up2srgb" in sys.argv:
        return up2srgb_main([a for a in sys.argv if a != "--up2srgb"])
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    argv = [a for a in sys.argv if a != "--bf16"]
    bf16 = len(argv) != len(sys.argv)
    parent = argv[1] if len(argv) > 1 and argv[1] != "-" else None
    reps = int(argv[2]) if len(argv) > 2 else 5
    lib = abi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    print("library %s md5 %s" % (abi.LIB_PATH, md5(abi.LIB_PATH)))
    print("version %s" % lib.avirhip_version().decode())
    if parent:
        print("parent  %s md5 %s" % (parent, md5(parent)))
    print("device  %s" % torch.cuda.get_device_name(0))
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"],
                             capture_output=True, text=True, timeout=60).stdout
        for l in out.split("\n"):
            if "sclk" in l or "mclk" in l or "fclk" in l:
                print("clocks  " + l.strip())
    except Exception as e:  # (the table stands without them)
        print("clocks  unavailable: %r" % (e,))
    TD = {abi.F32: torch.float32, abi.F16: torch.float16,
          abi.BF16: torch.bfloat16}
    ES = {abi.F32: 4, abi.F16: 2, abi.BF16: 2}
    for name, (sw, sh) in (("cfg3", (3840, 2160)), ("cfg2", (1920, 1080))):
        nw, nh = 2 * sw, 2 * sh
        base = synth.lcg_f32((sh, sw, 4))
        rows = [("a  f32->f32", lib, abi.F32, abi.F32, 0),
                ("b  f16->f16 fused", lib, abi.F16, abi.F16, 0),
                ("c  f16->f16 pack + output stage", lib, abi.F16, abi.F16,
                 abi.VARIANT_UP2_UNFUSED_IO),
                ("d  f32->f16", lib, abi.F32, abi.F16, 0)]
        pairs = [("b  f16->f16 fused", "c  f16->f16 pack + output stage")]
        if bf16:
            rows += [("e  bf16->bf16 fused", lib, abi.BF16, abi.BF16, 0),
                     ("f  bf16->bf16 pack + output stage", lib, abi.BF16,
                      abi.BF16, abi.VARIANT_UP2_UNFUSED_IO),
                     ("g  f32->bf16", lib, abi.F32, abi.BF16, 0)]
            pairs.append(("e  bf16->bf16 fused",
                          "f  bf16->bf16 pack + output stage"))
        if parent:
            rows.insert(0, ("a' f32->f32 parent build", abi.load_path(parent),
                            abi.F32, abi.F32, 0))
        run, keep, first = {}, [], {}
        for tag, L, ti, to, variant in rows:
            pair = sw * sh * 4 * ES[ti] + nw * nh * 4 * ES[to]
            n = max(2, -(-(512 << 20) // pair))
            ring = []
            for i in range(n):
                s = torch.from_numpy(np.roll(base, i, axis=0)).to(dev).to(TD[ti])
                d = torch.empty((nh, nw, 4), dtype=TD[to], device=dev)
                ring.append((s, d))
            with abi.using(L):
                r = avir_amd.CImageResizer(16)
                p = r.plan(sw, sh, nw, nh, 4, 0.0, None, ti, to)
            abi.check(L.avirhip_plan_set_path(p, abi.PATH_UP2), "path 4")
            if variant:
                abi.check(L.avirhip_plan_set_variant(p, variant), "variant")
            keep.append((r, ring))

            def once(L=L, p=p, ring=ring):
                t = 0.0
                ms = C.c_double()
                for s, d in ring:
                    abi.check(L.avirhip_time_resize(
                        p, s.data_ptr(), d.data_ptr(), 1, st, C.byref(ms)),
                        "time_resize")
                    t += ms.value
                return t / len(ring)
            run[tag] = (once, pair, n)
            first[tag] = ring[0][1]
        for tag in run:  # warm-up, clocks
            for _ in range(20):
                run[tag][0]()
        torch.cuda.synchronize()
        same = [torch.equal(first[x].view(torch.uint8),
                            first[y].view(torch.uint8)) for x, y in pairs]
        res = {tag: [] for tag in run}
        loops = 30 if name == "cfg3" else 60
        for _ in range(reps):
            for tag in run:
                res[tag].append(sum(run[tag][0]() for _ in range(loops)) / loops)
        print("%s (%dx%d -> %dx%d RGBA), ring pairs per row below, %d reps x "
              "%d ring passes:" % (name, sw, sh, nw, nh, reps, loops))
        for tag in run:
            v = sorted(res[tag])
            med = v[len(v) // 2]
            print("  %-34s %.4f ms  (min %.4f max %.4f)  %6.1f MB/call  "
                  "%.2f TB/s  ring %d" % (
                      tag, med, v[0], v[-1], run[tag][1] / 1e6,
                      run[tag][1] / med / 1e9, run[tag][2]), flush=True)
        print("  (b) and (c) bit-identical: %s" % same[0], flush=True)
        if bf16:
            print("  (e) and (f) bit-identical: %s" % same[1], flush=True)
        del keep, run, first
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
