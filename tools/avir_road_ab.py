#!/usr/bin/env python3
"""What the host dispatch of a call costs on two builds of the library, in one
process: PARENT.so, a copy of PARENT.so (the control: what loading the same
code a second time is worth) and the tree's library are loaded side by side,
each with its own plan on the same device images; timed loops of about 0.2 s
(avirhip_time_resize: HIP events around `iters` back-to-back calls) alternate
between the three, five times. Prints every loop's ms per call, then medians
and the difference to PARENT's median, this library beside the control; and
whether the three outputs are bit-identical.

Workloads: bench.py's cfg2, cfg3 and cfg4; one k_dnfh uint8 -> uint8 sRGB call
and one path-5 half -> half call, at the sizes of tools/half_timing.py; and
CLancIR's: bench.py's cfg5 and lanc_up2_rgba8, one path-5 half -> half call.

  python tools/avir_road_ab.py PARENT.so PARENT_COPY.so [REPS=5]
"""
import ctypes as C
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

# (name, sw, sh, nw, nh, type in, type out, ResBitDepth; 0: CLancIR, gamma)
WORK = [("cfg2", 1920, 1080, 3840, 2160, "f32", "f32", 16, False),
        ("cfg3", 3840, 2160, 7680, 4320, "f32", "f32", 16, False),
        ("cfg4", 3840, 2160, 1280, 720, "f32", "f32", 16, False),
        ("k_dnfh sRGB u8->u8", 3840, 2160, 1280, 720, "u8", "u8", 8, True),
        ("path 5 f16->f16", 1920, 1080, 2500, 1400, "f16", "f16", 16, False),
        ("cfg5", 3840, 2160, 7680, 4320, "f32", "f32", 0, False),
        ("lanc_up2_rgba8", 1920, 1080, 3840, 2160, "u8", "u8", 0, False),
        ("lancir path 5 f16->f16", 1920, 1080, 2500, 1400, "f16", "f16", 0,
         False)]


def main(argv):
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    reps = int(argv[2]) if len(argv) > 2 else 5
    this = abi.load()
    libs = [("parent", abi.load_path(argv[0])), ("control", abi.load_path(argv[1])),
            ("this", this)]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    TT = {"f32": (abi.F32, torch.float32), "f16": (abi.F16, torch.float16),
          "u8": (abi.U8, torch.uint8)}
    print("device %s" % torch.cuda.get_device_name(0))
    for name, sw, sh, nw, nh, tin, tout, bits, gamma in WORK:
        base = synth.lcg_f32((sh, sw, 4))
        s = torch.from_numpy(base).to(dev)
        s = (s * 255).to(torch.uint8) if tin == "u8" else s.to(TT[tin][1])
        run, keep = {}, []
        for tag, L in libs:
            v = None
            if gamma:
                v = avir_amd.CImageResizerVars()
                v.UseSRGBGamma, v.AlphaIndex = 1, 3
            with abi.using(L):
                if bits == 0:
                    r = avir_amd.CLancIR()
                    p = r.plan(sw, sh, nw, nh, 4, None, TT[tin][0], TT[tout][0])
                else:
                    r = avir_amd.CImageResizer(bits)
                    p = r.plan(sw, sh, nw, nh, 4, 0.0, v, TT[tin][0],
                               TT[tout][0])
            d = torch.zeros((nh, nw, 4), dtype=TT[tout][1], device=dev)
            keep.append((r, d))
            ms = C.c_double()

            def once(n, L=L, p=p, d=d, ms=ms):
                abi.check(L.avirhip_time_resize(p, s.data_ptr(), d.data_ptr(),
                                                n, st, C.byref(ms)), "time")
                return ms.value
            run[tag] = (once, L, p, d)
        for tag in run:
            run[tag][0](20)
        torch.cuda.synchronize()
        iters = max(10, int(200.0 / max(run["parent"][0](10), 1e-3)))
        same = all(torch.equal(run["parent"][3].view(torch.uint8),
                               run[t][3].view(torch.uint8)) for t in run)
        res = {tag: [] for tag in run}
        for i in range(reps):
            for tag in run:
                res[tag].append(run[tag][0](iters))
                print("%s rep %d %s %.5f ms" % (name, i, tag, res[tag][-1]),
                      flush=True)
        med = {t: sorted(v)[len(v) // 2] for t, v in res.items()}
        print("== %s (%dx%d -> %dx%d %s->%s), path %d, %d calls a loop: parent "
              "%.5f ms; this %+.2f %%, control %+.2f %%; parent's own spread "
              "%.2f %%; outputs bit-identical: %s" % (
                  name, sw, sh, nw, nh, tin, tout,
                  this.avirhip_plan_get_path(run["this"][2]), iters,
                  med["parent"], 100 * (med["this"] / med["parent"] - 1),
                  100 * (med["control"] / med["parent"] - 1),
                  100 * (max(res["parent"]) / min(res["parent"]) - 1), same),
              flush=True)
        del run, keep
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
