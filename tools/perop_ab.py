#!/usr/bin/env python3
"""The per-op executor's host work on two builds of the library, in one
process, the way tools/avir_road_ab.py times a road: PARENT.so, a copy of
PARENT.so (the control) and the tree's library side by side, loops of about
0.2 s alternating between the three, five times.

Workloads: two float plans and one of the double class on forced path 1 (the
per-op kernels: one launch per lowered op, so the driver's share is at its
largest), bench.py's cfg2 and cfg4 on their automatic paths, and the creation
of cfg3's plan (lowering and upload of its tables). Then, for every case of
tests/perop_cases.py, avirhip_plan_device_bytes after plan creation and after
the first call with PARENT.so and with this library.

  python tools/perop_ab.py PARENT.so PARENT_COPY.so [REPS=5]
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

# (name, sw, sh, nw, nh, class, forced path)
WORK = [("per-op f32 up", 1920, 1080, 2500, 1400, 1, 1),
        ("per-op f32 down", 3840, 2160, 1280, 720, 1, 1),
        ("per-op double class", 1920, 1080, 2500, 1400, 64, 1),
        ("cfg2", 1920, 1080, 3840, 2160, 1, 0),
        ("cfg4", 3840, 2160, 1280, 720, 1, 0)]


def report(name, res, extra):
    med = {t: sorted(v)[len(v) // 2] for t, v in res.items()}
    print("== %s: parent %.5f ms; this %+.2f %%, control %+.2f %%; parent's "
          "own spread %.2f %%%s" % (
              name, med["parent"], 100 * (med["this"] / med["parent"] - 1),
              100 * (med["control"] / med["parent"] - 1),
              100 * (max(res["parent"]) / min(res["parent"]) - 1), extra),
          flush=True)


def main(argv):
    import numpy as np
    import torch
    import avir_amd
    from avir_amd import abi, synth
    from tests import perop_cases as PC
    reps = int(argv[2]) if len(argv) > 2 else 5
    this = abi.load()
    libs = [("parent", abi.load_path(argv[0])),
            ("control", abi.load_path(argv[1])), ("this", this)]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    print("device %s" % torch.cuda.get_device_name(0))
    for name, sw, sh, nw, nh, fp, path in WORK:
        s = torch.from_numpy(synth.lcg_f32((sh, sw, 4))).to(dev)
        run, keep = {}, []
        for tag, L in libs:
            with abi.using(L):
                r = avir_amd.CImageResizer(16, aFpPack=fp)
                p = r.plan(sw, sh, nw, nh, 4)
            abi.check(L.avirhip_plan_set_path(p, path), "set_path")
            d = torch.zeros((nh, nw, 4), dtype=torch.float32, device=dev)
            keep.append((r, d))
            ms = C.c_double()

            def once(n, L=L, p=p, d=d, ms=ms):
                abi.check(L.avirhip_time_resize(p, s.data_ptr(), d.data_ptr(),
                                                n, st, C.byref(ms)), "time")
                return ms.value
            run[tag] = (once, L, p, d)
        for tag in run:
            run[tag][0](5)
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
        report("%s (%dx%d -> %dx%d), path %d, %d calls a loop" % (
            name, sw, sh, nw, nh, this.avirhip_plan_get_path(run["this"][2]),
            iters), res, "; outputs bit-identical: %s" % same)
        del run, keep
        torch.cuda.empty_cache()

    # plan creation, cfg3: a new resizer object each time (its cache is empty)
    res = {tag: [] for tag, _ in libs}
    for i in range(reps + 1):
        for tag, L in libs:
            t0 = time.perf_counter()
            for _ in range(20):
                with abi.using(L):
                    r = avir_amd.CImageResizer(16)
                    r.plan(3840, 2160, 7680, 4320, 4)
                del r
            ms = (time.perf_counter() - t0) * 1000 / 20
            if i > 0:  # (the first round warms up)
                res[tag].append(ms)
                print("cfg3 plan rep %d %s %.5f ms" % (i - 1, tag, ms),
                      flush=True)
    report("cfg3 plan creation (with the resizer object), 20 a loop", res, "")

    print("plan footprint, bytes after creation / after the first call")
    ok = True
    for c in PC.CASES:
        name, ch, fp, tin, tout = c
        _, (sw, sh, nw, nh), mode, bits, _, _ = PC.row(name)
        src = np.zeros((sh, sw, ch), tin)
        got = {}
        for tag, L in (libs[0], libs[2]):
            with abi.using(L):
                v = avir_amd.CImageResizerVars()
                v.BuildMode = mode
                r = avir_amd.CImageResizer(bits, aFpPack=fp)
                p = r.plan(sw, sh, nw, nh, ch, 0.0, v,
                           avir_amd._NP2T[np.dtype(tin)],
                           avir_amd._NP2T[np.dtype(tout)])
                abi.check(L.avirhip_plan_set_path(p, 1), "set_path")
                b0 = L.avirhip_plan_device_bytes(p)
                r.resize(src, nw, nh, 0.0, tout, v)
                got[tag] = (b0, L.avirhip_plan_device_bytes(p))
        ok = ok and got["parent"] == got["this"]
        print("%-40s parent %d / %d  this %d / %d" % (
            (PC.case_id(c),) + got["parent"] + got["this"]))
    print("footprints equal: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
