#!/usr/bin/env python3
"""Chunk-count sweep of the 2x marching kernel in ONE process: up2_run reads
AVIRHIP_UP2_NCHUNKS (the balanced split of that many chunks per strip) and
AVIRHIP_UP2_CQ (one uniform height) on every call, so one plan per workload is
timed under every setting, the settings alternating ROUNDS times -- no
box-to-box or process-to-process spread between the rows of the table.

Rows: `default` (the library's own choice), `cq C` (the uniform height the
rule before the split chose) and `n N`. Columns: median and every run in ms,
and the median against `default`.

usage: python tools/up2_chunk_sweep.py [ROUNDS=3] [workload[:N,N...] ...]
       workloads: cfg3 cfg2 up2_rgba8 (default: all three), each with the
       chunk counts to try (default: seven around the rule's choice)
"""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

# name -> (sw, sh, dtype, resbits, uniform cq of the former rule, chunk counts)
WORK = {"cfg3": (3840, 2160, "f32", 16, 134, range(14, 21)),
        "cfg2": (1920, 1080, "f32", 16, 70, range(13, 20)),
        "up2_rgba8": (1920, 1080, "u8", 8, 70, range(13, 20))}
KNOBS = ("AVIRHIP_UP2_NCHUNKS", "AVIRHIP_UP2_CQ")


def main():
    import torch
    import avir_amd
    from avir_amd import abi, synth
    args = sys.argv[1:]
    rounds = int(args.pop(0)) if args and args[0].isdigit() else 3
    lib = abi.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    for name in args or list(WORK):
        name, _, only = name.partition(":")
        sw, sh, dt, bits, cq0, ns = WORK[name]
        if only:
            ns = [int(x) for x in only.split(",")]
        u8 = dt == "u8"
        src = torch.from_numpy(synth.lcg_u8((sh, sw, 4)) if u8 else
                               synth.lcg_f32((sh, sw, 4))).to(dev)
        dst = torch.empty((2 * sh, 2 * sw, 4), dtype=src.dtype, device=dev)
        r = avir_amd.CImageResizer(bits)
        tc = abi.U8 if u8 else abi.F32
        p = r.plan(sw, sh, 2 * sw, 2 * sh, 4, 0.0, None, tc, tc)

        def step():
            abi.check(lib.avirhip_resize(p, src.data_ptr(), abi.MEM_DEVICE,
                                         dst.data_ptr(), abi.MEM_DEVICE, st),
                      "avirhip_resize")
        sets = [("default", {}), ("cq %d" % cq0, {"AVIRHIP_UP2_CQ": cq0})]
        sets += [("n %d" % n, {"AVIRHIP_UP2_NCHUNKS": n}) for n in ns]
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:  # settle the clocks
            for _ in range(50):
                step()
            torch.cuda.synchronize()
        ref = dst.clone()
        res = {k: [] for k, _ in sets}
        same = True
        steps = 300 if sh > 1080 else 800
        for _ in range(rounds):
            for k, env in sets:
                for v in KNOBS:
                    os.environ.pop(v, None)
                for a, b in env.items():
                    os.environ[a] = str(b)
                for _ in range(30):
                    step()
                torch.cuda.synchronize()
                same = same and torch.equal(dst, ref)
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    step()
                e1.record()
                torch.cuda.synchronize()
                res[k].append(e0.elapsed_time(e1) / steps)
        for v in KNOBS:
            os.environ.pop(v, None)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        print("%s (%dx%d -> %dx%d RGBA %s), path %d, %d steps per run, every "
              "setting bit-identical to default: %s" % (
                  name, sw, sh, 2 * sw, 2 * sh, dt,
                  lib.avirhip_plan_get_path(p), steps, same), flush=True)
        for k, _ in sets:
            print("  %-8s median %.4f ms (%+.2f %%)  runs %s" % (
                k, med[k], (med[k] / med["default"] - 1) * 100,
                " ".join("%.4f" % x for x in res[k])), flush=True)


if __name__ == "__main__":
    main()
