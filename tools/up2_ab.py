#!/usr/bin/env python3
"""Same-box, same-process A/B of two builds of the library on the 2x kernel's
workloads (cfg3: 3840x2160 -> 7680x4320 RGBA float, cfg2: 1920x1080 ->
3840x2160): both libraries are loaded side by side (abi.load_path), each with
its own plan, and the timed loops alternate between them REPS times -- no
box-to-box or process-to-process spread between the columns. The two results
are also compared bit for bit.

usage: python tools/up2_ab.py [OLD.so] [NEW.so] [REPS=5]
       (defaults: avir_amd/lib/libavirhip_old.so, avir_amd/lib/libavirhip.so)
"""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    import torch
    import avir_amd
    from avir_amd import abi, synth
    old = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, "avir_amd", "lib", "libavirhip_old.so")
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        ROOT, "avir_amd", "lib", "libavirhip.so")
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    libs = {"old": abi.load_path(old), "new": abi.load_path(new)}
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    for name, (sw, sh) in (("cfg3", (3840, 2160)), ("cfg2", (1920, 1080))):
        src = torch.from_numpy(synth.lcg_f32((sh, sw, 4))).to(dev)
        dst = {k: torch.empty((2 * sh, 2 * sw, 4), dtype=torch.float32,
                              device=dev) for k in libs}
        keep, steps = [], {}
        for k, L in libs.items():
            with abi.using(L):
                r = avir_amd.CImageResizer(16)
                p = r.plan(sw, sh, 2 * sw, 2 * sh, 4, 0.0, None, abi.F32,
                           abi.F32)
            keep.append(r)

            def step(L=L, p=p, d=dst[k]):
                abi.check(L.avirhip_resize(p, src.data_ptr(), abi.MEM_DEVICE,
                                           d.data_ptr(), abi.MEM_DEVICE, st),
                          "avirhip_resize")
            steps[k] = step
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:  # settle the clocks
            for k in libs:
                for _ in range(25):
                    steps[k]()
            torch.cuda.synchronize()
        same = torch.equal(dst["old"].view(torch.uint8),
                           dst["new"].view(torch.uint8))
        res = {k: [] for k in libs}
        n = 400 if name == "cfg3" else 1000
        for _ in range(reps):
            for k in libs:
                for _ in range(40):
                    steps[k]()
                torch.cuda.synchronize()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    steps[k]()
                e1.record()
                torch.cuda.synchronize()
                res[k].append(e0.elapsed_time(e1) / n)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        for k in libs:
            print("%s %s median %.4f ms (%+.2f %% vs old)  runs %s" % (
                name, k, med[k], (med[k] / med["old"] - 1) * 100,
                " ".join("%.4f" % x for x in res[k])), flush=True)
        print("%s outputs bit-identical: %s  (fnv1a64 new %s)" % (
            name, same, synth.fnv(dst["new"].cpu().numpy())), flush=True)


if __name__ == "__main__":
    main()
