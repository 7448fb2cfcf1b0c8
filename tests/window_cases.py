"""The case table of tests/test_gpu_window.py (avirhip_resize_window on every
kernel family), and what both that suite and the host-only share check of
tests/test_window_table.py need to read it: the front-end objects, the band
list and the host planner's band_source_rows of a case.

A case is (front end, sw, sh, nw, nh, ch, tin, tout, resbits, path, variant,
extras). `path` / `variant` are avirhip_plan_set_path / set_variant values
(include/avirhip.h; the vocabulary of tools/fuzz_values.py's `runs`). extras:
  build_mode       CImageResizerVars::BuildMode
  fp               aFpPack of CImageResizer (abi.FPCLASS_DOUBLE: double pipeline)
  gamma, alpha     UseSRGBGamma, AlphaIndex
  pad              elements added to the source row pitch (SrcScanlineSize /
                   CLancIRParams::SrcSSize = sw * ch + pad)
  k, ox, oy        explicit step / offsets (CLancIR: k is kx = ky)
  native           the plan reads a device window where it lies (k_up2 /
                   k_lanc2, float RGBA): the plan may not grow by a frame
  auto_path        path 0 only: the path the automatic choice is known to be
  host_dst         the bands are also computed into host destinations
  small            exempt from the window shares (one short k_up2 frame: a
                   geometry below the smallest chunk height of 62 source rows)
"""
import numpy as np
import avir_amd
from avir_amd import abi

U8, U16, F32, F64 = np.uint8, np.uint16, np.float32, np.float64
DBL = dict(fp=abi.FPCLASS_DOUBLE)
V_PLAIN = abi.VARIANT_UP2_PLAIN_V
V_DN2 = abi.VARIANT_DN_TWO_PASS
V_LADDER = abi.VARIANT_SACC_LADDER
V_UPG2 = abi.VARIANT_UPG_TWO_PASS
V_UPGF = abi.VARIANT_UPG_FUSED
V_OPT = abi.VARIANT_SACC_OPTIMISTIC

CASES = [
    # ---- generic per-op kernels
    ("avir", 300, 400, 420, 560, 4, F32, F32, 16, 1, 0, dict(host_dst=1)),
    ("avir", 360, 500, 200, 278, 3, U8, U8, 8, 1, 0, {}),
    # ---- LDS tiles: two-pass, fused
    ("avir", 500, 700, 320, 448, 4, F32, F32, 16, 2, 0, {}),
    ("avir", 350, 500, 167, 239, 4, F32, F32, 16, 3, 0, {}),
    # ---- k_up2, transposed vertical phase: the native (zero-copy) window
    ("avir", 200, 48, 400, 96, 4, F32, F32, 16, 4, 0,
     dict(native=1, small=1)),
    ("avir", 320, 416, 640, 832, 4, F32, F32, 16, 4, 0,
     dict(native=1, host_dst=1)),
    ("avir", 320, 416, 640, 832, 4, F32, F32, 16, 0, 0,
     dict(native=1, auto_path=4)),
    # ---- k_up2, plain vertical form
    ("avir", 256, 400, 512, 800, 4, F32, F32, 16, 4, V_PLAIN,
     dict(native=1, build_mode=1)),
    # ---- k_up2 with integer output / raw integer source: staged window
    ("avir", 321, 420, 642, 840, 3, U8, U8, 8, 4, 0, {}),
    ("avir", 322, 420, 644, 840, 4, U8, U8, 8, 4, 0, {}),
    ("avir", 322, 420, 644, 840, 4, U16, U16, 16, 4, 0, {}),
    # ---- k_lanc2: native, and with uint8 I/O (inner plan, raw loader)
    ("lancir", 320, 416, 640, 832, 4, F32, F32, 0, 4, 0, dict(native=1)),
    ("lancir", 320, 416, 640, 832, 4, U8, U8, 0, 4, 0, {}),
    ("lancir", 321, 416, 642, 832, 3, U8, U8, 0, 4, 0, {}),
    # ---- k_dnf; k_dnh + k_dnv
    ("avir", 600, 800, 300, 400, 4, F32, F32, 16, 0, 0, {}),
    ("avir", 600, 900, 200, 300, 4, F32, F32, 16, 0, 0, {}),
    ("avir", 600, 800, 300, 400, 4, F32, F32, 16, 2, V_DN2, {}),
    ("avir", 600, 800, 300, 400, 3, U8, U8, 8, 0, 0, {}),
    # ---- k_sacc2, the k_sacc ladder, the optimistic float form
    ("avir", 600, 805, 222, 298, 3, U8, U8, 8, 5, 0, dict(host_dst=1)),
    ("avir", 600, 805, 222, 298, 3, U8, U8, 8, 5, V_LADDER, {}),
    ("avir", 600, 805, 222, 298, 3, F32, F32, 16, 5, 0, {}),
    ("avir", 600, 805, 222, 298, 4, F32, F32, 16, 5, V_OPT, {}),
    ("avir", 600, 805, 222, 298, 4, F32, F32, 16, 5, 0, {}),
    # ---- k_gh2 / the gather kernels on 1 < k < 2
    ("avir", 600, 600, 400, 400, 4, F32, F32, 16, 5, 0, {}),
    # ---- k_gh + k_gv, k_gf: upsizing, general ratio
    ("avir", 300, 400, 460, 613, 4, F32, F32, 16, 5, V_UPG2, {}),
    ("avir", 300, 400, 460, 613, 4, F32, F32, 16, 5, V_UPGF, {}),
    ("avir", 300, 400, 460, 613, 3, U8, U8, 8, 5, V_UPG2, {}),
    ("avir", 300, 400, 460, 613, 3, U8, U8, 8, 5, V_UPGF, {}),
    # ---- CLancIR: k_lf, k_gv + k_gh, downsizing, the staged form of 2x
    ("lancir", 300, 400, 460, 613, 4, F32, F32, 0, 0, 0, dict(auto_path=5)),
    ("lancir", 300, 400, 460, 613, 3, U8, U8, 0, 5, 0, {}),
    ("lancir", 300, 400, 460, 613, 4, F32, F32, 0, 5, V_UPG2, {}),
    ("lancir", 600, 805, 222, 298, 3, U8, U8, 0, 0, 0, {}),
    ("lancir", 320, 416, 640, 832, 4, F32, F32, 0, 0, 0, dict(oy=0.4)),
    # ---- the double pipeline: tiles, per-op kernels, up64.hip
    ("avir", 400, 600, 250, 375, 4, F64, F64, 16, 0, 0,
     dict(DBL, auto_path=2)),
    ("avir", 400, 600, 250, 375, 3, F32, F32, 16, 1, 0, dict(DBL)),
    ("avir", 200, 400, 333, 666, 4, F64, F64, 16, 0, 0, dict(DBL)),
    ("avir", 200, 400, 400, 800, 3, F32, F64, 16, 0, 0, dict(DBL)),
    # ---- 1 and 2 channels on the RGBA fast paths (inner plans)
    ("avir", 300, 400, 460, 613, 1, F32, F32, 16, 0, 0, {}),
    ("avir", 600, 805, 222, 298, 2, F32, F32, 16, 0, 0, {}),
    ("lancir", 300, 400, 460, 613, 2, F32, F32, 0, 0, 0, {}),
    ("lancir", 600, 805, 222, 298, 1, F32, F32, 0, 0, 0, {}),
    # ---- sRGB gamma
    ("avir", 300, 400, 460, 613, 4, F32, F32, 16, 0, 0,
     dict(gamma=1, alpha=3)),
    ("avir", 600, 805, 222, 298, 3, U8, U8, 8, 0, 0,
     dict(gamma=1, alpha=-1)),
    # ---- padded source rows
    ("avir", 300, 400, 460, 613, 3, F32, F32, 16, 0, 0, dict(pad=3)),
    ("avir", 600, 805, 222, 298, 4, U8, U8, 8, 0, 0, dict(pad=3)),
    ("lancir", 300, 400, 460, 613, 3, U8, U8, 0, 0, 0, dict(pad=3)),
    ("lancir", 320, 416, 640, 832, 4, F32, F32, 0, 4, 0, dict(pad=2)),
    # ---- explicit offsets and steps: bands that read replicated edge rows
    ("avir", 300, 400, 460, 613, 4, F32, F32, 16, 0, 0, dict(oy=0.4)),
    ("avir", 600, 805, 222, 298, 4, F32, F32, 16, 0, 0, dict(oy=-0.7)),
    ("avir", 300, 500, 400, 300, 4, F32, F32, 16, 0, 0, dict(k=1.6)),
    ("lancir", 300, 400, 460, 613, 4, F32, F32, 0, 0, 0, dict(oy=-0.7)),
    ("lancir", 300, 500, 400, 300, 3, U8, U8, 0, 0, 0, dict(k=1.6, oy=0.4)),
]


def case_id(c):
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = c
    tag = "".join("-%s%s" % (k, "" if v == 1 else v)
                  for k, v in sorted(ex.items())
                  if k not in ("native", "host_dst", "small", "auto_path"))
    return "%s-%dx%d-%dx%d-c%d-%s-%s-p%dv%d%s" % (
        fe, sw, sh, nw, nh, ch, np.dtype(tin).name, np.dtype(tout).name, path,
        variant, tag)


IDS = [case_id(c) for c in CASES]


def pitch(c):
    """Elements per source row."""
    return c[1] * c[5] + c[11].get("pad", 0)


def front_end(c):
    """-> (front-end object, its vars / params argument)"""
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = c
    if fe == "lancir":
        k = float(ex.get("k", 0.0))
        P = avir_amd.CLancIRParams(pitch(c) if ex.get("pad") else 0, 0, k, k,
                                   float(ex.get("ox", 0.0)),
                                   float(ex.get("oy", 0.0)))
        return avir_amd.CLancIR(), P
    v = avir_amd.CImageResizerVars()
    v.BuildMode = ex.get("build_mode", -1)
    v.ox, v.oy = float(ex.get("ox", 0.0)), float(ex.get("oy", 0.0))
    v.UseSRGBGamma, v.AlphaIndex = ex.get("gamma", 0), ex.get("alpha", -1)
    return avir_amd.CImageResizer(bits, aFpPack=ex.get("fp", 1)), v


def host_source_rows(c, obj, arg, r0, r1):
    """The host planner's answer (no device plan): source rows of [r0, r1)."""
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = c
    ti, to = avir_amd._NP2T[np.dtype(tin)], avir_amd._NP2T[np.dtype(tout)]
    if fe == "lancir":
        return obj.band_source_rows(sw, sh, nw, nh, ch, r0, r1, arg, ti, to)
    return obj.band_source_rows(sw, sh, nw, nh, ch, r0, r1,
                                float(ex.get("k", 0.0)), arg, ti, to,
                                pitch(c) if ex.get("pad") else 0)


def bands(nh):
    """(name, row0, row1): the first and the last fifth, an inner fifth, one
    inner row, the whole frame."""
    f = nh // 5
    return [("first", 0, f), ("inner", 2 * f, 3 * f), ("last", nh - f, nh),
            ("row", nh // 2 + 1, nh // 2 + 2), ("frame", 0, nh)]
