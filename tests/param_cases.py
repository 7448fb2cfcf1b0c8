"""The case table of tests/test_gpu_params.py (every kernel family under
non-default CImageResizerParams) and of the host-only tests/test_params_table.py:
the parameter sets, the geometry classes with the paths / variants each frame
is forced onto, how a plan's chain shape is read from a PlanDesc, and the
EXPECTATION -- which forced path takes which chain shape, and why not.

The expectation is derived from the chain shape alone (expect() below restates
the host predicates of the kernels: up2.hip match_axis, gpass.hip
match_avir_axis + the vertical ring budget, fused.hip chain_ok); it is never a
record of what the library did. tests/test_gpu_params.py fails on a refusal the
table does not name and on an acceptance it names as refused.

A parameter set is the 8-tuple of tests.helpers.PRESETS (CorrFltAlpha,
CorrFltLen, IntFltAlpha, IntFltCutoff, IntFltLen, LPFltAlpha, LPFltBaseLen,
LPFltCutoffMult), or None: CImageResizerParamsDef through the default
constructor. The custom sets are one change from the default each; all of them
were resized with by the real reference on the CPU (no assertion trips) and
their plans agree with the reference planner's (tests/test_params_table.py
repeats both checks), so none needed a replacement value.
"""
import math
import numpy as np
from avir_amd import abi
from tests.helpers import PRESETS

U8, U16, F32, F64 = np.uint8, np.uint16, np.float32, np.float64

NAMES = ("CorrFltAlpha", "CorrFltLen", "IntFltAlpha", "IntFltCutoff",
         "IntFltLen", "LPFltAlpha", "LPFltBaseLen", "LPFltCutoffMult")
# CImageResizerParamsDef (avir.h:2262-2341; tests/test_params_table.py checks
# these against avirhip_params_preset(0))
DEF = (0.97946, 6.4262, 6.41341, 0.7372, 18.0, 4.76449, 7.55999999999998,
       0.79285)


def _mod(**kw):
    d = dict(zip(NAMES, DEF))
    d.update(kw)
    return tuple(d[n] for n in NAMES)


SETS = dict(PRESETS)
SETS.update({
    # the correction filter: 9 taps / latency 4, 3 taps / latency 1
    "corr8.2": _mod(CorrFltLen=8.2),
    "corr4.0": _mod(CorrFltLen=4.0),
    # the interpolation bank: 10 and 14 taps over the zero-stuffed view
    "int14": _mod(IntFltLen=14.0),
    "int22": _mod(IntFltLen=22.0),
    # the low-pass base length: every tap count of the downsizing side moves
    "lp5.2": _mod(LPFltBaseLen=5.2),
    "lp10.4": _mod(LPFltBaseLen=10.4),
    # another IntFltAlpha / IntFltCutoff pair. The fo[t] == fe[11-t] bit
    # symmetry of the exact-2x bank phases HOLDS for it -- as for every pair of
    # a scan of IntFltAlpha 1 .. 9 x IntFltCutoff 0.6 .. 0.8 and for every
    # preset, at 8 and at 16 bits: the bank is designed symmetric and the two
    # phases of an exact 2x are mirror images. No parameter breaks it, so the
    # plain form of k_up2 is reached by the variant flag alone
    # (test_params_table.py asserts the symmetry for every 12-tap set).
    "int_a2_c0.7": _mod(IntFltAlpha=2.0, IntFltCutoff=0.7),
})
SET_NAMES = sorted(SETS)

# calcFilterLength (avir.h:1316): 2 * ceil(CorrFltLen / 2) - 1 taps
SEVEN_TAP = ("def", "low", "high", "ultra", "int14", "int22", "lp5.2",
             "lp10.4", "int_a2_c0.7")
OTHER_TAP = ("ulr", "lr", "corr8.2", "corr4.0")


def set_params(name):
    """The 8 values of a set (the default's too)."""
    return SETS[name] if SETS[name] is not None else DEF


def corr_len_lat(name):
    """(taps, latency) of the correction filter by calcFilterLength."""
    n = 2 * int(math.ceil(set_params(name)[1] / 2.0)) - 1
    return n, n // 2


def product_params(name):
    """abi.Params of a set for CImageResizer(aParams=); None = default."""
    import ctypes as C
    if SETS[name] is None:
        return None
    P = abi.Params()
    abi.load().avirhip_params_preset(0, C.byref(P))
    for n, v in zip(NAMES, SETS[name]):
        setattr(P, n, v)
    return P


# ---- geometry classes --------------------------------------------------
# class -> [(frame, runs)]; frame = (sw, sh, nw, nh, ch, tin, tout, resbits,
# fpclass); runs = [(path, variant, environment)]
V_PLAIN = abi.VARIANT_UP2_PLAIN_V
V_DN2 = abi.VARIANT_DN_TWO_PASS
V_LADDER = abi.VARIANT_SACC_LADDER
V_UPG2 = abi.VARIANT_UPG_TWO_PASS
V_UPGF = abi.VARIANT_UPG_FUSED
V_OPT = abi.VARIANT_SACC_OPTIMISTIC
DBL = abi.FPCLASS_DOUBLE

_X2 = [(0, 0, {}), (1, 0, {}), (2, 0, {}), (4, 0, {}), (4, V_PLAIN, {})]
_UPG = [(0, 0, {}), (1, 0, {}), (2, 0, {}), (3, 0, {}), (5, V_UPG2, {}),
        (5, V_UPGF, {})]
_DN12 = [(0, 0, {}), (1, 0, {}), (5, 0, {"AVIRHIP_GH2_MIN_NT": "13"}),
         (5, 0, {"AVIRHIP_NO_GH2": "1"}), (5, 0, {})]
_WHOLE = [(0, 0, {}), (1, 0, {}), (2, V_DN2, {})]
_DBL = [(0, 0, {}), (0, 0, {"AVIRHIP_NO_UP64": "1"}), (1, 0, {})]

CLASSES = {
    # exact 2x (k_up2's smallest chunk is 62 source rows: 70 and 190 rows cut
    # one and several chunks)
    "x2": [
        ((96, 70, 192, 140, 4, F32, F32, 16, 1), _X2),
        ((322, 190, 644, 380, 4, F32, F32, 16, 1), _X2),
        ((321, 190, 642, 380, 3, U8, U8, 8, 1), _X2),
        ((322, 190, 644, 380, 4, U16, U16, 16, 1), _X2),
        ((96, 70, 192, 140, 1, F32, F32, 16, 1), _X2),
    ],
    "upg": [
        ((300, 200, 460, 307, 4, F32, F32, 16, 1), _UPG),
        ((300, 200, 460, 307, 3, U8, U8, 8, 1), _UPG),
    ],
    "dn12": [
        ((600, 400, 400, 267, 4, F32, F32, 16, 1), _DN12),
        ((600, 400, 461, 308, 4, F32, F32, 16, 1), _DN12),
    ],
    "whole": [
        ((600, 400, 300, 200, 4, F32, F32, 16, 1), _WHOLE),
        ((600, 402, 200, 134, 4, F32, F32, 16, 1), _WHOLE),
        ((600, 400, 300, 200, 3, U8, U8, 8, 1), _WHOLE),
        ((600, 402, 200, 134, 3, U8, U8, 8, 1), _WHOLE),
    ],
    "dn2p": [
        ((600, 405, 222, 150, 3, U8, U8, 8, 1),
         [(0, 0, {}), (1, 0, {}), (5, 0, {}), (5, V_LADDER, {})]),
        ((600, 405, 222, 150, 4, F32, F32, 16, 1),
         [(0, 0, {}), (1, 0, {}), (5, 0, {}), (5, V_OPT, {})]),
        ((600, 405, 222, 150, 3, F32, F32, 16, 1),
         [(0, 0, {}), (1, 0, {}), (5, 0, {})]),
    ],
    "mixed": [
        ((300, 400, 460, 150, 4, F32, F32, 16, 1),
         [(0, 0, {}), (1, 0, {}), (2, 0, {}), (5, 0, {})]),
    ],
    # the double pipeline; the reference is its variant 4
    "dbl": [
        ((97, 66, 194, 132, 4, F64, F64, 16, DBL), _DBL),
        ((200, 120, 333, 250, 4, F64, F64, 16, DBL), _DBL),
        ((400, 300, 250, 188, 4, F64, F64, 16, DBL), _DBL),
        ((97, 66, 194, 132, 3, F32, F32, 16, DBL), _DBL),
        ((200, 120, 333, 250, 3, F32, F32, 16, DBL), _DBL),
        ((400, 300, 250, 188, 3, F32, F32, 16, DBL), _DBL),
    ],
}
CLASS_NAMES = sorted(CLASSES)

# the automatic path at real sizes (plans only): (sw, sh, nw, nh, ch, type,
# resbits)
BIG = [
    (1920, 1080, 3840, 2160, 4, F32, 16),
    (3840, 2160, 1280, 720, 4, F32, 16),
    (1920, 1080, 2500, 1400, 3, U8, 8),
    (5184, 3456, 1920, 1280, 3, U8, 8),
]
# ... of the default set, from the comments of the automatic choice (api.cpp
# finalize_plan, gpass.hip gpass_preferred): exact 2x with float RGBA output
# keeps k_up2; a whole ratio on both axes keeps dn.hip inside the two-pass
# path; upsizing RGB uint8 takes the pass kernels from 2 Mpixel outputs on;
# integer sources downsized by k >= 2 on both axes take sacc.hip
BIG_DEFAULT_PATHS = (abi.PATH_UP2, abi.PATH_TILED, abi.PATH_GPASS,
                     abi.PATH_GPASS)


def geometries(cls):
    """The distinct (sw, sh, nw, nh) of a class, in table order."""
    out = []
    for frame, _ in CLASSES[cls]:
        if frame[:4] not in out:
            out.append(frame[:4])
    return out


# ---- the chain shape of a plan -----------------------------------------
def axis_shape(ax):
    """((kind name, resample_factor, flt_len, flt_latency, bank_filter_len),
    ...) of a PlanDesc axis."""
    return tuple((abi.STEP_NAMES[ax.steps[i].kind],
                  ax.steps[i].resample_factor, ax.steps[i].flt_len,
                  ax.steps[i].flt_latency, ax.steps[i].bank_filter_len)
                 for i in range(ax.n_steps))


def desc_shape(desc):
    """(horizontal axis shape, vertical axis shape) of a PlanDesc."""
    return axis_shape(desc.h), axis_shape(desc.v)


def _kinds(shape):
    return tuple(s[0] for s in shape)


def gather_taps(shape):
    """Taps per output of the axis' gather (api.cpp lower_axis): the bank's
    length, or every second tap of it over the zero-stuffed view."""
    for kind, rf, fl, lat, bank in shape:
        if kind == "RESIZE":
            return bank
        if kind == "RESIZE2":
            return (bank + 1) // 2
    return 0


def _fir(shape):
    for s in shape:
        if s[0] == "FIR":
            return s
    return None


UP = ("FIR", "UP_ZEROSTUFF", "RESIZE2")    # upsizing: FIR, bank over the view
DN12 = ("UP_ZEROSTUFF", "RESIZE2", "FIR")  # 1 < k < 2: gather, then FIR
DN = ("RESIZE", "FIR")                     # k >= 2: gather, then FIR


def _axis_up2(shape):
    f = _fir(shape)
    if _kinds(shape) != UP:
        return "not FIR -> zero-stuffed bank"
    if (f[1], f[2], f[3]) != (1, 7, 3):
        return "correction FIR of %d taps, latency %d (k_up2: 7 / 3)" % (
            f[2], f[3])
    if gather_taps(shape) != 12:
        return "%d-tap gather (k_up2: 12)" % gather_taps(shape)
    return None


def _axis_gpass(shape):
    kinds = _kinds(shape)
    if kinds not in (UP, DN12, DN, ("RESIZE",), ("UP_ZEROSTUFF", "RESIZE2")):
        return "chain %s" % (kinds,)
    f = _fir(shape)
    if f is not None and (f[1] != 1 or f[3] != 3):
        return "correction FIR of %d taps, latency %d (pass kernels: 7 / 3)" \
            % (f[2], f[3])
    nt = gather_taps(shape)
    if nt < 2 or nt > 64:
        return "%d-tap gather (pass kernels: 2 .. 64)" % nt
    # the vertical pass: register windows for 12 taps (FIR first) and 13 .. 25
    # (gather first); otherwise an LDS ring of next_pow2(nt + 1) rows (FIR
    # first) or next_pow2(nt + 13) + 8 rows (gather first) of 512 bytes next
    # to 13 KiB of queues in 64 KiB: up to 63 and 51 taps. (Gather-first axes
    # of k >= 2 run on sacc.hip where at most 15 outputs are alive at a
    # sample, which needs no ring; the bound below does not rely on it.)
    if kinds == UP and nt > 63:
        return "%d-tap ring exceeds the LDS budget" % nt
    if kinds != UP and not (13 <= nt <= 25) and nt > 51:
        return "%d-tap ring exceeds the LDS budget" % nt
    return None


def expect(shape_hv, frame, path):
    """-> None: the forced path runs this frame; or the reason it refuses.
    shape_hv = desc_shape() of the frame's plan."""
    sw, sh, nw, nh, ch, tin, tout, bits, fp = frame
    both = list(shape_hv)
    if path in (abi.PATH_AUTO, abi.PATH_GENERIC):
        return None
    upf = [s for s in both if "UP_FILTERED" in _kinds(s)]
    if path in (abi.PATH_TILED, abi.PATH_FUSED):
        # the tiles take any chain without a filtered upsample (chain_ok /
        # chain64_ok); their smallest tile (8 x 8 fused, 8 x 1 per pass)
        # keeps every chain of this table far below the LDS capacity
        if fp == DBL and path == abi.PATH_FUSED:
            return "the double pipeline has no fused tile"
        return "filtered upsample" if upf else None
    if fp == DBL:
        return "the double pipeline runs on tiles / up64.hip (path 2) only"
    if path == abi.PATH_UP2:
        if (nw, nh) != (2 * sw, 2 * sh):
            return "not an exact 2x"
        for s in both:
            why = _axis_up2(s)
            if why:
                return why
        return None
    if path == abi.PATH_GPASS:
        for s in both:
            why = _axis_gpass(s)
            if why:
                return why
        return None
    raise ValueError(path)


def expect_auto(shape_hv, frame):
    """The fast paths the automatic choice may land on: those that take the
    chain. Empty: the generic kernels."""
    return [p for p in (abi.PATH_TILED, abi.PATH_UP2, abi.PATH_GPASS)
            if expect(shape_hv, frame, p) is None]


def case_id(frame, path, variant, env):
    sw, sh, nw, nh, ch, tin, tout, bits, fp = frame
    return "%dx%d-%dx%d-c%d-%s-p%dv%d%s" % (
        sw, sh, nw, nh, ch, np.dtype(tin).name, path, variant,
        "".join("-%s=%s" % (k.replace("AVIRHIP_", ""), v)
                for k, v in sorted(env.items())))
