"""The inputs of tests/test_gpu_gp16.py and tests/test_gp16_table.py: general-
ratio resizing (path 5: k_gh / k_gh2 / k_gv, k_gf, k_sacc*) of half / bfloat16
images whose first pass reads (k_gh's typed loader, gp_load_raw kinds 4 / 5)
and whose last pass stores (gp_store_int_row) the caller's 16-bit pixels.

Expected bits, as tests/dnf16_cases.py defines them: the reference on the
exactly widened float32 source, its float32 result narrowed with numpy's
.astype(float16) or with the header's integer formula for bfloat16; compared
word for word, NaN equal to NaN. Shapes are the smallest that take each route
(tests/gpass_route_cases.py)."""
import numpy as np
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H
from tests.dnf16_cases import (T, NAN, case, same, bands, widen, narrow,
                               words, as_f32, from_f32, special_f16_source,
                               special_f32_source, special_classes)

P5 = abi.PATH_GPASS
V_UPG2, V_UPGF = abi.VARIANT_UPG_TWO_PASS, abi.VARIANT_UPG_FUSED

# name -> ((sw, sh, nw, nh), variant, what runs)
ROUTES = {
    # upsizing on both axes, the two pass kernels: both sides fused
    "up_two_pass": ((64, 48, 100, 77), V_UPG2, "k_gh, k_gv"),
    # ... in one launch: k_gf reads float RGBA only, the store side is fused
    "up_fused": ((64, 48, 100, 77), V_UPGF, "k_gf"),
    # 1 < k < 2 under 22 taps: the typed k_gh< POST, -1 >
    "between": ((520, 300, 346, 206), 0, "k_gh, k_gv"),
    # ... from 22 taps: k_gh2 behind the pack pass
    "between_gh2": ((927, 421, 482, 226), 0, "k_gh2, k_gv"),
    # k >= 2 on both axes: the accumulation kernels, the store side is fused
    "acc": ((300, 200, 100, 67), 0, "k_sacc"),
    # upsizing by 2.2 horizontally, k = 2.5 vertically
    "mixed": ((90, 300, 200, 120), 0, "k_gh, k_sacc"),
    # 129 = 2 * 64 + 1: k_gh's and k_gv's last strip is one column
    "last_strip": ((64, 48, 129, 77), V_UPG2, "k_gh, k_gv"),
    # a 49-pixel-wide source: one piece of 64 lanes, 15 of them clamped
    "narrow": ((49, 48, 77, 77), V_UPG2, "k_gh, k_gv"),
    # the planner gives 1- and 2-channel pixels of the small upsizing shapes
    # another chain (the tiles' material): this one is the pass kernels' at
    # every channel count
    "up_any_ch": ((100, 80, 157, 125), V_UPG2, "k_gh, k_gv"),
}
# channel counts of the same-type pairs per route (every other pair: 4), those
# at which the plan is the pass kernels' (tests/test_gp16_table.py)
CHANNELS = {"up_two_pass": [4, 3], "up_fused": [4, 3], "between": [4, 1, 2, 3],
            "between_gh2": [4, 1, 2, 3], "acc": [4, 1, 2, 3],
            "mixed": [4, 1, 2, 3], "last_strip": [4, 3], "narrow": [4],
            "up_any_ch": [4, 1, 2, 3]}
# the step kinds of an axis the pass kernels match (gpass.hip,
# match_avir_axis, after lowering): upsizing -- filter, 2x zero-stuffing,
# resize; 1 < k < 2 -- zero-stuffing, resize, filter; k >= 2 -- resize, filter
AX_UP, AX_BETWEEN, AX_DOWN = [0, 1, 4], [1, 4, 0], [3, 0]
AXES = {"up_two_pass": (AX_UP, AX_UP), "up_fused": (AX_UP, AX_UP),
        "between": (AX_BETWEEN, AX_BETWEEN),
        "between_gh2": (AX_BETWEEN, AX_BETWEEN), "acc": (AX_DOWN, AX_DOWN),
        "mixed": (AX_UP, AX_DOWN), "last_strip": (AX_UP, AX_UP),
        "narrow": (AX_UP, AX_UP), "up_any_ch": (AX_UP, AX_UP)}
# the routes whose same-type calls read AND store 16-bit pixels themselves
# (no float copy of either image on the plan)
BOTH_FUSED = ["up_two_pass", "between", "last_strip", "narrow", "up_any_ch"]
# ... whose last pass stores them behind the pack pass's float source copy
STORE_ONLY = ["acc", "up_fused"]

# (tin, tout): every source type into both 16-bit results, both 16-bit sources
# into every result the stage already stores
PAIRS = [("f16", "f16"), ("bf16", "bf16"), ("f16", "bf16"), ("bf16", "f16"),
         ("f32", "f16"), ("f32", "bf16"), ("u8", "f16"), ("f16", "f32"),
         ("bf16", "f32"), ("f16", "u8"), ("bf16", "u16")]
SAME = [("f16", "f16"), ("bf16", "bf16")]

# Images of fewer than four elements up to the end of the last source row a
# band reads: the typed loader's 8-byte load does not fit, the pack road runs.
# (sw, sh, nw, nh, ch). The planner gives sources this small another chain than
# the pass kernels' (tests/test_gp16_table.py), so forced path 5 refuses their
# plans and the automatic path alone runs them ...
TINY = [(3, 1, 5, 2, 1), (1, 3, 2, 5, 1), (1, 1, 3, 3, 3), (2, 1, 3, 1, 1),
        (3, 40, 5, 61, 1)]
# ... and the narrowest sources whose plans ARE the pass kernels': rows of
# three elements, so the loader's last-pixel shift runs in every band
THIN = [(3, 200, 120, 333, 1), (1, 200, 40, 333, 3)]

# forced chunk lengths of k_gh's row-ahead load (a chunk of one row never
# issues the second load)
GH_CHUNKS = [1, 2, 3, 5]

# the special-value frames: upsizing on the two pass kernels, downsizing
SPECIAL_UP = ((192, 144), (250, 187), V_UPG2)
SPECIAL_DN = ((384, 288), (250, 187), 0)


def geom(name):
    return ROUTES[name][0]


def variant(name):
    return ROUTES[name][1]


def padded(src, pitch, t):
    """(sh, sw, ch) -> rows `pitch` elements apart with NaN between them, the
    last one ending with its pixels (flat)."""
    sh, sw, ch = src.shape
    pad = np.array([NAN], np.uint16)[0] if t == "bf16" else np.float16(np.nan)
    flat = np.full(sh * pitch, pad, T[t][1])
    flat.reshape(sh, pitch)[:, :sw * ch] = src.reshape(sh, sw * ch)
    return np.ascontiguousarray(flat[:(sh - 1) * pitch + sw * ch])


# ---- special values -----------------------------------------------------------

def _denormal_block(src):
    """Half denormals (1 .. 1023 units of 2^-24) in a block of their own."""
    n = np.arange(40 * 60 * 4, dtype=np.uint32).reshape(40, 60, 4)
    bits = (1 + (n * 37) % 1023).astype(np.uint16)
    bits |= ((n & 1) << 15).astype(np.uint16)
    src[44:84, 100:160] = bits.view(np.float16)


def special_source(t, size, flushed=False):
    """The special-value frame of tests/dnf16_cases.py, sized `size`; the half
    frame also holds a block of half DENORMALS (`flushed`: that block zeroed,
    what a loader that flushes them would have read)."""
    if t != "f16":
        return special_f32_source(size)
    src = special_f16_source(size)
    _denormal_block(src)
    if flushed:
        blk = src[44:84, 100:160]
        blk[np.abs(blk.astype(np.float32)) < 2.0 ** -14] = 0
    return src


_SPECIAL = {}


def special_case(t, which, flushed=False):
    """-> (source, float32 reference, expected result in `t` elements) of
    SPECIAL_UP / SPECIAL_DN: t == "f16": the half frame; otherwise the float32
    frame (for a bfloat16 result; tests narrow it for a bfloat16 source)."""
    size, out, v = which
    key = (t, size, out, flushed)
    if key not in _SPECIAL:
        src = special_source(t, size, flushed)
        ref = H.checker_avir(src.astype(np.float32), out[0], out[1],
                             out_dtype=np.float32, resbits=16)
        src.setflags(write=False)
        ref.setflags(write=False)
        _SPECIAL[key] = (src, ref)
    src, ref = _SPECIAL[key]
    return src, ref, from_f32(ref, t)


def special_bf16_case(which):
    """The float32 frame narrowed to bfloat16 -> (source bits, float32
    reference of the widened source, expected bfloat16 bits)."""
    size, out, v = which
    key = ("bf16src", size, out)
    if key not in _SPECIAL:
        src = narrow(special_f32_source(size))
        ref = H.checker_avir(widen(src), out[0], out[1], out_dtype=np.float32,
                             resbits=16)
        src.setflags(write=False)
        ref.setflags(write=False)
        _SPECIAL[key] = (src, ref)
    src, ref = _SPECIAL[key]
    return src, ref, narrow(ref)
