"""The inputs of tests/test_gpu_lancgp16.py and tests/test_lancgp16_table.py:
CLancIR at general ratios (path 5: k_lf, the LANC forms of k_gv / k_gh) with
half / bfloat16 images whose first pass reads (raw kinds 4 / 5 of k_lf's row_px
and k_gv's raw_px) and whose last pass stores (gp_store_lancir_row< 3 >) the
caller's 16-bit pixels.

Expected bits, as tests/test_gpu_lanc2h.py defines them: the reference's
CLancIR (tests/helpers.py, checker_lancir) on the exactly widened float32
source; its float32 result narrowed with numpy's .astype(float16), or with
(u + 0x7fff + ((u >> 16) & 1)) >> 16 for bfloat16; integer results taken from
the reference directly. Compared word for word, every element, NaN equal to
NaN. bfloat16 host images are np.uint16 bit arrays."""
import numpy as np
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H
from tests.dnf16_cases import (T, NAN, same, widen, narrow, words, as_f32,
                               from_f32, isnan)

P5 = abi.PATH_GPASS
V_UPG2, V_UPGF = abi.VARIANT_UPG_TWO_PASS, abi.VARIANT_UPG_FUSED
V_UNFUSED = abi.VARIANT_UP2_UNFUSED_IO
MIB = 1 << 20

# (sw, sh, nw, nh)
# upsizing on both axes: k_lf -- 233 output columns are several strips, 97
# source columns two 64-pixel strips of the two-pass k_gv
UP = (97, 61, 233, 150)
# 2 * ceil(3 * k) taps when downsizing: 18 on both axes, 10 on both axes
DN18 = (333, 140, 120, 50)
DN10 = (200, 90, 133, 60)
# one axis down (10 taps), one up (6)
MIXED = (150, 40, 100, 100)
SHAPES = [UP, DN18, DN10, MIXED]
# the planner's tap counts the shapes were chosen for: (horizontal, vertical)
TAPS = {UP: (6, 6), DN18: (18, 18), DN10: (10, 10), MIXED: (10, 6)}
# 28 vertical taps: beyond k_gv's register windows (24), the LDS-window form
# reads float rows only -- the source goes through the pack pass
TALL = (100, 400, 100, 90)
# a source of 40 columns: narrower than whole-pixel lanes are used for (> 48)
NARROW = (40, 80, 100, 200)
# 1-3 channels: width * channels even and odd multiples of two
CH_SHAPES = [(98, 61, 235, 150), (100, 60, 40, 33)]
# held memory: k_lf; the two pass kernels
HELD_UP = (640, 360, 1500, 844)
HELD_DN = (640, 360, 300, 170)
# special values: 97 x 61 up and down (16 taps horizontally, 16 vertically)
SPECIAL_UP = (97, 61, 233, 150)
SPECIAL_DN = (97, 61, 40, 25)

TYPES = ["f16", "bf16", "f32", "u8", "u16"]
H16 = ("f16", "bf16")
# every pair with a 16-bit float type on at least one side
PAIRS = [(a, b) for a in TYPES for b in TYPES if a in H16 or b in H16]
SAME = [("f16", "f16"), ("bf16", "bf16")]

LF_CHUNKS = [1, 7, 9, 13]   # the 8-row ring wraps from 9 on
GV_CHUNKS = [1, 4, 5]


def roads(geom):
    """(path, variant) of every road a shape is run on."""
    r = [(0, 0), (P5, 0)]
    if geom == UP:
        r += [(P5, V_UPGF), (P5, V_UPG2)]
    return r


def source(shape, t, seed):
    if t == "u8":
        return rb.lcg_u8(shape, seed=seed)
    if t == "u16":
        a = rb.lcg_f32(shape, seed=seed)
        return (a * np.float32(65535)).astype(np.uint16)
    a = rb.lcg_f32(shape, seed=seed)
    return narrow(a) if t == "bf16" else a.astype(T[t][1])


def ref_input(src, t):
    """What the reference is given: the exactly widened float32 source of a
    half / bfloat16 one, any other source as it is."""
    return as_f32(src, t) if t in H16 else src


_REF = {}


def case(geom, tin, tout, ch=4):
    """(source, the expected result in `tout` elements): the reference runs
    once per source type, geometry, channel count and class of result (float /
    uint8 / uint16); shared by every test, never written to."""
    sw, sh, nw, nh = geom
    rt = tout if tout in ("u8", "u16") else "f32"
    key = (geom, tin, rt, ch)
    if key not in _REF:
        src = source((sh, sw, ch), tin, seed=sw + sh + ch)
        ref = H.checker_lancir(ref_input(src, tin), nw, nh,
                               out_dtype=T[rt][1])
        src.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (src, ref)
    src, ref = _REF[key]
    return src, from_f32(ref, tout)


def bands(nh):
    """Thirds, and one band with odd bounds."""
    cuts = sorted({0, nh // 3, max(nh - 5, nh // 3), nh})
    b = [(a, c) for a, c in zip(cuts[:-1], cuts[1:]) if c > a]
    odd = (7, 29) if nh >= 30 else ((1, 4) if nh >= 5 else None)
    return b, odd


def padded(src, pitch, t):
    """(sh, sw, ch) -> rows `pitch` elements apart with NaN (integer types:
    77) between them, the last one ending with its pixels (flat)."""
    sh, sw, ch = src.shape
    pad = (np.array([NAN], np.uint16)[0] if t == "bf16" else
           np.float16(np.nan) if t == "f16" else 77)
    flat = np.full(sh * pitch, pad, T[t][1])
    flat.reshape(sh, pitch)[:, :sw * ch] = src.reshape(sh, sw * ch)
    return np.ascontiguousarray(flat[:(sh - 1) * pitch + sw * ch])


# ---- special values -----------------------------------------------------------

BF16_MAX = 0x7f7f  # bfloat16's largest finite value
DENORMALS = (slice(40, 61), slice(56, 97))  # of the half frame


def special_f16_source():
    """97 x 61 half RGBA pixels: +-Inf, NaN and -0 of the source's own, a block
    of half denormals, +-65504, and a block of 64000 whose Lanczos overshoot
    is finite in float32 and beyond 65504."""
    sw, sh = SPECIAL_UP[:2]
    a = rb.lcg_f32((sh, sw, 4), seed=9)
    src = a.astype(np.float16)
    n = np.arange(21 * 41 * 4, dtype=np.uint32).reshape(21, 41, 4)
    bits = (1 + (n * 37) % 1023).astype(np.uint16)
    bits |= ((n & 1) << 15).astype(np.uint16)
    # denormals of both signs, down to the frame's corner: the 16-tap windows
    # of the downsizing shape must fit inside the block
    src[DENORMALS] = bits.view(np.float16)
    # ... and in it the smallest negative denormal behind a field of zeros: at
    # the edge the float32 result is a fraction of it, which narrows to -0
    src[40:61, 76:97] = 0
    src[46:61, 86:97] = np.array([0x8001], np.uint16).view(np.float16)[0]
    src[4:24, 6:40] = 64000
    src[30, 50] = [65504, -65504, 65504, -65504]
    src[2, 3] = [0.0, -0.0, 0.0, -0.0]
    src[34, 80] = [np.inf, 1.0, 1.0, 1.0]
    src[38, 88] = [1.0, -np.inf, 1.0, 1.0]
    src[28, 70] = [1.0, 1.0, np.nan, 1.0]
    return src


def special_bf16_source():
    """97 x 61 bfloat16 RGBA pixels: every exponent (0 .. 255: denormals, Inf
    and NaN among them) with four mantissas and both signs in a block of rows
    of its own, a block of the largest finite value, -0, the smallest denormal
    in a field of zeros, and ordinary pixels around."""
    sw, sh = SPECIAL_UP[:2]
    src = narrow(rb.lcg_f32((sh, sw, 4), seed=9))
    src[2, 3] = [0x0000, 0x8000, 0x0000, 0x8000]
    src[4:10, 6:30] = BF16_MAX
    # the smallest negative denormal inside a field of zeros: at its edge the
    # float32 result is a fraction of it, which narrows to -0
    src[8:26, 34:66] = 0
    src[13:21, 42:58] = 0x8001
    e = np.arange(256, dtype=np.uint16)
    blk = np.zeros((32, 8, 4), np.uint16)
    for i, m in enumerate((0x00, 0x01, 0x40, 0x7f)):
        pat = ((e << 7) | m).reshape(32, 8)
        blk[:, :, i] = pat
    blk[:, 1::2, :] |= 0x8000
    # (the exponents ascend down the block: the non-finite ones are its last
    # row, so what they poison stays a corner of the frame)
    src[26:58, 80:88] = blk
    return src


_SPECIAL = {}


def special_case(tin, tout, geom):
    """-> (source, the reference's result before narrowing, expected result in
    `tout` elements) of the special-value frame of `tin` elements."""
    rt = tout if tout in ("u8", "u16") else "f32"
    key = (tin, rt, geom)
    if key not in _SPECIAL:
        src = special_f16_source() if tin == "f16" else special_bf16_source()
        ref = H.checker_lancir(as_f32(src, tin), geom[2], geom[3],
                               out_dtype=T[rt][1])
        src.setflags(write=False)
        ref.setflags(write=False)
        _SPECIAL[key] = (src, ref)
    src, ref = _SPECIAL[key]
    return src, ref, from_f32(ref, tout)


def special_classes(t, ref, want):
    """Counts of the classes the special-value frames are there for (`ref`:
    the float32 result, `want`: narrowed to `t`)."""
    wf = as_f32(want, t)
    tiny = 2.0 ** -14 if t == "f16" else 2.0 ** -126
    return dict(
        finite=int(np.isfinite(wf).sum()),
        fin_to_inf=int((np.isfinite(ref) & np.isinf(wf)).sum()),
        pos_inf=int((np.isinf(wf) & (wf > 0)).sum()),
        neg_inf=int((np.isinf(wf) & (wf < 0)).sum()),
        nan=int(np.isnan(wf).sum()),
        denormal=int(((wf != 0) & (np.abs(wf) < tiny)).sum()),
        neg_zero=int(((wf == 0) & np.signbit(wf)).sum()),
        size=int(wf.size))
