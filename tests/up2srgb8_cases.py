"""The inputs of tests/test_gpu_up2srgb8.py and tests/test_up2srgb8_table.py:
exact-2x upsizing of 8-bit images with sRGB gamma (UseSRGBGamma; k_up2's
IO 8 / 9 and SRC 313 / 314 kinds, up2.hip).

Expected bits: the reference (tests/helpers.py, checker_avir, gamma=True,
alpha=..., resbits=8) on the caller's own source; compared word for word, NaN
equal to NaN (a float32 result under gamma is the linear image)."""
import numpy as np
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H
from tests import dnsrgb8_cases as DN

T = DN.T

# (sw, sh, nw, nh). Strips are 64 output columns, marching steps 8 source rows:
# three full strips and a last one two columns wide; one full strip and a
# 16-column one; a frame under the smallest chunk; several chunks under the
# default split (the shapes window_cases.py runs on path 4 at ResBitDepth 8)
SMALL = [(97, 80, 194, 160), (40, 80, 80, 160), (200, 48, 400, 96)]
RGBA_BIG = (322, 420, 644, 840)
RGB_BIG = (321, 420, 642, 840)
SEAMS = SMALL[0]


def shapes(ch):
    """A grey image's plan is k_up2's from the planner's cost model only at the
    two larger shapes (tests/test_up2srgb8_table.py pins which is which); below
    it filters the zero-stuffed image whole, and the call is not path 4's."""
    if ch == 1:
        return [RGB_BIG, RGBA_BIG]
    return SMALL + [RGB_BIG if ch == 3 else RGBA_BIG]


ALL_SHAPES = SMALL + [RGBA_BIG, RGB_BIG]

# Small frames whose plans ARE the transposed form's (found with transposed()
# below), for what the larger two do not reach in the kernel's gamma kinds: a
# frame shorter than the smallest chunk (46 source rows: five marching steps
# and 6 rows in the last), and a 16-column last strip (336 = 5 * 64 + 16)
SHORT = (640, 46, 1280, 92)
STRIP16 = (168, 180, 336, 360)

# The library offers the kernel's gamma kinds by frame size (api.cpp:
# up2srgb_raw_minpix / up2srgb_raw_maxpix, up2srgb_store_maxpix, in source
# pixels, read per call). The tests of the kinds themselves run with the
# bounds wide open; the test of the bounds drives each from both sides.
RAW_MIN = "AVIRHIP_UP2SRGB_RAW_MINPIX"
RAW_MAX = "AVIRHIP_UP2SRGB_RAW_MAXPIX"
STORE_MAX = "AVIRHIP_UP2SRGB_STORE_MAXPIX"
WIDE = {RAW_MIN: "0", RAW_MAX: "1000000000", STORE_MAX: "1000000000"}

PARENT = ["pack pass", "k_up2", "output stage"]


def transposed(geom, ch=4):
    """Whether the plan of the shape runs the kernel's transposed form, the one
    the fused loads and stores live in (up2_vt: both axes' interpolation phases
    bit-symmetric) -- read off the product planner's description on the CPU.
    At ResBitDepth 8 the planner takes, for the smaller frames, a bank of
    order 1 at the fraction x = 0.5: the taps are ftp + ftp2 * 0.5 in float,
    symmetric in value and not in bits, and the call runs the plain form
    (the pack pass, k_up2< false >, the output stage, with or without gamma:
    tests/avir_road_cases.py's `up2_u8c4_short`). A bank of order 0, or x = 0,
    gives the stored taps themselves."""
    sw, sh, nw, nh = geom
    r, d = H.product_desc(sw, sh, nw, nh, ch, resbits=8, in_type=abi.U8,
                          out_type=abi.U8)
    try:
        ok = True
        for ax in (d.contents.h, d.contents.v):
            st = ax.steps[ax.n_steps - 1]
            ok &= (st.bank_order == 0 or
                   all(st.rpos[j].x == 0.0 for j in range(st.out_len)))
    finally:
        H.free_product_desc(r, d)
    return bool(ok)


def road(geom, ch, raw):
    """The tags of a uint8-result gamma call on path 4: the kernel alone
    behind a uint8 RGB / RGBA source (`raw`), the pack pass in front of it
    behind any other; the road from before these kinds where the plan runs the
    plain form."""
    if not transposed(geom, ch):
        return PARENT
    return ["k_up2"] if raw else ["pack pass", "k_up2"]

# (tin, tout, channels, AlphaIndex): the raw kinds (uint8 on both sides), the
# store kinds behind the pack pass's linear copy of a float, a grey and a
# uint16 source, and the road from before these kinds (a float result)
CASES = [("u8", "u8", 4, -1), ("u8", "u8", 4, 3), ("u8", "u8", 4, 0),
         ("u8", "u8", 3, -1), ("f32", "u8", 4, 3), ("f32", "u8", 3, -1),
         ("f32", "u8", 1, -1), ("u16", "u8", 4, 3), ("u8", "f32", 4, 3)]
# what AVIRHIP_VARIANT_UP2_UNFUSED_IO is compared on
PAIRS = [c for c in CASES if c[1] == "u8"]

bands = DN.bands
words = DN.words
gvars = DN.gvars
same = DN.same
reference = DN.reference


def source(shape, t, seed):
    """Mid-range pixels: upsized LCG noise at full range clamps a tenth of
    its bytes, and the comparison would be one of clamps."""
    a = (64 + rb.lcg_u8(shape, seed=seed) // 2).astype(np.uint8)
    if t == "u8":
        return a
    if t == "u16":
        return a.astype(np.uint16) * 257
    return (a.astype(np.float32) / np.float32(255.0)).astype(np.float32)


def case(geom, tin, tout, ch=4, alpha=-1):
    """(source, the reference's result) of such pixels, seed sw + sh."""
    sw, sh, nw, nh = geom
    return reference(("up2", geom, tin, tout, ch, alpha),
                     lambda: source((sh, sw, ch), tin, sw + sh), nw, nh, tout,
                     alpha)


# ---- every threshold ----------------------------------------------------------

RAMP = (200, 128, 400, 256)
# (the same frame where the plan is the transposed form's: the kernel's stage)
RAMP_BIG = (322, 420, 644, 840)


def ramp_source(geom=RAMP):
    """Every byte value as a result, and the clamps at both ends."""
    sw, sh = geom[:2]
    a = rb.lcg_u8((sh, sw, 4), seed=7)
    rows = (np.arange(sh, dtype=np.int64) * 255 // (sh - 1)).astype(np.uint8)
    a[:, :100] = rows[:, None, None]
    a[0:20, 100:150] = 0
    a[20:40, 100:150] = 255
    return a


def ramp_case(geom=RAMP):
    return reference(("up2 ramp", geom), lambda: ramp_source(geom), geom[2],
                     geom[3], "u8", 3)


# ---- special values -------------------------------------------------------------

SPECIAL = SMALL[0]
SPECIAL_BIG = RGBA_BIG


def special_source(geom=SPECIAL):
    """float32 pixels whose linear results leave the range the thresholds
    were searched in (|v| > 16), overflow, and are not numbers
    (dnsrgb8_cases.special_source's recipe on this frame)."""
    sw, sh = geom[:2]
    f = source((sh, sw, 4), "f32", 9)
    f[4:24, 6:40] = 40
    f[30:40, 10:40] = -30
    f[46:56, 50:80] = 3e38
    f[62, 20] = [np.inf, 1, 1, 1]
    f[66, 60] = [1, -np.inf, 1, 1]
    f[72, 40] = [1, 1, np.nan, 1]
    return f


def special_case(tout="u8", geom=SPECIAL):
    return reference(("up2 special", tout, geom),
                     lambda: special_source(geom), geom[2], geom[3], tout, 3)
