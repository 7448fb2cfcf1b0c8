"""The inputs of tests/test_gpu_dnsrgb8.py and tests/test_dnsrgb8_table.py:
whole-ratio (2x, 3x) downsizing of 8-bit images with sRGB gamma
(UseSRGBGamma; k_dnfh's DH_S8 kinds, dnf.hip).

Expected bits: the reference (tests/helpers.py, checker_avir, gamma=True,
alpha=..., resbits=8) on the caller's own source; compared word for word, NaN
equal to NaN (a float32 result under gamma is the linear image)."""
import numpy as np
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H
from tests import dnf16_cases as D16

T = {"u8": (abi.U8, np.uint8), "u16": (abi.U16, np.uint16),
     "f32": (abi.F32, np.float32)}

# (sw, sh, nw, nh): dnf16_cases.DNF_SHAPES -- the smallest at which strips,
# chunks and every (KH, KV) form occur
SHAPES = [
    (600, 400, 300, 200),   # K = 2
    (600, 402, 200, 134),   # K = 3
    (384, 216, 192, 72),    # form 23
    (390, 260, 130, 130),   # form 32
    (254, 200, 127, 100),   # the last strip is one column wide
    (129, 93, 43, 31),      # K = 3, 43 = 42 + 1
]
K2, K3 = SHAPES[0], SHAPES[1]
assert sorted(SHAPES) == sorted(D16.DNF_SHAPES)
# At ResBitDepth 8 the planner gives two of those other plans than at 16
# (a 2x axis gets the plan k_dnf matches -- resize, correction filter -- only
# from more outputs on): 390x260 -> 130x130 and 254x200 -> 127x100 run the
# tiles behind the pack pass, with the reference's bits like every call. The
# smallest shapes found that ARE the kernel's in their place (tests/
# test_dnsrgb8_table.py pins which is which): form 32, and K = 2 with a last
# strip one column wide
EXTRA_SHAPES = [(390, 600, 130, 300), (254, 300, 127, 150)]
NOT_DNF = [SHAPES[3], SHAPES[4]]
DNF_SHAPES = [g for g in SHAPES if g not in NOT_DNF] + EXTRA_SHAPES

# (tin, tout, channels): the three instantiated pairs -- (S8, S8), (S8, F32),
# (F32, S8) behind the pack pass's linear copy of a float, an RGB, a grey and
# a uint16 source
PAIRS = [("u8", "u8", 4), ("u8", "f32", 4), ("f32", "u8", 4),
         ("f32", "u8", 3), ("f32", "u8", 1), ("u16", "u8", 4)]
ALPHAS = (-1, 3, 0)

bands = D16.bands
words = D16.words


def alphas(ch):
    """AlphaIndex 3 and 0 name a channel of 4-channel pixels only."""
    return ALPHAS if ch == 4 else (-1,)


def gvars(alpha):
    """CImageResizerVars with UseSRGBGamma and this AlphaIndex."""
    import avir_amd
    v = avir_amd.CImageResizerVars()
    v.UseSRGBGamma = 1
    v.AlphaIndex = alpha
    return v


def source(shape, t, seed):
    if t == "u8":
        return rb.lcg_u8(shape, seed=seed)
    if t == "u16":
        return rb.lcg_u8(shape, seed=seed).astype(np.uint16) * 257
    return rb.lcg_f32(shape, seed=seed)


_REF = {}


def reference(key, make, nw, nh, tout, alpha):
    """The reference's result of `make()`, once per key; read-only."""
    if key not in _REF:
        src = make()
        ref = H.checker_avir(src, nw, nh, out_dtype=T[tout][1], resbits=8,
                             gamma=True, alpha=alpha)
        src.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (src, ref)
    return _REF[key]


def case(geom, tin, tout, ch=4, alpha=-1):
    """(source, the reference's result) of lcg pixels, seed sw + sh."""
    sw, sh, nw, nh = geom
    return reference((geom, tin, tout, ch, alpha),
                     lambda: source((sh, sw, ch), tin, sw + sh), nw, nh, tout,
                     alpha)


def same(got, want, what):
    """Word for word; NaN == NaN whatever the payload."""
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype, what
    bad = words(got) != words(want)
    if want.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    n = int(bad.sum())
    print("%s: %d of %d elements differ" % (what, n, want.size))
    assert n == 0, "%s: %d of %d elements differ, first at %r" % (
        what, n, want.size, tuple(np.argwhere(bad)[0]))


# ---- every threshold ----------------------------------------------------------

RAMP = (600, 400, 300, 200)


def ramp_source():
    """Every byte value as a result, and the clamps at both ends."""
    sw, sh = RAMP[:2]
    a = rb.lcg_u8((sh, sw, 4), seed=7)
    idx = np.arange(a.size, dtype=np.int64).reshape(a.shape)
    a[:, :150] = ((idx // 37) % 256)[:, :150].astype(np.uint8)
    rows = (np.arange(sh, dtype=np.int64) * 255 // 399).astype(np.uint8)
    a[:, 150:300] = rows[:, None, None]
    a[0:60, 300:450] = 0
    a[60:120, 300:450] = 255
    return a


def ramp_case():
    return reference("ramp", ramp_source, RAMP[2], RAMP[3], "u8", 3)


# ---- special values -------------------------------------------------------------

SPECIAL = (192, 144, 64, 48)
SPECIAL_BIG = (384, 288, 128, 96)


def special_source(geom=SPECIAL):
    """float32 pixels whose linear results leave the range the thresholds
    were searched in (|v| > 16), overflow, and are not numbers."""
    sw, sh = geom[:2]
    f = rb.lcg_f32((sh, sw, 4), seed=9)
    f[6:40, 8:60] = 40
    f[90:100, 20:60] = -30
    f[110:120, 100:140] = 3e38
    f[60, 175] = [np.inf, 1, 1, 1]
    f[70, 180] = [1, -np.inf, 1, 1]
    f[80, 170] = [1, 1, np.nan, 1]
    return f


def special_case(geom=SPECIAL, tout="u8"):
    return reference(("special", geom, tout), lambda: special_source(geom),
                     geom[2], geom[3], tout, 3)
