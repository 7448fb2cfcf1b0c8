"""The inputs of tests/test_gpu_dnf16.py and tests/test_dnf16_table.py: whole-
ratio (2x, 3x) downsizing of half / bfloat16 RGBA images (k_dnfh, dnf.hip).

Expected bits, as tests/test_gpu_lanc2h.py defines them: the reference
(tests/helpers.py, checker_avir, resbits=16) on the exactly widened float32
source, its float32 result narrowed with numpy's .astype(float16), or with
(u + 0x7fff + ((u >> 16) & 1)) >> 16 for bfloat16; compared word for word, NaN
equal to NaN. bfloat16 host images are np.uint16 bit arrays."""
import numpy as np
from avir_amd import abi
from tests import refbind as rb
from tests import helpers as H

# element types by name: (type code, numpy type of the host array)
T = {"bf16": (abi.BF16, np.uint16), "f16": (abi.F16, np.float16),
     "f32": (abi.F32, np.float32), "u8": (abi.U8, np.uint8),
     "u16": (abi.U16, np.uint16)}
NAN = 0x7fc0  # a bfloat16 NaN

# (tin, tout): every instantiated (SRC, OUT) pair of k_dnfh, and the integer
# output stage behind a 16-bit source
PAIRS = [("f16", "f16"), ("bf16", "bf16"), ("f16", "bf16"), ("bf16", "f16"),
         ("f32", "f16"), ("f32", "bf16"), ("f16", "f32"), ("bf16", "f32"),
         ("f16", "u8"), ("bf16", "u16")]

# (sw, sh, nw, nh). Strips are 42 output columns, chunks 8 output rows at these
# sizes (dn_run_hv's rule: at least 8 rows, one workgroup per compute unit).
SHAPES = [
    (600, 400, 300, 200),   # K = 2: 8 strips x 25 chunks
    (600, 402, 200, 134),   # K = 3
    (384, 216, 192, 72),    # K = 2 along x, 3 along y: kernel form 23
    (384, 216, 128, 108),   # form 32
    (170, 122, 85, 61),     # 85 = 2 * 42 + 1: the last strip is one column
    (129, 93, 43, 31),      # 43 = 42 + 1, K = 3
    (24, 24, 8, 8),         # every halo clamps
]
K2, K3 = SHAPES[0], SHAPES[1]
# The planner gives a 2x axis the plan k_dnf / k_dnfh match (resize + correction
# filter, two steps) only from about 96 outputs on; under that it puts a filter
# in front and the call runs the tiles (tests/test_dnf16_table.py pins which
# shapes are which). So (170, 122 -> 85, 61) and (384, 216 -> 128, 108) above
# never reach the kernel; these do: K = 2 with a last strip one column wide
# (127 = 3 * 42 + 1), and the kernel form 32
EXTRA_SHAPES = [(254, 200, 127, 100), (390, 260, 130, 130)]
# the shapes whose plans are k_dnfh's for certain (a call that ran it leaves
# no float copy on the plan)
DNF_SHAPES = SHAPES[:3] + [SHAPES[5]] + EXTRA_SHAPES

# the special-value frame and its four results (K = 22, 33, 23, 32)
SPECIAL_SRC = (192, 144)
SPECIAL_OUT = [(96, 72), (64, 48), (96, 48), (64, 72)]
# ... of which (64, 48) alone is k_dnfh's (see EXTRA_SHAPES): the same pixels in
# a frame twice the size, whose four results all are
SPECIAL_BIG_SRC = (384, 288)
SPECIAL_BIG_OUT = [(192, 144), (128, 96), (192, 96), (128, 144)]


def widen(b):
    """bfloat16 bits -> float32, exact for every bit pattern."""
    return (np.ascontiguousarray(b).astype(np.uint32) << 16).view(np.float32)


def narrow(f):
    """float32 -> bfloat16 bits: the contract's integer formula; NaN -> a NaN."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(f)] = NAN
    return r


def isnan(a, t):
    return np.isnan(widen(a)) if t == "bf16" else (
        np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool))


def as_f32(a, t):
    return widen(a) if t == "bf16" else (
        a.astype(np.float32) if t == "f16" else a)


def from_f32(res, t):
    if t == "bf16":
        return narrow(res)
    if t == "f16":
        with np.errstate(over="ignore", invalid="ignore"):
            return res.astype(np.float16)
    return res


def source(shape, t, seed):
    if t == "u8":
        return rb.lcg_u8(shape, seed=seed)
    a = rb.lcg_f32(shape, seed=seed)
    return narrow(a) if t == "bf16" else a.astype(T[t][1])


_REF = {}


def case(geom, tin, tout="f32", ch=4):
    """(source, the expected result in `tout` elements): the reference runs
    once per source type, geometry and class of result (float / uint8 /
    uint16); shared by every test, never written to."""
    sw, sh, nw, nh = geom
    rt = tout if tout in ("u8", "u16") else "f32"
    key = (geom, tin, rt, ch)
    if key not in _REF:
        src = source((sh, sw, ch), tin, seed=sw + sh)
        ref = H.checker_avir(as_f32(src, tin), nw, nh, out_dtype=T[rt][1],
                             resbits=16 if rt != "u8" else 8)
        src.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (src, ref)
    src, ref = _REF[key]
    return src, from_f32(ref, tout)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(got, want, tout, what):
    """Word for word; NaN == NaN whatever the payload."""
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype, what
    bad = words(got) != words(want)
    bad &= ~(isnan(got, tout) & isnan(want, tout))
    n = int(bad.sum())
    print("%s: %d of %d elements differ" % (what, n, want.size))
    assert n == 0, "%s: %d of %d elements differ, first at %r" % (
        what, n, want.size, tuple(np.argwhere(bad)[0]))


def bands(nh):
    """Thirds, and one band with odd bounds inside a chunk of 8 rows."""
    cuts = sorted({0, nh // 3, max(nh - 5, nh // 3), nh})
    b = [(a, c) for a, c in zip(cuts[:-1], cuts[1:]) if c > a]
    odd = (9, 15) if nh >= 16 else ((1, 4) if nh >= 5 else None)
    return b, odd


# ---- special values -----------------------------------------------------------

def _special_pixels(src):
    src[2, 3] = [0.0, -0.0, 0.0, -0.0]
    src[60, 175] = [np.inf, 1.0, 1.0, 1.0]
    src[70, 180] = [1.0, -np.inf, 1.0, 1.0]
    src[80, 170] = [1.0, 1.0, np.nan, 1.0]


def special_f16_source(size=SPECIAL_SRC):
    """Half pixels whose results are half denormals (rows 100.. under 2^-14),
    +-Inf and NaN of the source's own, and finite float32 values beyond 65504
    (the 64000 block's overshoot)."""
    sw, sh = size
    a = rb.lcg_f32((sh, sw, 4), seed=9)
    a[100:] *= np.float32(6e-5)
    src = a.astype(np.float16)
    src[50, 90] = [65504, -65504, 65504, -65504]
    src[6:40, 8:60] = 64000
    _special_pixels(src)
    return src


def special_f32_source(size=SPECIAL_SRC):
    """float32 pixels for a bfloat16 result: float32 denormals (rows 100..),
    +-Inf and NaN, a block near 1e38. (Finite results that round beyond the
    largest bfloat16 cannot come out of this pipeline: partial sums overflow
    float32 first.)"""
    sw, sh = size
    src = rb.lcg_f32((sh, sw, 4), seed=9)
    src[100:] *= np.float32(1.1e-38)
    src[50, 90] = [65504, -65504, 65504, -65504]
    src[6:40, 8:60] = np.float32(1e38) * (
        1 - np.float32(0.12) * rb.lcg_f32((34, 52, 4), seed=4))
    _special_pixels(src)
    return src


_SPECIAL = {}


def special_case(t, out, size=SPECIAL_SRC):
    """(source, expected result) of the special-value frame for a half result
    of a half source (t == "f16") or a bfloat16 result of a float32 source."""
    key = (t, out, size)
    if key not in _SPECIAL:
        src = (special_f16_source(size) if t == "f16"
               else special_f32_source(size))
        ref = H.checker_avir(src.astype(np.float32), out[0], out[1],
                             out_dtype=np.float32, resbits=16)
        src.setflags(write=False)
        ref.setflags(write=False)
        _SPECIAL[key] = (src, ref)
    src, ref = _SPECIAL[key]
    return src, ref, from_f32(ref, t)


def special_classes(t, ref, want):
    """Counts of the classes the special-value frame is there for."""
    wf = as_f32(want, t)
    tiny = 2.0 ** -14 if t == "f16" else 2.0 ** -126
    return dict(
        fin_to_inf=int((np.isfinite(ref) & np.isinf(wf)).sum()),
        pos_inf=int((np.isinf(ref) & (ref > 0)).sum()),
        neg_inf=int((np.isinf(ref) & (ref < 0)).sum()),
        nan=int(np.isnan(ref).sum()),
        denormal=int(((wf != 0) & (np.abs(wf) < tiny)).sum()),
        size=int(ref.size))
