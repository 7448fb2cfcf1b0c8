"""The inputs of tests/test_gpu_sacc16.py and tests/test_sacc16_table.py:
downsizing by a non-integer ratio of 2 or more (path 5) of half / bfloat16
images whose first pass -- the streaming-accumulation kernels of sacc.hip,
k_sacc< 4 / 5 > and k_sacc2< 4 / 5 > -- reads the caller's 16-bit pixels where
they lie.

Expected bits, as tests/dnf16_cases.py defines them: the reference on the
exactly widened float32 source, its float32 result narrowed with numpy's
.astype(float16) or with the header's integer formula for bfloat16; compared
word for word, NaN equal to NaN."""
import numpy as np
from avir_amd import abi
from tests import helpers as H
from tests.dnf16_cases import (T, NAN, case, same, bands, widen, narrow,
                               words, as_f32, from_f32, special_classes)
from tests.gp16_cases import PAIRS, SAME, padded, special_source

P5 = abi.PATH_GPASS
V_OPT = abi.VARIANT_SACC_OPTIMISTIC

# frames of fewer source pixels keep the pack pass in front (gpass.hip,
# sa16_minpix): their float copy is under 1 MiB
FLOOR = 65536

# the step kinds of an axis (tests/gp16_cases.py): k >= 2 -- resize, filter;
# upsizing -- filter, 2x zero-stuffing, resize
AX_DOWN, AX_UP = [3, 0], [0, 1, 4]

# name -> ((sw, sh, nw, nh), (horizontal, vertical) step kinds, what it is for)
SHAPES = {
    "acc": ((400, 300, 150, 113), (AX_DOWN, AX_DOWN),
            "whole 8-sample groups; 300 rows = 4 strips + 44"),
    "acc_odd": ((333, 211, 121, 79), (AX_DOWN, AX_DOWN),
                "an odd width; a last strip of 19 rows"),
    "mixed_h": ((600, 120, 220, 200), (AX_DOWN, AX_UP),
                "horizontal k >= 2, vertical upsizing (k_sacc, then k_gv)"),
    "wide": ((1031, 67, 377, 25), (AX_DOWN, AX_DOWN),
             "long rows; a last strip of 3 lanes"),
    # the narrowest rows: every group is an edge group; 7 and 5 pixels are
    # below k_sacc2's 8; every row's last group is clamped
    "w9": ((9, 8000, 4, 3000), (AX_DOWN, AX_DOWN), "rows of 9 pixels"),
    "w8": ((8, 8200, 3, 3000), (AX_DOWN, AX_DOWN), "rows of 8 pixels"),
    "w7": ((7, 10000, 3, 3600), (AX_DOWN, AX_DOWN), "rows of 7 pixels"),
    "w5": ((5, 14000, 2, 5000), (AX_DOWN, AX_DOWN), "rows of 5 pixels"),
    "floor": ((300, 200, 100, 67), (AX_DOWN, AX_DOWN),
              "60,000 pixels, below the floor: the pack pass's road"),
}
NARROW = ["w9", "w8", "w7", "w5"]
# the shapes of the every-pair test and of the held-memory test
PAIR_SHAPES = ["acc", "acc_odd", "mixed_h"]
HELD_SHAPES = ["acc", "acc_odd", "mixed_h", "wide"]

# the automatic path takes a 16-bit source with both axes on the accumulation
# kernels from this many source pixels on (gpass.hip, sa16_auto_minpix: path 5
# measured ahead of the tiles at 2560x1440, behind at 1920x1080) ...
AUTO_MINPIX = 3600000
# ... the smallest measured shape over it ((sw, sh, nw, nh), channels), and
# shapes under it
AUTO_P5 = [((2560, 1440, 1000, 563), 4)]
AUTO_BEFORE = [(1920, 1080, 700, 394), (400, 300, 150, 113),
               (300, 200, 100, 67)]

# forced chunk lengths (AVIRHIP_SA_CHUNK) of the seam test
CHUNKS = [1, 2, 3, 5, 17]

# the special-value frame (tests/gp16_cases.py: special_source)
SPECIAL = ((384, 288), (150, 113))


def geom(name):
    return SHAPES[name][0]


def pixels(name):
    sw, sh, nw, nh = geom(name)
    return sw * sh


_SPECIAL = {}


def special_case(t):
    """-> (source in `t` elements, float32 reference of the widened source,
    expected result in `t` elements) of SPECIAL. Half: the half frame with its
    block of denormals; bfloat16: the float32 frame narrowed."""
    size, out = SPECIAL
    if t not in _SPECIAL:
        src = special_source("f16", size) if t == "f16" else narrow(
            special_source("bf16", size))
        ref = H.checker_avir(as_f32(src, t), out[0], out[1],
                             out_dtype=np.float32, resbits=16)
        src.setflags(write=False)
        ref.setflags(write=False)
        _SPECIAL[t] = (src, ref)
    src, ref = _SPECIAL[t]
    return src, ref, from_f32(ref, t)


def finite_of(src, t):
    """The special frame with its non-finite elements replaced by 1."""
    f = as_f32(src, t).copy()
    f[~np.isfinite(f)] = 1.0
    return from_f32(f, t)
