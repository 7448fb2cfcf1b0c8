"""The cases of the per-op executor's own test (tests/test_gpu_perop.py): the
kernels of generic.hip's launch_op and api.cpp's run_generic, which run float
plans in float and the double class in double from ONE text. Each shape is
there for the op kinds its chain lowers to; `steps` names, for the horizontal
axis, each step's kind and the fields that make it the case it is, and
tests/test_perop_table.py holds the product planner to them in both classes,
so that a planner change cannot quietly empty a row.

A row: name, (sw, sh, nw, nh), BuildMode, ResBitDepth, channel counts, steps."""
import numpy as np
from avir_amd import abi

FLT, DBL = 1, abi.FPCLASS_DOUBLE

_FIR7 = ("FIR", dict(edge_pixel_count=3, flt_len=7))
_UPF = ("UP_FILTERED", dict(resample_factor=2, prefix_dc_len=">0",
                            suffix_dc_len=">0"))
UPG = (37, 21, 100, 57)

ROWS = [
    # OP_FIR, OP_UPF with both DC tails, OP_GATHER over VIEW_RAW
    ("up_order0", UPG, 0, 8, (3, 1, 4),
     [_FIR7, _UPF, ("RESIZE", dict(bank_order=0))]),
    # an order-1 bank: the ftp + ftp2 * x expansion of lower_axis
    ("up_order1", UPG, 0, 16, (3,),
     [_FIR7, _UPF, ("RESIZE", dict(bank_order=1))]),
    # VIEW_ZS and zs_mmax
    ("up_zerostuff", UPG, 1, 16, (3,),
     [_FIR7, ("UP_ZEROSTUFF", dict(resample_factor=2)), ("RESIZE2", {})]),
    # downsizing, a FIR behind a gather
    ("down", (64, 48, 24, 18), 0, 8, (3,),
     [("FIR", dict(edge_pixel_count=3, flt_len=11)), ("RESIZE", {}),
      ("FIR", {})]),
    # a filtered upsample as the first op (up_inprefix 5)
    ("upf_first", (40, 30, 33, 26), 0, 8, (3,),
     [("UP_FILTERED", dict(in_prefix=5)), ("RESIZE", {}), ("FIR", {})]),
    # a frame smaller than one 64 x 4 block
    ("tiny", (7, 5, 13, 11), -1, 8, (3,),
     [("FIR", {}), ("UP_FILTERED", {}), ("RESIZE", {})]),
]

# (name, channels, class, source type, result type): float images in both
# classes; on the double class one uint8 and one float64 case as well, so that
# its pack pass, its in-place result and its integer output stage each run
# once around the shared driver
CASES = [(r[0], ch, fp, np.float32, np.float32)
         for r in ROWS for ch in r[4] for fp in (FLT, DBL)]
CASES += [("up_order0", 3, DBL, np.uint8, np.uint8),
          ("up_order0", 3, DBL, np.float64, np.float64)]


def row(name):
    return [r for r in ROWS if r[0] == name][0]


def case_id(c):
    return "%s-c%d-%s-%s-%s" % (c[0], c[1], "dbl" if c[2] == DBL else "flt",
                                np.dtype(c[3]).name, np.dtype(c[4]).name)
