"""The case table of tests/test_gpu_placement.py (every kernel family with the
output grid placed off the source frame by k / ox / oy) and of the host-only
tests/test_placement_table.py: the cases, how an output's source window is read
from a plan description, the defining property of each placement, the bands,
and the EXPECTATION -- whether the forced path takes the plan.

A case is (row, window case, (horizontal placement, vertical placement)):
`row` names the line of the family list the case belongs to (ROWS), the window
case is a 12-tuple of tests/window_cases.py (front end, sw, sh, nw, nh, ch,
tin, tout, resbits, path, variant, extras) whose extras carry k, ox, oy.

Output j of an axis samples the source at o + j * |k| (k < 0: o is the offset
as given; k > 0: the grid is centred, o += (k - 1) / 2; avir.h:4714-4736,
lancir.h:435-457). The placements are properties of the planner's answer
(windows() below: the source samples an output reads, before the edge clamp):

  shift_in   a whole-pixel shift: the first window starts >= 32 samples before
             sample 0, the last one ends inside the frame
  shift_out  the last window ends >= 32 samples past in_len - 1, the first one
             starts inside the frame
  both_out   both of these overhangs at once
  crop       every window strictly inside the frame, the window starts span
             less than a third of the axis
  outside    the first or the last fifth of the outputs reads nothing but the
             replicated edge sample (vertically: band_source_rows of that band
             is the frame's first or last row alone)
  half       a whole step (2 or 3) at a half-pixel phase: the gather has the
             same coefficients for every output, dn.hip's dn_match takes it
  cover      the grid covers the frame (the un-shifted explicit-k form of 2x)

32 exceeds every default tap count a side, one 8-row marching step, the 8-row
rings of k_lf / k_gf and the 5-deep queue of k_gv; the offsets used are 37 to
130 (and further for shift_out), so whole strips and chunks of replicated
samples occur.

expect() restates the host predicates (up2.hip match_axis, lanc2.hip
match_lanc_axis, gpass.hip match_avir_axis / match_lancir_axis, fused.hip
chain_ok) from the chain shape and the start table of the description; it is
never a record of what the library did.
"""
import ctypes as C
import numpy as np
from avir_amd import abi
from tests import param_cases as PC
from tests import window_cases as W
from tests.helpers import product_desc, free_product_desc

U8, F32, F64 = np.uint8, np.float32, np.float64
V_DN2, V_LADDER, V_OPT = W.V_DN2, W.V_LADDER, W.V_OPT
V_UPG2, V_UPGF = W.V_UPG2, W.V_UPGF
OVERHANG = 32

PLACEMENTS = ("shift_in", "shift_out", "both_out", "crop", "outside", "half",
              "cover")

# the lines of the family list; every one needs two placed cases its forced
# path ran (tests/test_gpu_placement.py), "x2" and "lanc2" excepted: their
# shifted cases are refused, their un-shifted explicit-k case runs
ROWS = ("dn", "sacc", "gh2", "upg", "x2", "lancir", "lanc2", "tiles",
        "generic", "double", "pitch_gamma")


def _c(row, fe, geom, ch, t, bits, path, variant, k, ox, oy, ph, pv, **ex):
    sw, sh, nw, nh = geom
    ex = dict(ex, k=k, ox=ox, oy=oy)
    return (row, (fe, sw, sh, nw, nh, ch, t, t, bits, path, variant, ex),
            (ph, pv))


def _a(row, *a, **ex):
    return _c(row, "avir", *a, **ex)


def _l(row, *a, **ex):
    return _c(row, "lancir", *a, **ex)


CASES = [
    # ---- k_dnf (path 2) and k_dnh + k_dnv (V_DN2): k = -2 from 600x800,
    # k = -3 from 600x900
    _a("dn", (600, 800, 300, 400), 4, F32, 16, 2, 0, -2, -64, -37,
       "shift_in", "shift_in"),
    _a("dn", (600, 800, 300, 400), 4, F32, 16, 2, 0, -2, 250, 170,
       "shift_out", "shift_out"),
    _a("dn", (600, 800, 300, 400), 4, F32, 16, 2, V_DN2, -2, 250, -37,
       "shift_out", "shift_in"),
    _a("dn", (600, 900, 60, 90), 3, U8, 8, 2, 0, -3, 101, 77,
       "crop", "crop"),
    _a("dn", (600, 900, 260, 360), 4, F32, 16, 2, 0, -3, -90, -80,
       "both_out", "both_out"),
    _a("dn", (600, 800, 380, 300), 3, U8, 8, 2, V_DN2, -2, -70, 300,
       "both_out", "shift_out"),
    _a("dn", (600, 800, 90, 200), 4, F32, 16, 2, 0, -2, 211, -130,
       "crop", "outside"),
    _a("dn", (600, 900, 150, 150), 3, U8, 8, 2, V_DN2, -3, -90, 600,
       "shift_in", "outside"),
    _a("dn", (600, 800, 280, 390), 4, F32, 16, 2, 0, 2.0, 0, 0,
       "half", "half"),
    _a("dn", (600, 900, 200, 300), 3, U8, 8, 2, V_DN2, 3.0, 0.5, -0.5,
       "half", "half"),
    _a("dn", (600, 800, 250, 300), 4, F32, 16, 2, V_DN2, -2, 37.5, -40.5,
       "half", "half"),
    _a("dn", (600, 800, 300, 300), 3, U8, 8, 2, 0, -2, -64, 300,
       "shift_in", "shift_out"),
    # (a fractional offset at a whole step keeps one coefficient row too:
    # dn_match takes it -- placement_cases.dn_matches -- at any phase)
    _a("dn", (600, 800, 90, 200), 4, F32, 16, 2, 0, -2, 211.3, -130.6,
       "crop", "outside"),
    # ---- k_sacc2 (RGB uint8), the ladder, RGB float, the optimistic and the
    # exact float RGBA form: k = -2.7, and k = -2 at a fractional offset
    _a("sacc", (600, 805, 222, 148), 3, U8, 8, 5, 0, -2.7, -100, -64,
       "shift_in", "shift_in"),
    _a("sacc", (600, 805, 222, 148), 3, U8, 8, 5, V_LADDER, -2.7, 200, -100,
       "shift_out", "shift_in"),
    _a("sacc", (600, 805, 70, 150), 3, F32, 16, 5, 0, -2.7, 205, -130,
       "crop", "outside"),
    _a("sacc", (600, 805, 222, 200), 4, F32, 16, 5, V_OPT, -2.7, -90, 400,
       "shift_in", "shift_out"),
    _a("sacc", (600, 805, 222, 90), 4, F32, 16, 5, 0, -2.7, 200, 283,
       "shift_out", "crop"),
    _a("sacc", (600, 805, 90, 200), 3, U8, 8, 5, 0, -2.0, 211.3, -130.6,
       "crop", "outside"),
    _a("sacc", (600, 805, 90, 120), 4, F32, 16, 5, 0, -2.0, 211.3, 283.7,
       "crop", "crop"),
    _a("sacc", (600, 805, 120, 90), 3, U8, 8, 5, V_LADDER, -2.7, 400, 283,
       "outside", "crop"),
    _a("sacc", (600, 805, 222, 90), 3, F32, 16, 5, 0, -2.7, -100, 283,
       "shift_in", "crop"),
    _a("sacc", (600, 805, 150, 222), 3, U8, 8, 5, 0, -2.7, -130, 400,
       "outside", "shift_out"),
    # ---- k_gh2 / the gather kernels on 1 < k < 2
    _a("gh2", (600, 600, 300, 300), 4, F32, 16, 5, 0, -1.5, -90, -64,
       "shift_in", "shift_in"),
    _a("gh2", (600, 600, 300, 120), 4, F32, 16, 5, 0, -1.5, 300, 211,
       "shift_out", "crop"),
    _a("gh2", (600, 600, 120, 300), 4, F32, 16, 5, 0, -1.5, 200, 300,
       "crop", "shift_out"),
    # ---- k_gh + k_gv (V_UPG2), k_gf (V_UPGF): k = -0.652 and k = -0.31
    _a("upg", (300, 400, 460, 613), 4, F32, 16, 5, V_UPG2, -0.652, -64, -37,
       "shift_in", "shift_in"),
    _a("upg", (300, 400, 460, 613), 4, F32, 16, 5, V_UPGF, -0.652, 100, 200,
       "shift_out", "shift_out"),
    _a("upg", (300, 400, 300, 600), 3, U8, 8, 5, V_UPG2, -0.31, 100.3, -60,
       "crop", "outside"),
    _a("upg", (300, 400, 460, 300), 3, U8, 8, 5, V_UPGF, -0.31, 200, 150.3,
       "outside", "crop"),
    _a("upg", (300, 400, 460, 613), 4, F32, 16, 5, V_UPGF, -0.31, -64, 300,
       "shift_in", "shift_out"),
    _a("upg", (300, 400, 460, 613), 4, F32, 16, 5, V_UPG2, -0.31, 200, -37,
       "shift_out", "shift_in"),
    _a("upg", (300, 400, 460, 613), 3, U8, 8, 5, V_UPG2, -0.652, -64, 200,
       "shift_in", "shift_out"),
    _a("upg", (300, 400, 460, 613), 3, U8, 8, 5, V_UPGF, -0.652, 100, -37,
       "shift_out", "shift_in"),
    # ---- exact 2x: whole-pixel shifts are not k_up2's (match_axis), the
    # un-shifted explicit form is
    _a("x2", (320, 416, 640, 832), 4, F32, 16, 4, 0, -0.5, -30, 40,
       "shift_in", "shift_out"),
    _a("x2", (320, 416, 640, 832), 4, F32, 16, 0, 0, -0.5, -30, 40,
       "shift_in", "shift_out"),
    _a("x2", (320, 416, 640, 832), 4, F32, 16, 5, 0, -0.5, -30, 40,
       "shift_in", "shift_out"),
    _a("x2", (320, 416, 640, 832), 4, F32, 16, 4, 0, -0.5, -64, -37,
       "shift_in", "shift_in"),
    _a("x2", (320, 416, 640, 832), 4, F32, 16, 5, 0, -0.5, 200, -37,
       "shift_out", "shift_in"),
    _a("x2", (320, 416, 640, 832), 4, F32, 16, 4, 0, 0.5, 0, 0,
       "cover", "cover"),
    # ---- CLancIR: k_lf (float RGBA, RGB uint8 raw rows), the two pass
    # kernels, downsizing RGB uint8
    _l("lancir", (300, 400, 460, 613), 4, F32, 0, 5, 0, -0.652, -64, -37,
       "shift_in", "shift_in"),
    _l("lancir", (300, 400, 460, 613), 3, U8, 0, 5, 0, -0.652, 100, 200,
       "shift_out", "shift_out"),
    _l("lancir", (300, 400, 300, 600), 4, F32, 0, 5, 0, -0.31, 100.3, -60,
       "crop", "outside"),
    _l("lancir", (300, 400, 460, 613), 4, F32, 0, 5, V_UPG2, -0.652, 100, -37,
       "shift_out", "shift_in"),
    _l("lancir", (300, 400, 460, 300), 4, F32, 0, 5, V_UPG2, -0.31, 200, 150.3,
       "outside", "crop"),
    _l("lancir", (600, 805, 222, 200), 3, U8, 0, 5, 0, -2.7, -100, 400,
       "shift_in", "shift_out"),
    _l("lancir", (600, 805, 70, 150), 3, U8, 0, 5, 0, -2.7, 205, -130,
       "crop", "outside"),
    # ---- ... and its exact 2x: shifted on k_lanc2 (refused) and on the
    # automatic path, un-shifted on k_lanc2
    _l("lanc2", (320, 416, 640, 832), 4, F32, 0, 4, 0, -0.5, -30, 40,
       "shift_in", "shift_out"),
    _l("lanc2", (320, 416, 640, 832), 4, F32, 0, 0, 0, -0.5, -30, 40,
       "shift_in", "shift_out"),
    _l("lanc2", (320, 416, 640, 832), 4, F32, 0, 4, 0, 0.5, 0, 0,
       "cover", "cover"),
    # ---- LDS tiles: two-pass (2), fused (3)
    _a("tiles", (500, 700, 320, 140), 4, F32, 16, 2, 0, -1.5625, -90, 250,
       "shift_in", "crop"),
    _a("tiles", (500, 700, 100, 200), 4, F32, 16, 2, 0, -1.5625, 170, -130,
       "crop", "outside"),
    _a("tiles", (350, 500, 167, 75), 4, F32, 16, 3, 0, -2.096, -64, 170,
       "shift_in", "crop"),
    _a("tiles", (350, 500, 50, 150), 4, F32, 16, 3, 0, -2.096, 120, -130,
       "crop", "outside"),
    # ---- the generic per-op kernels (1)
    _a("generic", (300, 400, 420, 150), 4, F32, 16, 1, 0, -0.714, -64, 150,
       "shift_in", "crop"),
    _a("generic", (360, 500, 200, 150), 3, U8, 8, 1, 0, -1.8, -90, -130,
       "shift_in", "outside"),
    # ---- the double pipeline: up64.hip, the tiles
    _a("double", (200, 400, 333, 200), 4, F64, 16, 2, 0, -0.6, 100, 150,
       "shift_out", "crop", fp=abi.FPCLASS_DOUBLE),
    _a("double", (400, 600, 250, 120), 4, F64, 16, 2, 0, -1.6, 200, 200,
       "shift_out", "crop", fp=abi.FPCLASS_DOUBLE),
    # ---- a padded pitch, sRGB gamma
    _a("pitch_gamma", (300, 400, 460, 613), 3, F32, 16, 0, 0, -0.652, -64, 200,
       "shift_in", "shift_out", pad=3),
    _a("pitch_gamma", (300, 400, 150, 300), 4, F32, 16, 0, 0, -0.652, 100, -64,
       "crop", "outside", gamma=1, alpha=3),
]


def case_id(c):
    row, w, (ph, pv) = c
    return "%s-%s-%s-%s" % (row, W.case_id(w), ph, pv)


IDS = [case_id(c) for c in CASES]


# ---- descriptions ---------------------------------------------------------
def _ty(t):
    return {np.dtype(U8): abi.U8, np.dtype(np.uint16): abi.U16,
            np.dtype(F32): abi.F32, np.dtype(F64): abi.F64}[np.dtype(t)]


class Desc(object):
    """`with Desc(case) as d`: the product planner's description of a case
    (PlanDesc or LancirDesc), freed on exit."""

    def __init__(self, c):
        self.w = c[1]

    def __enter__(self):
        fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = self.w
        lib = abi.load()
        if fe == "lancir":
            self.l = C.c_void_p()
            abi.check(lib.avirhip_lancir_create(C.byref(self.l)), "create")
            p = abi.LancirParams()
            lib.avirhip_lancir_params_default(C.byref(p))
            p.SrcSSize = W.pitch(self.w) if ex.get("pad") else 0
            p.kx = p.ky = float(ex["k"])
            p.ox, p.oy = float(ex["ox"]), float(ex["oy"])
            self.d = C.POINTER(abi.LancirDesc)()
            abi.check(lib.avirhip_lancir_build_desc(
                self.l, sw, sh, nw, nh, ch, C.byref(p), _ty(tin), _ty(tout),
                C.byref(self.d)), "lancir_build_desc")
        else:
            self.r, self.d = product_desc(
                sw, sh, nw, nh, ch, k=ex["k"], in_type=_ty(tin),
                out_type=_ty(tout), resbits=bits, ox=ex["ox"], oy=ex["oy"],
                sstride=W.pitch(self.w) if ex.get("pad") else 0,
                fpclass=ex.get("fp", 1))
        return self.d.contents

    def __exit__(self, *a):
        lib = abi.load()
        if self.w[0] == "lancir":
            lib.avirhip_lancir_desc_free(self.d)
            lib.avirhip_lancir_destroy(self.l)
        else:
            free_product_desc(self.r, self.d)
        return False


# ---- the source window of every output ------------------------------------
def gather_table(s, zs):
    """(start, ntaps) of a RESIZE / RESIZE2 step as api.cpp lower_axis makes
    them: over the zero-stuffed view every second tap, half the offset."""
    r = np.ctypeslib.as_array(s.rpos, shape=(s.out_len,))
    stp = 2 if zs else 1
    offs = r["src_offs_px"].astype(np.int64)
    assert not (offs % stp).any()
    return offs // stp, (r["fl"].astype(np.int64) + stp - 1) // stp


def _avir_windows(ax, clamped):
    ops, zs = [], False
    for i in range(ax.n_steps):
        s = ax.steps[i]
        if s.kind == abi.STEP_FIR:
            ops.append(("fir", s.resample_factor, s.flt_latency,
                        s.edge_pixel_count, s.out_len))
        elif s.kind == abi.STEP_UP_ZEROSTUFF:
            zs = True
        elif s.kind in (abi.STEP_RESIZE, abi.STEP_RESIZE2):
            start, nt = gather_table(s, zs)
            end = start + nt - 1
            # (the ends of a range of outputs then give the range's extent)
            assert (np.diff(start) >= 0).all() and (np.diff(end) >= 0).all()
            ops.append(("gather", start, end, None, s.out_len))
            zs = False
        else:
            raise ValueError("no windows through a filtered upsample")
    a = b = np.arange(ops[-1][4], dtype=np.int64)
    for i in range(len(ops) - 1, -1, -1):
        op = ops[i]
        # (need_range: an op's outputs are addressed through the edge clamp.
        # Where the grid lies shows without it: an upsizing axis filters the
        # source row first and replicates the ends of the FILTERED row, so
        # its clamped windows never leave the frame by more than 6 samples)
        if clamped or op[0] == "gather":
            a, b = np.clip(a, 0, op[4] - 1), np.clip(b, 0, op[4] - 1)
        if op[0] == "fir":
            rf, lat, e = op[1], op[2], op[3]
            a, b = rf * (a - e) - lat, rf * (b - e) + lat
        else:
            a, b = op[1][a], op[2][b]
    return a, b


def _lancir_windows(ax):
    pos = np.ctypeslib.as_array(ax.pos, shape=(ax.dst_len,))
    lo = pos["so"].astype(np.int64) - ax.padl
    return lo, lo + ax.kernel_len - 1


def windows(c, d, axis, clamped=False):
    """(lo, hi): the first and last source sample every output of axis "h" /
    "v" reads, from the description -- as the grid places them, before any
    edge clamp; `clamped`: through the clamps of the intermediate rows (the
    source range itself is still kept as it falls)."""
    ax = getattr(d, axis)
    if c[1][0] == "lancir":
        return _lancir_windows(ax)
    return _avir_windows(ax, clamped)


def axis_lens(c, axis):
    """(source length, output length) of an axis."""
    w = c[1]
    return (w[1], w[3]) if axis == "h" else (w[2], w[4])


def origin(c, axis):
    """Where output 0 samples the source, from the call's arguments."""
    ex = c[1][11]
    k, o = float(ex["k"]), float(ex["ox" if axis == "h" else "oy"])
    return o + (k - 1.0) * 0.5 if k > 0 else o


def outside_fifth(lo, hi, in_len):
    """"first" / "last": the fifth of the outputs whose windows lie at or
    beyond an edge of the axis entirely; None."""
    f = len(lo) // 5
    if (hi[:f] <= 0).all():
        return "first"
    if (lo[len(lo) - f:] >= in_len - 1).all():
        return "last"
    return None


def same_taps(s):
    """Whether every output of a RESIZE step takes the same coefficients."""
    r = np.ctypeslib.as_array(s.rpos, shape=(s.out_len,))
    return all((r[f].view(np.uint32 if f == "x" else r[f].dtype) ==
                r[f].view(np.uint32 if f == "x" else r[f].dtype)[0]).all()
               for f in ("phase", "x", "fl", "ftp_off"))


def dn_matches(ax):
    """dn.hip dn_match from the description: RESIZE + 7-tap FIR, a whole
    step K with the tap count dn.hip has, one coefficient row. -> K or 0."""
    if PC._kinds(PC.axis_shape(ax)) != PC.DN:
        return 0
    g, f = ax.steps[0], ax.steps[1]
    if (g.out_len < 8 or f.resample_factor != 1 or f.edge_pixel_count != 0 or
            f.flt_latency != 3):
        return 0
    start, nt = gather_table(g, False)
    K = int(start[1] - start[0])
    if (K, g.bank_filter_len) not in ((2, 24), (3, 38)):
        return 0
    if ((nt != g.bank_filter_len).any() or (np.diff(start) != K).any() or
            not same_taps(g)):
        return 0
    return K


def placement_holds(c, d, axis):
    """None when axis "h" / "v" of the case is placed as its name says; or
    what is wrong."""
    name = c[2][0 if axis == "h" else 1]
    in_len, out_len = axis_lens(c, axis)
    lo, hi = windows(c, d, axis)
    assert len(lo) == out_len
    first, last, end = int(lo[0]), int(hi[-1]), in_len - 1
    o = origin(c, axis)
    if name == "shift_in":
        ok = o == int(o) and first <= -OVERHANG and last <= end
    elif name == "shift_out":
        ok = o == int(o) and last >= end + OVERHANG and first >= 0
    elif name == "both_out":
        ok = first <= -OVERHANG and last >= end + OVERHANG
    elif name == "crop":
        ok = first > 0 and last < end and \
            (int(lo[-1]) - first) * 3 < in_len
    elif name == "outside":
        ok = outside_fifth(lo, hi, in_len) is not None
    elif name == "half":
        ok = abs(o - np.floor(o)) == 0.5 and dn_matches(getattr(d, axis)) != 0
    elif name == "cover":
        ok = -OVERHANG < first <= 0 and end <= last < end + OVERHANG
    else:
        raise ValueError(name)
    return None if ok else "%s %s: windows [%d, %d] .. [%d, %d] of %d" % (
        axis, name, first, int(hi[0]), int(lo[-1]), last, in_len)


def bands(c, d):
    """(name, row0, row1): the first fifth, one inner row, the last fifth, the
    whole frame. A vertically `outside` case has its off-frame fifth among
    them by the definition of the placement."""
    nh = c[1][4]
    f = nh // 5
    return [("first", 0, f), ("row", nh // 2 + 1, nh // 2 + 2),
            ("last", nh - f, nh), ("frame", 0, nh)]


# ---- the expectation ------------------------------------------------------
def _up2_start_table(s, zs_step):
    """up2.hip match_axis on the gather of a FIR -> zero-stuff -> bank axis."""
    start, nt = gather_table(s, True)
    j = np.arange(s.out_len)
    want = (j >> 1) - np.where(j & 1, 2, 3)
    if (start != want).any():
        n = int((start != want).argmax())
        return "output %d starts at sample %d of the filtered row, k_up2 " \
            "reads %d" % (n, start[n], want[n])
    if (nt != 12).any():
        return "an output of fewer than 12 taps"
    if int(start[-1]) + 11 > zs_step.in_len - 1 + zs_step.out_suffix // 2:
        return "the last window passes the zero-stuffed view"
    r = np.ctypeslib.as_array(s.rpos, shape=(s.out_len,))
    for par in (0, 1):
        for f in ("phase", "x", "fl", "ftp_off"):
            v = r[f][par::2].view(np.uint32 if f == "x" else r[f].dtype)
            if (v != v[0]).any():
                return "coefficients differ between outputs of one parity"
    return None


def _gather_step(ax):
    for i in range(ax.n_steps):
        if ax.steps[i].kind in (abi.STEP_RESIZE, abi.STEP_RESIZE2):
            return ax.steps[i], ax.steps[i - 1] if i else None
    return None, None


def _avir_expect(c, d, path):
    fe, sw, sh, nw, nh, ch, tin, tout, bits, _, variant, ex = c[1]
    frame = (sw, sh, nw, nh, ch, tin, tout, bits, ex.get("fp", 1))
    shape = PC.desc_shape(d)
    # (chain shape: what tests/param_cases.py says of it)
    why = PC.expect(shape, frame, path)
    if why is not None or path in (0, 1, 2, 3):
        return why
    for ax in (d.h, d.v):
        g, before = _gather_step(ax)
        zs = g.kind == abi.STEP_RESIZE2
        start, nt = gather_table(g, zs)
        if path == abi.PATH_UP2:
            why = _up2_start_table(g, before)
            if why:
                return why
        else:
            if (nt != PC.gather_taps(PC.axis_shape(ax))).any():
                return "an output of fewer taps than the bank"
            if (np.diff(start) < 0).any():
                return "the starts do not ascend"
    return None


def _lancir_expect(c, d, path):
    fe, sw, sh, nw, nh, ch, tin, tout, bits, _, variant, ex = c[1]
    if path in (0, 1):
        return None
    if path in (2, 3):
        return "CLancIR has no tiles"
    for ax in (d.v, d.h):
        pos = np.ctypeslib.as_array(ax.pos, shape=(ax.dst_len,))
        start = pos["so"].astype(np.int64) - ax.padl
        if path == abi.PATH_UP2:
            # lanc2.hip match_lanc_axis
            if ax.kernel_len != 6 or ax.dst_len != 2 * ax.src_len or \
                    ax.n_filters != 2:
                return "not a 6-tap exact 2x of two filters"
            j = np.arange(ax.dst_len)
            want = (j >> 1) - np.where(j & 1, 2, 3)
            if (start != want).any():
                n = int((start != want).argmax())
                return "output %d starts at sample %d, k_lanc2 reads %d" % (
                    n, start[n], want[n])
            fi = pos["flt_index"]
            if fi[0] == fi[1] or (fi[0::2] != fi[0]).any() or \
                    (fi[1::2] != fi[1]).any():
                return "filters do not alternate"
        else:
            # gpass.hip match_lancir_axis
            if ax.kernel_len < 2 or ax.kernel_len > 64 or ax.kernel_len & 1:
                return "kernel of %d taps" % ax.kernel_len
            if ch != 4 and ax.kernel_len < 4:
                return "kernel of %d taps on a padded image" % ax.kernel_len
            if (np.diff(start) < 0).any():
                return "the starts do not ascend"
    return None


def expect(c, d, path=None):
    """-> None: the forced path takes the plan of the case; or the reason it
    refuses. d = the case's description (Desc)."""
    path = c[1][9] if path is None else path
    if c[1][0] == "lancir":
        return _lancir_expect(c, d, path)
    return _avir_expect(c, d, path)
